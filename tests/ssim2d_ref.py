"""Torch / numpy restatement of the spatial image loss (csrc/ssim2d.hip, `ops.image_loss2d_grad`), written for the tests.

The standard SSIM: an 11x11 Gaussian window (sigma 1.5) as a grouped F.conv2d over H x W of every colour channel, zero
padding 5 -- loss_utils.ssim (src/utils/loss_utils.py:57-97) as it computes on CHW images.  `dtype` is a parameter: fp64 is
the reference of the GPU tests, fp32 the yardstick whose own error against fp64 sets their tolerance (`bound`).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
R = 5


def window1d():
    """gaussian(11, 1.5) in fp32, built as the library builds it: exp in double, rounded to fp32, summed in fp32 in index
    order, divided in fp32."""
    g = np.array([np.float32(math.exp(-((i - 5) ** 2) / (2.0 * 1.5 * 1.5))) for i in range(11)], np.float32)
    s = np.float32(0.0)
    for x in g:
        s = np.float32(s + x)
    return (g / s).astype(np.float32)


def window2d(dtype):
    """G = g g^T from the fp32 g: exact products in fp64, rounded ones in fp32 (create_window's .mm in fp32)."""
    g = torch.from_numpy(window1d()).to(dtype)
    return (g[:, None] @ g[None, :]).to(dtype)


def _conv(img, dtype):
    """G * img on (V,3,H,W), per channel, zero padding 5."""
    w = window2d(dtype).expand(3, 1, 11, 11).contiguous()
    return F.conv2d(img, w, padding=R, groups=3)


def masked(pred, target, mask, dtype):
    x, y = pred.to(dtype), target.to(dtype)
    if mask is not None:
        m = mask.to(dtype)[:, None]
        x, y = x * m, y * m
    return x, y


def ssim_map(x, y, dtype=torch.float64):
    """S (V,3,H,W) of x, y (already masked)."""
    x, y = x.to(dtype), y.to(dtype)
    mu1, mu2 = _conv(x, dtype), _conv(y, dtype)
    s11 = _conv(x * x, dtype) - mu1 * mu1
    s22 = _conv(y * y, dtype) - mu2 * mu2
    s12 = _conv(x * y, dtype) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def dssim_dx(x, y, dtype=torch.float64):
    """The analytic d(sum S)/dx (V,3,H,W): G*D1 + 2 x G*D2 + y G*D3 with D1 = dS/dmu1 (total), D2 = dS/dE[xx], D3 = dS/dE[xy]."""
    x, y = x.to(dtype), y.to(dtype)
    mu1, mu2 = _conv(x, dtype), _conv(y, dtype)
    s11 = _conv(x * x, dtype) - mu1 * mu1
    s22 = _conv(y * y, dtype) - mu2 * mu2
    s12 = _conv(x * y, dtype) - mu1 * mu2
    A, B = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    C, D = mu1 * mu1 + mu2 * mu2 + C1, s11 + s22 + C2
    S = A * B / (C * D)
    D1 = 2 * mu2 * (B - A) / (C * D) - S * 2 * mu1 / C + S * 2 * mu1 / D
    D2 = -S / D
    D3 = 2 * A / (C * D)
    return _conv(D1, dtype) + 2 * x * _conv(D2, dtype) + y * _conv(D3, dtype)


def loss2d(pred, target, w_l1=0.8, w_ssim=0.2, grad_scale=1.0, loss_offset=0.0, mask=None, dtype=torch.float64):
    """What `ops.image_loss2d_grad` returns, in `dtype` on the CPU: dict(sums (3,), view_sums (V,2), grad (V,3,H,W), map)."""
    x, y = masked(pred.cpu(), target.cpu(), None if mask is None else mask.cpu(), dtype)
    S = ssim_map(x, y, dtype)
    l1_v = (x - y).abs().sum((1, 2, 3))
    ss_v = S.sum((1, 2, 3))
    l1, ss = l1_v.sum(), ss_v.sum()
    g = grad_scale * (w_l1 * torch.sign(x - y) - w_ssim * dssim_dx(x, y, dtype))
    if mask is not None:
        g = g * mask.cpu().to(dtype)[:, None]
    return dict(sums=torch.stack([l1, ss, grad_scale * (w_l1 * l1 - w_ssim * ss) + loss_offset]), view_sums=torch.stack([l1_v, ss_v], 1),
                grad=g, map=S)


def settled_blocks(pred, target, bw, bh):
    """numpy bool (V, ceil(H/bh), ceil(W/bw)): the block is settled -- pred - target == 0 in fp32, in every channel, over the
    block dilated by 10 px and clipped to the image (NaN - NaN is not 0).  pred, target: (V,3,H,W), already masked."""
    p, t = (np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float32) for a in (pred, target))
    with np.errstate(invalid="ignore"):
        same = ((p - t) == 0).all(1)
    V, H, W = same.shape
    out = np.zeros((V, (H + bh - 1) // bh, (W + bw - 1) // bw), bool)
    for v in range(V):
        for by in range(out.shape[1]):
            for bx in range(out.shape[2]):
                out[v, by, bx] = same[v, max(by * bh - 2 * R, 0):min((by + 1) * bh + 2 * R, H), max(bx * bw - 2 * R, 0):min((bx + 1) * bw + 2 * R, W)].all()
    return out


def block_mask(settled, H, W, bw, bh):
    """(V,H,W) bool: the pixel lies in a settled block."""
    return np.repeat(np.repeat(settled, bh, 1), bw, 2)[:, :H, :W]


def rel(a, r):
    """|a - r| / |r| of two numbers (absolute for r == 0)."""
    a, r = float(a), float(r)
    return abs(a - r) / abs(r) if r != 0 else abs(a - r)


def grad_rows(g):
    """(V,3,H,W) -> the (view, channel, image row) lines as the rows of `util.row_rel_err`."""
    return g.reshape(-1, g.shape[-1])


def bound(e32):
    """The project's tolerance convention: the kernel's error against the fp64 restatement is at most 8 * max(e32, 2^-23), e32
    the fp32 restatement's own error against fp64 in the same metric."""
    return 8.0 * max(float(e32), 2.0 ** -23)


def smooth_images(V, H, W, seed, diff_boxes=None):
    """A smooth random target in [0.1, 0.9] and a pred that differs from it only inside `diff_boxes` (list per view of
    (y0, y1, x0, x1); None: everywhere) by a smooth perturbation.  fp32 CPU tensors (V,3,H,W)."""
    g = torch.Generator().manual_seed(seed)
    def field():
        lo = torch.rand((V, 3, max(H // 6, 2), max(W // 6, 2)), generator=g)
        return F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True)
    tgt = (0.1 + 0.8 * field()).float()
    d = (field() - 0.5) * 0.3
    if diff_boxes is not None:
        keep = torch.zeros((V, 1, H, W))
        for v, boxes in enumerate(diff_boxes):
            for y0, y1, x0, x1 in boxes:
                keep[v, :, y0:y1, x0:x1] = 1.0
        d = d * keep
    pred = (tgt + d).clamp(0.0, 1.0).float()
    return pred.contiguous(), tgt.contiguous()


# ---------------------------------------------------------------------------
# the committed inputs of tests/test_gpu_ssim2d.py (tests/test_ssim2d_cpu.py checks the condition on them)
# ---------------------------------------------------------------------------
def sizes(bw, bh):
    """(H, W) of the GPU tests for a library whose block is bw x bh."""
    return [(5, 7), (16, 16), (bh + 1, bw + 1), (bh, bw), (33, 47), (56, 40)]


def case_boxes(V, H, W):
    """Where pred differs from target: view 0 near (0,0), view 1 near (H-1,W-1), view 2 everywhere."""
    qh, qw = H // 4 + 1, W // 4 + 1
    return [[(0, qh, 0, qw)], [(H - qh, H, W - qw, W)], [(0, H, 0, W)]][:V]


def case_images(V, H, W):
    """The (pred, target) fp32 CPU pair of the case; the seed is a function of the shape."""
    return smooth_images(V, H, W, seed=1000 * V + 37 * H + W, diff_boxes=case_boxes(V, H, W))


SETTLING_SIZES = [(33, 47), (56, 40)]      # the sizes at which the inputs must hold both a settled and a listed block

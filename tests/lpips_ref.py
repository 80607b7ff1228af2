"""Restatement of LPIPS (mgr_lpips, manus_amd/lpips.py) in plain CPU torch at a chosen dtype, for the tests.

    in = ((x * mask) [* 2 - 1] - shift) / scale;  f_k = taps of the backbone;  fh = f / (sqrt(sum_c f^2) + 1e-10)
    d = sum_k mean_hw sum_c lin_k[c] (fh0 - fh1)^2

The definition is restated from the public one (the `lpips` package, torchvision's vgg16 / alexnet): neither package nor any
weight file was available when this was written, so nothing here pins parity with the real package.

The backward takes the DECISIONS as inputs -- every ReLU mask and every pooling winner -- and returns the gradient for exactly
those decisions: a ReLU is a multiplication by its mask, a pool a gather at its winners, everything else is smooth.  A pixel
whose tap features are all zero contributes a zero gradient (autograd through sqrt gives NaN there).
"""
import math

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# ("c", Cin, Cout, K, stride, pad, tap) / ("p", K)
VGG = [("c", 3, 64, 3, 1, 1, -1), ("c", 64, 64, 3, 1, 1, 0), ("p", 2),
       ("c", 64, 128, 3, 1, 1, -1), ("c", 128, 128, 3, 1, 1, 1), ("p", 2),
       ("c", 128, 256, 3, 1, 1, -1), ("c", 256, 256, 3, 1, 1, -1), ("c", 256, 256, 3, 1, 1, 2), ("p", 2),
       ("c", 256, 512, 3, 1, 1, -1), ("c", 512, 512, 3, 1, 1, -1), ("c", 512, 512, 3, 1, 1, 3), ("p", 2),
       ("c", 512, 512, 3, 1, 1, -1), ("c", 512, 512, 3, 1, 1, -1), ("c", 512, 512, 3, 1, 1, 4)]
ALEX = [("c", 3, 64, 11, 4, 2, 0), ("p", 3), ("c", 64, 192, 5, 1, 2, 1), ("p", 3), ("c", 192, 384, 3, 1, 1, 2),
        ("c", 384, 256, 3, 1, 1, 3), ("c", 256, 256, 3, 1, 1, 4)]
OPS = {"vgg": VGG, "alex": ALEX}
CONV_INDEX = {"vgg": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28), "alex": (0, 3, 6, 8, 10)}


def make_weights(net, seed):
    """Seeded stand-in weights: randn * sqrt(2 / fan_in), randn biases, |randn| lin weights (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    w, b, lin = [], [], []
    for op in OPS[net]:
        if op[0] != "c":
            continue
        _, ci, co, k, _, _, tap = op
        w.append(torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k)))
        b.append(torch.randn(co, generator=g))
        if tap >= 0:
            lin.append(torch.randn(co, generator=g).abs())
    return {"w": w, "b": b, "lin": lin}


def state_dicts(net, wts):
    """The two state dicts a user supplies, with the keys of torchvision's checkpoint and of the lpips package's."""
    sd = {}
    for i, w, b in zip(CONV_INDEX[net], wts["w"], wts["b"]):
        sd["features.%d.weight" % i] = w
        sd["features.%d.bias" % i] = b
    return sd, {"lin%d.model.1.weight" % k: l.reshape(1, -1, 1, 1) for k, l in enumerate(wts["lin"])}


def scaled(x, mask, normalize, dtype):
    x = x.to(dtype)
    if mask is not None:
        x = x * mask.to(dtype)[None]
    if normalize:
        x = 2 * x - 1
    return (x - torch.tensor(SHIFT, dtype=dtype)[:, None, None]) / torch.tensor(SCALE, dtype=dtype)[:, None, None]


def windows2(a):
    """(C,H,W) -> (C,Ho,Wo,4): the 2x2 stride-2 windows in row-major order."""
    C, H, W = a.shape
    Ho, Wo = H // 2, W // 2
    return a[:, :2 * Ho, :2 * Wo].reshape(C, Ho, 2, Wo, 2).permute(0, 1, 3, 2, 4).reshape(C, Ho, Wo, 4)


def winners2(a):
    """First maximum of every 2x2 window in row-major order (as torch's max_pool2d)."""
    v = windows2(a)
    m, idx = v[..., 0], torch.zeros(v.shape[:-1], dtype=torch.long)
    for j in range(1, 4):
        better = v[..., j] > m
        idx = torch.where(better, torch.full_like(idx, j), idx)
        m = torch.where(better, v[..., j], m)
    return idx


def decisions_of(net, acts):
    """The decisions a set of stored post-ReLU convolution outputs (layer order) implies."""
    relu, pool, ci = [], [], 0
    for op in OPS[net]:
        if op[0] == "c":
            relu.append(acts[ci] > 0)
            ci += 1
        else:
            pool.append(winners2(acts[ci - 1]) if op[1] == 2 else None)
    return {"relu": relu, "pool": pool}


def features(net, wts, x, dtype, decisions=None):
    """x: the scaled image (3,H,W).  Returns {"pre", "act": per convolution, "tap": the five taps, "win": the windows of every
    2x2 pool}.  With decisions the ReLUs and pools are frozen to them."""
    out = {"pre": [], "act": [], "tap": [None] * 5, "win": []}
    cur, ci, pi = x.to(dtype), 0, 0
    for op in OPS[net]:
        if op[0] == "c":
            _, _, _, k, s, p, tap = op
            pre = F.conv2d(cur[None], wts["w"][ci].to(dtype), wts["b"][ci].to(dtype), stride=s, padding=p)[0]
            cur = torch.relu(pre) if decisions is None else pre * decisions["relu"][ci].to(dtype)
            out["pre"].append(pre)
            out["act"].append(cur)
            if tap >= 0:
                out["tap"][tap] = cur
            ci += 1
        else:
            k = op[1]
            if k == 2:
                v = windows2(cur)
                out["win"].append(v)
                if decisions is None:
                    cur = F.max_pool2d(cur[None], 2, 2)[0]
                else:
                    cur = torch.gather(v, -1, decisions["pool"][pi][..., None])[..., 0]
            else:
                out["win"].append(None)
                cur = F.max_pool2d(cur[None], k, 2)[0]
            pi += 1
    return out


def head(f0, f1, lin, dtype):
    """s_k of one tap; f (C,h,w)."""
    n0 = torch.sqrt((f0 * f0).sum(0, keepdim=True)) + 1e-10
    n1 = torch.sqrt((f1 * f1).sum(0, keepdim=True)) + 1e-10
    d = f0 / n0 - f1 / n1
    return (lin.to(dtype)[:, None, None] * d * d).sum(0).mean()


def head_grad(f0, f1, lin, dtype):
    """d s_k / d f0, zero at pixels whose f0 is all zero."""
    r0 = torch.sqrt((f0 * f0).sum(0, keepdim=True))
    n0 = r0 + 1e-10
    n1 = torch.sqrt((f1 * f1).sum(0, keepdim=True)) + 1e-10
    d = f0 / n0 - f1 / n1
    gu = 2 * lin.to(dtype)[:, None, None] * d / (f0.shape[1] * f0.shape[2])
    dot = (gu * f0).sum(0, keepdim=True)
    ok = r0 > 0
    safe = torch.where(ok, r0, torch.ones_like(r0))
    g = gu / n0 - dot * f0 / (n0 * n0 * safe)
    return torch.where(ok, g, torch.zeros_like(g))


def forward(net, wts, x0, x1, mask=None, normalize=False, dtype=torch.float64, decisions=None):
    """One image pair (3,H,W).  Returns (value, features of x0, features of x1); decisions freeze x0's network only."""
    a = features(net, wts, scaled(x0, mask, normalize, dtype), dtype, decisions)
    b = features(net, wts, scaled(x1, mask, normalize, dtype), dtype)
    val = sum(head(a["tap"][k], b["tap"][k], wts["lin"][k], dtype) for k in range(5))
    return val, a, b


def backward(net, wts, fa, fb, decisions, shape, mask=None, normalize=False, dtype=torch.float64):
    """d value / d x0 for the given decisions; fa / fb: `features` of the two images (their taps are used), shape = (H, W)."""
    assert net == "vgg"
    ops = OPS[net]
    n_conv = sum(1 for op in ops if op[0] == "c")
    ci, pi = n_conv, sum(1 for op in ops if op[0] == "p")
    g = None
    for op in reversed(ops):
        if op[0] == "c":
            ci -= 1
            tap = op[6]
            if tap >= 0:
                hg = head_grad(fa["tap"][tap].to(dtype), fb["tap"][tap].to(dtype), wts["lin"][tap], dtype)
                g = hg if g is None else g + hg
            g = g * decisions["relu"][ci].to(dtype)
            g = F.conv_transpose2d(g[None], wts["w"][ci].to(dtype), stride=1, padding=op[5])[0]
        else:
            pi -= 1
            idx = decisions["pool"][pi]
            C, Ho, Wo = idx.shape
            src = fa["act"][ci - 1]
            full = torch.zeros((C, Ho, Wo, 4), dtype=dtype).scatter_(-1, idx[..., None], g[..., None])
            gi = torch.zeros((C,) + tuple(src.shape[1:]), dtype=dtype)
            gi[:, :2 * Ho, :2 * Wo] = full.reshape(C, Ho, Wo, 2, 2).permute(0, 1, 3, 2, 4).reshape(C, 2 * Ho, 2 * Wo)
            g = gi
    g = g / torch.tensor(SCALE, dtype=dtype)[:, None, None]
    if normalize:
        g = g * 2
    if mask is not None:
        g = g * mask.to(dtype)[None]
    return g


def rel_err(a, r):
    """max|a - r| / max|r| of two tensors."""
    a, r = a.double(), r.double()
    den = float(r.abs().max())
    return float((a - r).abs().max()) / (den if den > 0 else 1.0)


def compare_decisions(net, dev, f64, f32):
    """Device decisions against the fp64 restatement's own.  Returns per layer (kind, index, n, differing, not at a threshold):
    a differing decision is 'at a threshold' if its fp64 margin (|pre-activation| of a ReLU, the gap between the two largest
    window values of a pool) is within 16x the layer's measured max |fp32 - fp64| pre-activation difference."""
    own = decisions_of(net, f64["act"])
    rows = []
    ci = pi = 0
    for op in OPS[net]:
        if op[0] == "c":
            tol = 16 * float((f32["pre"][ci].double() - f64["pre"][ci]).abs().max())
            diff = dev["relu"][ci] != own["relu"][ci]
            margin = f64["pre"][ci].abs()
            rows.append(("relu", ci, diff.numel(), int(diff.sum()), int((diff & (margin > tol)).sum())))
            ci += 1
        else:
            if op[1] == 2:
                tol = 16 * float((f32["pre"][ci - 1].double() - f64["pre"][ci - 1]).abs().max())
                diff = dev["pool"][pi] != own["pool"][pi]
                top = torch.topk(f64["win"][pi], 2, dim=-1).values
                margin = top[..., 0] - top[..., 1]
                rows.append(("pool", pi, diff.numel(), int(diff.sum()), int((diff & (margin > tol)).sum())))
            pi += 1
    return rows


# (W, H, seed) of the gradient tests: tests/test_lpips_cpu.py asserts that the caps of the decision comparison hold at these
# seeds for the fp32 restatement against fp64
GRAD_CASES = ((40, 24, 1), (33, 17, 2))


def images(seed, V, H, W):
    """pred, target (V,3,H,W) in [0,1] and a fractional mask (V,H,W) with zeros, ones and fractions."""
    g = torch.Generator().manual_seed(1000 + seed)
    pred, target = torch.rand((V, 3, H, W), generator=g), torch.rand((V, 3, H, W), generator=g)
    mask = (torch.rand((V, H, W), generator=g) * 3 - 1).clamp(0, 1)
    return pred, target, mask

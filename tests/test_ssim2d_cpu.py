"""CPU: the restatement of the spatial image loss (tests/ssim2d_ref.py) against autograd and central differences, the
settled-block rule, the C surface of mgr_image_loss2d (symbols, signatures, block word, workspace size, every refusal that
is decided before the device), the new ABI constant, the condition on the inputs of tests/test_gpu_ssim2d.py, and the
ValueErrors of the `ssim=` keywords.  With tests/golden/ssim2d.npz: the restatement against the reference's own ssim() on
CHW images.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ssim2d_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_image_loss2d_workspace_bytes": 3, "mgr_image_loss2d_block": 0, "mgr_image_loss2d": 17}
WANT = dict(MGR_IL2D_DENSE=1)      # the table of tests/test_abi_constants.py for the flags of mgr_image_loss2d


def _pair(H=24, W=30, V=2, seed=3):
    pred, tgt = R.smooth_images(V, H, W, seed)
    return pred.double(), tgt.double()


def test_analytic_gradient_equals_autograd_and_central_differences():
    x, y = _pair()
    x = x.clone().requires_grad_(True)
    (g_auto,) = torch.autograd.grad(R.ssim_map(x, y).sum(), x)
    g = R.dssim_dx(x.detach(), y)
    e = float((g - g_auto).abs().max())
    print("analytic against fp64 autograd: %.3g" % e)
    assert e <= 1e-11
    x0 = x.detach()
    gen = torch.Generator().manual_seed(0)
    h = 1e-6
    for _ in range(12):
        v, c = int(torch.randint(0, x0.shape[0], (1,), generator=gen)), int(torch.randint(0, 3, (1,), generator=gen))
        i, j = (int(torch.randint(0, n, (1,), generator=gen)) for n in x0.shape[2:])
        if _ < 4:       # the four corners too
            i, j = (0, x0.shape[2] - 1)[_ & 1], (0, x0.shape[3] - 1)[_ >> 1]
        xp, xm = x0.clone(), x0.clone()
        xp[v, c, i, j] += h
        xm[v, c, i, j] -= h
        fd = float(R.ssim_map(xp, y).sum() - R.ssim_map(xm, y).sum()) / (2 * h)
        assert abs(fd - float(g[v, c, i, j])) <= 1e-6 * max(1.0, abs(fd)), (v, c, i, j, fd, float(g[v, c, i, j]))
    # the whole loss: value and gradient of loss2d against autograd of its own value
    m = (torch.rand((2, 24, 30), generator=gen) * 3 - 1).clamp(0, 1).double()
    xr = x0.clone().requires_grad_(True)
    xm_, ym_ = R.masked(xr, y, m, torch.float64)
    val = 0.37 * (0.8 * (xm_ - ym_).abs().sum() - 0.2 * R.ssim_map(xm_, ym_).sum()) + 0.5
    (g_auto,) = torch.autograd.grad(val, xr)
    out = R.loss2d(x0, y, 0.8, 0.2, 0.37, 0.5, mask=m)
    val = val.detach()
    assert abs(float(out["sums"][2]) - float(val)) <= 1e-12 * abs(float(val))
    assert float((out["grad"] - g_auto).abs().max()) <= 1e-12


def test_far_from_any_difference_the_map_is_one_and_the_gradient_zero():
    """What justifies the settled rule: beyond 5 px of a difference S is 1, beyond 10 px the gradient is 0."""
    H, W = 40, 56
    _, tgt = R.smooth_images(1, H, W, 9)
    pred = tgt.clone()
    pred[0, :, 17:23, 25:31] += 0.2
    S, g = R.ssim_map(pred, tgt), R.dssim_dx(pred, tgt)
    far5 = torch.ones((H, W), dtype=torch.bool)
    far5[17 - 5:23 + 5, 25 - 5:31 + 5] = False
    far10 = torch.ones((H, W), dtype=torch.bool)
    far10[17 - 10:23 + 10, 25 - 10:31 + 10] = False
    eS, eg = float((S[0][:, far5] - 1).abs().max()), float(g[0][:, far10].abs().max())
    print("|S - 1| beyond 5 px %.3g, |dS/dx| beyond 10 px %.3g" % (eS, eg))
    assert eS <= 1e-12 and eg <= 1e-12
    # ... and one pixel closer the gradient is not zero: 10 px is exact
    near = torch.zeros((H, W), dtype=torch.bool)
    near[17 - 10:23 + 10, 25 - 10:31 + 10] = True
    near[17 - 9:23 + 9, 25 - 9:31 + 9] = False
    assert float(g[0][:, near].abs().max()) > 1e-9
    # settled_blocks is that rule
    st = R.settled_blocks(pred, tgt, 32, 16)
    assert st.shape == (1, 3, 2)
    assert not st[0, 1, 0] and not st[0, 1, 1] and not st[0, 0, 0]      # rows 7..33 and columns 15..41 reach them
    assert st[0, 2].tolist() == [False, False]                             # block rows 32..39 dilated reach row 22
    pred2 = tgt.clone()
    pred2[0, 0, 0, 0] += 0.1
    st = R.settled_blocks(pred2, tgt, 32, 16)
    assert st[0].tolist() == [[False, True], [True, True], [True, True]]      # block row 1 dilated starts at row 6
    nan = tgt.clone()
    nan[0, 1, 39, 55] = float("nan")
    assert R.settled_blocks(nan, nan, 32, 16)[0].tolist() == [[True, True], [True, False], [True, False]]


def test_spatial_differs_from_rows_on_a_vertical_blur():
    """A pair that differs only by a vertical blur: the rows variant (the window never spans two image rows) and the spatial
    one disagree.  Recorded on this seed: rows 0.96727 -- it hardly
    sees the blur -- spatial 0.78893."""
    _, tgt = R.smooth_images(1, 40, 56, 21)
    tgt = (0.5 * tgt + 0.5 * torch.rand(tgt.shape, generator=torch.Generator().manual_seed(2))).double()
    k = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64).reshape(1, 1, 3, 1).expand(3, 1, 3, 1)
    pred = torch.nn.functional.conv2d(torch.nn.functional.pad(tgt, (0, 0, 1, 1), mode="replicate"), k, groups=3)
    spatial = float(R.ssim_map(pred, tgt).mean())
    # the rows variant, restated: ssim() on HWC images = the window over the (W,3) plane of every image row
    g2 = R.window2d(torch.float64)

    def conv_rows(a):      # a (H,W,3): H groups
        return torch.nn.functional.conv2d(a[None], g2.expand(a.shape[0], 1, 11, 11).contiguous(), padding=5, groups=a.shape[0])[0]

    a, b = pred[0].permute(1, 2, 0), tgt[0].permute(1, 2, 0)
    mu1, mu2 = conv_rows(a), conv_rows(b)
    s11, s22, s12 = conv_rows(a * a) - mu1 * mu1, conv_rows(b * b) - mu2 * mu2, conv_rows(a * b) - mu1 * mu2
    rows = float((((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 * mu1 + mu2 * mu2 + R.C1) * (s11 + s22 + R.C2))).mean())
    print("vertical blur: rows %.5f spatial %.5f" % (rows, spatial))
    assert abs(rows - spatial) > 1e-3
    assert abs(rows - 0.96727) <= 5e-5 and abs(spatial - 0.78893) <= 5e-5


def _declared_args(header, name):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, "include/manus_hip.h does not declare " + name
    args = [a.strip() for a in m.group(1).split(",")]
    return [] if args == ["void"] else args


def test_symbols_and_signatures():
    from manus_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in NEW_ENTRIES.items():
        assert len(_declared_args(header, name)) == arity, name
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, bound = _lib.SIGNATURES[name]
        assert len(bound) == arity and res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int), name
        assert hasattr(so, name), "%s is not exported by the built library" % name
    args = _declared_args(header, "mgr_image_loss2d")
    assert args[:6] == ["int V", "int H", "int W", "const float* pred", "const float* target", "const float* mask"]
    assert args[6:10] == ["float w_l1", "float w_ssim", "float grad_scale", "float loss_offset"]
    assert args[10:] == ["float* dL_dpred", "float* sums", "float* view_sums", "int flags", "void* workspace", "size_t workspace_bytes", "void* stream"]
    bound = _lib.SIGNATURES["mgr_image_loss2d"][1]
    assert bound[6:10] == [ctypes.c_float] * 4 and bound[13] is ctypes.c_int and bound[15] is ctypes.c_size_t
    assert "ssim2d.hip" in build.SOURCES


def test_the_new_constant():
    from manus_amd import _lib
    import test_abi_constants as A
    hdr = A._header_values(os.path.join(ROOT, "include", "manus_hip.h"))
    for name, value in WANT.items():
        assert hdr.get(name) == value, (name, hdr.get(name))
        assert getattr(_lib, name) == value, name
    assert {n for n in hdr if n.startswith("MGR_IL2D_")} == set(WANT) == {n for n in vars(_lib) if n.startswith("MGR_IL2D_")}


def test_block_word_and_workspace_bytes():
    from manus_amd import _lib, ops
    L = _lib.lib()
    word = L.mgr_image_loss2d_block()
    bw, bh = word >> 16, word & 0xFFFF
    assert (bw, bh) == ops.image_loss2d_block()
    assert 8 <= bw <= 256 and 8 <= bh <= 256 and bw % 2 == 0
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -3, 4), (4, 4, -2)):
        assert L.mgr_image_loss2d_workspace_bytes(*bad) == 0, bad
    sizes = [L.mgr_image_loss2d_workspace_bytes(V, 1080, 1920) for V in (1, 2, 8)]
    assert 0 < sizes[0] < sizes[1] < sizes[2]
    # no per-pixel floats: a bit per pixel, a word per block and the sum slots -- well under a byte per pixel
    assert sizes[2] < 8 * 1080 * 1920
    assert L.mgr_image_loss2d_workspace_bytes(1, 5, 7) > 0


P = ctypes.c_void_p(0x1000)          # a fake pointer: a refusal never dereferences it


def test_refusals_decided_before_the_device():
    from manus_amd import _lib
    L = _lib.lib()
    big = 1 << 30

    def run(V=2, H=20, W=30, pred=P, target=P, mask=None, grad=P, sums=P, vs=P, flags=0, ws=P, nbytes=big):
        return L.mgr_image_loss2d(V, H, W, pred, target, mask, 0.8, 0.2, 1.0, 0.0, grad, sums, vs, flags, ws, nbytes, None)

    for kw in (dict(V=0), dict(H=0), dict(W=0), dict(V=-1), dict(H=-5), dict(W=-1)):
        assert run(**kw) == _lib.MGR_EINVAL, kw
        assert b"sizes" in L.mgr_last_error()
    for kw in (dict(pred=None), dict(target=None), dict(sums=None), dict(ws=None)):
        assert run(**kw) == _lib.MGR_EINVAL, kw
        assert b"null" in L.mgr_last_error()
    for kw in (dict(H=65536), dict(V=65536)):
        assert run(**kw) == _lib.MGR_EINVAL, kw
        assert b"grid" in L.mgr_last_error()
    assert run(H=40000, W=40000) == _lib.MGR_EINVAL                     # 3 H W beyond the fixed-point range of a view's sums
    assert run(flags=2) == _lib.MGR_EINVAL and b"flag" in L.mgr_last_error()
    need = L.mgr_image_loss2d_workspace_bytes(2, 20, 30)
    assert run(nbytes=need - 1) == _lib.MGR_ENOMEM and b"workspace" in L.mgr_last_error()
    assert run(nbytes=0) == _lib.MGR_ENOMEM


def test_gpu_test_inputs_hold_settled_and_listed_blocks():
    """A condition on the committed inputs of tests/test_gpu_ssim2d.py, for the library's block size."""
    from manus_amd import ops
    bw, bh = ops.image_loss2d_block()
    assert set(R.SETTLING_SIZES) <= set(R.sizes(bw, bh))
    for H, W in R.SETTLING_SIZES:
        for V in (1, 3):
            pred, tgt = R.case_images(V, H, W)
            st = R.settled_blocks(pred, tgt, bw, bh)
            assert st.any() and not st.all(), (V, H, W, st.tolist())
            assert st[0].any() and not st[0].all()                      # in one view
            if V == 3:
                assert not st[2].any()                                  # the view that differs everywhere
    # every case differs somewhere, and the mask of the mask test holds 0, 1 and fractions at every size
    for H, W in R.sizes(bw, bh):
        for V in (1, 3):
            pred, tgt = R.case_images(V, H, W)
            assert all(bool((pred[v] != tgt[v]).any()) for v in range(V)), (V, H, W)
            m = (torch.rand((V, H, W), generator=torch.Generator().manual_seed(5)) * 3 - 1).clamp(0, 1)
            assert ((m > 0) & (m < 1)).any() and (m == 0).any() and (m == 1).any()


def test_value_errors_of_the_ssim_keywords():
    from manus_amd import losses, validation
    from manus_amd.engine import HipViewCompute, Trainer
    for bad in ("columns", None, "Spatial", 2):
        with pytest.raises(ValueError, match="ssim must be"):
            HipViewCompute(None, None, None, ssim=bad)
        with pytest.raises(ValueError, match="ssim must be"):
            Trainer.validate(None, [0], ssim=bad)
        with pytest.raises(ValueError, match="ssim must be"):
            validation.validation_step(None, {}, ssim=bad)
        with pytest.raises(ValueError, match="ssim must be"):
            losses.rgb_ssim_loss(None, None, ssim=bad)
    # the attribute is asked again at the step
    hc = HipViewCompute.__new__(HipViewCompute)
    hc.ssim = "rows"
    assert hc._ssim_mode() == "rows"
    hc.ssim = "spatial"
    assert hc._ssim_mode() == "spatial"
    hc.ssim = "both"
    with pytest.raises(ValueError, match="ssim must be"):
        hc._ssim_mode()


def test_restatement_against_the_reference_on_chw_images(golden_dir):
    """tests/golden/ssim2d.npz (tests/golden/make_ssim2d_golden.py): the reference's ssim() on two CHW pairs."""
    z = np.load(os.path.join(golden_dir, "ssim2d.npz"))
    for k in range(int(z["n_pairs"])):
        a, b = torch.from_numpy(z["img1_%d" % k]), torch.from_numpy(z["img2_%d" % k])
        want = float(z["ssim_%d" % k])
        got32 = float(R.ssim_map(a[None], b[None], torch.float32).mean())
        got64 = float(R.ssim_map(a[None], b[None], torch.float64).mean())
        print("pair %d: reference %.9g, restatement fp32 %.9g, fp64 %.9g" % (k, want, got32, got64))
        assert abs(got32 - want) <= 2e-6 and abs(got64 - want) <= 2e-5

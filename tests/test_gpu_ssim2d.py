"""GPU: the spatial image loss `ops.image_loss2d_grad` (mgr_image_loss2d, csrc/ssim2d.hip) against the fp64 restatement of
tests/ssim2d_ref.py, and the exact properties of its settled blocks, sums and mask.

Tolerance: the project's convention (ssim2d_ref.bound) -- the kernel's error against fp64 is at most 8 * max(e32, 2^-23), e32
the fp32 restatement's own error against fp64 in the same metric.  The gradient is judged with `row_rel_err` over the (view,
channel, image row) lines.  Every figure is printed before it is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ssim2d_ref as R
from util import row_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
W_L1, W_SSIM = 0.8, 0.2


@functools.lru_cache(maxsize=None)
def block():
    from manus_amd import ops
    return ops.image_loss2d_block()


SIZE_KEYS = ["5x7", "16x16", "block+1", "block", "33x47", "56x40"]      # ssim2d_ref.sizes, named without asking the library


def resolve(shape):
    """(V, size key) -> (V, H, W): the two block-sized cases take the library's block when the test runs."""
    V, key = shape
    H, W = dict(zip(SIZE_KEYS, R.sizes(*block())))[key]
    return V, H, W


@functools.lru_cache(maxsize=None)
def case(V, H, W):
    """(pred, target) on the device and the fp64 / fp32 restatements of the standard call, computed once."""
    pred, tgt = R.case_images(V, H, W)
    kw = dict(w_l1=W_L1, w_ssim=W_SSIM, grad_scale=1.0 / (3 * H * W), loss_offset=W_SSIM * V)
    return pred.to(DEV), tgt.to(DEV), R.loss2d(pred, tgt, dtype=torch.float64, **kw), R.loss2d(pred, tgt, dtype=torch.float32, **kw), kw


def call(pred, tgt, kw, **more):
    from manus_amd import ops
    return ops.image_loss2d_grad(pred, tgt, kw["w_l1"], kw["w_ssim"], kw["grad_scale"], kw["loss_offset"], **more)


def judge(name, got, r64, r32, kw):
    """sums, view_sums and gradient of `got` against the fp64 restatement, each within the bound of the fp32 one.

    sums[2] = grad_scale (w_l1 sums[0] - w_ssim sums[1]) + loss_offset is a difference of nearly equal terms (w_ssim * mean S
    against the offset w_ssim of "1 - ssim"), so its own relative error says nothing: it is judged in absolute terms against
    what the bounds of sums[0] and sums[1] allow it, grad_scale (w_l1 b0 |sums[0]| + w_ssim b1 |sums[1]|), plus one fp32
    rounding of the result."""
    sums, view_sums, g = got
    worst, b = [], []
    for k in range(2):
        e, e32 = R.rel(sums[k], r64["sums"][k]), R.rel(r32["sums"][k], r64["sums"][k])
        print("%s sums[%d] err %.3g  e32 %.3g  bound %.3g" % (name, k, e, e32, R.bound(e32)))
        worst.append((e, R.bound(e32)))
        b.append(R.bound(e32) * abs(float(r64["sums"][k])))
    e = abs(float(sums[2]) - float(r64["sums"][2]))
    allowed = kw["grad_scale"] * (kw["w_l1"] * b[0] + kw["w_ssim"] * b[1]) + 2.0 ** -24 * abs(float(r64["sums"][2]))
    print("%s sums[2] %.9g abs err %.3g  allowed %.3g" % (name, float(sums[2]), e, allowed))
    worst.append((e, allowed))
    vs, v64, v32 = view_sums.cpu().double(), r64["view_sums"], r32["view_sums"].double()
    for k in range(2):
        e = max(R.rel(a, b) for a, b in zip(vs[:, k], v64[:, k]))
        e32 = max(R.rel(a, b) for a, b in zip(v32[:, k], v64[:, k]))
        print("%s view_sums[:,%d] err %.3g  e32 %.3g  bound %.3g" % (name, k, e, e32, R.bound(e32)))
        worst.append((e, R.bound(e32)))
    if g is not None:
        e, e32 = row_rel_err(R.grad_rows(g), R.grad_rows(r64["grad"])), row_rel_err(R.grad_rows(r32["grad"]), R.grad_rows(r64["grad"]))
        print("%s gradient row_rel_err %.3g  e32 %.3g  bound %.3g" % (name, e, e32, R.bound(e32)))
        worst.append((e, R.bound(e32)))
    for e, b in worst:
        assert e <= b, (name, e, b)


def pytest_generate_tests(metafunc):
    if "shape" in metafunc.fixturenames:
        metafunc.parametrize("shape", [(V, key) for key in SIZE_KEYS for V in (1, 3)], ids=lambda s: "V%d_%s" % s)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "settling"])
def test_against_the_fp64_restatement(shape, dense):
    shape = resolve(shape)
    pred, tgt, r64, r32, kw = case(*shape)
    judge("V%d %dx%d %s" % (shape + ("dense" if dense else "settling",)), call(pred, tgt, kw, dense=dense), r64, r32, kw)


def test_more_blocks_than_persistent_workgroups():
    """825 blocks against 768 resident workgroups: the kernel's loop over the list takes a second turn."""
    V, H, W = 1, 25 * block()[1], 33 * block()[0]
    pred, tgt, r64, r32, kw = case(V, H, W)
    judge("V1 %dx%d dense" % (H, W), call(pred, tgt, kw, dense=True), r64, r32, kw)


def test_settled_blocks_have_zero_gradient_and_count_in_full(shape):
    shape = resolve(shape)
    V, H, W = shape
    pred, tgt, r64, r32, kw = case(*shape)
    bw, bh = block()
    settled = R.block_mask(R.settled_blocks(pred.cpu(), tgt.cpu(), bw, bh), H, W, bw, bh)
    s_d, _, g_d = call(pred, tgt, kw, dense=True)
    s_s, _, g_s = call(pred, tgt, kw)
    m = torch.from_numpy(settled).to(DEV)[:, None].expand_as(g_s)
    print("settled pixels %d of %d; dense |g| there at most %.3g" % (int(settled.sum()), settled.size, float(g_d[m].abs().max()) if m.any() else 0.0))
    assert (g_s[m] == 0).all()
    assert torch.equal(g_s[~m], g_d[~m])          # a listed block computes what the dense call computes
    e, e32 = R.rel(s_s[1], s_d[1]), R.rel(r32["sums"][1], r64["sums"][1])
    print("sum S settling %.9g dense %.9g: %.3g, bound %.3g" % (float(s_s[1]), float(s_d[1]), e, R.bound(e32)))
    assert e <= R.bound(e32)
    assert torch.equal(s_s[0], s_d[0])            # a settled block's L1 sum is exactly 0 either way


@pytest.mark.parametrize("corner", ["first", "last"])
@pytest.mark.parametrize("size", [(5, 7), (33, 47), (56, 40)], ids=lambda s: "%dx%d" % s)
def test_a_difference_confined_to_a_corner_pixel(size, corner):
    H, W = size
    _, tgt = R.case_images(1, H, W)
    pred = tgt.clone()
    y, x = (0, 0) if corner == "first" else (H - 1, W - 1)
    pred[0, :, y, x] += 0.25
    kw = dict(w_l1=W_L1, w_ssim=W_SSIM, grad_scale=1.0 / (3 * H * W), loss_offset=W_SSIM)
    r64, r32 = R.loss2d(pred, tgt, dtype=torch.float64, **kw), R.loss2d(pred, tgt, dtype=torch.float32, **kw)
    for dense in (True, False):
        judge("%dx%d pixel (%d,%d) %s" % (H, W, y, x, "dense" if dense else "settling"), call(pred.to(DEV), tgt.to(DEV), kw, dense=dense), r64, r32, kw)


def test_equal_images(shape):
    shape = resolve(shape)
    V, H, W = shape
    _, tgt, _, _, kw = case(*shape)
    sums, view_sums, g = call(tgt.clone(), tgt, kw)
    assert float(sums[0]) == 0.0 and float(sums[1]) == float(3 * H * W * V)
    assert (view_sums[:, 0] == 0).all() and (view_sums[:, 1] == float(3 * H * W)).all()
    assert (g == 0).all()


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "settling"])
def test_forward_only_gives_the_same_sums(shape, dense):
    shape = resolve(shape)
    pred, tgt, _, _, kw = case(*shape)
    s1, v1, g1 = call(pred, tgt, kw, dense=dense)
    s0, v0, g0 = call(pred, tgt, kw, dense=dense, need_grad=False)
    assert g0 is None and g1 is not None
    assert torch.equal(s0, s1) and torch.equal(v0, v1)


def test_fractional_mask_is_premultiplication(shape):
    shape = resolve(shape)
    V, H, W = shape
    pred, tgt, _, _, kw = case(*shape)
    g = torch.Generator().manual_seed(5)
    m = (torch.rand((V, H, W), generator=g) * 3 - 1).clamp(0, 1).to(DEV)
    assert ((m > 0) & (m < 1)).any() and (m == 0).any() and (m == 1).any()
    for dense in (True, False):
        s_m, v_m, g_m = call(pred, tgt, kw, mask=m, dense=dense)
        s_p, v_p, g_p = call(pred * m[:, None], tgt * m[:, None], kw, dense=dense)
        assert torch.equal(s_m, s_p) and torch.equal(v_m, v_p)
        assert torch.equal(g_m, m[:, None] * g_p)
    s_f, v_f, _ = call(pred, tgt, kw, mask=m, need_grad=False)
    assert torch.equal(s_f, s_m) and torch.equal(v_f, v_m)


@pytest.mark.parametrize("size", [(33, 47), (56, 40)], ids=lambda s: "%dx%d" % s)
def test_three_views_are_three_calls_of_one_view(size):
    H, W = size
    pred, tgt, _, _, kw = case(3, H, W)
    for dense in (True, False):
        _, v3, g3 = call(pred, tgt, kw, dense=dense)
        for v in range(3):
            _, v1, g1 = call(pred[v:v + 1].contiguous(), tgt[v:v + 1].contiguous(), kw, dense=dense)
            assert torch.equal(v1[0], v3[v]) and torch.equal(g1[0], g3[v]), (dense, v)


def test_two_runs_give_equal_bits(shape):
    shape = resolve(shape)
    pred, tgt, _, _, kw = case(*shape)
    a, b = call(pred, tgt, kw), call(pred, tgt, kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = call(pred, tgt, kw, dense=True), call(pred, tgt, kw, dense=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("size", [(33, 47), (56, 40)], ids=lambda s: "%dx%d" % s)
def test_a_nan_stays_in_its_view(size):
    H, W = size
    pred, tgt, _, _, kw = case(3, H, W)
    _, clean, _ = call(pred, tgt, kw)
    for where in ("pred", "target"):
        p, t = pred.clone(), tgt.clone()
        (p if where == "pred" else t)[1, 1, H // 2, W // 2] = float("nan")
        for dense in (True, False):
            sums, vs, _ = call(p, t, kw, dense=dense)
            assert torch.isnan(sums).all() and torch.isnan(vs[1]).all(), (where, dense)
            if not dense:
                assert torch.equal(vs[0], clean[0]) and torch.equal(vs[2], clean[2]), where
            else:
                assert torch.isfinite(vs[0]).all() and torch.isfinite(vs[2]).all()
    # equal NaNs are not equal pixels: the block is listed, not settled
    p = tgt.clone()
    p[1, 0, 3, 3] = float("nan")
    t = p.clone()
    sums, vs, _ = call(p, t, kw)
    assert torch.isnan(vs[1]).all() and float(vs[0, 1]) == float(3 * H * W)


def test_short_workspace_is_refused_with_nothing_touched():
    from manus_amd import _lib
    V, H, W = 3, 33, 47
    pred, tgt, _, _, kw = case(V, H, W)
    L = _lib.lib()
    nbytes = int(L.mgr_image_loss2d_workspace_bytes(V, H, W))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    nan = float("nan")
    sums, vs, g = torch.full((3,), nan, device=DEV), torch.full((V, 2), nan, device=DEV), torch.full_like(pred, nan)
    rc = L.mgr_image_loss2d(V, H, W, _lib.ptr(pred), _lib.ptr(tgt), None, W_L1, W_SSIM, 1.0, 0.0, _lib.ptr(g), _lib.ptr(sums), _lib.ptr(vs), 0,
                            _lib.ptr(ws), nbytes - 1, _lib.stream())
    torch.cuda.synchronize()
    assert rc == _lib.MGR_ENOMEM and b"workspace" in L.mgr_last_error()
    assert torch.isnan(sums).all() and torch.isnan(vs).all() and torch.isnan(g).all() and not ws.any()
    rc = L.mgr_image_loss2d(V, H, W, _lib.ptr(pred), _lib.ptr(tgt), None, W_L1, W_SSIM, 1.0, 0.0, _lib.ptr(g), _lib.ptr(sums), _lib.ptr(vs), 0,
                            _lib.ptr(ws), nbytes, _lib.stream())
    assert rc == 0 and torch.isfinite(sums).all() and torch.isfinite(g).all()


def test_ssim_chw_under_autograd(shape):
    shape = resolve(shape)
    from manus_amd import losses, ops
    V, H, W = shape
    pred, tgt, r64, _, _ = case(*shape)
    x = pred.clone().requires_grad_(True)
    val = losses.ssim_chw(x, tgt)
    (g,) = torch.autograd.grad(val, x)
    val = val.detach()
    n = 3 * H * W * V
    sums, _, g_op = ops.image_loss2d_grad(pred, tgt, 0.0, 1.0, 1.0 / n)
    assert torch.equal(g, -g_op)
    assert abs(float(val) - float(sums[1]) / n) <= 1e-6 * abs(float(val))
    assert abs(float(val) - float(r64["sums"][1]) / n) <= 1e-5
    if V == 1:      # a single (3,H,W) image, and no graph when nothing asks for a gradient
        v1 = losses.ssim_chw(pred[0], tgt[0])
        assert not v1.requires_grad and torch.equal(v1, val)


def test_rgb_ssim_loss_spatial_on_hwc_images():
    from manus_amd import losses, ops
    H, W = 33, 47
    pred, tgt, _, _, _ = case(1, H, W)
    x = pred[0].permute(1, 2, 0).contiguous().requires_grad_(True)
    gt = tgt.permute(0, 2, 3, 1).contiguous()                      # (1,H,W,3) like the reference's batch
    loss = losses.rgb_ssim_loss(x, gt, 0.8, 0.2, ssim="spatial")
    loss.backward()
    loss = loss.detach()
    sums, _, g = ops.image_loss2d_grad(pred, tgt, 0.8, 0.2, 1.0 / (3 * H * W), 0.2)
    # loss = fp32(-0.2 mean S + 0.8 mean|d|) + fp32(0.2), the op adds the offset in double: three fp32 roundings near 0.2
    assert abs(float(loss) - float(sums[2])) <= 3 * 2.0 ** -24 * 0.2
    assert torch.equal(x.grad, g[0].permute(1, 2, 0))
    rows = losses.rgb_ssim_loss(x.detach(), gt, 0.8, 0.2)
    assert torch.equal(rows, losses.rgb_ssim_loss(x.detach(), gt, 0.8, 0.2, ssim="rows")) and float(rows) != float(loss)
    with pytest.raises(ValueError):
        losses.rgb_ssim_loss(x, gt, ssim="columns")

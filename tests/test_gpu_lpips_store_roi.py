"""GPU: windows, cached taps and batches in the bf16 storage mode of LPIPS (mgr_lpips_roi_batch_st, mgr_lpips_roi_taps_batch_st;
`LPIPS(operands="bf16", storage="bf16")`).

The windowed distance is DEFINED as the plain call on contiguous crops and the batched call as the sequential one, so every
check here is `torch.equal`.  Stand-in weights of seed 0; the frame is 56x40 (AlexNet: 80x48).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FW, FH = 56, 40
RECTS = [(5, 3, 33, 17), (16, 24, 40, 16), (0, 0, 56, 40), (7, 9, 16, 16)]      # odd offset; right and bottom borders; frame; minimum


@functools.lru_cache(maxsize=None)
def model(net, storage="bf16"):
    from manus_amd.lpips import LPIPS
    wts = R.make_weights(net, 0)
    return LPIPS.from_state_dicts(*R.state_dicts(net, wts), net=net, operands="bf16", storage=storage), wts


@functools.lru_cache(maxsize=None)
def frames(seed=21, V=1, H=FH, W=FW):
    return tuple(x.to(DEV) for x in R.images(seed, V, H, W))


def crop(t, r):
    x0, y0, w, h = r
    return t[..., y0:y0 + h, x0:x0 + w].contiguous()


def inside(r, H=FH, W=FW):
    m = torch.zeros((H, W), dtype=torch.bool, device=DEV)
    x0, y0, w, h = r
    m[y0:y0 + h, x0:x0 + w] = True
    return m


@pytest.mark.parametrize("rect", RECTS)
def test_window_is_the_call_on_crops(rect):
    m, _ = model("vgg")
    pred, target, mask = frames()
    vals, g = m.values_grad(pred, target, need_grad=True, grad_scale=0.7, rects=[rect])
    vals, g = vals.clone(), g.clone()
    cv, cg = m.values_grad(crop(pred, rect), crop(target, rect), need_grad=True, grad_scale=0.7)
    assert float(cv[0]) > 0
    assert torch.equal(vals, cv) and torch.equal(crop(g, rect), cg)
    if rect == (0, 0, FW, FH):
        pv, pg = m.values_grad(pred, target, need_grad=True, grad_scale=0.7)
        assert torch.equal(vals, pv) and torch.equal(g, pg)
    vf, gf = m.values_grad(pred, target, need_grad=False, rects=[rect])
    assert gf is None and torch.equal(vf, vals)
    v2, g2 = m.values_grad(pred, target, need_grad=True, grad_scale=0.7, rects=[rect])
    assert torch.equal(v2, vals) and torch.equal(g2, g)
    # the mode is in use
    vo, _ = model("vgg", "fp32")[0].values_grad(pred, target, need_grad=False, rects=[rect])
    assert not torch.equal(vo, vals)
    # masked and normalized, written and accumulated
    for accumulate in (False, True):
        prior = torch.randn(pred.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
        buf = prior.clone()
        vm, _ = m.values_grad(pred, target, mask, normalize=True, need_grad=True, rects=[rect], out_grad=buf, accumulate=accumulate)
        vm = vm.clone()
        cv, cg = m.values_grad(crop(pred, rect), crop(target, rect), crop(mask, rect), normalize=True, need_grad=True)
        assert torch.equal(vm, cv)
        assert torch.equal(crop(buf, rect), crop(prior, rect) + cg if accumulate else cg)


@pytest.mark.parametrize("rect", RECTS[:2])
def test_outside_the_window(rect):
    m, _ = model("vgg")
    pred, target, _ = frames()
    ins = inside(rect)
    buf = torch.full_like(pred, float("nan"))
    m.values_grad(pred, target, need_grad=True, rects=[rect], out_grad=buf, accumulate=False)
    assert bool((buf[0][:, ~ins] == 0).all())
    assert bool(torch.isfinite(buf[0][:, ins]).all()) and bool((buf[0][:, ins] != 0).any())
    prior = torch.randn(pred.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    buf = prior.clone()
    m.values_grad(pred, target, need_grad=True, grad_scale=1.5, rects=[rect], out_grad=buf, accumulate=True)
    _, cg = m.values_grad(crop(pred, rect), crop(target, rect), need_grad=True, grad_scale=1.5)
    assert torch.equal(buf[0][:, ~ins], prior[0][:, ~ins])
    assert torch.equal(crop(buf, rect), crop(prior, rect) + cg)


def test_cached_taps():
    from manus_amd._lib import ManusHipError, lib
    m, _ = model("vgg")
    pred, target, mask = frames(22, 3)
    rects = [(5, 3, 33, 17), (0, 0, 0, 0), (30, 2, 21, 38)]
    for mk, normalize in ((None, False), (mask, True)):
        v0, g0 = m.values_grad(pred, target, mk, normalize=normalize, need_grad=True, grad_scale=0.3, rects=rects)
        v0, g0 = v0.clone(), g0.clone()
        taps = m.target_taps(target, rects, mk, normalize)
        assert taps.storage == "bf16" and taps.bufs[1] is None
        assert taps.bufs[0].numel() == lib().mgr_lpips_taps_bytes_st(0, 17, 33, 1) < lib().mgr_lpips_taps_bytes(0, 17, 33)
        for tgt in (target, None):
            v1, g1 = m.values_grad(pred, tgt, mk, normalize=normalize, need_grad=True, grad_scale=0.3, rects=rects, target_taps=taps)
            assert torch.equal(v1, v0) and torch.equal(g1, g0), (normalize, tgt is None)
        v2, _ = m.values_grad(pred, None, mk, normalize=normalize, need_grad=False, rects=rects, target_taps=taps)
        assert torch.equal(v2, v0)
    # taps built under the other storage are refused, both ways
    taps = m.target_taps(target, rects)
    mo, _ = model("vgg", "fp32")
    with pytest.raises(ManusHipError, match="target_taps"):
        mo.values_grad(pred, target, need_grad=False, rects=rects, target_taps=taps)
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, need_grad=False, rects=rects, target_taps=mo.target_taps(target, rects))
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, need_grad=False, normalize=True, rects=rects, target_taps=taps)


BATCH_RECTS = [(5, 3, 24, 16), (0, 0, 33, 17), (20, 20, 24, 16), (0, 0, 0, 0), (7, 9, 16, 16), (23, 23, 33, 17), (30, 1, 24, 16)]


def raw_taps(m, target, mask, normalize, max_batch):
    """Every view's tap buffer of BATCH_RECTS after mgr_lpips_roi_taps_batch_st wrote into buffers pre-filled with one byte
    value; max_batch = 1 builds them view by view."""
    from manus_amd import _lib
    from manus_amd._lib import check, lib, ptr, stream
    V = len(BATCH_RECTS)
    r = np.ascontiguousarray(np.asarray(BATCH_RECTS, np.int32))
    rp = r.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    bufs = [torch.full((int(lib().mgr_lpips_taps_bytes_st(0, q[3], q[2], 1)),), 0x5A, dtype=torch.uint8, device=DEV) if q[2] else None
            for q in BATCH_RECTS]
    n = int(lib().mgr_lpips_roi_batch_workspace_bytes_st(0, V, rp, 0, max_batch, 1))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    outs = (ctypes.c_void_p * V)(*[None if b is None else ptr(b) for b in bufs])
    check(lib().mgr_lpips_roi_taps_batch_st(0, V, FH, FW, rp, ptr(target), ptr(mask), ptr(m.blob), m.blob.numel(), int(normalize), outs,
                                            max_batch, ptr(ws), n, stream(), _lib.MGR_LPIPS_BF16, _lib.MGR_LPIPS_STORE_BF16),
          "mgr_lpips_roi_taps_batch_st")
    torch.cuda.synchronize()
    return bufs


def test_batched_is_the_sequential_call():
    """Six views of 24x16 / 33x17 / 16x16 and an empty one with B = 4: values, gradient frames and the tap buffers."""
    m, _ = model("vgg")
    V = len(BATCH_RECTS)
    pred, target, mask = frames(31, V)
    scales = [0.25 * (v + 1) for v in range(V)]
    for mk, normalize in ((None, False), (mask, True)):
        v0, g0 = m.values_grad(pred, target, mk, normalize=normalize, need_grad=True, rects=BATCH_RECTS, grad_scales=scales)
        v0, g0 = v0.clone(), g0.clone()
        v1, g1 = m.values_grad(pred, target, mk, normalize=normalize, need_grad=True, rects=BATCH_RECTS, grad_scales=scales, batch=4)
        assert torch.equal(v1, v0) and torch.equal(g1, g0)
        assert float(v0[3]) == 0 and bool((g0[3] == 0).all()) and bool((v0[[0, 1, 2, 4, 5, 6]] > 0).all())
        t_bat = m.target_taps(target, BATCH_RECTS, mk, normalize, batch=4)
        # whole buffers, byte for byte (pre-filled: the padding between the taps of a buffer is written by nobody)
        for a, b in zip(raw_taps(m, target, mk, normalize, 1), raw_taps(m, target, mk, normalize, 4)):
            assert (a is None and b is None) or torch.equal(a, b)
        v2, g2 = m.values_grad(pred, None, mk, normalize=normalize, need_grad=True, rects=BATCH_RECTS, grad_scales=scales, batch=4,
                               target_taps=t_bat)
        assert torch.equal(v2, v0) and torch.equal(g2, g0)
        vf, _ = m.values_grad(pred, target, mk, normalize=normalize, need_grad=False, rects=BATCH_RECTS, batch=4)
        assert torch.equal(vf, v0)
    # accumulated
    prior = torch.randn(pred.shape, generator=torch.Generator().manual_seed(6)).to(DEV)
    buf = prior.clone()
    m.values_grad(pred, target, need_grad=True, rects=BATCH_RECTS, grad_scales=scales, batch=4, out_grad=buf, accumulate=True)
    ref = prior.clone()
    m.values_grad(pred, target, need_grad=True, rects=BATCH_RECTS, grad_scales=scales, out_grad=ref, accumulate=True)
    assert torch.equal(buf, ref) and torch.equal(buf[3], prior[3])


def test_seventeen_equal_views_in_two_chunks():
    m, _ = model("vgg")
    V = 17
    pred, target, _ = frames(32, V)
    rects = [((3 * v) % 30, (2 * v) % 20, 24, 16) for v in range(V)]
    v0, g0 = m.values_grad(pred, target, need_grad=True, rects=rects)
    v0, g0 = v0.clone(), g0.clone()
    v1, g1 = m.values_grad(pred, target, need_grad=True, rects=rects, batch=32)
    assert torch.equal(v1, v0) and torch.equal(g1, g0) and bool((v0 > 0).all())


def test_a_nan_view_leaves_the_others_bits():
    m, _ = model("vgg")
    pred, target, _ = frames(33, 4)
    rects = [(5, 3, 24, 16)] * 4
    v0, g0 = m.values_grad(pred, target, need_grad=True, rects=rects, batch=4)
    v0, g0 = v0.clone(), g0.clone()
    bad = pred.clone()
    bad[2] = float("nan")
    v1, g1 = m.values_grad(bad, target, need_grad=True, rects=rects, batch=4)
    keep = [0, 1, 3]
    assert torch.equal(v1[keep], v0[keep]) and torch.equal(g1[keep], g0[keep])
    assert not bool(torch.isfinite(v1[2]))


def test_a_short_workspace_is_refused_with_nothing_touched():
    from manus_amd import _lib
    from manus_amd._lib import lib, ptr, stream
    m, _ = model("vgg")
    V = 3
    pred, target, _ = frames(34, V)
    rects = np.array([(5, 3, 24, 16)] * V, np.int32)
    rp = rects.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    L = lib()
    need = L.mgr_lpips_roi_batch_workspace_bytes_st(0, V, rp, 1, 4, 1)
    one = L.mgr_lpips_roi_batch_workspace_bytes_st(0, V, rp, 1, 1, 1)
    assert one < need < L.mgr_lpips_roi_batch_workspace_bytes(0, V, rp, 1, 4)
    ws = torch.full((need,), 7, dtype=torch.uint8, device=DEV)
    vals, g = torch.full((V,), -3.0, device=DEV), torch.full_like(pred, -3.0)
    scales = (ctypes.c_float * V)(*[1.0] * V)
    rc = L.mgr_lpips_roi_batch_st(0, V, FH, FW, rp, ptr(pred), ptr(target), None, ptr(m.blob), m.blob.numel(), 0, scales, ptr(vals), ptr(g), 0,
                                  None, ptr(ws), need - 1, stream(), _lib.MGR_LPIPS_BF16, 4, _lib.MGR_LPIPS_STORE_BF16)
    torch.cuda.synchronize()
    assert rc == _lib.MGR_ENOMEM and "workspace" in L.mgr_last_error().decode()
    assert bool((vals == -3.0).all()) and bool((g == -3.0).all()) and bool((ws == 7).all())
    taps = [torch.full((L.mgr_lpips_taps_bytes_st(0, 16, 24, 1),), 7, dtype=torch.uint8, device=DEV) for _ in range(V)]
    need0 = L.mgr_lpips_roi_batch_workspace_bytes_st(0, V, rp, 0, 4, 1)
    rc = L.mgr_lpips_roi_taps_batch_st(0, V, FH, FW, rp, ptr(target), None, ptr(m.blob), m.blob.numel(), 0,
                                       (ctypes.c_void_p * V)(*[ptr(t) for t in taps]), 4, ptr(ws), need0 - 1, stream(), _lib.MGR_LPIPS_BF16,
                                       _lib.MGR_LPIPS_STORE_BF16)
    torch.cuda.synchronize()
    assert rc == _lib.MGR_ENOMEM and all(bool((t == 7).all()) for t in taps) and bool((ws == 7).all())


def test_alexnet_forward_only():
    from manus_amd._lib import ManusHipError
    a, _ = model("alex")
    pred, target, mask = frames(23, 2, 48, 80)
    rect = (9, 5, 67, 35)
    vals, g = a.values_grad(pred, target, mask, need_grad=False, rects=[rect, rect])
    cv, _ = a.values_grad(crop(pred, rect), crop(target, rect), crop(mask, rect), need_grad=False)
    assert g is None and bool((cv > 0).all()) and torch.equal(vals, cv)
    vb, _ = a.values_grad(pred, target, mask, need_grad=False, rects=[rect, rect], batch=2)
    assert torch.equal(vb, cv)
    buf = torch.full_like(pred, -3.0)
    with pytest.raises(ManusHipError, match="forward only"):
        a.values_grad(pred, target, need_grad=True, rects=[rect, rect], out_grad=buf)
    torch.cuda.synchronize()
    assert bool((buf == -3.0).all())

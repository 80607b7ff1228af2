"""GPU: a step's equal-size windows as one batched call (mgr_lpips_roi_batch_op, mgr_lpips_roi_taps_batch_op;
`LPIPS.values_grad(rects=, batch=B)`, `LPIPS.target_taps(batch=B)`).

In every kernel of csrc/lpips.hip an output depends on the sizes alone, so the batched call is DEFINED as the sequential one:
every check here is `torch.equal` against `batch=0`, values and gradient frames.  Stand-in weights (tests/lpips_ref.py); VGG on
a 56x40 frame (minimum window 16x16), AlexNet on 80x48 (minimum 31x31); every view has its own image.
"""
import functools

import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FW, FH = 56, 40
# two of 24x16 (an odd offset; the bottom-right corner), two of 33x17 (two column tiles with a ragged edge, five rows), the
# minimum, and an empty view
BASIC = [(5, 3, 24, 16), (1, 2, 33, 17), (32, 24, 24, 16), (0, 0, 0, 0), (23, 20, 33, 17), (7, 9, 16, 16)]
B = 4


@functools.lru_cache(maxsize=None)
def model(net, operands="fp32"):
    from manus_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(*R.state_dicts(net, R.make_weights(net, 0)), net=net, operands=operands)


@functools.lru_cache(maxsize=None)
def frames(seed=31, V=len(BASIC), H=FH, W=FW):
    return tuple(x.to(DEV) for x in R.images(seed, V, H, W))


def pair(m, pred, target, rects, batch, mask=None, prior=None, **kw):
    """(values, gradient frames) of the sequential call and of the batched one, on equal output buffers."""
    out = []
    for b in (0, batch):
        buf = None if prior is None else prior.clone()
        v, g = m.values_grad(pred, target, mask, rects=rects, batch=b, out_grad=buf, **kw)
        out.append((v.clone(), None if g is None else g.clone()))
    return out


def check_live(rects, vals, g):
    for v, r in enumerate(rects):
        if r[2] and r[3]:
            assert float(vals[v]) > 0 and bool((g[v] != 0).any()), v
        else:
            assert float(vals[v]) == 0


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_basic_set(operands):
    m = model("vgg", operands)
    pred, target, _ = frames()
    (v0, g0), (v1, g1) = pair(m, pred, target, BASIC, B, need_grad=True, grad_scale=0.7)
    check_live(BASIC, v0, g0)
    assert torch.equal(v1, v0) and torch.equal(g1, g0)
    assert bool((g1[3] == 0).all())
    # two runs give equal bits
    v2, g2 = m.values_grad(pred, target, rects=BASIC, batch=B, need_grad=True, grad_scale=0.7)
    assert torch.equal(v2, v0) and torch.equal(g2, g0)
    # forward only
    (f0, n0), (f1, n1) = pair(m, pred, target, BASIC, B, need_grad=False)
    assert n0 is None and n1 is None and torch.equal(f1, f0) and torch.equal(f0, v0)


@pytest.mark.parametrize("accumulate", [False, True])
def test_written_and_accumulated(accumulate):
    m = model("vgg")
    pred, target, _ = frames()
    if accumulate:
        prior = torch.randn(pred.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    else:
        prior = torch.full_like(pred, float("nan"))
    (v0, g0), (v1, g1) = pair(m, pred, target, BASIC, B, prior=prior, need_grad=True, grad_scale=1.5, accumulate=accumulate)
    assert torch.equal(v1, v0) and torch.equal(g1, g0)
    if accumulate:
        assert torch.equal(g1[3], prior[3]) and not torch.equal(g1[0], prior[0])
    else:
        # one launch per chunk wrote every view's whole frame, zeros outside its rectangle
        assert bool(torch.isfinite(g1).all()) and bool((g1[3] == 0).all())
        for v, (x0, y0, w, h) in enumerate(BASIC):
            ins = torch.zeros((FH, FW), dtype=torch.bool, device=DEV)
            ins[y0:y0 + h, x0:x0 + w] = True
            assert bool((g1[v][:, ~ins] == 0).all()), v


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_mask_normalize_and_per_view_scales(operands):
    m = model("vgg", operands)
    pred, target, mask = frames()
    scales = [0.5, 2.0, 1.0, 3.0, 0.25, 1.5]
    (v0, g0), (v1, g1) = pair(m, pred, target, BASIC, B, mask=mask, normalize=True, need_grad=True, grad_scales=scales)
    check_live(BASIC, v0, g0)
    assert torch.equal(v1, v0) and torch.equal(g1, g0)
    # the scales are per view: another scale for view 2 changes that view's gradient alone
    scales2 = list(scales)
    scales2[2] = 4.0
    _, g2 = m.values_grad(pred, target, mask, normalize=True, need_grad=True, rects=BASIC, grad_scales=scales2, batch=B)
    assert not torch.equal(g2[2], g0[2])
    assert all(torch.equal(g2[v], g0[v]) for v in (0, 1, 3, 4, 5))


def test_chunking():
    """Five views of one size with B = 2: chunks of 2, 2 and 1."""
    m = model("vgg")
    pred, target, _ = frames(32, 5)
    rects = [(5, 3, 24, 16), (0, 0, 24, 16), (32, 24, 24, 16), (11, 7, 24, 16), (31, 1, 24, 16)]
    (v0, g0), (v1, g1) = pair(m, pred, target, rects, 2, need_grad=True, grad_scale=0.9)
    check_live(rects, v0, g0)
    assert torch.equal(v1, v0) and torch.equal(g1, g0)
    assert len({float(x) for x in v0}) == 5          # (every view its own image)


def test_beyond_lp_max_batch():
    """Seventeen views of 16x16 with B = 32: chunks of LP_MAX_BATCH = 16 and 1."""
    from manus_amd.lpips import LP_MAX_BATCH
    assert LP_MAX_BATCH == 16
    m = model("vgg")
    pred, target, _ = frames(33, 17)
    rects = [((3 * i) % 41, (5 * i) % 25, 16, 16) for i in range(17)]
    (v0, g0), (v1, g1) = pair(m, pred, target, rects, 32, need_grad=True)
    check_live(rects, v0, g0)
    assert torch.equal(v1, v0) and torch.equal(g1, g0)


def test_isolation():
    """One view's render filled with NaN leaves every other view's value and gradient bit for bit unchanged."""
    m = model("vgg")
    pred, target, _ = frames()
    v0, g0 = m.values_grad(pred, target, rects=BASIC, batch=B, need_grad=True)
    v0, g0 = v0.clone(), g0.clone()
    bad = pred.clone()
    bad[2] = float("nan")          # (view 2 shares its chunk with view 0)
    v1, g1 = m.values_grad(bad, target, rects=BASIC, batch=B, need_grad=True)
    for v in (0, 1, 3, 4, 5):
        assert torch.equal(v1[v], v0[v]) and torch.equal(g1[v], g0[v]), v
    assert not bool(torch.isfinite(v1[2]))


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_cached_taps(operands):
    from manus_amd._lib import ManusHipError
    m = model("vgg", operands)
    pred, target, mask = frames()
    for mk, normalize in ((None, False), (mask, True)):
        t0 = m.target_taps(target, BASIC, mk, normalize)
        t1 = m.target_taps(target, BASIC, mk, normalize, batch=B)
        assert t1.bufs[3] is None and t0.bufs[3] is None
        # (the padding between the taps of a buffer is written by nobody: compare the taps themselves)
        for v, r in enumerate(BASIC):
            if t0.bufs[v] is None:
                continue
            assert t1.bufs[v].numel() == t0.bufs[v].numel()
            for off, n in tap_spans(r[3], r[2]):
                assert torch.equal(t1.bufs[v][off:off + n], t0.bufs[v][off:off + n]), (v, off)
        # each view's buffer ends up exactly as the one-view entry leaves it
        for a, b in zip(raw_taps(m, 0, target, mk, BASIC, normalize, 0, FH, FW), raw_taps(m, 0, target, mk, BASIC, normalize, B, FH, FW)):
            assert (a is None and b is None) or torch.equal(a, b)
        v0, g0 = m.values_grad(pred, target, mk, normalize=normalize, need_grad=True, grad_scale=0.3, rects=BASIC)
        v0, g0 = v0.clone(), g0.clone()
        for taps in (t0, t1):
            for tgt in (target, None):
                v1, g1 = m.values_grad(pred, tgt, mk, normalize=normalize, need_grad=True, grad_scale=0.3, rects=BASIC, target_taps=taps,
                                       batch=B)
                assert torch.equal(v1, v0) and torch.equal(g1, g0), (normalize, tgt is None)
        v2, _ = m.values_grad(pred, None, mk, normalize=normalize, need_grad=False, rects=BASIC, target_taps=t1, batch=B)
        assert torch.equal(v2, v0)
    # taps with another setting are still refused
    taps = m.target_taps(target, BASIC, batch=B)
    other = [(6, 3, 24, 16)] + BASIC[1:]
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, need_grad=False, rects=other, target_taps=taps, batch=B)
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, need_grad=False, normalize=True, rects=BASIC, target_taps=taps, batch=B)
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, mask, need_grad=False, rects=BASIC, target_taps=taps, batch=B)


def raw_taps(m, net, target, mask, rects, normalize, batch, H, W):
    """Every view's tap buffer after the C entries wrote into buffers pre-filled with one byte value: the one-view entry view by
    view (batch = 0) or the batched entry.  Whole buffers, the padding between the taps included."""
    import ctypes
    import numpy as np
    from manus_amd._lib import check, lib, ptr, stream
    V = len(rects)
    r = np.ascontiguousarray(np.asarray(rects, np.int32))
    rp = r.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    bufs = [torch.full((int(lib().mgr_lpips_taps_bytes(net, q[3], q[2])),), 0x5A, dtype=torch.uint8, device=DEV) if q[2] else None
            for q in rects]
    n = int(lib().mgr_lpips_roi_batch_workspace_bytes(net, V, rp, 0, max(batch, 1)))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    if batch:
        outs = (ctypes.c_void_p * V)(*[None if b is None else ptr(b) for b in bufs])
        check(lib().mgr_lpips_roi_taps_batch_op(net, V, H, W, rp, ptr(target), ptr(mask), ptr(m.blob), m.blob.numel(), int(normalize), outs,
                                                batch, ptr(ws), n, stream(), m._op), "mgr_lpips_roi_taps_batch_op")
    else:
        for v in range(V):
            if bufs[v] is not None:
                check(lib().mgr_lpips_roi_taps_op(net, H, W, r[v].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ptr(target[v]),
                                                  None if mask is None else ptr(mask[v]), ptr(m.blob), m.blob.numel(), int(normalize),
                                                  ptr(bufs[v]), ptr(ws), n, stream(), m._op), "mgr_lpips_roi_taps_op")
    torch.cuda.synchronize()
    return bufs


def tap_spans(h, w, net="vgg"):
    """(byte offset, bytes) of the five taps inside a view's tap buffer: the tap region of the one-view layout."""
    from manus_amd.lpips import TAP_CHANNELS, layout
    lay = layout(net, h, w, 0)
    sizes = []
    hh, ww = h, w
    for k, c in enumerate(TAP_CHANNELS[net]):
        sizes.append(4 * c * hh * ww)
        hh, ww = hh // 2, ww // 2
    return [(lay["tap"][k] - lay["tap"][0], sizes[k]) for k in range(5)]


def test_mixed_taps_through_the_c_abi():
    """The C ABI allows a chunk in which some views have cached taps and others not (the Python layer never produces it): the
    target tower runs for the others alone."""
    import ctypes
    import numpy as np
    from manus_amd._lib import check, lib, ptr, stream
    m = model("vgg")
    pred, target, _ = frames()
    v0, g0 = m.values_grad(pred, target, rects=BASIC, need_grad=True, grad_scale=0.6)
    v0, g0 = v0.clone(), g0.clone()
    taps = m.target_taps(target, BASIC)
    V = len(BASIC)
    rects = np.ascontiguousarray(np.asarray(BASIC, np.int32))
    rp = rects.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    some = (ctypes.c_void_p * V)(*[ptr(taps.bufs[v]) if v in (2, 4) else None for v in range(V)])      # one view of each chunk
    n = int(lib().mgr_lpips_roi_batch_workspace_bytes(0, V, rp, 1, B))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    vals, g = torch.empty(V, device=DEV), torch.full_like(pred, float("nan"))
    check(lib().mgr_lpips_roi_batch_op(0, V, FH, FW, rp, ptr(pred), ptr(target), None, ptr(m.blob), m.blob.numel(), 0,
                                       (ctypes.c_float * V)(*([0.6] * V)), ptr(vals), ptr(g), 0, some, ptr(ws), n, stream(), 0, B),
          "mgr_lpips_roi_batch_op")
    assert torch.equal(vals, v0) and torch.equal(g, g0)


def test_alexnet_forward_only():
    from manus_amd._lib import ManusHipError
    a = model("alex")
    pred, target, mask = frames(34, 3, 48, 80)
    rects = [(9, 5, 31, 31), (40, 15, 40, 33), (49, 17, 31, 31)]
    (v0, n0), (v1, n1) = pair(a, pred, target, rects, B, mask=mask, need_grad=False)
    assert n0 is None and n1 is None and all(float(x) > 0 for x in v0) and torch.equal(v1, v0)
    for x, y in zip(raw_taps(a, 1, target, mask, rects, False, 0, 48, 80), raw_taps(a, 1, target, mask, rects, False, B, 48, 80)):
        assert torch.equal(x, y) and bool((x != 0x5A).any())
    t1 = a.target_taps(target, rects, mask, batch=B)
    v2, _ = a.values_grad(pred, None, mask, need_grad=False, rects=rects, target_taps=t1, batch=B)
    assert torch.equal(v2, v0)
    buf = torch.full_like(pred, -3.0)
    with pytest.raises(ManusHipError, match="forward only"):
        a.values_grad(pred, target, need_grad=True, rects=rects, out_grad=buf, batch=B)
    torch.cuda.synchronize()
    assert bool((buf == -3.0).all())


def test_enomem_leaves_the_outputs_alone():
    """A workspace of the sequential size is too short for a chunk of two: refused before the first launch."""
    import ctypes
    import numpy as np
    from manus_amd._lib import MGR_ENOMEM, lib, ptr, stream
    m = model("vgg")
    pred, target, _ = frames()
    V = len(BASIC)
    rects = np.ascontiguousarray(np.asarray(BASIC, np.int32))
    rp = rects.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    short = int(lib().mgr_lpips_roi_workspace_bytes(0, V, rp, 1))
    assert short < lib().mgr_lpips_roi_batch_workspace_bytes(0, V, rp, 1, B)
    ws = torch.empty(short, dtype=torch.uint8, device=DEV)
    vals, g = torch.full((V,), -3.0, device=DEV), torch.full_like(pred, -3.0)
    for accumulate in (0, 1):
        rc = lib().mgr_lpips_roi_batch_op(0, V, FH, FW, rp, ptr(pred), ptr(target), None, ptr(m.blob), m.blob.numel(), 0,
                                          (ctypes.c_float * V)(*([1.0] * V)), ptr(vals), ptr(g), accumulate, None, ptr(ws), short, stream(),
                                          0, B)
        assert rc == MGR_ENOMEM and "workspace" in lib().mgr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((vals == -3.0).all()) and bool((g == -3.0).all())
    # the taps build alike
    bufs = [torch.full((max(int(lib().mgr_lpips_taps_bytes(0, r[3], r[2])), 1),), 7, dtype=torch.uint8, device=DEV) for r in BASIC]
    outs = (ctypes.c_void_p * V)(*[ptr(b) if r[2] else None for b, r in zip(bufs, BASIC)])
    short = int(lib().mgr_lpips_roi_batch_workspace_bytes(0, V, rp, 0, 1))
    rc = lib().mgr_lpips_roi_taps_batch_op(0, V, FH, FW, rp, ptr(target), None, ptr(m.blob), m.blob.numel(), 0, outs, B, ptr(ws), short,
                                           stream(), 0)
    assert rc == MGR_ENOMEM
    torch.cuda.synchronize()
    assert all(bool((b == 7).all()) for b in bufs)

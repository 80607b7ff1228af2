"""GPU: LPIPS on a per-view window (mgr_lpips_roi_op, mgr_lpips_roi_taps_op; `LPIPS.values_grad(rects=)`, `LPIPS.target_taps`).

The windowed distance is DEFINED as the plain call on contiguous crops, so nearly every check here is `torch.equal` against
that call; one case pins the window to the fp64 restatement (tests/lpips_ref.py) as well, within the bound of
test_gpu_lpips.py: 8 * max(e32, 2^-23), e32 the fp32 restatement's own error against fp64.  Stand-in weights; the frame is
56x40 (AlexNet: 80x48).
"""
import functools

import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
DEV = "cuda"
FW, FH = 56, 40
RECTS = [(5, 3, 33, 17), (16, 24, 40, 16), (0, 0, 56, 40), (7, 9, 16, 16)]      # odd offset; right and bottom borders; frame; minimum


def bound(e32):
    return 8 * max(e32, EPS)


@functools.lru_cache(maxsize=None)
def model(net, operands="fp32"):
    from manus_amd.lpips import LPIPS
    wts = R.make_weights(net, 0)
    return LPIPS.from_state_dicts(*R.state_dicts(net, wts), net=net, operands=operands), wts


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


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
@pytest.mark.parametrize("rect", RECTS)
def test_window_is_the_call_on_crops(operands, rect):
    m, _ = model("vgg", operands)
    pred, target, _ = frames()
    vals, g = m.values_grad(pred, target, need_grad=True, grad_scale=0.7, rects=[rect])
    vals, g = vals.clone(), g.clone()
    cv, cg = m.values_grad(crop(pred, rect), crop(target, rect), need_grad=True, grad_scale=0.7)
    assert float(cv[0]) > 0
    assert torch.equal(vals, cv) and torch.equal(crop(g, rect), cg)
    if rect == (0, 0, FW, FH):
        pv, pg = m.values_grad(pred, target, need_grad=True, grad_scale=0.7)
        assert torch.equal(vals, pv) and torch.equal(g, pg)
    # forward only: the same value
    vf, gf = m.values_grad(pred, target, need_grad=False, rects=[rect])
    assert gf is None and torch.equal(vf, vals)
    # determinism: two runs give equal bits
    v2, g2 = m.values_grad(pred, target, need_grad=True, grad_scale=0.7, rects=[rect])
    assert torch.equal(v2, vals) and torch.equal(g2, g)


@pytest.mark.parametrize("rect", RECTS[:2])
def test_outside_is_zero_when_written(rect):
    m, _ = model("vgg")
    pred, target, _ = frames()
    buf = torch.full_like(pred, float("nan"))
    m.values_grad(pred, target, need_grad=True, rects=[rect], out_grad=buf, accumulate=False)
    ins = inside(rect)
    assert bool((buf[0][:, ~ins] == 0).all())
    assert bool(torch.isfinite(buf[0][:, ins]).all()) and bool((buf[0][:, ins] != 0).any())


@pytest.mark.parametrize("rect", RECTS[:2])
def test_outside_is_untouched_when_accumulated(rect):
    m, _ = model("vgg")
    pred, target, _ = frames()
    prior = torch.randn(pred.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    buf = prior.clone()
    m.values_grad(pred, target, need_grad=True, grad_scale=1.5, rects=[rect], out_grad=buf, accumulate=True)
    _, cg = m.values_grad(crop(pred, rect), crop(target, rect), need_grad=True, grad_scale=1.5)
    ins = inside(rect)
    assert torch.equal(buf[0][:, ~ins], prior[0][:, ~ins])
    assert torch.equal(crop(buf, rect), crop(prior, rect) + cg)


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_masked_and_normalized(operands):
    m, _ = model("vgg", operands)
    pred, target, mask = frames()
    rect = RECTS[0]
    for accumulate in (False, True):
        prior = torch.randn(pred.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
        buf = prior.clone()
        vals, _ = m.values_grad(pred, target, mask, normalize=True, need_grad=True, rects=[rect], out_grad=buf, accumulate=accumulate)
        vals = vals.clone()
        cv, cg = m.values_grad(crop(pred, rect), crop(target, rect), crop(mask, rect), normalize=True, need_grad=True)
        assert torch.equal(vals, cv)
        assert torch.equal(crop(buf, rect), crop(prior, rect) + cg if accumulate else cg)


def test_views_with_their_own_rects_and_scales():
    m, _ = model("vgg")
    pred, target, mask = frames(22, 3)
    rects = [(5, 3, 33, 17), (0, 0, 0, 0), (30, 2, 21, 38)]
    scales = (0.5, 2.0, 1.0)
    vals, g = m.values_grad(pred, target, mask, need_grad=True, rects=rects, grad_scales=scales)
    vals, g = vals.clone(), g.clone()
    for v in range(3):
        vv, gv = m.values_grad(pred[v:v + 1], target[v:v + 1], mask[v:v + 1], need_grad=True, rects=[rects[v]], grad_scale=scales[v])
        assert torch.equal(vv[0], vals[v]) and torch.equal(gv[0], g[v]), v
    assert float(vals[1]) == 0.0 and bool((g[1] == 0).all())
    assert float(vals[0]) > 0 and float(vals[2]) > 0
    # accumulate: the empty view's plane is untouched
    prior = torch.randn(pred.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    buf = prior.clone()
    m.values_grad(pred, target, mask, need_grad=True, rects=rects, grad_scales=scales, out_grad=buf, accumulate=True)
    assert torch.equal(buf[1], prior[1]) and torch.equal(buf, prior + g)
    # two runs give equal bits
    v2, g2 = m.values_grad(pred, target, mask, need_grad=True, rects=rects, grad_scales=scales)
    assert torch.equal(v2, vals) and torch.equal(g2, g)


def test_window_against_the_checker():
    m, wts = model("vgg")
    pred, target, _ = frames()
    rect = RECTS[0]
    vals, _ = m.values_grad(pred, target, need_grad=False, rects=[rect])
    p, t = crop(pred, rect)[0].cpu(), crop(target, rect)[0].cpu()
    r64 = float(R.forward("vgg", wts, p, t)[0])
    r32 = float(R.forward("vgg", wts, p, t, dtype=torch.float32)[0])
    e32, e = abs(r32 - r64) / abs(r64), abs(float(vals[0]) - r64) / abs(r64)
    print("window %s: value %.6g, device %.3g, fp32 restatement %.3g" % (rect, r64, e, e32))
    assert e <= bound(e32), (e, e32)


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_cached_taps(operands):
    from manus_amd._lib import ManusHipError, lib
    m, _ = model("vgg", operands)
    pred, target, mask = frames(22, 3)
    rects = [(5, 3, 33, 17), (0, 0, 0, 0), (30, 2, 21, 38)]
    for mk, normalize in ((None, False), (mask, True)):
        v0, g0 = m.values_grad(pred, target, mk, normalize=normalize, need_grad=True, grad_scale=0.3, rects=rects)
        v0, g0 = v0.clone(), g0.clone()
        taps = m.target_taps(target, rects, mk, normalize)
        assert taps.bufs[1] is None and taps.bufs[0].numel() == lib().mgr_lpips_taps_bytes(0, 17, 33)
        for tgt in (target, None):
            v1, g1 = m.values_grad(pred, tgt, mk, normalize=normalize, need_grad=True, grad_scale=0.3, rects=rects, target_taps=taps)
            assert torch.equal(v1, v0) and torch.equal(g1, g0), (normalize, tgt is None)
        v2, _ = m.values_grad(pred, None, mk, normalize=normalize, need_grad=False, rects=rects, target_taps=taps)
        assert torch.equal(v2, v0)
    # taps of other rects, flags or of the other operand mode are refused
    taps = m.target_taps(target, rects)
    other = [(6, 3, 33, 17), (0, 0, 0, 0), (30, 2, 21, 38)]
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, need_grad=False, rects=other, target_taps=taps)
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, need_grad=False, normalize=True, rects=rects, target_taps=taps)
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(pred, target, mask, need_grad=False, rects=rects, target_taps=taps)
    m2, _ = model("vgg", "bf16" if operands == "fp32" else "fp32")
    with pytest.raises(ManusHipError, match="target_taps"):
        m2.values_grad(pred, target, need_grad=False, rects=rects, target_taps=taps)
    with pytest.raises(ManusHipError, match="target or target_taps"):
        m.values_grad(pred, None, need_grad=False, rects=rects)


def test_alexnet_forward_only():
    from manus_amd._lib import ManusHipError
    a, _ = model("alex")
    pred, target, mask = frames(23, 1, 48, 80)
    rect = (9, 5, 67, 35)
    vals, g = a.values_grad(pred, target, mask, need_grad=False, rects=[rect])
    cv, _ = a.values_grad(crop(pred, rect), crop(target, rect), crop(mask, rect), need_grad=False)
    assert g is None and float(cv[0]) > 0 and torch.equal(vals, cv)
    buf = torch.full_like(pred, -3.0)
    with pytest.raises(ManusHipError, match="forward only"):
        a.values_grad(pred, target, need_grad=True, rects=[rect], out_grad=buf)
    torch.cuda.synchronize()
    assert bool((buf == -3.0).all())


@pytest.mark.parametrize("rect,why", [((30, 20, 40, 16), "not inside"), ((5, 3, 33, 40), "not inside"), ((-1, 3, 33, 17), "not inside"),
                                      ((5, 3, -16, 16), "negative"), ((5, 3, 15, 16), "too small"), ((5, 3, 16, 15), "too small")])
def test_refusals_leave_the_outputs_alone(rect, why):
    from manus_amd._lib import ManusHipError
    m, _ = model("vgg")
    pred, target, _ = frames(22, 3)
    good = (5, 3, 33, 17)
    for accumulate in (False, True):
        buf = torch.full_like(pred, -3.0)
        with pytest.raises(ManusHipError, match=why):
            # the bad rectangle is the LAST view's: the views before it must not have run either
            m.values_grad(pred, target, need_grad=True, rects=[good, good, rect], out_grad=buf, accumulate=accumulate)
        torch.cuda.synchronize()
        assert bool((buf == -3.0).all())
    with pytest.raises(ManusHipError, match=why):
        m.target_taps(target, [good, good, rect])

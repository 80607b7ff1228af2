"""GPU: LPIPS (mgr_lpips, csrc/lpips.hip) against its restatement (tests/lpips_ref.py).

Bounds: 8 * max(e32, 2^-23) with e32 the fp32 restatement's own error against fp64 in the same norm, measured in the test (the
rule of the articulation edge tests: the kernel's summation order differs from torch's).  Stand-in weights from seeded
generators (no weight file ships); VGG at 40x24 and 33x17 (pooled sizes 5 -> 2 and 3 -> 1, W no multiple of 32), AlexNet at
67x35.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from util import max_rel_err, row_rel_err

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
DEV = "cuda"


def bound(e32):
    return 8 * max(e32, EPS)


@functools.lru_cache(maxsize=None)
def model(net, seed=0):
    from manus_amd.lpips import LPIPS
    wts = R.make_weights(net, seed)
    return LPIPS.from_state_dicts(*R.state_dicts(net, wts), net=net), wts


def device_acts(m, net, H, W, ref_feats, ref_tgt):
    """Every stored activation of the model's workspace (the last view of the last call), through mgr_lpips_layout."""
    from manus_amd.lpips import layout
    lay = layout(net, H, W, True)
    torch.cuda.synchronize()
    ws = m._ws

    def read(off, shape):
        n = shape[0] * shape[1] * shape[2]
        return ws[off:off + 4 * n].view(torch.float32).reshape(shape).cpu()

    acts = [read(o, a.shape) for o, a in zip(lay["act"], ref_feats["act"])]
    taps = [read(o, a.shape) for o, a in zip(lay["tap"], ref_tgt["tap"])]
    return acts, taps


# ---------------------------------------------------------------------------
# lane maps
# ---------------------------------------------------------------------------
def _one_hot(n_out, n_in):
    """Output channel j picks input channel c(j) at tap (ky(j), kx(j)): an asymmetric assignment."""
    w = torch.zeros((n_out, n_in, 3, 3))
    for j in range(n_out):
        w[j, (7 * j + 3) % n_in, (j // 3) % 3, j % 3] = 1.0
    return w


@pytest.mark.parametrize("cin,cout,W,H", [(5, 33, 37, 9), (64, 64, 40, 24)])
def test_lane_maps_one_hot_forward(cin, cout, W, H):
    from manus_amd.lpips import conv2d
    g = torch.Generator().manual_seed(3)
    x = torch.randn((cin, H, W), generator=g)
    w = _one_hot(cout, cin)
    y = conv2d(x.to(DEV), w.to(DEV), None, 1, 1, relu=False).cpu()
    want = torch.zeros((cout, H, W))
    xp = F.pad(x, (1, 1, 1, 1))
    for j in range(cout):
        want[j] = xp[(7 * j + 3) % cin, (j // 3) % 3:(j // 3) % 3 + H, j % 3:j % 3 + W]
    assert torch.equal(y, want)


@pytest.mark.parametrize("cin,cout,W,H", [(5, 33, 37, 9), (64, 64, 40, 24)])
def test_lane_maps_one_hot_data_gradient(cin, cout, W, H):
    """The transposed run takes `cin` channels and gives `cout`: the layer's own (Cout, Cin) are (cin, cout).  Every output
    channel receives from exactly one (channel, tap), so the result is a shifted plane bit for bit."""
    from manus_amd.lpips import conv2d
    g = torch.Generator().manual_seed(4)
    x = torch.randn((cin, H, W), generator=g)
    w = _one_hot(cout, cin).permute(1, 0, 2, 3).contiguous()        # layer (Cout = cin, Cin = cout)
    y = conv2d(x.to(DEV), w.to(DEV), None, 1, 1, relu=False, transposed=True).cpu()
    want = torch.zeros((cout, H, W))
    xp = F.pad(x, (1, 1, 1, 1))
    for j in range(cout):
        ky, kx = (j // 3) % 3, j % 3       # gin[p] = gout[p - (k - 1)]: the opposite shift
        want[j] = xp[(7 * j + 3) % cin, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
    assert torch.equal(y, want)
    # and the ReLU gate: positions where the gate is not positive contribute nothing
    gate = torch.randn((cin, H, W), generator=g)
    y = conv2d(x.to(DEV), w.to(DEV), None, 1, 1, relu=False, transposed=True, gate=gate.to(DEV)).cpu()
    xg = F.pad(x * (gate > 0), (1, 1, 1, 1))
    for j in range(cout):
        ky, kx = (j // 3) % 3, j % 3
        want[j] = xg[(7 * j + 3) % cin, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
    assert torch.equal(y, want)


# ---------------------------------------------------------------------------
# convolution alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,s,p,W,H", [(3, 64, 3, 1, 1, 40, 24), (5, 33, 3, 1, 1, 37, 9), (64, 128, 3, 1, 1, 33, 17),
                                                (512, 512, 3, 1, 1, 5, 3), (3, 64, 11, 4, 2, 67, 35), (64, 192, 5, 1, 2, 67, 35)])
def test_convolution_against_fp64(cin, cout, k, s, p, W, H):
    from manus_amd.lpips import conv2d
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn((cin, H, W), generator=g)
    w = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g)
    ref = torch.relu(F.conv2d(x.double()[None], w.double(), b.double(), stride=s, padding=p))[0]
    r32 = torch.relu(F.conv2d(x[None], w, b, stride=s, padding=p))[0]
    y = conv2d(x.to(DEV), w.to(DEV), b.to(DEV), s, p, relu=True).cpu()
    e32, e = row_rel_err(r32, ref), row_rel_err(y, ref)
    print("conv %s: device %.3g, fp32 restatement %.3g" % ((cin, cout, k, s, p), e, e32))
    assert e <= bound(e32), (e, e32)


# ---------------------------------------------------------------------------
# the whole call
# ---------------------------------------------------------------------------
def _call(net, W, H, V=1, seed=1, normalize=False, masked=False, need_grad=False, **kw):
    m, wts = model(net)
    pred, target, mask = R.images(seed, V, H, W)
    mk = mask if masked else None
    vals, g = m.values_grad(pred.to(DEV), target.to(DEV), None if mk is None else mk.to(DEV), normalize=normalize, need_grad=need_grad, **kw)
    return m, wts, pred, target, mk, vals, g


@pytest.mark.parametrize("net,W,H", [("vgg", 40, 24), ("vgg", 33, 17), ("alex", 67, 35)])
def test_every_stored_activation(net, W, H):
    m, wts, pred, target, _, vals, _ = _call(net, W, H, need_grad=(net == "vgg"))
    _, fa, fb = R.forward(net, wts, pred[0], target[0])
    _, fa32, fb32 = R.forward(net, wts, pred[0], target[0], dtype=torch.float32)
    acts, taps = device_acts(m, net, H, W, fa, fb)
    for name, dev, r64, r32 in [("act%d" % i, a, fa["act"][i], fa32["act"][i]) for i, a in enumerate(acts)] + \
                               [("tap%d" % k, t, fb["tap"][k], fb32["tap"][k]) for k, t in enumerate(taps)]:
        e32, e = row_rel_err(r32, r64), row_rel_err(dev, r64)
        print("%s %s: device %.3g, fp32 restatement %.3g" % (net, name, e, e32))
        assert e <= bound(e32), (name, e, e32)


@pytest.mark.parametrize("net,W,H", [("vgg", 40, 24), ("vgg", 33, 17), ("alex", 67, 35)])
@pytest.mark.parametrize("V,normalize,masked", [(1, False, False), (3, False, True), (1, True, True), (3, True, False)])
def test_values(net, W, H, V, normalize, masked):
    m, wts, pred, target, mk, vals, _ = _call(net, W, H, V=V, normalize=normalize, masked=masked)
    vals = vals.cpu()
    for v in range(V):
        mv = None if mk is None else mk[v]
        r64 = float(R.forward(net, wts, pred[v], target[v], mv, normalize)[0])
        r32 = float(R.forward(net, wts, pred[v], target[v], mv, normalize, dtype=torch.float32)[0])
        e32, e = abs(r32 - r64) / abs(r64), abs(float(vals[v]) - r64) / abs(r64)
        print("%s V=%d view %d: value %.6g, device %.3g, fp32 restatement %.3g" % (net, V, v, r64, e, e32))
        assert e <= bound(e32), (v, e, e32)


def test_identical_images_give_exactly_zero():
    m, _ = model("vgg")
    pred, _, mask = R.images(5, 2, 24, 40)
    x = pred.to(DEV)
    vals, g = m.values_grad(x, x.clone(), mask.to(DEV), need_grad=True, grad_scale=3.0)
    assert bool((vals == 0).all()) and bool((g == 0).all())
    a, _ = model("alex")
    pred, _, _ = R.images(5, 1, 35, 67)
    vals, _ = a.values_grad(pred.to(DEV), pred.to(DEV), need_grad=False)
    assert bool((vals == 0).all())


@pytest.mark.parametrize("W,H,seed", R.GRAD_CASES)
@pytest.mark.parametrize("normalize,masked", [(False, False), (True, True)])
def test_gradient_for_the_device_decisions(W, H, seed, normalize, masked):
    m, wts, pred, target, mk, vals, g = _call("vgg", W, H, seed=seed, normalize=normalize, masked=masked, need_grad=True, grad_scale=1.0)
    mv = None if mk is None else mk[0]
    _, fa, fb = R.forward("vgg", wts, pred[0], target[0], mv, normalize)
    _, fa32, _ = R.forward("vgg", wts, pred[0], target[0], mv, normalize, dtype=torch.float32)
    acts, _ = device_acts(m, "vgg", H, W, fa, fb)
    dec = R.decisions_of("vgg", acts)
    # the device's decisions against the fp64 restatement's own
    for kind, i, n, differing, off_threshold in R.compare_decisions("vgg", dec, fa, fa32):
        print("%s %d: %d of %d decisions differ, %d not at a threshold" % (kind, i, differing, n, off_threshold))
        assert off_threshold == 0, (kind, i, differing, off_threshold)
        assert differing <= 1e-3 * n, (kind, i, differing, n)
    for k in range(5):
        assert bool(((acts[[1, 3, 6, 9, 12][k]] ** 2).sum(0) > 0).all()), "a pixel with all-zero tap features"
    # the gradient for exactly those decisions
    grads = {}
    for dt in (torch.float64, torch.float32):
        _, fz, fzb = R.forward("vgg", wts, pred[0], target[0], mv, normalize, dtype=dt, decisions=dec)
        grads[dt] = R.backward("vgg", wts, fz, fzb, dec, (H, W), mv, normalize, dtype=dt)
    e32, e = max_rel_err(grads[torch.float32], grads[torch.float64]), max_rel_err(g[0].cpu(), grads[torch.float64])
    print("gradient %dx%d: device %.3g, fp32 restatement %.3g" % (W, H, e, e32))
    assert e <= bound(e32), (e, e32)


# ---------------------------------------------------------------------------
# call semantics
# ---------------------------------------------------------------------------
def test_accumulate_reproducible_and_views_independent():
    m, _ = model("vgg")
    pred, target, mask = (x.to(DEV) for x in R.images(7, 3, 24, 40))
    v0, g0 = m.values_grad(pred, target, mask, need_grad=True, grad_scale=0.5)
    v0, g0 = v0.clone(), g0.clone()
    # two runs give equal bits
    v1, g1 = m.values_grad(pred, target, mask, need_grad=True, grad_scale=0.5)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    # accumulate = 1 equals accumulate = 0 plus the prior content
    prior = torch.randn_like(pred)
    acc = prior.clone()
    m.values_grad(pred, target, mask, need_grad=True, grad_scale=0.5, out_grad=acc, accumulate=True)
    assert torch.equal(acc, prior + g0)
    # V = 3 equals three V = 1 calls, bit for bit
    for v in range(3):
        vv, gv = m.values_grad(pred[v:v + 1], target[v:v + 1], mask[v:v + 1], need_grad=True, grad_scale=0.5)
        assert torch.equal(vv[0], v0[v]) and torch.equal(gv[0], g0[v])
    # forward only gives the same values
    vf, gf = m.values_grad(pred, target, mask, need_grad=False)
    assert gf is None and torch.equal(vf, v0)


def test_autograd_surface_matches_the_direct_call():
    from manus_amd import losses
    m, _ = model("vgg")
    pred, target, _ = (x.to(DEV) for x in R.images(8, 2, 24, 40))
    vals, g = m.values_grad(pred, target, need_grad=True)
    vals, g = vals.clone(), g.clone()
    x = pred.clone().requires_grad_(True)
    d = m(x, target)
    assert d.shape == (2, 1, 1, 1) and torch.equal(d.reshape(-1), vals)
    coef = torch.tensor([0.25, 2.0], device=DEV)
    (d.reshape(-1) * coef).sum().backward()
    assert torch.equal(x.grad, g * coef.reshape(-1, 1, 1, 1))
    # no gradient asked: none computed; AlexNet is forward only
    assert not m(pred, target).requires_grad
    a, _ = model("alex")
    pa, ta, _ = (t.to(DEV) for t in R.images(8, 1, 35, 67))
    assert a(pa, ta).shape == (1, 1, 1, 1)
    from manus_amd._lib import ManusHipError
    with pytest.raises(ManusHipError, match="forward only"):
        a(pa.clone().requires_grad_(True), ta)
    # losses.lpips_loss: the reference's HWC call
    hwc = pred[0].permute(1, 2, 0).contiguous().requires_grad_(True)
    loss = losses.lpips_loss(hwc, target[:1].permute(0, 2, 3, 1), m)
    assert torch.equal(loss, vals[0])
    loss.backward()
    assert torch.equal(hwc.grad, g[0].permute(1, 2, 0))


def test_descent():
    m, _ = model("vgg")
    pred, target, _ = (x.to(DEV) for x in R.images(9, 1, 24, 40))
    x = pred.clone()
    v0, g = m.values_grad(x, target, need_grad=True)
    lr = 0.05 * float(v0[0]) / float((g * g).sum())     # a step that would remove 5 % of the value if the value were linear
    last = float(v0[0])
    for _ in range(20):
        x = x - lr * g
        v, g = m.values_grad(x, target, need_grad=True)
        assert float(v[0]) < last, (float(v[0]), last)
        last = float(v[0])

"""GPU: the bf16 storage mode of LPIPS (the mgr_lpips*_st entries with MGR_LPIPS_STORE_BF16; the blocked paths of k_lp_conv16,
k_lp_pool_b, k_lp_pool2_bwd_b, k_lp_head_b of csrc/lpips.hip) against tests/lpips_store_ref.py.

Bars.  Integer maps: exact (`torch.equal`), a bf16 output being rb(fp64 convolution).  One convolution on random data, read
unrounded through y_storage = fp32: the project's 8 * max(e32, 2^-23) in row_rel_err against fp64 of the given (rounded)
operands; its bf16 output is rb of that fp32 output, bit for bit.  Forward: every stored activation is rb(the operand mode's)
of the same call, bit for bit (tests/test_lpips_store_cpu.py has the argument).  End to end against the fp64 restatement: 2 x
the storage emulation's own distance, the bar and the reason of tests/test_gpu_lpips_bf16.py.  Stand-in weights of seed 0.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import lpips_bf16_ref as B
import lpips_ref as R
import lpips_store_ref as S
from util import max_rel_err, row_rel_err

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
DEV = "cuda"
COMBOS = (("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16"))


def bound(e32):
    return 8 * max(e32, EPS)


@functools.lru_cache(maxsize=None)
def model(net, storage="bf16"):
    from manus_amd.lpips import LPIPS
    wts = B.weights(net)
    return LPIPS.from_state_dicts(*R.state_dicts(net, wts), net=net, operands="bf16", storage=storage), wts


def stored(m, net, H, W, need_grad=True):
    """(pred's stored activations, the target's taps) of the model's last call (its last view), fp32 on the host, read through
    the layout entry of the model's storage."""
    from manus_amd.lpips import layout, unpack_blocked
    lay = layout(net, H, W, need_grad, storage=m.storage)
    shapes, taps = S.conv_shapes(net, H, W)
    torch.cuda.synchronize()
    ws = m._ws

    def read(off, shape):
        C, h, w = shape
        if m.storage == "bf16":
            return unpack_blocked(ws[off:off + 2 * ((C + 7) // 8) * 8 * h * w], C, h, w).cpu()
        return ws[off:off + 4 * C * h * w].view(torch.float32).reshape(shape).cpu()

    return [read(o, s) for o, s in zip(lay["act"], shapes)], [read(lay["tap"][k], shapes[taps[k]]) for k in range(5)]


def conv(x, w, b=None, s=1, p=0, **kw):
    from manus_amd.lpips import conv2d
    return conv2d(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), s, p, operands="bf16",
                  **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}).cpu()


# ---------------------------------------------------------------------------
# 1. exact integer maps, all four storage combinations
# ---------------------------------------------------------------------------
# the forward shapes of test_gpu_lpips_bf16.py, then Cout = 3, 40, 72, 96 with W = 31, 33, 37, 65 and H = 1, 5, 9
INT_SHAPES = [(3, 64, 3, 1, 1, 40, 24), (5, 33, 3, 1, 1, 37, 9), (8, 65, 3, 1, 1, 31, 5), (17, 1, 3, 1, 1, 33, 1), (64, 64, 3, 1, 1, 32, 4),
              (512, 512, 3, 1, 1, 5, 3), (3, 64, 11, 4, 2, 67, 35), (64, 192, 5, 1, 2, 13, 7),
              (8, 3, 3, 1, 1, 33, 5), (16, 40, 3, 1, 1, 65, 9), (40, 72, 3, 1, 1, 31, 1), (72, 96, 3, 1, 1, 37, 5), (96, 40, 3, 1, 1, 33, 9)]


def _ints(g, shape):
    return torch.randint(-3, 4, shape, generator=g).float()


def _check_int(y_raw, want, ys):
    """y_raw: what the kernel wrote (fp32 tensor, or the blocked bytes)."""
    from manus_amd.lpips import unpack_blocked
    C, h, w = want.shape
    if ys == "fp32":
        assert torch.equal(y_raw.cpu(), want.float())
        return
    full = unpack_blocked(y_raw.cpu(), C, h, w, pads=True)
    assert torch.equal(full[:C].double(), S.rb(want))
    assert bool((full[C:] == 0).all()), "pad lanes"
    assert bool((y_raw.cpu().view(torch.int16).reshape(-1, h, w, 8).permute(0, 3, 1, 2).reshape(-1, h, w)[C:] == 0).all()), "pad lanes' bits"


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("cin,cout,k,s,p,W,H", INT_SHAPES)
def test_integer_maps_forward(cin, cout, k, s, p, W, H, gated):
    """Integers in [-3, 3]: every product and partial sum is an integer below 2^24, so every summation order gives the same
    bits, and bf16 holds the operands exactly; the ONE rounding of a bf16 output is rb of the exact result."""
    g = torch.Generator().manual_seed(100 + cin + cout)
    x, w, b = _ints(g, (cin, H, W)), _ints(g, (cout, cin, k, k)), _ints(g, (cout,))
    gate = torch.randn((cin, H, W), generator=g) if gated else None
    xg = x * (gate > 0) if gated else x
    want = F.conv2d(xg.double()[None], w.double(), b.double(), stride=s, padding=p)[0]
    assert float(want.abs().max()) < 2 ** 24
    for xs, ys in COMBOS:
        y = conv(x, w, b, s, p, relu=False, gate=gate, x_storage=xs, y_storage=ys, raw=True)
        _check_int(y, want, ys)
    # with the ReLU
    y = conv(x, w, b, s, p, relu=True, gate=gate, x_storage="bf16", y_storage="bf16")
    assert torch.equal(y.double(), S.rb(torch.relu(want)))


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("cin,cout,k,s,p,W,H", [c for c in INT_SHAPES if c[3] == 1])
def test_integer_maps_data_gradient(cin, cout, k, s, p, W, H, gated):
    """The transposed run takes `cin` channels and gives `cout`: the layer's own (Cout, Cin) are (cin, cout)."""
    g = torch.Generator().manual_seed(200 + cin + cout)
    x, w = _ints(g, (cin, H, W)), _ints(g, (cin, cout, k, k))
    gate = torch.randn((cin, H, W), generator=g) if gated else None
    xg = x * (gate > 0) if gated else x
    want = F.conv_transpose2d(xg.double()[None], w.double(), stride=1, padding=p)[0]
    for xs, ys in COMBOS:
        y = conv(x, w, None, 1, p, relu=False, transposed=True, gate=gate, x_storage=xs, y_storage=ys, raw=True)
        _check_int(y, want, ys)


# ---------------------------------------------------------------------------
# 2. one convolution on random data, bf16 in and out
# ---------------------------------------------------------------------------
CONV_SHAPES = [(3, 64, 3, 1, 1, 40, 24), (5, 33, 3, 1, 1, 37, 9), (64, 128, 3, 1, 1, 33, 17), (512, 512, 3, 1, 1, 5, 3),
               (3, 64, 11, 4, 2, 67, 35), (64, 192, 5, 1, 2, 67, 35)]


def _conv_inputs(cin, cout, k, H, W):
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn((cin, H, W), generator=g)
    w = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    return g, x, w, torch.randn(cout, generator=g)


@pytest.mark.parametrize("cin,cout,k,s,p,W,H", CONV_SHAPES)
def test_convolution_bf16_in_and_out(cin, cout, k, s, p, W, H):
    _, x, w, b = _conv_inputs(cin, cout, k, H, W)
    ref = B.conv(x, w, b, s, p)                  # fp64 of rb(x), rb(w): the blocked input IS rb(x)
    r32 = B.conv(x, w, b, s, p, dtype=torch.float32)
    y32 = conv(x, w, b, s, p, relu=True, x_storage="bf16", y_storage="fp32")
    e32, e = row_rel_err(r32, ref), row_rel_err(y32, ref)
    print("conv16 bf16 -> fp32 %s: device %.3g, fp32 of the rounded operands %.3g, ratio %.2f of the bar" % ((cin, cout, k, s, p), e, e32, e / bound(e32)))
    assert e <= bound(e32), (e, e32)
    y16 = conv(x, w, b, s, p, relu=True, x_storage="bf16", y_storage="bf16")
    assert torch.equal(y16.double(), S.rb(y32))
    # the blocked input gives the bits of the fp32 input that holds the same values
    assert torch.equal(y32, conv(S.rb(x).float(), w, b, s, p, relu=True))


@pytest.mark.parametrize("cin,cout,k,s,p,W,H", [CONV_SHAPES[1], CONV_SHAPES[2], CONV_SHAPES[3]])
def test_data_gradient_bf16_in_and_out(cin, cout, k, s, p, W, H):
    g, _, w, _ = _conv_inputs(cin, cout, k, H, W)
    gy, gate = torch.randn((cout, H, W), generator=g), torch.randn((cout, H, W), generator=g)
    ref = B.conv_data_grad(gy, w, p, gate)
    r32 = B.conv_data_grad(gy, w, p, gate, dtype=torch.float32)
    y32 = conv(gy, w, None, 1, p, relu=False, transposed=True, gate=gate, x_storage="bf16", y_storage="fp32")
    e32, e = row_rel_err(r32, ref), row_rel_err(y32, ref)
    print("conv16 data gradient bf16 -> fp32 %s: device %.3g, fp32 of the rounded operands %.3g, ratio %.2f of the bar" % ((cin, cout), e, e32, e / bound(e32)))
    assert e <= bound(e32), (e, e32)
    y16 = conv(gy, w, None, 1, p, relu=False, transposed=True, gate=gate, x_storage="bf16", y_storage="bf16")
    assert torch.equal(y16.double(), S.rb(y32))


# ---------------------------------------------------------------------------
# 3. the forward is the operand mode's, rounded once; the value is the head formula of the stored taps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("net,W,H", [("vgg", 40, 24), ("vgg", 33, 17), ("vgg", 16, 16), ("alex", 67, 35)])
def test_forward_identity_and_value(net, W, H):
    ms, wts = model(net)
    mo, _ = model(net, "fp32")
    pred, target, _ = R.images(1, 1, H, W)
    need = net == "vgg"
    vs, _ = ms.values_grad(pred.to(DEV), target.to(DEV), need_grad=need)
    mo.values_grad(pred.to(DEV), target.to(DEV), need_grad=need)
    acts_s, taps_s = stored(ms, net, H, W, need)
    acts_o, taps_o = stored(mo, net, H, W, need)
    for i, (a, b) in enumerate(zip(acts_s, acts_o)):
        assert torch.equal(a.double(), S.rb(b)), (net, i)
    for k, (a, b) in enumerate(zip(taps_s, taps_o)):
        assert torch.equal(a.double(), S.rb(b)), (net, "target tap", k)
    # the value: the head formula on the device's own taps
    _, tap_conv = S.conv_shapes(net, H, W)
    v64 = sum(R.head(acts_s[tap_conv[k]].double(), taps_s[k].double(), wts["lin"][k], torch.float64) for k in range(5))
    v32 = sum(R.head(acts_s[tap_conv[k]], taps_s[k], wts["lin"][k], torch.float32) for k in range(5))
    e32, e = abs(float(v32) - float(v64)) / float(v64), abs(float(vs[0]) - float(v64)) / float(v64)
    print("%s %dx%d value: device %.3g, the formula in fp32 %.3g, ratio %.2f of the bar" % (net, W, H, e, e32, e / bound(e32)))
    assert e <= bound(e32), (e, e32)


# ---------------------------------------------------------------------------
# 4. end to end against the fp64 restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,seed", S.CASES)
def test_end_to_end_against_the_fp64_restatement(W, H, seed):
    c = S.case(W, H, seed)
    m, wts = model("vgg")
    vals, g = m.values_grad(c["pred"].to(DEV), c["target"].to(DEV), need_grad=True, grad_scale=1.0)
    acts, _ = stored(m, "vgg", H, W)
    for i, (a, r) in enumerate(zip(acts, c["f64"]["act"])):
        e = R.rel_err(a, r)
        print("%dx%d seed %d act%d: device %.3g, emulation %.3g, ratio %.2f" % (W, H, seed, i, e, c["act_err"][i], e / c["act_err"][i]))
        assert e <= 2 * c["act_err"][i], (i, e, c["act_err"][i])
    worst = max(S.case(*k)["value_err"] for k in S.CASES)
    ev = abs(float(vals[0]) - c["value64"]) / abs(c["value64"])
    print("%dx%d seed %d value: device %.3g (emulation %.3g here, %.3g at its largest), ratio %.2f" % (W, H, seed, ev, c["value_err"], worst, ev / worst))
    assert ev <= 2 * worst, (ev, worst)
    # the gradient for the device's own decisions: the ReLU masks and the first maxima of its STORED activations
    _, tap_conv = S.conv_shapes("vgg", H, W)
    for k in range(5):
        assert bool(((acts[tap_conv[k]] ** 2).sum(0) > 0).all()), "a pixel with all-zero tap features"
    dec = R.decisions_of("vgg", acts)
    g64 = B.grad64(wts, c["pred"][0], c["target"][0], dec, H, W)
    e, cos = max_rel_err(g[0].cpu(), g64), B.cosine(g[0].cpu(), g64)
    # beside the operand mode on the device
    mo, _ = model("vgg", "fp32")
    vo, go = mo.values_grad(c["pred"].to(DEV), c["target"].to(DEV), need_grad=True, grad_scale=1.0)
    acts_o, _ = stored(mo, "vgg", H, W)
    g64o = B.grad64(wts, c["pred"][0], c["target"][0], R.decisions_of("vgg", acts_o), H, W)
    eo, coso = max_rel_err(go[0].cpu(), g64o), B.cosine(go[0].cpu(), g64o)
    evo = abs(float(vo[0]) - c["value64"]) / abs(c["value64"])
    print("%dx%d seed %d gradient: device %.3g, emulation %.3g, ratio %.2f; cosine %.6f, emulation %.6f, ratio of the defects %.2f; "
          "to the operand mode on the device: value error x%.2f, gradient error x%.2f, cosine defect x%.2f"
          % (W, H, seed, e, c["grad_err"], e / c["grad_err"], cos, c["grad_cos"], (1 - cos) / (1 - c["grad_cos"]), ev / evo, e / eo,
             (1 - cos) / (1 - coso)))
    assert e <= 2 * c["grad_err"], (e, c["grad_err"])
    assert cos >= 1 - 2 * (1 - c["grad_cos"]), (cos, c["grad_cos"])


# ---------------------------------------------------------------------------
# 5. call semantics
# ---------------------------------------------------------------------------
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


def test_accumulate_reproducible_and_views_independent():
    m, _ = model("vgg")
    pred, target, mask = (x.to(DEV) for x in R.images(7, 3, 24, 40))
    v0, g0 = m.values_grad(pred, target, mask, normalize=True, need_grad=True, grad_scale=0.5)
    v0, g0 = v0.clone(), g0.clone()
    assert bool((v0 > 0).all()) and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert bool((g0[mask[:, None].expand_as(g0) == 0] == 0).all())
    v1, g1 = m.values_grad(pred, target, mask, normalize=True, need_grad=True, grad_scale=0.5)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    prior = torch.randn_like(pred)
    acc = prior.clone()
    m.values_grad(pred, target, mask, normalize=True, need_grad=True, grad_scale=0.5, out_grad=acc, accumulate=True)
    assert torch.equal(acc, prior + g0)
    for v in range(3):
        vv, gv = m.values_grad(pred[v:v + 1], target[v:v + 1], mask[v:v + 1], normalize=True, need_grad=True, grad_scale=0.5)
        assert torch.equal(vv[0], v0[v]) and torch.equal(gv[0], g0[v])
    vf, gf = m.values_grad(pred, target, mask, normalize=True, need_grad=False)
    assert gf is None and torch.equal(vf, v0)
    # the mode is in use: the same operands with fp32 storage give other bits, and a smaller workspace is kept
    mo, _ = model("vgg", "fp32")
    vo, _ = mo.values_grad(pred, target, mask, normalize=True, need_grad=True)
    assert not torch.equal(vo, v0)
    assert m._ws.numel() < mo._ws.numel()
    # the autograd surface
    x = pred.clone().requires_grad_(True)
    d = m(x, target)
    v2, g2 = m.values_grad(pred, target, need_grad=True)
    assert torch.equal(d.reshape(-1), v2)
    d.sum().backward()
    assert torch.equal(x.grad, g2)


def test_descent():
    """tests/test_gpu_lpips.py::test_descent in the storage mode: the value falls at every one of 20 steps."""
    m, _ = model("vgg")
    pred, target, _ = (x.to(DEV) for x in R.images(9, 1, 24, 40))
    x = pred.clone()
    v0, g = m.values_grad(x, target, need_grad=True)
    lr = 0.05 * float(v0[0]) / float((g * g).sum())
    last = float(v0[0])
    for _ in range(20):
        x = x - lr * g
        v, g = m.values_grad(x, target, need_grad=True)
        assert float(v[0]) < last, (float(v[0]), last)
        last = float(v[0])

"""GPU: the bf16 operand mode of LPIPS (mgr_lpips_op / mgr_lpips_conv_op with MGR_LPIPS_BF16, k_lp_conv16 of csrc/lpips.hip)
against tests/lpips_bf16_ref.py.

Bars.  One convolution against fp64 OF THE ROUNDED OPERANDS: 8 * max(e32, 2^-23) in row_rel_err, e32 being torch's fp32
convolution of the same rounded operands against that fp64 (the project's rule: what remains is the order of fp32 sums).  End
to end against the fp64 restatement of lpips_ref: 2 x the emulation's own distance (tests/test_lpips_bf16_cpu.py prints it) --
device and emulation round activations that differ in their last fp32 bits, so single operands land one bf16 step apart, and
the sums are random walks over the same number of terms.  Stand-in weights of seed 0.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import lpips_bf16_ref as B
import lpips_ref as R
from util import max_rel_err, row_rel_err

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
DEV = "cuda"
VGG_TAP_CONV = (1, 3, 6, 9, 12)


def bound(e32):
    return 8 * max(e32, EPS)


@functools.lru_cache(maxsize=None)
def model(net, operands="bf16"):
    from manus_amd.lpips import LPIPS
    wts = B.weights(net)
    return LPIPS.from_state_dicts(*R.state_dicts(net, wts), net=net, operands=operands), wts


def device_acts(m, net, H, W, shapes):
    """Every stored activation of pred in the model's workspace (the last view of the last call), through mgr_lpips_layout."""
    from manus_amd.lpips import layout
    lay = layout(net, H, W, True)
    torch.cuda.synchronize()
    ws = m._ws
    out = []
    for off, shape in zip(lay["act"], shapes):
        n = shape[0] * shape[1] * shape[2]
        out.append(ws[off:off + 4 * n].view(torch.float32).reshape(shape).cpu())
    return out


def conv16(x, w, b=None, s=1, p=0, **kw):
    from manus_amd.lpips import conv2d
    return conv2d(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), s, p, operands="bf16",
                  **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}).cpu()


# ---------------------------------------------------------------------------
# 1. exact integer maps
# ---------------------------------------------------------------------------
def _ints(g, shape):
    return torch.randint(-3, 4, shape, generator=g).float()


@pytest.mark.parametrize("cin,cout,k,s,p,W,H", [(3, 64, 3, 1, 1, 40, 24), (5, 33, 3, 1, 1, 37, 9), (8, 65, 3, 1, 1, 31, 5), (17, 1, 3, 1, 1, 33, 1),
                                                (64, 64, 3, 1, 1, 32, 4), (512, 512, 3, 1, 1, 5, 3), (3, 64, 11, 4, 2, 67, 35),
                                                (64, 192, 5, 1, 2, 13, 7)])
def test_integer_maps_forward(cin, cout, k, s, p, W, H):
    """Integers in [-3, 3]: every product and partial sum is an integer below 2^24, so every summation order gives the same
    bits, and bf16 holds the operands exactly."""
    g = torch.Generator().manual_seed(100 + cin + cout)
    x, w, b = _ints(g, (cin, H, W)), _ints(g, (cout, cin, k, k)), _ints(g, (cout,))
    want = F.conv2d(x.double()[None], w.double(), b.double(), stride=s, padding=p)[0]
    assert float(want.abs().max()) < 2 ** 24
    y = conv16(x, w, b, s, p, relu=False)
    assert torch.equal(y, want.float())


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("cin,cout,W,H", [(5, 33, 37, 9), (64, 64, 40, 24), (512, 512, 5, 3)])
def test_integer_maps_data_gradient(cin, cout, W, H, gated):
    """The transposed run takes `cin` channels and gives `cout`: the layer's own (Cout, Cin) are (cin, cout)."""
    g = torch.Generator().manual_seed(200 + cin + cout)
    x, w = _ints(g, (cin, H, W)), _ints(g, (cin, cout, 3, 3))
    gate = torch.randn((cin, H, W), generator=g) if gated else None
    xg = x * (gate > 0) if gated else x
    want = F.conv_transpose2d(xg.double()[None], w.double(), stride=1, padding=1)[0]
    y = conv16(x, w, None, 1, 1, relu=False, transposed=True, gate=gate)
    assert torch.equal(y, want.float())


# ---------------------------------------------------------------------------
# 2. one convolution against fp64 of the rounded operands
# ---------------------------------------------------------------------------
CONV_SHAPES = [(3, 64, 3, 1, 1, 40, 24), (5, 33, 3, 1, 1, 37, 9), (64, 128, 3, 1, 1, 33, 17), (512, 512, 3, 1, 1, 5, 3),
               (3, 64, 11, 4, 2, 67, 35), (64, 192, 5, 1, 2, 67, 35)]


def _conv_inputs(cin, cout, k, H, W):
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn((cin, H, W), generator=g)
    w = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    return g, x, w, torch.randn(cout, generator=g)


@pytest.mark.parametrize("cin,cout,k,s,p,W,H", CONV_SHAPES)
def test_convolution_against_fp64_of_the_rounded_operands(cin, cout, k, s, p, W, H):
    _, x, w, b = _conv_inputs(cin, cout, k, H, W)
    ref = B.conv(x, w, b, s, p)
    r32 = B.conv(x, w, b, s, p, dtype=torch.float32)
    y = conv16(x, w, b, s, p, relu=True)
    e32, e = row_rel_err(r32, ref), row_rel_err(y, ref)
    print("conv16 %s: device %.3g, fp32 of the rounded operands %.3g, ratio %.2f of the bar" % ((cin, cout, k, s, p), e, e32, e / bound(e32)))
    assert e <= bound(e32), (e, e32)


@pytest.mark.parametrize("cin,cout,k,s,p,W,H", [CONV_SHAPES[1], CONV_SHAPES[2], CONV_SHAPES[3]])
def test_data_gradient_against_fp64_of_the_rounded_operands(cin, cout, k, s, p, W, H):
    g, _, w, _ = _conv_inputs(cin, cout, k, H, W)
    gy, gate = torch.randn((cout, H, W), generator=g), torch.randn((cout, H, W), generator=g)
    ref = B.conv_data_grad(gy, w, p, gate)
    r32 = B.conv_data_grad(gy, w, p, gate, dtype=torch.float32)
    y = conv16(gy, w, None, 1, p, relu=False, transposed=True, gate=gate)
    e32, e = row_rel_err(r32, ref), row_rel_err(y, ref)
    print("conv16 data gradient %s: device %.3g, fp32 of the rounded operands %.3g, ratio %.2f of the bar" % ((cin, cout), e, e32, e / bound(e32)))
    assert e <= bound(e32), (e, e32)


# ---------------------------------------------------------------------------
# 3. every stored activation, teacher-forced
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("net,W,H", [("vgg", 40, 24), ("vgg", 33, 17), ("alex", 67, 35)])
def test_every_stored_activation_teacher_forced(net, W, H):
    """Convolution i >= 1 against fp64 on rb of the device's OWN stored input (max-pooled on the host where a pool lies
    between).  Convolution 0's input, the scaled image, is not stored: test_end_to_end judges it."""
    m, wts = model(net)
    pred, target, _ = R.images(1, 1, H, W)
    m.values_grad(pred.to(DEV), target.to(DEV), need_grad=(net == "vgg"))
    shapes = [a.shape for a in R.features(net, wts, torch.zeros((3, H, W)), torch.float32)["act"]]
    acts = device_acts(m, net, H, W, shapes)
    ci, cur = 0, None
    for op in R.OPS[net]:
        if op[0] == "p":
            cur = F.max_pool2d(cur[None], op[1], 2)[0]
            continue
        _, _, _, k, s, p, _ = op
        if ci >= 1:
            ref = B.conv(cur, wts["w"][ci], wts["b"][ci], s, p)
            r32 = B.conv(cur, wts["w"][ci], wts["b"][ci], s, p, dtype=torch.float32)
            e32, e = row_rel_err(r32, ref), row_rel_err(acts[ci], ref)
            print("%s %dx%d act%d: device %.3g, fp32 of the rounded operands %.3g, ratio %.2f of the bar" % (net, W, H, ci, e, e32, e / bound(e32)))
            assert e <= bound(e32), (ci, e, e32)
        cur = acts[ci]
        ci += 1


# ---------------------------------------------------------------------------
# 4. end to end against the fp64 restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,seed", B.CASES)
def test_end_to_end_against_the_fp64_restatement(W, H, seed):
    c = B.case(W, H, seed)
    m, wts = model("vgg")
    vals, g = m.values_grad(c["pred"].to(DEV), c["target"].to(DEV), need_grad=True, grad_scale=1.0)
    acts = device_acts(m, "vgg", H, W, [a.shape for a in c["f64"]["act"]])
    for i, (a, r) in enumerate(zip(acts, c["f64"]["act"])):
        e = R.rel_err(a, r)
        print("%dx%d seed %d act%d: device %.3g, emulation %.3g, ratio %.2f" % (W, H, seed, i, e, c["act_err"][i], e / c["act_err"][i]))
        assert e <= 2 * c["act_err"][i], (i, e, c["act_err"][i])
    worst = max(B.case(*k)["value_err"] for k in B.CASES)
    ev = abs(float(vals[0]) - c["value64"]) / abs(c["value64"])
    print("%dx%d seed %d value: device %.3g (emulation %.3g here, %.3g at its largest), ratio %.2f" % (W, H, seed, ev, c["value_err"], worst, ev / worst))
    assert ev <= 2 * worst, (ev, worst)
    # the gradient for the device's own decisions
    for k in range(5):
        assert bool(((acts[VGG_TAP_CONV[k]] ** 2).sum(0) > 0).all()), "a pixel with all-zero tap features"
    dec = R.decisions_of("vgg", acts)
    g64 = B.grad64(wts, c["pred"][0], c["target"][0], dec, H, W)
    e, cos = max_rel_err(g[0].cpu(), g64), B.cosine(g[0].cpu(), g64)
    print("%dx%d seed %d gradient: device %.3g, emulation %.3g, ratio %.2f; cosine %.6f, emulation %.6f, ratio of the defects %.2f"
          % (W, H, seed, e, c["grad_err"], e / c["grad_err"], cos, c["grad_cos"], (1 - cos) / (1 - c["grad_cos"])))
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
    v0, g0 = m.values_grad(pred, target, mask, need_grad=True, grad_scale=0.5)
    v0, g0 = v0.clone(), g0.clone()
    assert bool((v0 > 0).all()) and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    v1, g1 = m.values_grad(pred, target, mask, need_grad=True, grad_scale=0.5)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    prior = torch.randn_like(pred)
    acc = prior.clone()
    m.values_grad(pred, target, mask, need_grad=True, grad_scale=0.5, out_grad=acc, accumulate=True)
    assert torch.equal(acc, prior + g0)
    for v in range(3):
        vv, gv = m.values_grad(pred[v:v + 1], target[v:v + 1], mask[v:v + 1], need_grad=True, grad_scale=0.5)
        assert torch.equal(vv[0], v0[v]) and torch.equal(gv[0], g0[v])
    vf, gf = m.values_grad(pred, target, mask, need_grad=False)
    assert gf is None and torch.equal(vf, v0)
    # the mode is in use: the fp32 object gives other bits
    vf32, _ = model("vgg", "fp32")[0].values_grad(pred, target, mask, need_grad=False)
    assert not torch.equal(vf32, v0)


def test_autograd_surface_matches_the_direct_call():
    from manus_amd import losses
    from manus_amd._lib import ManusHipError
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
    assert not m(pred, target).requires_grad
    a, _ = model("alex")
    pa, ta, _ = (t.to(DEV) for t in R.images(8, 1, 35, 67))
    assert a(pa, ta).shape == (1, 1, 1, 1)
    with pytest.raises(ManusHipError, match="forward only"):
        a(pa.clone().requires_grad_(True), ta)
    hwc = pred[0].permute(1, 2, 0).contiguous().requires_grad_(True)
    loss = losses.lpips_loss(hwc, target[:1].permute(0, 2, 3, 1), m)
    assert torch.equal(loss, vals[0])
    loss.backward()
    assert torch.equal(hwc.grad, g[0].permute(1, 2, 0))


def test_fp32_operands_give_the_bits_of_the_existing_entries():
    """LPIPS(operands="fp32") and the *_op entries with MGR_LPIPS_F32 against mgr_lpips_net_pack / mgr_lpips / mgr_lpips_conv."""
    import ctypes
    from manus_amd import _lib
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.lpips import CONV_INDEX, TAP_CHANNELS, conv2d
    L = lib()
    m, wts = model("vgg", "fp32")
    assert m.operands == "fp32"
    pred, target, mask = (x.to(DEV) for x in R.images(7, 2, 24, 40))
    v_new, g_new = m.values_grad(pred, target, mask, need_grad=True, grad_scale=0.5)
    # the existing entries by hand
    sd, lin = R.state_dicts("vgg", wts)
    ws_ = [sd["features.%d.weight" % i].to(DEV).contiguous() for i in CONV_INDEX["vgg"]]
    bs_ = [sd["features.%d.bias" % i].to(DEV).contiguous() for i in CONV_INDEX["vgg"]]
    ls_ = [lin["lin%d.model.1.weight" % k].to(DEV).contiguous() for k in range(len(TAP_CHANNELS["vgg"]))]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    nbytes = int(L.mgr_lpips_net_bytes(0))
    assert nbytes == m.blob.numel() == int(L.mgr_lpips_net_bytes_op(0, _lib.MGR_LPIPS_F32))
    blob = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    check(L.mgr_lpips_net_pack(0, arr(ws_), arr(bs_), arr(ls_), ptr(blob), nbytes, stream()), "mgr_lpips_net_pack")
    wsz = int(L.mgr_lpips_workspace_bytes(0, 24, 40, 1))
    work = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    v_old, g_old = torch.empty(2, device=DEV), torch.empty_like(pred)
    check(L.mgr_lpips(0, 2, 24, 40, ptr(pred), ptr(target), ptr(mask), ptr(blob), nbytes, 0, 0.5, ptr(v_old), ptr(g_old), 0, ptr(work), wsz,
                      stream()), "mgr_lpips")
    torch.cuda.synchronize()
    assert torch.equal(v_new, v_old) and torch.equal(g_new, g_old)
    # one convolution
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn((5, 9, 37), generator=g).to(DEV), torch.randn((33, 5, 3, 3), generator=g).to(DEV), torch.randn(33, generator=g).to(DEV)
    y_new = conv2d(x, w, b, 1, 1, operands="fp32")
    y_def = conv2d(x, w, b, 1, 1)
    n = int(L.mgr_lpips_conv_scratch_bytes(5, 33, 3, 3))
    scratch, y_old = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty_like(y_new)
    check(L.mgr_lpips_conv(5, 33, 9, 37, 3, 3, 1, 1, ptr(x), None, ptr(w), ptr(b), 1, 0, ptr(y_old), ptr(scratch), n, stream()), "mgr_lpips_conv")
    assert torch.equal(y_new, y_old) and torch.equal(y_def, y_old)


# ---------------------------------------------------------------------------
# 6. descent
# ---------------------------------------------------------------------------
def test_descent_in_both_modes():
    """tests/test_gpu_lpips.py::test_descent in both modes: the bf16 gradient must remove at least half of the value reduction
    the fp32 run (the parent's code, the yardstick) removes in its 20 steps."""
    pred, target, _ = (x.to(DEV) for x in R.images(9, 1, 24, 40))
    removed = {}
    for operands in ("fp32", "bf16"):
        m, _ = model("vgg", operands)
        x = pred.clone()
        v0, g = m.values_grad(x, target, need_grad=True)
        first = float(v0[0])
        lr = 0.05 * first / float((g * g).sum())
        for _ in range(20):
            x = x - lr * g
            v, g = m.values_grad(x, target, need_grad=True)
        removed[operands] = (first - float(v[0])) / first
        print("descent %s: %.6g -> %.6g, %.4f of the value removed" % (operands, first, float(v[0]), removed[operands]))
    assert removed["fp32"] > 0
    assert removed["bf16"] >= 0.5 * removed["fp32"], removed

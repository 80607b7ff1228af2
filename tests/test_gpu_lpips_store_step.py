"""GPU: the LPIPS term in bf16 storage mode on the training step (HipViewCompute(lpips=LPIPS(operands="bf16", storage="bf16")),
both routes), with windows, cached target taps and batches, and a model swap.  The scene of tests/test_gpu_lpips_step.py: 64x48,
2000 Gaussians, 3 views; stand-in weights (tests/lpips_ref.py).

Fused against modular with the term on is printed, and asserted at the fp32 bar of 1e-4 only where the two routes' loss_lpips
agree bit for bit: the routes' images differ in their last bits, which moves bf16 roundings of the first layer's input
(tests/test_gpu_lpips_bf16_step.py has the caveat).
"""
import functools

import pytest
import torch

import lpips_ref as R
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, W, H, N = 3, 64, 48, 2000
IDS = list(range(V))
RECTS = [(8, 6, 40, 30), (0, 0, 32, 24), (23, 17, 40, 30)]
KW = dict(loss="l1+ssim", persistent_grads=False)


@functools.lru_cache(maxsize=None)
def net(storage="bf16"):
    from manus_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(*R.state_dicts("vgg", R.make_weights("vgg", 0)), net="vgg", operands="bf16", storage=storage)


@functools.lru_cache(maxsize=None)
def scene():
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=N, kind="hand", seed=6, grid_res=24, n_cameras=V, width=W, height=H, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device=DEV)
    g = torch.Generator().manual_seed(11)
    return sc, camera_table(sc["cameras"], DEV), torch.rand((V, 3, H, W), generator=g).to(DEV), torch.rand((V, 3, H, W), generator=g).to(DEV)


def clone_out(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def compute(fused, targets=None, lpips=None, **kw):
    from manus_amd.engine import HipViewCompute
    sc, ct, tg, _ = scene()
    return HipViewCompute(sc, tg if targets is None else targets, ct, fused=fused, lpips=net() if lpips is None else lpips, w_lpips=0.1, **KW,
                          **kw)


def step(hc):
    return clone_out(hc(IDS, 1.0 / V))


def same(a, b, what):
    for k in ("loss", "loss_lpips", "grad2d", "vis", "radii"):
        assert torch.equal(a[k], b[k]), (what, k)
    for k, g in b["grads"].items():
        assert torch.equal(a["grads"][k], g), (what, k)


def test_the_term_on_both_routes():
    from manus_amd.engine import HipViewCompute
    sc, ct, tg, _ = scene()
    lp = net()
    assert (lp.operands, lp.storage) == ("bf16", "bf16")
    outs = {}
    for fused in (True, False):
        off = clone_out(HipViewCompute(sc, tg, ct, fused=fused, **KW)(IDS, 1.0 / V))
        hc = compute(fused)
        on = step(hc)
        outs[fused] = on
        # the term's value: scale * sum_v d_v of a direct call of the same object on the step's image, in the step's arithmetic
        if fused:
            img = hc.last_image
        else:
            with torch.no_grad():
                img = hc.forward_views(IDS)[0]
        direct = float(lp.values_grad(img.detach().contiguous(), tg, need_grad=False)[0].sum() * (1.0 / V))
        got = float(on["loss_lpips"])
        print("fused %s: loss_lpips %.9e, direct %.9e" % (fused, got, direct))
        assert got > 0 and abs(got - direct) <= 5e-8 * direct
        assert abs(float(on["loss"]) - (float(off["loss"]) + 0.1 * got)) <= 1e-6 * abs(float(on["loss"]))
        for k, g in on["grads"].items():
            assert bool(torch.isfinite(g).all()), k
            assert not torch.equal(g, off["grads"][k]), (fused, k)
        assert not torch.equal(on["grad2d"], off["grad2d"])
        assert torch.equal(on["vis"], off["vis"])
        # the mode is in use: the fp32-storage object gives another term
        assert float(step(compute(fused, lpips=net("fp32")))["loss_lpips"]) != got
    of, om = outs[True], outs[False]
    bitwise = torch.equal(of["loss_lpips"], om["loss_lpips"])
    print("bf16 storage, term on: loss fused %.7e modular %.7e; loss_lpips fused %.9e modular %.9e (relative difference %.3g, bit for bit: %s)"
          % (float(of["loss"]), float(om["loss"]), float(of["loss_lpips"]), float(om["loss_lpips"]),
             abs(float(of["loss_lpips"]) - float(om["loss_lpips"])) / float(om["loss_lpips"]), bitwise))
    errs = {k: max_rel_err(of["grads"][k].cpu().numpy(), g.cpu().numpy()) for k, g in om["grads"].items()}
    errs["grad2d"] = max_rel_err(of["grad2d"].cpu().numpy(), om["grad2d"].cpu().numpy())
    for k, e in errs.items():
        print("%-16s fused against modular %.3g" % (k, e))
    if bitwise:
        assert all(e <= 1e-4 for e in errs.values()), errs


@functools.lru_cache(maxsize=None)
def windowed(fused):
    return step(compute(fused, lpips_rects=RECTS))


@pytest.mark.parametrize("fused", [True, False])
def test_cached_targets_and_batches_change_no_bit(fused):
    sc, ct, tg, other = scene()
    ref = windowed(fused)
    assert float(ref["loss_lpips"]) > 0
    hc = compute(fused, targets=tg.clone(), lpips_rects=RECTS, lpips_cache_targets=True, lpips_batch=8)
    same(step(hc), ref, "first step")
    taps = hc._cache[tuple(IDS)]["lpips"]["taps"]
    assert taps is not None and taps.storage == "bf16" and taps.nbytes > 0
    same(step(hc), ref, "second step")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is taps
    hc.lpips_batch = 0
    same(step(hc), ref, "batch switched off on kept taps")
    hc.lpips_cache_targets = False
    same(step(hc), ref, "cache switched off")
    hc.lpips_cache_targets, hc.lpips_batch = True, 8
    # new targets
    hc.targets.data.copy_(other)
    torch.cuda.synchronize()
    hc.view_constants_changed()
    fresh = step(compute(fused, targets=other, lpips_rects=RECTS))
    assert float(fresh["loss_lpips"]) != float(ref["loss_lpips"])
    same(step(hc), fresh, "after new targets")
    same(step(hc), fresh, "after new targets, second step")


@pytest.mark.parametrize("fused", [True, False])
def test_a_model_of_the_other_storage_rebuilds_the_taps(fused):
    ref16, ref32 = windowed(fused), step(compute(fused, lpips=net("fp32"), lpips_rects=RECTS))
    assert float(ref16["loss_lpips"]) != float(ref32["loss_lpips"])
    hc = compute(fused, lpips_rects=RECTS, lpips_cache_targets=True, lpips_batch=8)
    same(step(hc), ref16, "bf16 storage")
    taps = hc._cache[tuple(IDS)]["lpips"]["taps"]
    assert taps.storage == "bf16"
    for lp, ref, storage in ((net("fp32"), ref32, "fp32"), (net(), ref16, "bf16")):
        hc.lpips = lp
        same(step(hc), ref, "swapped to %s storage" % storage)       # neither refused by TargetTaps.matches nor reused
        now = hc._cache[tuple(IDS)]["lpips"]["taps"]
        assert now is not taps and now.storage == storage
        taps = now
    assert taps.nbytes < ref_bytes(net("fp32"))


def ref_bytes(lp):
    return lp.target_taps(scene()[2], RECTS).nbytes

"""GPU: the LPIPS term in bf16 operand mode on the training step (HipViewCompute(lpips=LPIPS(..., operands="bf16")), both
routes), the Trainer's start_lpips_iter and the LPIPS column of the validation pass.  The scene of tests/test_gpu_lpips_step.py:
64x48, 2000 Gaussians, 3 views; stand-in weights (tests/lpips_ref.py).

Fused against modular with the term on is printed, not asserted: the two routes' images differ in their last bits, which moves
bf16 roundings of the first layer's input, so the fp32 bar of 1e-4 has no claim on it.
"""
import csv
import functools
import os

import pytest
import torch

import lpips_ref as R
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, W, H, N = 3, 64, 48, 2000


@functools.lru_cache(maxsize=None)
def net(name):
    from manus_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(*R.state_dicts(name, R.make_weights(name, 0)), net=name, operands="bf16")


@functools.lru_cache(maxsize=None)
def scene():
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=N, kind="hand", seed=6, grid_res=24, n_cameras=V, width=W, height=H, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device=DEV)
    g = torch.Generator().manual_seed(11)
    return sc, camera_table(sc["cameras"], DEV), torch.rand((V, 3, H, W), generator=g).to(DEV)


def clone_out(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def test_the_term_on_both_routes():
    from manus_amd.engine import HipViewCompute
    sc, ct, tg = scene()
    ids = list(range(V))
    lp = net("vgg")
    assert lp.operands == "bf16"
    outs = {}
    for fused in (True, False):
        kw = dict(fused=fused, loss="l1+ssim", persistent_grads=False)
        off = clone_out(HipViewCompute(sc, tg, ct, **kw)(ids, 1.0 / V))
        hc = HipViewCompute(sc, tg, ct, lpips=lp, w_lpips=0.1, **kw)
        on = clone_out(hc(ids, 1.0 / V))
        outs[fused] = on
        # the term's value: scale * sum_v d_v of a direct call of the same object on the step's image
        if fused:
            img = hc.last_image
        else:
            with torch.no_grad():
                img = hc.forward_views(ids)[0]
        direct = float(lp.values_grad(img.detach().contiguous(), tg, need_grad=False)[0].sum()) / V
        got = float(on["loss_lpips"])
        print("fused %s: loss_lpips %.7e, direct %.7e" % (fused, got, direct))
        assert got > 0 and abs(got - direct) <= 1e-6 * direct
        assert abs(float(on["loss"]) - (float(off["loss"]) + 0.1 * got)) <= 1e-6 * abs(float(on["loss"]))
        # the term reaches every leaf, and grad2d through the image
        for k, g in on["grads"].items():
            assert bool(torch.isfinite(g).all()), k
            assert not torch.equal(g, off["grads"][k]), (fused, k)
        assert not torch.equal(on["grad2d"], off["grad2d"])
        assert torch.equal(on["vis"], off["vis"])
    # a measurement, not a check (see the module docstring)
    of, om = outs[True], outs[False]
    print("bf16 term on: loss fused %.7e modular %.7e; loss_lpips fused %.7e modular %.7e (relative difference %.3g)"
          % (float(of["loss"]), float(om["loss"]), float(of["loss_lpips"]), float(om["loss_lpips"]),
             abs(float(of["loss_lpips"]) - float(om["loss_lpips"])) / float(om["loss_lpips"])))
    for k, g in om["grads"].items():
        print("%-16s fused against modular %.3g" % (k, max_rel_err(of["grads"][k].cpu().numpy(), g.cpu().numpy())))
    print("grad2d fused against modular %.3g" % max_rel_err(of["grad2d"].cpu().numpy(), om["grad2d"].cpu().numpy()))


def test_trainer_schedule():
    from manus_amd.engine import HipViewCompute, Trainer
    sc, ct, tg = scene()
    opts = dict(densify_from_step=1000, densification_interval=1000, densify_until_step=2000, opacity_reset_interval=100000)
    compute = HipViewCompute(sc, tg, ct, loss="l1+ssim", lpips=net("vgg"), w_lpips=0.1)
    t = Trainer(compute, V, extent=0.3, opts=opts, spatial_lr_scale=0.05, bg_white=False, start_lpips_iter=2)
    for step in range(4):
        out = t.train_step()
        if step < 2:
            assert "loss_lpips" not in out and compute.last_lpips is None and not compute.lpips_on, step
        else:
            assert float(out["loss_lpips"]) > 0 and compute.last_lpips is not None and compute.lpips_on, step
    with pytest.raises(ValueError, match="forward only"):
        HipViewCompute(sc, tg, ct, lpips=net("alex"), w_lpips=0.1)


def test_validation_fills_the_csv_column(tmp_path):
    from manus_amd.engine import HipViewCompute, Trainer
    from manus_amd.validation import Validator
    from manus_amd.synthetic import camera_table, make_scene
    Wv, Hv = 80, 48                 # AlexNet needs 67x35 at least
    sc = make_scene(n_gaussians=N, kind="hand", seed=6, grid_res=24, n_cameras=V, width=Wv, height=Hv, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device=DEV)
    ct = camera_table(sc["cameras"], DEV)
    g = torch.Generator().manual_seed(12)
    tg = torch.rand((V, 3, Hv, Wv), generator=g).to(DEV)
    masks = (torch.rand((V, Hv, Wv), generator=g) * 3 - 1).clamp(0, 1).to(DEV)
    opts = dict(densify_from_step=1000, densification_interval=1000, densify_until_step=2000, opacity_reset_interval=100000)
    t = Trainer(HipViewCompute(sc, tg, ct, loss="l1+ssim"), V, extent=0.3, opts=opts, spatial_lr_scale=0.05, bg_white=False)
    alex = net("alex")
    val = Validator(str(tmp_path), "exp")
    val.start()
    res = t.validate([2, 0, 1], masks=masks, validator=val, group=2, lpips=alex)
    row = val.end(0)
    with torch.no_grad():
        img = torch.cat([t.compute.forward_views([2, 0])[0], t.compute.forward_views([1])[0]])
    direct = alex.values_grad(img, tg[[2, 0, 1]].contiguous(), masks, need_grad=False)[0].cpu().tolist()
    assert res["lpips"] == direct and all(d > 0 for d in direct)
    with open(os.path.join(str(tmp_path), "val_results", "val_results.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0][4] == "lpips" and abs(float(rows[1][4]) - sum(direct) / V) <= 1e-12 and abs(float(row[4]) - sum(direct) / V) <= 1e-12

"""GPU: the LPIPS term on the training step (HipViewCompute(lpips=, w_lpips=), both routes), the Trainer's start_lpips_iter and
the LPIPS column of the validation pass.  64x48, 2000 Gaussians, 3 views; stand-in weights (tests/lpips_ref.py).

The fused route adds the term's gradient into dL/dimage, which the image loss leaves unwritten under empty background tiles:
that buffer itself is not compared, only what the backward makes of it.
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
BAR = 1e-4          # the repository's fused-against-modular bar on leaf gradients (max-rel-err)


@functools.lru_cache(maxsize=None)
def net(name):
    from manus_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(*R.state_dicts(name, R.make_weights(name, 0)), net=name)


@functools.lru_cache(maxsize=None)
def scene():
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=N, kind="hand", seed=6, grid_res=24, n_cameras=V, width=W, height=H, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device=DEV)
    g = torch.Generator().manual_seed(11)
    return sc, camera_table(sc["cameras"], DEV), torch.rand((V, 3, H, W), generator=g).to(DEV)


def clone_out(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


@pytest.mark.parametrize("fused", [True, False])
def test_off_means_off(fused):
    from manus_amd.engine import HipViewCompute
    sc, ct, tg = scene()
    ids = list(range(V))
    kw = dict(fused=fused, loss="l1+ssim", persistent_grads=False)
    ref = clone_out(HipViewCompute(sc, tg, ct, **kw)(ids, 1.0 / V))
    gated = HipViewCompute(sc, tg, ct, lpips=net("vgg"), w_lpips=0.1, **kw)
    gated.lpips_on = False
    for name, hc in (("lpips_on False", gated), ("w_lpips 0", HipViewCompute(sc, tg, ct, lpips=net("vgg"), w_lpips=0.0, **kw))):
        out = hc(ids, 1.0 / V)
        assert "loss_lpips" not in out and hc.last_lpips is None, name
        assert torch.equal(out["loss"], ref["loss"]), name
        for k in ("grad2d", "vis", "radii"):
            assert torch.equal(out[k], ref[k]), (name, k)
        for k, g in ref["grads"].items():
            assert torch.equal(out["grads"][k], g), (name, k)
    # and the gate opens again
    gated.lpips_on = True
    out = gated(ids, 1.0 / V)
    assert float(out["loss_lpips"]) > 0 and not torch.equal(out["grads"]["_features_dc"], ref["grads"]["_features_dc"])


def test_fused_against_modular_with_the_term_on():
    from manus_amd.engine import HipViewCompute
    sc, ct, tg = scene()
    ids = list(range(V))
    outs = {}
    for fused in (True, False):
        for w in (0.0, 0.1):
            hc = HipViewCompute(sc, tg, ct, fused=fused, loss="l1+ssim", persistent_grads=False, lpips=net("vgg"), w_lpips=w)
            outs[fused, w] = clone_out(hc(ids, 1.0 / V))
    of, om = outs[True, 0.1], outs[False, 0.1]
    # the term's value: scale * sum_v d_v of a direct call on the step's image
    hc = HipViewCompute(sc, tg, ct, fused=True, loss="l1+ssim", persistent_grads=False)
    hc(ids, 1.0 / V)
    direct = net("vgg").values_grad(hc.last_image, tg, need_grad=False)[0].sum() / V
    assert abs(float(of["loss_lpips"]) - float(direct)) <= 1e-6 * float(direct)
    for o, off in ((of, outs[True, 0.0]), (om, outs[False, 0.0])):
        assert abs(float(o["loss"]) - (float(off["loss"]) + 0.1 * float(o["loss_lpips"]))) <= 1e-6 * abs(float(o["loss"]))
    a, b = float(of["loss"]), float(om["loss"])
    print("loss fused %.7e modular %.7e; lpips term %.6e" % (a, b, float(of["loss_lpips"])))
    assert abs(a - b) <= BAR * abs(b)
    worst = 0.0
    for k, g in om["grads"].items():
        e = max_rel_err(of["grads"][k].cpu().numpy(), g.cpu().numpy())
        # what the term adds to this leaf, against the same step with the term off (a measurement: the term must reach the leaf)
        share = max_rel_err(g.cpu().numpy(), outs[False, 0.0]["grads"][k].cpu().numpy())
        print("%-16s fused against modular %.3g; the term changes it by %.3g of its maximum" % (k, e, share))
        worst = max(worst, e)
    e2d = max_rel_err(of["grad2d"].cpu().numpy(), om["grad2d"].cpu().numpy())
    print("grad2d fused against modular %.3g" % e2d)
    assert worst < BAR, worst
    assert e2d < BAR, e2d
    assert torch.equal(of["vis"], om["vis"])
    # the gradient travels through the image: grad2d sees the term on both routes
    for fused in (True, False):
        assert not torch.equal(outs[fused, 0.1]["grad2d"], outs[fused, 0.0]["grad2d"])


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
    # no network: the schedule has no effect
    plain = HipViewCompute(sc, tg, ct, loss="l1+ssim")
    t = Trainer(plain, V, extent=0.3, opts=opts, spatial_lr_scale=0.05, bg_white=False, start_lpips_iter=0)
    assert "loss_lpips" not in t.train_step() and plain.lpips_on
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
    # ... which are the values of the masked images
    plain = alex.values_grad(img * masks[:, None], tg[[2, 0, 1]] * masks[:, None], need_grad=False)[0].cpu().tolist()
    assert plain == direct
    with open(os.path.join(str(tmp_path), "val_results", "val_results.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0][4] == "lpips" and abs(float(rows[1][4]) - sum(direct) / V) <= 1e-12 and abs(float(row[4]) - sum(direct) / V) <= 1e-12
    # without a network the field stays empty
    val2 = Validator(str(tmp_path / "b"), "exp")
    val2.start()
    res2 = t.validate([0], validator=val2)
    assert "lpips" not in res2 and val2.end(0)[4] == ""

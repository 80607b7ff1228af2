"""GPU: the spatial SSIM on the training step (HipViewCompute(ssim=), both routes), on the validation pass and under a
Trainer.  64x48, 2000 Gaussians, 3 views: the scene of the other step tests; stand-in LPIPS weights (tests/lpips_ref.py).
"""
import csv
import functools
import os

import pytest
import torch

import lpips_ref as LR
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, W, H, N = 3, 64, 48, 2000
BAR = 1e-4          # the repository's fused-against-modular bar on leaf gradients (max-rel-err)
OPTS = dict(densify_from_step=1000, densification_interval=1000, densify_until_step=2000, opacity_reset_interval=100000)


@functools.lru_cache(maxsize=None)
def scene():
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=N, kind="hand", seed=6, grid_res=24, n_cameras=V, width=W, height=H, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device=DEV)
    g = torch.Generator().manual_seed(11)
    return sc, camera_table(sc["cameras"], DEV), torch.rand((V, 3, H, W), generator=g).to(DEV)


@functools.lru_cache(maxsize=None)
def vgg():
    from manus_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(*LR.state_dicts("vgg", LR.make_weights("vgg", 0)), net="vgg")


def clone_out(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def step(**kw):
    from manus_amd.engine import HipViewCompute
    sc, ct, tg = scene()
    kw.setdefault("loss", "l1+ssim")
    hc = HipViewCompute(sc, tg, ct, persistent_grads=False, **kw)
    return hc, clone_out(hc(list(range(V)), 1.0 / V))


def compare(a, b, what, grad2d=True):
    """fused (a) against modular (b): loss, leaf gradients, grad2d at the bar; vis equal.  -> the worst leaf error.
    grad2d=False with a map term on: there the fused route's grad2d stays the colour loss's statistic and the modular
    route's includes the map term (HipViewCompute's docstring), whatever the SSIM kind."""
    la, lb = float(a["loss"]), float(b["loss"])
    print("%s: loss fused %.7e modular %.7e" % (what, la, lb))
    assert abs(la - lb) <= BAR * abs(lb)
    worst = 0.0
    for k, g in b["grads"].items():
        e = max_rel_err(a["grads"][k].cpu().numpy(), g.cpu().numpy())
        print("%s: %-16s fused against modular %.3g" % (what, k, e))
        worst = max(worst, e)
    e2d = max_rel_err(a["grad2d"].cpu().numpy(), b["grad2d"].cpu().numpy()) if grad2d else 0.0
    print("%s: grad2d fused against modular %.3g" % (what, e2d))
    assert worst < BAR and e2d < BAR, (worst, e2d)
    assert torch.equal(a["vis"], b["vis"])
    return worst


@pytest.mark.parametrize("fused", [True, False])
def test_rows_is_the_step_without_the_keyword(fused):
    _, ref = step(fused=fused)
    _, out = step(fused=fused, ssim="rows")
    assert "loss_ssim" not in out and set(out) == set(ref)
    assert torch.equal(out["loss"], ref["loss"])
    for k in ("grad2d", "vis", "radii"):
        assert torch.equal(out[k], ref[k]), k
    for k, g in ref["grads"].items():
        assert torch.equal(out["grads"][k], g), k
    # loss="l1": the attribute has no effect (the L1 kernel folds its workgroups' sums with a float atomic, so the VALUE of two
    # runs agrees to rounding, not in its bits; the gradients are sign / n and what the backward makes of them: equal bits)
    _, l1 = step(fused=fused, loss="l1")
    _, l1s = step(fused=fused, loss="l1", ssim="spatial")
    assert "loss_ssim" not in l1s and abs(float(l1["loss"]) - float(l1s["loss"])) <= 1e-6 * abs(float(l1["loss"]))
    for k, g in l1["grads"].items():
        assert torch.equal(l1s["grads"][k], g), k


def test_spatial_step_on_both_routes():
    """Measured on an MI355X: fused against modular, worst leaf 1.1e-6, grad2d 1.9e-7 (figures: DESIGN.md section 6, row f20)."""
    from manus_amd import ops
    _, _, tg = scene()
    hc, of = step(fused=True, ssim="spatial")
    _, om = step(fused=False, ssim="spatial")
    # the value: scale * sum_v [w_rgb mean|d_v| + w_ssim (1 - mean S_v)] of a direct call on the step's image
    _, vs, _ = ops.image_loss2d_grad(hc.last_image, tg, need_grad=False)
    n = float(3 * H * W)
    vs = vs.double().cpu()
    direct = float((0.8 * vs[:, 0] / n + 0.2 * (1.0 - vs[:, 1] / n)).sum() / V)
    term = float((1.0 - vs[:, 1] / n).sum() / V)
    print("loss %.7e direct %.7e; loss_ssim %.7e direct %.7e" % (float(of["loss"]), direct, float(of["loss_ssim"]), term))
    assert abs(float(of["loss"]) - direct) <= 1e-6 * abs(direct)
    for o in (of, om):
        assert abs(float(o["loss_ssim"]) - term) <= 1e-5 * abs(term)
    compare(of, om, "spatial")
    # it is another loss than the rows variant
    _, rows = step(fused=True)
    assert abs(float(rows["loss"]) - float(of["loss"])) > 1e-4 * abs(float(rows["loss"]))
    # the attribute is settable after construction, and asked at the step
    hc.ssim = "rows"
    out = hc(list(range(V)), 1.0 / V)
    assert "loss_ssim" not in out and torch.equal(out["loss"], rows["loss"])
    hc.ssim = "both"
    with pytest.raises(ValueError, match="ssim must be"):
        hc(list(range(V)), 1.0 / V)


def test_the_term_reaches_the_leaves():
    """Against the same step with w_ssim = 0: the share of each leaf's maximum that the term changes.  Measured on an
    MI355X: DESIGN.md section 6, row f20.  The colour leaf must move by at least 1 % of its maximum: the term carries a
    fifth of the loss weight and its per-pixel gradient is of the order of the L1 term's."""
    for fused in (True, False):
        _, on = step(fused=fused, ssim="spatial")
        _, off = step(fused=fused, ssim="spatial", w_ssim=0.0)
        shares = {k: max_rel_err(on["grads"][k].cpu().numpy(), g.cpu().numpy()) for k, g in off["grads"].items()}
        print("fused %s: the term changes " % fused + ", ".join("%s by %.3g" % kv for kv in shares.items()))
        assert shares["_features_dc"] >= 1e-2 and all(v > 0 for v in shares.values())
        assert not torch.equal(on["grad2d"], off["grad2d"])      # it travels through the image


def test_with_a_mask_term_and_lpips_on():
    g = torch.Generator().manual_seed(13)
    masks = (torch.rand((V, H, W), generator=g) > 0.5).float().to(DEV)
    kw = dict(ssim="spatial", mask_targets=masks, w_mask=0.5, lpips=vgg(), w_lpips=0.1)
    _, of = step(fused=True, **kw)
    _, om = step(fused=False, **kw)
    for o in (of, om):
        assert float(o["loss_lpips"]) > 0 and float(o["loss_mask"]) > 0 and float(o["loss_ssim"]) > 0
    compare(of, om, "spatial + mask + lpips", grad2d=False)


def trainer(**kw):
    from manus_amd.engine import HipViewCompute, Trainer
    sc, ct, tg = scene()
    return Trainer(HipViewCompute(sc, tg, ct, loss="l1+ssim", **kw), V, extent=0.3, opts=OPTS, spatial_lr_scale=0.05, bg_white=False)


def test_validate_spatial_is_the_direct_call_per_view(tmp_path):
    from manus_amd import ops
    from manus_amd.validation import Validator, validation_step
    _, _, tg = scene()
    g = torch.Generator().manual_seed(12)
    masks = (torch.rand((V, H, W), generator=g) * 3 - 1).clamp(0, 1).to(DEV)
    t = trainer()
    ids = [2, 0, 1]
    val = Validator(str(tmp_path), "exp")
    val.start()
    res = t.validate(ids, masks=masks, validator=val, group=2, ssim="spatial")
    row = val.end(0)
    with torch.no_grad():
        img = torch.cat([t.compute.forward_views([2, 0])[0], t.compute.forward_views([1])[0]])
    tgt = tg[ids].contiguous()
    _, vs, _ = ops.image_loss2d_grad(img, tgt, 0.0, 1.0, mask=masks, need_grad=False)
    direct = (vs[:, 1] / float(3 * H * W)).cpu().tolist()
    assert res["ssim"] == direct and res["ssim_kind"] == "spatial"
    # ... which are the values of the masked images
    _, vp, _ = ops.image_loss2d_grad(img * masks[:, None], tgt * masks[:, None], 0.0, 1.0, need_grad=False)
    assert torch.equal(vp, vs)
    with open(os.path.join(str(tmp_path), "val_results", "val_results.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0][3] == "ssim" and abs(float(rows[1][3]) - sum(direct) / V) <= 1e-12 and abs(float(row[3]) - sum(direct) / V) <= 1e-12
    # without the keyword: unchanged -- the rows statistic of eval.hip; PSNR and the triptych do not depend on the kind
    plain = t.validate(ids, masks=masks, group=2)
    rows_res = t.validate(ids, masks=masks, group=2, ssim="rows")
    ss = ops.eval_views(img, tgt, masks)[1]
    assert plain["ssim"] == (ss / float(3 * H * W)).cpu().tolist() == rows_res["ssim"] and plain["ssim_kind"] == "rows"
    assert plain["ssim"] != res["ssim"] and plain["psnr"] == res["psnr"] and torch.equal(plain["images"], res["images"])
    # the single-view form
    batch = {"rgb": tgt[0].permute(1, 2, 0).contiguous(), "mask": masks[0][..., None]}
    one = validation_step(img[0].permute(1, 2, 0).contiguous(), batch, ssim="spatial")
    assert float(one["ssim"]) == direct[0] and one["ssim_kind"] == "spatial"
    old = validation_step(img[0].permute(1, 2, 0).contiguous(), batch)
    assert float(old["ssim"]) == plain["ssim"][0] and old["ssim_kind"] == "rows" and torch.equal(old["image"], one["image"])


def test_a_trainer_runs_with_the_spatial_term():
    t = trainer(ssim="spatial")
    outs = [t.train_step() for _ in range(3)]
    losses = [float(o["loss"]) for o in outs]
    print("losses", losses, "loss_ssim", [float(o["loss_ssim"]) for o in outs])
    assert all("loss_ssim" in o for o in outs)
    assert losses[2] < losses[0]

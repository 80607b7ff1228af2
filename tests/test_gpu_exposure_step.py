"""GPU: the per-camera exposure on the training step (HipViewCompute(exposure=, exposure_ids=), both routes).  64x48, 2000
Gaussians, 3 views: the scene of the other step tests; stand-in LPIPS weights (tests/lpips_ref.py)."""
import functools

import pytest
import torch

import exposure_ref as R
import lpips_ref as LR
from exposure_ref import F32, check_rows
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, W, H, N = 3, 64, 48, 2000
BAR = 1e-4          # the repository's fused-against-modular bar on leaf gradients (max-rel-err)
IDS = list(range(V))
RECTS = [(8, 6, 40, 30), (0, 0, 32, 24), (20, 16, 44, 32)]


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


def table(C=V, identity=False):
    return (R.identity_table(C) if identity else R.table(C, seed=21)).to(F32).to(DEV).contiguous()


def clone_out(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def compute(**kw):
    from manus_amd.engine import HipViewCompute
    sc, ct, tg = scene()
    kw.setdefault("loss", "l1+ssim")
    return HipViewCompute(sc, tg, ct, persistent_grads=False, **kw)


def run(hc):
    return clone_out(hc(IDS, 1.0 / V))


def step(**kw):
    hc = compute(**kw)
    return hc, run(hc)


def same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        if isinstance(a[k], dict):
            for q in a[k]:
                assert torch.equal(a[k][q], b[k][q]), (what, k, q)
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), (what, k)


def compare(a, b, what, grad2d=True):
    """fused (a) against modular (b): loss, leaf gradients, d_exposure and grad2d at the bar; vis equal."""
    la, lb = float(a["loss"]), float(b["loss"])
    print("%s: loss fused %.7e modular %.7e" % (what, la, lb))
    assert abs(la - lb) <= BAR * abs(lb)
    worst = 0.0
    for k, g in b["grads"].items():
        e = max_rel_err(a["grads"][k].cpu().numpy(), g.cpu().numpy())
        print("%s: %-16s fused against modular %.3g" % (what, k, e))
        worst = max(worst, e)
    eE = max_rel_err(a["d_exposure"].cpu().numpy(), b["d_exposure"].cpu().numpy())
    e2d = max_rel_err(a["grad2d"].cpu().numpy(), b["grad2d"].cpu().numpy()) if grad2d else 0.0
    print("%s: d_exposure fused against modular %.3g, grad2d %.3g" % (what, eE, e2d))
    assert worst < BAR and eE < BAR and e2d < BAR, (worst, eE, e2d)
    assert torch.equal(a["vis"], b["vis"])
    return worst


@pytest.mark.parametrize("fused", [True, False])
def test_off_is_the_step_without_the_keyword(fused):
    _, ref = step(fused=fused)
    assert "d_exposure" not in ref
    hc, none = step(fused=fused, exposure=None)
    same(none, ref, "exposure=None")
    assert hc.last_corrected is None
    hc = compute(fused=fused, exposure=table())
    hc.exposure_on = False
    same(run(hc), ref, "exposure_on=False")
    assert hc.last_corrected is None
    # ... and on again: another step, with a table gradient
    hc.exposure_on = True
    on = run(hc)
    assert tuple(on["d_exposure"].shape) == (V, 3, 4) and not torch.equal(on["loss"], ref["loss"])
    # the parity hook is a gradient with respect to the render: it bypasses the correction
    if fused:
        g = torch.Generator().manual_seed(5)
        g_img = torch.randn((V, 3, H, W), generator=g).to(DEV) / (H * W)
        a = clone_out(hc._step_direct(IDS, 1.0 / V, g_img=g_img))
        b = clone_out(compute(fused=True)._step_direct(IDS, 1.0 / V, g_img=g_img))
        same(a, b, "g_img given")


@pytest.mark.parametrize("fused", [True, False])
def test_identity_table_is_the_dense_step(fused):
    _, _, tg = scene()
    _, dense = step(fused=fused, sparse_loss=False)
    hc, out = step(fused=fused, exposure=table(identity=True))
    assert torch.equal(out["loss"], dense["loss"])
    for k, g in dense["grads"].items():
        assert torch.equal(out["grads"][k], g), k
    for k in ("grad2d", "vis", "radii"):
        assert torch.equal(out[k], dense[k]), k
    assert torch.equal(hc.last_corrected, hc.last_image)
    # d_exposure: the restatement on the raw render and the dense loss's gradient
    _, g = hc._image_loss(hc.last_image, tg, 1.0 / V)
    img64, g64 = hc.last_image.double().cpu(), g.double().cpu()
    _, dE64 = R.backward_ref(img64, R.identity_table(V), IDS, g64)
    _, dE32 = R.backward_ref(img64, R.identity_table(V), IDS, g64, F32)
    check_rows("d_exposure fused=%s" % fused, R.view_rows(out["d_exposure"]), R.view_rows(dE64), R.view_rows(dE32))


def test_a_table_on_both_routes():
    hf, of = step(fused=True, exposure=table())
    hm, om = step(fused=False, exposure=table())
    compare(of, om, "table")
    # last_image stays the raw render, last_corrected is the table applied to it
    from manus_amd import ops
    for hc in (hf, hm):
        assert torch.equal(hc.last_corrected, ops.exposure_forward(hc.last_image, hc.exposure, torch.tensor(IDS, dtype=torch.int32, device=DEV)))
        assert not torch.equal(hc.last_corrected, hc.last_image)
    # the term reaches the leaves: the share of each leaf's maximum that the table changes, against the dense step without it
    for fused, on in ((True, of), (False, om)):
        _, off = step(fused=fused, sparse_loss=False)
        shares = {k: max_rel_err(on["grads"][k].cpu().numpy(), g.cpu().numpy()) for k, g in off["grads"].items()}
        print("fused %s: the table changes " % fused + ", ".join("%s by %.3g" % kv for kv in shares.items()))
        assert all(s > BAR for s in shares.values()), shares      # above the bar the two routes agree at: not rounding


def _mask():
    g = torch.Generator().manual_seed(13)
    return (torch.rand((V, H, W), generator=g) > 0.5).float().to(DEV)


@pytest.mark.parametrize("case", ["l1", "spatial", "mask", "lpips", "lpips_window", "lpips_batch", "all"])
def test_other_terms_with_a_table(case):
    kw = dict(l1=dict(loss="l1"), spatial=dict(ssim="spatial"), mask=dict(mask_targets=_mask(), w_mask=0.5),
              lpips=dict(lpips=vgg(), w_lpips=0.1), lpips_window=dict(lpips=vgg(), w_lpips=0.1, lpips_rects=RECTS),
              lpips_batch=dict(lpips=vgg(), w_lpips=0.1, lpips_rects=[RECTS[0]] * V, lpips_batch=4),
              all=dict(ssim="spatial", mask_targets=_mask(), w_mask=0.5, lpips=vgg(), w_lpips=0.1, lpips_rects=RECTS))[case]
    hf, of = step(fused=True, exposure=table(), **kw)
    _, om = step(fused=False, exposure=table(), **kw)
    compare(of, om, case, grad2d="mask_targets" not in kw)
    if "lpips" in kw:
        # the value is the direct call on the corrected image
        _, _, tg = scene()
        rects = kw.get("lpips_rects")
        d = vgg().values_grad(hf.last_corrected, tg, need_grad=False, **(dict(rects=rects) if rects else {}))[0].double().cpu()
        fac = torch.tensor([r[2] * r[3] / float(W * H) for r in rects], dtype=torch.float64) if rects else 1.0
        direct = float((d * fac).sum() / V)
        print("%s: loss_lpips %.7e direct on last_corrected %.7e" % (case, float(of["loss_lpips"]), direct))
        assert abs(float(of["loss_lpips"]) - direct) <= 1e-5 * abs(direct)
        raw = float((vgg().values_grad(hf.last_image, tg, need_grad=False, **(dict(rects=rects) if rects else {}))[0].double().cpu() * fac).sum() / V)
        assert abs(raw - direct) > 1e-4 * abs(direct)      # (not the raw render's)


def test_shared_rows_and_a_view_without_one():
    ids = [1, -1, 1]
    E = table(2)
    _, of = step(fused=True, exposure=E, exposure_ids=ids)
    hm, om = step(fused=False, exposure=E, exposure_ids=ids)
    compare(of, om, "shared")
    for o in (of, om):
        assert bool((o["d_exposure"][1] == 0).all()) and bool((o["d_exposure"][0] != 0).any()) and bool((o["d_exposure"][2] != 0).any())
    assert torch.equal(hm.last_corrected[1], hm.last_image[1]) and not torch.equal(hm.last_corrected[0], hm.last_image[0])
    # a step over a subset of the views takes the rows of THOSE views
    hc = compute(fused=True, exposure=E, exposure_ids=[0, 1, -1])
    out = clone_out(hc([2, 0], 0.5))
    assert bool((out["d_exposure"][0] == 0).all()) and bool((out["d_exposure"][1] != 0).any())
    # refused at the step: ids of another length, a table of another shape
    hc.exposure_ids = [0, 1]
    with pytest.raises(ValueError, match="exposure_ids"):
        hc(IDS, 1.0 / V)
    hc.exposure_ids, hc.exposure = None, table(2)
    with pytest.raises(ValueError, match="exposure_ids"):
        hc(IDS, 1.0 / V)

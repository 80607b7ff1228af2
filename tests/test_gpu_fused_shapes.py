"""GPU: the fused step (mgr_views_forward / mgr_views_backward) at small, ragged and empty-view shapes (tests/fused_shapes.py;
the cases' conditions are proved on the CPU oracle in tests/test_fused_shapes_cpu.py).

  non-empty cases  the oracle on identical blend inputs at the north-star bars (fused_oracle.assert_north_star, the integer state
                   of the oracle's own projection as tests/test_gpu_fullsize.py judges it); the modular route and run-to-run
                   bit equality at the bars of tests/test_gpu_fused.py; a full step with the image loss, its value against the
                   fp64 restatement on the step's own image, its leaf gradients equal with the span list on and off
  empty cases      exact: the image of a view that sees nothing is the background in every element, its statistics, gradient
                   rows and pose gradient are zero; a step with one empty view is, in its gradients, the step over the other views
  sequences        a step whose views see nothing, between two full steps of one compute object with kept buffers
  N = 0            pinned: background images, empty gradients (decision: DESIGN.md section 3)

Every bar is the project's own, unchanged.  The one that scales with the image -- assert_north_star's pixel centres, 1.1e-6 * width,
measured at 1920 px -- holds at 7 to 200 px as it is: the kernels lie 9.5e-7 to 3.2e-5 px from the torch chain, the bar is 7.7e-6
to 2.2e-4 (closest: `tall`, 6.7e-6 against 1.4e-5).  The fp32 oracle's own distance from the fp64 oracle is printed beside it (the
yardstick such a bar would be re-derived from, had it not held).  Measured figures: DESIGN.md section 3."""
import functools

import numpy as np
import pytest
import torch

import fused_shapes as fs
import regimes as rg
import ssim2d_ref as R
from fused_oracle import assert_north_star, run_fused_vs_oracle
from test_gpu_fullsize import assert_own_projection
from test_gpu_fused import check_fused_equals_modular, check_fused_run_to_run_determinism
from test_gpu_image_loss import _ref_sums64
from util import keep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W_RGB, W_SSIM = 0.8, 0.2


@functools.lru_cache(maxsize=None)
def cpu_scene(name, extra_away=False):
    return fs.case_scene(name, extra_away)


@functools.lru_cache(maxsize=None)
def dev_scene(name, extra_away=False):
    from manus_amd.synthetic import camera_table
    sc = cpu_scene(name, extra_away)
    return rg.to_device(sc, DEV), camera_table(sc["cameras"], DEV)


@functools.lru_cache(maxsize=None)
def facts_of(name):
    """The case's conditions on the CPU oracle, once per case (a scene that is not its case fails every test that uses it)."""
    sc, c = cpu_scene(name), fs.spec(name)
    facts = [fs.view_facts(sc, v) for v in range(c["views"])]
    fs.assert_case(name, facts, sc, "gpu")
    return facts


@functools.lru_cache(maxsize=None)
def targets_of(name, extra_away=False):
    """Targets: the render of the perturbed model (background wherever it renders nothing), plus foreground in the last
    column of the last row of every view -- an empty tile in most cases, the unpaired row and the scalar tail of the loss."""
    from manus_amd.engine import HipViewCompute
    scd, ct = dev_scene(name, extra_away)
    V, H, W = int(ct.shape[0]), int(scd["height"]), int(scd["width"])
    g = torch.Generator().manual_seed(3)
    tgt_scene = dict(scd)
    tgt_scene["params"] = {k: (v + 0.02 * v.abs().mean() * torch.randn(v.shape, generator=g).to(DEV)) for k, v in scd["params"].items()}
    with torch.no_grad():
        tg = HipViewCompute(tgt_scene, torch.zeros((V, 3, H, W), device=DEV), ct).forward_views_fused(list(range(V)))[0].clone().contiguous()
    tg[:, :, H - 1, W - 1] = 0.25
    return tg


def _report(tag, res, yard):
    """One line per case, the figures of DESIGN.md's table of shape deviations: everything assert_north_star reads."""
    print("SHAPE", tag, "dpsnr %.1e img_max %.2e img_mean %.1e frac %.1e sums9 %.2e grad2d %.1e" % (res["dpsnr"], res["img_max"], res["img_mean"], res["img_frac_2e6"], res["sums9"], res["grad2d"]),
          " ".join("%s %.1e" % (k, e) for k, e in res["grads"].items()),
          "proj_pix %.2e (bar %.2e, fp32 oracle from fp64 %.2e) proj_conic %.1e proj_col %.1e" % (res["proj_pix"], 1.1e-6 * res["width"], yard, res["proj_conic"], res["proj_col"]),
          "ambiguous %d flipped %d stop-flipped %d violations %d pairs %s" % (res["ambiguous"], res["flips"], res["stop_flips"], res["stop_violations"], res["num_rendered"]))


# ---------------------------------------------------------------------------------------------------------------
# non-empty cases
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fs.NONEMPTY + ["empty_first", "empty_middle", "empty_last"])
def test_fused_matches_oracle_at_shape(name):
    """The fused route against the oracle on identical blend inputs, threshold flips accounted for; the oracle's own
    projection gives the same radii and pair counts, or every difference is listed and explained.  (The three cases with one
    view turned away run too: an empty view between two full ones, in the records the comparison reads back.)"""
    c = fs.spec(name)
    facts_of(name)
    res = run_fused_vs_oracle(own_projection=True, **fs.oracle_args(name))
    assert len(res["regime"]) == c["views"]
    fs.assert_case(name, res["regime"], tag="kernels' records")       # ... and on the kernels' own records
    _report(name, res, fs.projection_yardstick(cpu_scene(name), c["views"])[0])
    assert_north_star(res, name)
    assert_own_projection(res, c["n"], name)


@pytest.mark.parametrize("name", fs.NONEMPTY)
def test_fused_equals_modular_at_shape(name):
    """tests/test_gpu_fused.py::test_fused_equals_modular and ::test_fused_run_to_run_determinism, their assertions and
    thresholds, at the case's sizes."""
    facts_of(name)
    scd, ct = dev_scene(name)
    check_fused_equals_modular(scd, ct)
    check_fused_run_to_run_determinism(scd, ct, fs.spec(name)["views"])


def _loss_scales(V, H, W, scale):
    """(k, const) of HipViewCompute._loss_scales at loss_weight 1."""
    return scale / (3 * H * W), W_SSIM * scale * V


@pytest.mark.parametrize("name", fs.NONEMPTY)
def test_full_step_with_the_image_loss_at_shape(name):
    """loss="l1+ssim", rows and spatial.  Rows: the tile-aware span list from target maps, from the targets, and off (the full
    comparison) -- the value against the fp64 restatement on the step's own image (the bound of tests/test_gpu_image_loss.py),
    the leaf gradients and statistics equal in every bit between the three.  Spatial: the value against ssim2d_ref in fp64, judged
    as tests/test_gpu_ssim2d.py judges it (ssim2d_ref.bound of the fp32 restatement's own error on the two sums it is formed from)."""
    from manus_amd.engine import HipViewCompute
    facts_of(name)
    scd, ct = dev_scene(name)
    tg = targets_of(name)
    V, H, W = int(ct.shape[0]), int(scd["height"]), int(scd["width"])
    ids, scale = list(range(V)), 1.0 / V
    k, const = _loss_scales(V, H, W, scale)
    outs = {}
    for route, kw, tmap in (("mapped", dict(sparse_loss=True), True), ("listed", dict(sparse_loss=True), False), ("full", dict(sparse_loss=False), True)):
        hc = HipViewCompute(scd, tg, ct, loss="l1+ssim", persistent_grads=False, **kw)
        hc.target_map = tmap
        out = keep(hc(ids, scale))
        want = float(_ref_sums64(hc.last_image, tg, k, const, W_RGB, W_SSIM)[2])
        print("LOSS %s %s rows: %.7e fp64 %.7e" % (name, route, float(out["loss"]), want))
        assert abs(float(out["loss"]) - want) <= 1e-5 * max(1.0, abs(want)), (name, route)
        outs[route] = (out, hc.last_image.clone())
    ref, ref_img = outs["full"]
    for route in ("mapped", "listed"):
        out, img = outs[route]
        for key, g in ref["grads"].items():
            assert torch.equal(out["grads"][key], g), (name, route, key)
        assert torch.equal(out["grad2d"], ref["grad2d"]) and torch.equal(out["vis"], ref["vis"]) and torch.equal(out["radii"], ref["radii"]), (name, route)
        assert torch.equal(img, ref_img), (name, route)
    assert all(torch.isfinite(g).all() for g in ref["grads"].values())
    hc = HipViewCompute(scd, tg, ct, loss="l1+ssim", ssim="spatial", persistent_grads=False)
    out = keep(hc(ids, scale))
    # tests/test_gpu_ssim2d.py::judge: the value is a difference of nearly equal terms (w_ssim * mean S against the offset of
    # "1 - ssim"), so it is judged in absolute terms against what the bounds of its two sums allow, plus one rounding of the result
    r64 = R.loss2d(hc.last_image, tg, W_RGB, W_SSIM, k, const, dtype=torch.float64)["sums"]
    r32 = R.loss2d(hc.last_image, tg, W_RGB, W_SSIM, k, const, dtype=torch.float32)["sums"]
    b = [R.bound(R.rel(r32[i], r64[i])) * abs(float(r64[i])) for i in range(2)]
    allowed = k * (W_RGB * b[0] + W_SSIM * b[1]) + 2.0 ** -24 * abs(float(r64[2]))
    e = abs(float(out["loss"]) - float(r64[2]))
    print("LOSS %s spatial: %.7e fp64 %.7e abs err %.2e allowed %.2e" % (name, float(out["loss"]), float(r64[2]), e, allowed))
    assert e <= allowed, (name, e, allowed)
    assert torch.equal(hc.last_image, ref_img) and torch.equal(out["vis"], ref["vis"])
    assert all(torch.isfinite(g).all() for g in out["grads"].values())


# ---------------------------------------------------------------------------------------------------------------
# empty views: exact references
# ---------------------------------------------------------------------------------------------------------------
def _bg_image(bg, H, W):
    return bg.view(3, 1, 1).expand(3, H, W)


def _nan_kept_image(hc, V, H, W):
    """The image buffer a compute object with kept buffers will use on its first step, filled with NaN."""
    N = hc.params["_xyz"].shape[0]
    hc._kept.begin(N, hc.n_art, hc.device)
    hc._kept.get((V, 3, H, W), ("image", V, H, W), zeroed=False).fill_(float("nan"))


def _view_loss64(img, tgt, scale):
    """scale * (the "l1+ssim" rows loss of one view) in fp64."""
    _, H, W = img.shape
    k, const = _loss_scales(1, H, W, scale)
    return float(_ref_sums64(img[None], tgt[None], k, const, W_RGB, W_SSIM)[2])


@pytest.mark.parametrize("bg", ["white", "coloured"])
@pytest.mark.parametrize("name", fs.EMPTY)
def test_views_that_see_nothing(name, bg):
    from manus_amd.engine import HipViewCompute
    c, cond = fs.spec(name), fs.conditions(name)
    facts_of(name)
    scd, ct = dev_scene(name)
    scd = dict(scd, bg=torch.ones(3, device=DEV) if bg == "white" else torch.tensor([0.2, 0.4, 0.6], device=DEV))
    V, H, W, n = c["views"], c["H"], c["W"], c["n"]
    tg = targets_of("nine_ranges")                 # (a target with a hand in it for every view, the empty ones included)
    ids, scale = list(range(V)), 1.0 / V
    dark = cond["empty_views"] if not cond["nothing_listed"] else ids        # the views whose image is the background alone
    lit = [v for v in ids if v not in dark]
    bgi = _bg_image(scd["bg"], H, W)
    fresh = HipViewCompute(scd, tg, ct, loss="l1+ssim", persistent_grads=False)
    want = keep(fresh(ids, scale))
    want_img = fresh.last_image.clone()
    for v in dark:
        assert torch.equal(want_img[v], bgi), (name, v)
    assert torch.equal(fresh.last_radii[cond["empty_views"]], torch.zeros_like(fresh.last_radii[cond["empty_views"]]))
    assert all(torch.isfinite(g).all() for g in want["grads"].values())
    if not lit:
        # nothing contributes anywhere: every leaf gradient row is exactly zero, and the loss is the targets' against the background
        for key, g in want["grads"].items():
            assert not g.any(), (name, key)
        assert not want["grad2d"].any()
        if cond["nothing_listed"]:       # below 1/255: radii positive, seen by every view, in no list
            assert torch.equal(want["vis"], torch.full_like(want["vis"], float(V))) and bool((want["radii"] > 0).all())
        else:
            assert not want["vis"].any() and not want["radii"].any()
        loss64 = sum(_view_loss64(bgi, tg[v], scale) for v in ids)
        assert abs(float(want["loss"]) - loss64) <= 1e-5 * max(1.0, abs(loss64)), (name, float(want["loss"]), loss64)
    else:
        # one view empty: in its gradients and statistics the step is the step over the other two, at the same scale; its loss is
        # that step's plus the empty view's loss against its target
        two = HipViewCompute(scd, tg, ct, loss="l1+ssim", persistent_grads=False)
        o2 = keep(two(lit, scale))
        for key, g in o2["grads"].items():
            assert torch.equal(want["grads"][key], g), (name, key, float((want["grads"][key] - g).abs().max()), float(g.abs().max()))
        assert torch.equal(want["grad2d"], o2["grad2d"]) and torch.equal(want["vis"], o2["vis"]) and torch.equal(want["radii"], o2["radii"])
        assert torch.equal(want_img[lit], two.last_image)
        extra = sum(_view_loss64(bgi, tg[v], scale) for v in dark)
        got = float(want["loss"]) - float(o2["loss"])
        print("EMPTY %s %s: loss %.7e, two views %.7e, difference %.7e, empty view in fp64 %.7e" % (name, bg, float(want["loss"]), float(o2["loss"]), got, extra))
        assert abs(got - extra) <= 2e-5 * max(1.0, abs(float(want["loss"]))), (name, got, extra)
    # pose gradient: nothing flows into the pose of a view that sees nothing; the rest of the step is unchanged
    posed = HipViewCompute(scd, tg, ct, loss="l1+ssim", persistent_grads=False, pose_grad=True)
    op = keep(posed(ids, scale))
    assert op["d_transforms"].shape[0] == V and bool(torch.isfinite(op["d_transforms"]).all())
    for v in dark:
        assert not op["d_transforms"][v].any(), (name, v)
    for v in lit:
        assert op["d_transforms"][v].any(), (name, v)
    for key, g in want["grads"].items():
        assert torch.equal(op["grads"][key], g), (name, "pose", key)
    # kept buffers: the first step into an image buffer full of NaN, the second and third with the selective fills in use
    kept = HipViewCompute(scd, tg, ct, loss="l1+ssim", persistent_grads=True)
    _nan_kept_image(kept, V, H, W)
    for it in range(3):
        assert (kept._pg_ws is not None and kept._pimg_ws is not None) == (it > 0), (name, it)
        ok = kept(ids, scale)
        for key, g in want["grads"].items():
            assert torch.equal(ok["grads"][key], g), (name, "kept", it, key)
        assert torch.equal(ok["grad2d"], want["grad2d"]) and torch.equal(ok["vis"], want["vis"]) and torch.equal(ok["radii"], want["radii"]), (name, it)
        assert torch.equal(kept.last_image, want_img), (name, "kept image", it)
        assert torch.equal(ok["loss"], want["loss"]), (name, "kept loss", it)


# ---------------------------------------------------------------------------------------------------------------
# sequences on one compute object: a step that sees nothing (in one view, in all) between two full steps
# ---------------------------------------------------------------------------------------------------------------
def _snapshot(hc, out):
    o = keep(out)
    o["image"] = hc.last_image.clone()
    return o


def _same_step(a, b, tag):
    for key, g in b["grads"].items():
        assert torch.equal(a["grads"][key], g), (tag, key)
    for key in ("grad2d", "vis", "radii", "image", "loss"):
        assert torch.equal(a[key], b[key]), (tag, key)


@pytest.mark.parametrize("run_lists", [1, 0])
@pytest.mark.parametrize("middle", ["one_view_empty", "all_views_empty"])
def test_a_step_that_sees_nothing_between_two_full_steps(middle, run_lists):
    """Kept buffers on (the default), the depth cut off, run lists on and off: views [0, 1, 2], then a view set with the
    turned-round cameras, then [0, 1, 2] again -- and twice more round.  Every step equals, in every bit of its gradients,
    statistics, image and loss, the same step of a fresh object: the selective zero fill of the step after the empty one
    starts from an active list of nothing (all views empty) or of fewer rows, and the empty step must have zeroed every row
    the full step before it wrote."""
    from manus_amd._lib import lib
    from manus_amd.engine import HipViewCompute
    facts_of("nine_ranges")
    scd, ct = dev_scene("nine_ranges", True)
    tg = targets_of("nine_ranges", True)
    full, mid = [0, 1, 2], ([0, 4, 2] if middle == "one_view_empty" else [3, 4, 5])
    scale = 1.0 / 3
    prev = lib().mgr_views_backward_run_lists(run_lists)
    try:
        want = {}
        for key, ids in (("full", full), ("mid", mid)):      # the fresh objects first: the kept object then owns the workspace's row state
            hc = HipViewCompute(scd, tg, ct, loss="l1+ssim", depth_cut=False)
            want[key] = _snapshot(hc, hc(ids, scale))
        assert want["full"]["grads"]["_xyz"].any()
        if middle == "all_views_empty":
            assert not any(g.any() for g in want["mid"]["grads"].values()) and not want["mid"]["vis"].any()
            assert torch.equal(want["mid"]["image"], torch.ones_like(want["mid"]["image"]))
        hc = HipViewCompute(scd, tg, ct, loss="l1+ssim", depth_cut=False)
        assert hc.persistent_grads and not hc.depth_cut
        selective = []
        for it, (key, ids) in enumerate((("full", full), ("mid", mid), ("full", full), ("mid", mid), ("full", full))):
            _same_step(_snapshot(hc, hc(ids, scale)), want[key], (middle, run_lists, it, key))
            selective.append(hc._pg_ws is not None and hc._pimg_ws is not None)
        assert all(selective), selective       # the kept object did own the row / tile state from step to step
    finally:
        lib().mgr_views_backward_run_lists(prev)


# ---------------------------------------------------------------------------------------------------------------
# N = 0: everything pruned
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hand", "object"])
def test_a_model_without_gaussians_renders_the_background(kind):
    """The path below HipViewCompute at N = 0, as read: every launch of mgr_views_forward that touches
    per-Gaussian storage is inside `if (N > 0)` (k_inst_fwd, the depth-ordered binning chain, the repair); the tile scan, the blend
    and k_fwd_items run on zero tile counts exactly as they do for the operator route's N = 0 (test_edge_cases_empty_and_culled);
    mgr_views_backward returns before its first launch; the host skips the skin weights (n_art = 0) and the active list
    (N > 0).  So the step is defined, and pinned here: background images, empty gradients, the loss of the background against
    the targets; pose_grad is refused by the constructor (no articulated Gaussians)."""
    from manus_amd.engine import HipViewCompute
    scd, ct = dev_scene("five" if kind == "hand" else "object_odd")
    c = fs.spec("five" if kind == "hand" else "object_odd")
    V, H, W = c["views"], c["H"], c["W"]
    sc0 = dict(scd, kind=kind, N=0, n_hand=0, params={k: v[:0].contiguous() for k, v in scd["params"].items()},
               bg=torch.tensor([0.2, 0.4, 0.6], device=DEV))
    tg = torch.rand((V, 3, H, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    ids, scale = list(range(V)), 1.0 / V
    bgi = _bg_image(sc0["bg"], H, W)
    with pytest.raises(ValueError, match="pose_grad needs articulated Gaussians"):
        HipViewCompute(sc0, tg, ct, loss="l1+ssim", pose_grad=True)
    for kw in (dict(persistent_grads=False), dict(persistent_grads=True), dict(persistent_grads=False, sparse_loss=False), dict(persistent_grads=False, loss="l1")):
        kw.setdefault("loss", "l1+ssim")
        hc = HipViewCompute(sc0, tg, ct, **kw)
        assert hc.n_art == 0
        for it in range(2):
            out = hc(ids, scale)
            assert torch.equal(hc.last_image, bgi[None].expand(V, 3, H, W)), (kind, kw, it)
            assert hc.last_radii.shape == (V, 0)
            assert {k: tuple(g.shape) for k, g in out["grads"].items()} == {k: tuple(v.shape) for k, v in sc0["params"].items()}
            assert out["grad2d"].shape == out["vis"].shape == out["radii"].shape == (0,)
            assert hc.last_active is None
            if kw["loss"] == "l1":
                want = scale * sum(float((bgi.double().cpu() - tg[v].double().cpu()).abs().mean()) for v in ids)
            else:
                want = sum(_view_loss64(bgi, tg[v], scale) for v in ids)
            assert abs(float(out["loss"]) - want) <= 1e-5 * max(1.0, abs(want)), (kind, kw, float(out["loss"]), want)

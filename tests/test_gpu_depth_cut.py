"""GPU: the depth cut of the fused step (mgr_views_forward, debug bit 8; include/manus_hip.h).

A forward leaves, per tile whose pixels all saturated, the depth in front of which they had stopped; the next forward of the
same views drops the instances behind it from that tile's list.  What must hold:
  * image, radii, loss and every leaf gradient are BIT FOR BIT those of the step without the cut, while the binning handles
    fewer pairs;
  * hints that no longer fit the scene (here: every opacity lowered, so that the walks go deeper) are detected -- the step is
    flagged like a pair-capacity overflow -- and the re-run without the cut is exact again, as is the step after it;
  * view sets that alternate keep their own hints;
  * a Trainer with the cut follows the trajectory of one without it, through the optimizer steps that move the model under
    the hints, a densification and an opacity reset.
There is no reference counterpart (upstream re-bins everything every step); the parity bar is equality with our own
uncut step, which the other GPU tests tie to the oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAVES = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")


def _scene(V=4, n=40000, W=256, H=192, seed=3, sigma_range=(2e-3, 5e-3)):
    from manus_amd.synthetic import camera_table, make_scene
    # opaque, fairly large Gaussians on the hand, seen from close: the interior tiles saturate, the silhouette does not
    sc = make_scene(n_gaussians=n, kind="hand", seed=seed, grid_res=32, n_cameras=V, width=W, height=H, cam_radius=0.45,
                    sigma_range=sigma_range, device=DEV)
    sc["params"]["_opacity"] = sc["params"]["_opacity"] + 2.0
    g = torch.Generator().manual_seed(seed + 100)
    targets = torch.rand((V, 3, H, W), generator=g).to(DEV)
    return sc, targets, camera_table(sc["cameras"], DEV)


def _compute(sc, targets, ct, cut):
    from manus_amd.engine import HipViewCompute
    return HipViewCompute(sc, targets, ct, loss="l1+ssim", depth_cut=cut)


def _surviving_pairs(compute, V, N, W, H):
    """Pairs the binning of the most recent forward put into the tile lists."""
    from manus_amd import rasterizer
    ws = rasterizer.context(DEV).last_ws
    off = compute._layout(ws, V, N, W, H)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    return int(ws.buf[off[7] + 4 * V * T: off[7] + 4 * V * T + 4].view(torch.int32).item())


def _same(a, b):
    assert torch.equal(a["loss"], b["loss"]), (float(a["loss"]), float(b["loss"]))
    assert torch.equal(a["radii"], b["radii"])
    for k in LEAVES:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert torch.equal(a["grad2d"], b["grad2d"]) and torch.equal(a["vis"], b["vis"])


@pytest.fixture
def fenced():
    from manus_amd import rasterizer
    ctx = rasterizer.context(DEV)
    ctx.clear()
    ctx.cut_retries = 0
    rasterizer.set_sync_policy(True)
    yield ctx
    rasterizer.set_sync_policy(True)
    ctx.clear()


def _warm(compute, views):
    """One step with host syncs (learns the pair capacity), then the fenced mode the cut needs."""
    from manus_amd import rasterizer
    compute(views)
    rasterizer.check_overflow(DEV)
    rasterizer.set_sync_policy(False, DEV)


def test_cut_step_equals_the_full_step_and_bins_fewer_pairs(fenced):
    from manus_amd import rasterizer
    V, W, H = 4, 256, 192
    sc, targets, ct = _scene(V=V, W=W, H=H)
    N = sc["params"]["_xyz"].shape[0]
    views = list(range(V))
    ref = _compute(sc, targets, ct, cut=False)
    _warm(ref, views)
    want = ref(views)
    img_want = ref.last_image.clone()
    full = _surviving_pairs(ref, V, N, W, H)
    rasterizer.check_overflow(DEV)

    rasterizer.set_sync_policy(True, DEV)
    cmp_ = _compute(sc, targets, ct, cut=True)
    _warm(cmp_, views)
    first = cmp_(views)                       # fenced, no hints of these views under this key yet: full lists
    assert _surviving_pairs(cmp_, V, N, W, H) == full
    _same(first, want)
    for _ in range(3):                        # hints of the step before: cut lists, same results, and stable
        got = cmp_(views)
        cut = _surviving_pairs(cmp_, V, N, W, H)
        _same(got, want)
        assert torch.equal(cmp_.last_image, img_want)
    assert rasterizer.check_overflow(DEV) > 0           # (returns the rectangle pair count; raises if a step was flagged)
    assert fenced.cut_retries == 0
    print("pairs in the lists: %d full, %d with the cut (%.2f)" % (full, cut, cut / full))
    assert cut < 0.8 * full, (cut, full)


def test_outdated_hints_are_flagged_and_the_rerun_is_exact(fenced):
    from manus_amd import rasterizer
    from manus_amd._lib import ManusHipError
    V, W, H = 2, 256, 192
    sc, targets, ct = _scene(V=V, W=W, H=H, seed=5)
    views = list(range(V))
    # the model the hints will be outdated for: every Gaussian far more transparent -> the walks need entries the cut removed
    sc2 = dict(sc)
    sc2["params"] = {k: (v - 4.0 if k == "_opacity" else v).detach().clone() for k, v in sc["params"].items()}
    ref = _compute(sc2, targets, ct, cut=False)
    _warm(ref, views)
    want = ref(views)
    rasterizer.check_overflow(DEV)
    rasterizer.set_sync_policy(True, DEV)
    cmp_ = _compute(sc, targets, ct, cut=True)
    cmp_.cut_repair = False                    # (the path without the on-device repair: flag, re-run)
    _warm(cmp_, views)
    cmp_(views)
    cmp_(views)
    rasterizer.poll(DEV)
    with torch.no_grad():
        cmp_.params["_opacity"].sub_(4.0)      # the model changes under the hints
    cmp_(views)                                # cut lists against the new model
    with pytest.raises(ManusHipError):
        rasterizer.poll(DEV)
    assert fenced.cut_retries == 1
    again = cmp_(views)                        # the re-run: no cut, fresh hints
    rasterizer.poll(DEV)
    _same(again, want)
    nxt = cmp_(views)                          # and the step after it, on the fresh hints
    rasterizer.poll(DEV)
    _same(nxt, want)
    assert fenced.cut_retries == 1


def _moving_model_run(fenced, V, W, H, n, steps, d_opacity, margin, seed=5, penalty=16, **scene_kw):
    """A model whose opacities fall by d_opacity per step (the walks lengthen under the hints of the step before), rendered
    by a compute object without the cut -- all states first: two objects taking turns on one workspace would wipe the hints --
    and then by one with the cut and tight margins.  Returns (repaired quadrants, flagged forwards)."""
    from manus_amd import rasterizer
    from manus_amd._lib import ManusHipError
    from util import keep
    sc, targets, ct = _scene(V=V, n=n, W=W, H=H, seed=seed, **scene_kw)
    views = list(range(V))
    ref = _compute(sc, targets, ct, cut=False)
    _warm(ref, views)
    wants = []
    for _ in range(steps):
        with torch.no_grad():
            ref.params["_opacity"].sub_(d_opacity)
        ref.mark_params_changed()
        wants.append((keep(ref(views)), ref.last_image.clone()))
    rasterizer.check_overflow(DEV)
    rasterizer.set_sync_policy(True, DEV)
    cmp_ = _compute(sc, targets, ct, cut=True)
    cmp_.cut_margin, cmp_.cut_penalty = margin, penalty
    _warm(cmp_, views)
    cmp_(views)
    cmp_(views)
    rasterizer.poll(DEV)
    flagged = 0
    for want, img_want in wants:
        with torch.no_grad():
            cmp_.params["_opacity"].sub_(d_opacity)
        cmp_.mark_params_changed()
        got = cmp_(views)
        try:
            rasterizer.poll(DEV)
        except ManusHipError:             # a capacity of the repair exceeded: the legacy answer, still exact
            flagged += 1
            got = cmp_(views)
            rasterizer.poll(DEV)
        _same(got, want)
        assert torch.equal(cmp_.last_image, img_want)
    return fenced.cut_repairs, flagged


def test_tiles_that_run_out_are_repaired_on_the_device(fenced):
    """Forward debug bit 2048: quadrants whose cut list runs out under an unsaturated pixel are completed by k_repair_scan /
    k_repair_blend -- image, loss and every gradient stay bit for bit those of the full lists, step after step, without a
    flagged forward; the per-tile countdown then keeps the tiles that ran out off the hints for a while."""
    fenced.cut_repairs = 0
    repairs, flagged = _moving_model_run(fenced, V=2, W=256, H=192, n=40000, steps=8, d_opacity=0.15, margin=0.25)
    print("repaired quadrants over 8 steps: %d, flagged forwards: %d" % (repairs, flagged))
    assert repairs > 0
    assert flagged == 0, flagged


def test_repair_capacity_exceeded_falls_back_to_the_flag(fenced):
    """Every opacity far lower at once: more quadrants run out than the repair has units for (64 at this workspace size) -- the
    forward is flagged like before round 6 and the re-run on full lists is exact."""
    fenced.cut_repairs = 0
    _, flagged = _moving_model_run(fenced, V=2, W=256, H=192, n=40000, steps=2, d_opacity=3.0, margin=0.25)
    assert flagged >= 1


@pytest.mark.parametrize("W,H,steps", [(6016, 4000, 3), (8192, 4320, 1)])
def test_repair_on_a_grid_beyond_65536_tiles(fenced, W, H, steps):
    """k_repair_scan keeps one bit per tile of a view in LDS, for at most mgr_raster_repair_max_tiles() tiles.  On a larger grid
    (94 000 / 138 240 tiles) the repair stays off -- checked on the host before anything runs --, a tile that runs out flags
    the forward, and every step, re-runs included, is bit for bit the step without the cut."""
    from manus_amd._lib import lib
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert T > lib().mgr_raster_repair_max_tiles() == 65536
    fenced.cut_repairs = 0
    # small Gaussians (rectangles of at most 64 tiles are cut), enough of them that the interior tiles saturate
    repairs, flagged = _moving_model_run(fenced, V=1, W=W, H=H, n=300000, steps=steps, d_opacity=0.15, margin=0.25,
                                         sigma_range=(3e-4, 8e-4))
    print("%dx%d: %d tiles, repaired quadrants %d, flagged forwards %d" % (W, H, T, repairs, flagged))
    assert repairs == 0


def test_alternating_view_sets_keep_their_hints(fenced):
    from manus_amd import rasterizer
    V, W, H = 4, 256, 192
    sc, targets, ct = _scene(V=V, W=W, H=H, seed=7)
    N = sc["params"]["_xyz"].shape[0]
    a, b = [0, 1], [2, 3]
    ref = _compute(sc, targets, ct, cut=False)
    _warm(ref, a)
    from util import keep
    want_a, want_b = keep(ref(a)), keep(ref(b))     # (one compute object: its outputs are kept buffers)
    full_b = _surviving_pairs(ref, 2, N, W, H)
    rasterizer.check_overflow(DEV)
    rasterizer.set_sync_policy(True, DEV)
    cmp_ = _compute(sc, targets, ct, cut=True)
    _warm(cmp_, a)
    for rnd in range(3):
        _same(cmp_(a), want_a)
        _same(cmp_(b), want_b)
        pairs_b = _surviving_pairs(cmp_, 2, N, W, H)
        assert (pairs_b == full_b) if rnd == 0 else (pairs_b < full_b), (rnd, pairs_b, full_b)
    rasterizer.check_overflow(DEV)
    assert fenced.cut_retries == 0


def test_trainer_with_the_cut_follows_the_trainer_without(fenced):
    from manus_amd.engine import Trainer
    V, W, H = 3, 192, 128
    out = {}
    for cut in (False, True):
        fenced.clear()
        torch.manual_seed(0)
        sc, targets, ct = _scene(V=V, n=12000, W=W, H=H, seed=11)
        compute = _compute(sc, targets, ct, cut=cut)
        opts = dict(densify_from_step=4, densification_interval=6, densify_until_step=1000, opacity_reset_interval=9,
                    percent_dense=0.01, densify_grad_threshold=5e-5)
        tr = Trainer(compute, V, extent=0.3, opts=opts, spatial_lr_scale=0.05, bg_white=False, depth_cut=cut)
        losses = []
        for _ in range(14):
            torch.manual_seed(100 + tr.global_step)          # the split noise of a densification
            losses.append(float(tr.train_step()["loss"]))
        out[cut] = (losses, tr.opt.N, {k: v.detach().clone() for k, v in tr.compute.params.items()}, tr.retries,
                    fenced.cut_retries)
    (l0, n0, p0, _, _), (l1, n1, p1, retries, flagged) = out[False], out[True]
    print("losses", [round(x, 5) for x in l1], "N", n1, "re-run steps", retries, "flagged forwards", flagged)
    assert n0 == n1 and l0 == l1, (n0, n1, [(i, a, b) for i, (a, b) in enumerate(zip(l0, l1)) if a != b][:3], out[False][3:])
    for k in LEAVES:      # bit patterns: a Gaussian that left the skin-weight grid carries NaN (like the reference), NaN != NaN
        d = p0[k].view(torch.int32) != p1[k].view(torch.int32)
        assert not bool(d.any()), (k, int(d.sum()), p0[k][d][:4], p1[k][d][:4])


def test_depth_cut_at_the_bench_size(fenced):
    """BASELINE config 3 at full size (300 000 Gaussians, 8 views of 1920 x 1080, the bench's scene): the step with the
    depth cut is bit for bit the step without it, no forward is flagged, and the lists hold less than 40 % of the pairs."""
    from manus_amd import rasterizer
    from manus_amd.synthetic import camera_table, make_scene
    V, N, W, H = 8, 300000, 1920, 1080
    sc = make_scene(n_gaussians=N, kind="hand", seed=0, n_cameras=V, width=W, height=H, device=DEV)
    ct = camera_table(sc["cameras"], DEV)
    targets = torch.rand((V, 3, H, W), generator=torch.Generator().manual_seed(9)).to(DEV)
    views = list(range(V))
    ref = _compute(sc, targets, ct, cut=False)
    _warm(ref, views)
    want = ref(views)
    img = ref.last_image.clone()
    full = _surviving_pairs(ref, V, N, W, H)
    rasterizer.check_overflow(DEV)
    rasterizer.set_sync_policy(True, DEV)
    c = _compute(sc, targets, ct, cut=True)
    _warm(c, views)
    c(views)
    for _ in range(2):
        got = c(views)
        _same(got, want)
        assert torch.equal(c.last_image, img)
    cut = _surviving_pairs(c, V, N, W, H)
    rasterizer.check_overflow(DEV)
    print("pairs in the lists at the bench size: %d full, %d with the cut (%.3f)" % (full, cut, cut / full))
    assert fenced.cut_retries == 0 and cut < 0.4 * full


def test_repair_at_the_bench_size_under_adam(fenced):
    """BASELINE config 3 at full size with the fused Adam step in the loop (the reference's learning rates): the model moves
    under the hints every step, a handful of tiles run out per step and are repaired on the device -- gradients, statistics
    and images of every step equal those of the same trajectory rendered from full lists, and no forward is flagged."""
    from manus_amd import rasterizer
    from manus_amd._lib import ManusHipError
    from manus_amd.optim import GaussianOptimizer
    from manus_amd.synthetic import camera_table, make_scene
    from util import keep
    V, N, W, H = 8, 300000, 1920, 1080
    sc = make_scene(n_gaussians=N, kind="hand", seed=0, n_cameras=V, width=W, height=H, device=DEV)
    ct = camera_table(sc["cameras"], DEV)
    targets = torch.rand((V, 3, H, W), generator=torch.Generator().manual_seed(9)).to(DEV)
    views = list(range(V))
    steps = 12
    fenced.cut_repairs = 0

    def run(cut):
        rasterizer.set_sync_policy(True, DEV)
        c = _compute(sc, targets, ct, cut=cut)
        opt = GaussianOptimizer(c.params, adopt=True)
        _warm(c, views)
        c(views)
        c(views)
        outs = []
        for _ in range(steps):
            o = c(views, 1.0 / V)
            try:
                rasterizer.poll(DEV)
            except ManusHipError:        # (a walk outran its depth window: rare, answered by the step on full lists -- exact too)
                o = c(views, 1.0 / V)
                rasterizer.poll(DEV)
            outs.append((keep(o) if cut is False else o, c.last_image.clone() if cut is False else c.last_image))
            if cut:
                want, img_want = ref_outs[len(outs) - 1]
                _same(o, want)
                assert torch.equal(c.last_image, img_want)
            opt.update_learning_rate(opt.state_step + 1)
            opt.step(o["grads"])
            c.mark_params_changed()
        pairs = _surviving_pairs(c, V, N, W, H)
        rasterizer.check_overflow(DEV)
        return outs, pairs

    ref_outs, full = run(False)
    fenced.clear()
    _, cut = run(True)
    print("bench size under Adam: %d pairs in full lists, %d with the cut; %d quadrants repaired over %d steps, %d flagged forwards"
          % (full, cut, fenced.cut_repairs, steps, fenced.cut_retries))
    assert fenced.cut_repairs > 0 and fenced.cut_retries <= 2 and cut < 0.6 * full

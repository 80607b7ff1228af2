"""GPU: `engine.Trainer(exposure=)` with an `exposure.ExposureRefiner` -- against hand-written loops, bit for bit (the step is
bit-reproducible at this size: DESIGN.md section 6, frame ingest) --, `Trainer.validate(exposure=True)`, and the recovery of
planted per-camera gains end to end.

Set-up of tests/test_gpu_pose_trainer.py: a synthetic capture of 3 frames x 4 cameras at 64x48, 2000 Gaussians, l1+ssim step on
both routes, 3 views per step, densification and pruning off through `opts` except in the test that crosses one."""
import functools
import os

import pytest
import torch

import exposure_ref as R
from test_gpu_frames import BASE
from test_gpu_pose_trainer import KW, OPTS

from manus_amd import dataset as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, IDS, STEPS, SEED = 3, [0, 1, 2], 6, 2
FROM, EVERY = 2, 2
STATE = ("E", "m", "v")


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    from manus_amd.frames import FrameStore
    path = str(tmp_path_factory.mktemp("exposure_trainer"))
    D.write_tree(os.path.join(path, "grasp_1.npz"), D.synthetic_sequence(33, n_frames=3, n_cams=4, width=64, height=48))
    ds = D.SequenceDataset(path, dict(BASE, width=64, height=48, resize_factor=1.0), "train")
    return ds, FrameStore.from_dataset(ds, device=DEV)


def build(ds, fused=True, extras=False):
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table
    scene, targets = D.hand_scene_from_batch(ds.view_batch(IDS), ds[0]["bones_rest"], 2000, grid_res=24, seed=1, device=DEV)
    return HipViewCompute(scene, targets, camera_table(scene["cameras"], DEV), loss="l1+ssim", fused=fused, pose_grad=extras, skin_grid_grad=extras)


def refiner(store, **kw):
    from manus_amd.exposure import ExposureRefiner
    return ExposureRefiner(store.camera_keys, device=DEV, **dict(dict(frozen=(store.camera_keys[0],)), **kw))


def others(ds, hc):
    from manus_amd.optim import SkinGridRefiner
    from manus_amd.pose import PoseRefiner
    return (PoseRefiner(ds.index_list, hc.s["rest"].shape[0], hc.s["rest"], 2e-3, 1e-3, device=DEV), SkinGridRefiner(hc.grid, lr=2e-3, prior_weight=0.5))


def schedule(store):
    from manus_amd.engine import FrameSchedule
    return FrameSchedule(store, V, seed=SEED)


def snapshot(hc, ref, extra=None):
    out = {k: v.detach().clone() for k, v in hc.params.items()}
    out.update({k: getattr(ref, k).clone() for k in STATE})
    out.update({k: v.clone() for k, v in (extra or {}).items()})
    return out


def same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def compare(a, b, what):
    assert len(a) == len(b)
    for gs, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x["loss"], y["loss"]), (what, gs)
        assert x["steps"] == y["steps"], (what, gs)
        same(x["state"], y["state"], "%s, step %d" % (what, gs))


def _extra_state(pose, grid, hc):
    return {} if pose is None else dict(rotvec=pose.rotvec, trans=pose.trans, grid=hc.grid.data)


def trainer_run(capture, fused=True, steps=STEPS, extras=False, on_step=None, exposure=True):
    from manus_amd.engine import Trainer
    ds, store = capture
    hc = build(ds, fused, extras)
    ref = refiner(store)
    kw = dict(KW)
    pose = grid = None
    if extras:
        pose, grid = others(ds, hc)
        kw.update(pose=pose, pose_from_iter=1, pose_every=2, skin_grid=grid, skin_grid_from_iter=1, skin_grid_every=2)
    if exposure:
        kw.update(exposure=ref, exposure_from_iter=FROM, exposure_every=EVERY)
    tr = Trainer(hc, V, frames=schedule(store), **kw)
    log = []
    for gs in range(steps):
        if on_step is not None:
            on_step(gs, tr, hc)
        out = tr.train_step()
        assert out["changed"] is False
        assert ("d_exposure" in out) == (exposure and gs >= FROM), gs
        if exposure and gs >= FROM:
            assert hc.exposure_ids[:V] == tr.exposure.rows_of(store, tr.last_items)     # the ids follow the drawn items
        log.append(dict(loss=out["loss"].detach().clone(), state=snapshot(hc, tr.exposure or ref, _extra_state(pose, grid, hc)),
                        steps=(tr.exposure or ref).steps))
    return log, hc, tr


def hand_loop(capture, fused=True, steps=STEPS, extras=False):
    """The same steps written out: items, load_step, the table rows of the items, the step, the Gaussians' optimizer, the pose
    corrections' step, the grid's step, the table's step."""
    from manus_amd.optim import GaussianOptimizer
    ds, store = capture
    hc = build(ds, fused, extras)
    ref = refiner(store)
    ref.attach(hc, [-1] * int(hc.cams.shape[0]))
    pose, grid = others(ds, hc) if extras else (None, None)
    sched = schedule(store)
    opt = GaussianOptimizer(hc.params, opts=OPTS, spatial_lr_scale=0.05, adopt=True)
    log = []
    for gs in range(steps):
        items = sched.items(gs)
        store.load_step(hc, items, masks=hc.mask_targets is not None, lpips_rects=hc.lpips_rects is not None, scene_masks=True)
        rows = ref.rows_of(store, items)
        hc.exposure_ids = rows + list(hc.exposure_ids[len(rows):])
        hc.exposure_on = gs >= FROM
        side = extras and gs >= 1 and (gs - 1) % 2 == 0
        if side:
            frames = pose.frames_of(store, items)
            pose.apply(hc, IDS, frames)
        out = hc(IDS, 1.0 / V)
        rec = dict(loss=out["loss"].detach().clone())
        opt.update_learning_rate(gs)
        opt.step(out["grads"])
        hc.mark_params_changed()
        if side:
            pose.step(out["d_transforms"], IDS, frames)
            grid.step(out["d_skin_grid"])
        if gs >= FROM and (gs - FROM) % EVERY == 0:
            ref.step(out["d_exposure"], IDS, rows)
        rec.update(state=snapshot(hc, ref, _extra_state(pose, grid, hc)), steps=ref.steps)
        log.append(rec)
    return log


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_equals_the_hand_written_loop(capture, fused):
    a, hc, tr = trainer_run(capture, fused)
    compare(a, hand_loop(capture, fused), "fused=%s" % fused)
    assert [r["steps"] for r in a] == [0, 0, 1, 1, 2, 2]
    ident = R.identity_table(4).float().to(DEV)
    assert torch.equal(a[1]["state"]["E"], ident) and not torch.equal(a[2]["state"]["E"], ident)
    assert torch.equal(a[3]["state"]["E"], a[2]["state"]["E"])            # off schedule: the gradient is formed and ignored
    assert torch.equal(a[5]["state"]["E"][0], ident[0])                   # the frozen camera never moves
    assert not bool(a[5]["state"]["m"][0].any())
    # steps 0 and 1: the Trainer without the keyword
    plain = trainer_run(capture, fused, steps=4, exposure=False)[0]
    leaves = list(hc.params)
    for gs in range(2):
        assert torch.equal(plain[gs]["loss"], a[gs]["loss"])
        for k in leaves:
            assert torch.equal(plain[gs]["state"][k], a[gs]["state"][k]), (gs, k)
    # (step 2 runs with the identity table, which moves behind it: step 3 is the first that sees another image)
    assert not torch.equal(plain[3]["loss"], a[3]["loss"])


def test_together_with_pose_and_skin_grid(capture):
    a = trainer_run(capture, extras=True)[0]
    compare(a, hand_loop(capture, extras=True), "with pose= and skin_grid=")
    assert float(a[5]["state"]["rotvec"].abs().max()) > 0.0 and not torch.equal(a[0]["state"]["grid"], a[1]["state"]["grid"])
    assert [r["steps"] for r in a] == [0, 0, 1, 1, 2, 2]


def test_state_through_a_checkpoint_resumes_bit_for_bit(capture, tmp_path):
    from manus_amd import checkpoint
    _, store = capture
    a = trainer_run(capture)[0]
    swapped = []

    def swap(gs, tr, hc):
        if gs != 4:
            return
        path = checkpoint.save_checkpoint(str(tmp_path), hc.params, 0, gs, 0.0, extra_state={"exposure_refiner": tr.exposure.state_dict()})
        state = checkpoint.load_checkpoint(path, return_checkpoint=True)[2]["exposure_refiner"]
        assert sorted(state) == sorted(["camera_keys", "steps", "E", "m", "v"])
        fresh = refiner(store)
        fresh.load_state_dict(state)
        assert fresh.steps == 1
        fresh.attach(hc, hc.exposure_ids)
        swapped.append(fresh)
        tr.exposure = fresh

    log, hc, tr = trainer_run(capture, on_step=swap)
    assert len(swapped) == 1 and tr.exposure is swapped[0] and hc.exposure is swapped[0].E and tr.exposure.steps == 2
    compare(a, log, "through a checkpoint")


def test_across_a_densification_that_changes_n(capture):
    """Fixed views, one table row per view row, densification on: Trainer(exposure=) against a Trainer without it and the
    switch / step by hand around train_step."""
    from manus_amd.engine import Trainer
    from manus_amd.exposure import ExposureRefiner
    ds, _ = capture
    opts = dict(OPTS, densify_from_step=0, densify_until_step=100, densification_interval=2, min_opacity_threshold=0.3)
    logs = []
    for by_hand in (False, True):
        torch.manual_seed(0)                       # (the split noise of a densification)
        hc = build(ds)
        ref = ExposureRefiner(["a", "b", "c"], device=DEV)
        kw = dict(KW, opts=opts)
        if by_hand:
            ref.attach(hc)
            tr = Trainer(hc, V, **kw)
        else:
            tr = Trainer(hc, V, exposure=ref, exposure_from_iter=1, exposure_every=1, **kw)
            assert hc.exposure is ref.E and hc.exposure_ids == IDS
        log = []
        for gs in range(5):
            if by_hand:
                hc.exposure_on = gs >= 1
            out = tr.train_step()
            if by_hand and gs >= 1:
                ref.step(out["d_exposure"], IDS, IDS)
            log.append(dict(loss=out["loss"].detach().clone(), state=snapshot(tr.compute, ref), steps=ref.steps, N=tr.opt.N))
        logs.append(log)
    compare(logs[0], logs[1], "across a densification")
    ns = [r["N"] for r in logs[0]]
    assert ns == [r["N"] for r in logs[1]] and len(set(ns)) > 1, ns
    assert [r["steps"] for r in logs[0]] == [0, 1, 2, 3, 4]


def test_more_than_one_rank_is_refused(capture):
    from manus_amd.engine import Trainer
    ds, store = capture
    with pytest.raises(ValueError, match="world_size == 1"):
        Trainer(build(ds), V, world_size=2, exposure=refiner(store), **KW)


def test_validate_on_the_corrected_render(capture):
    from manus_amd import ops
    from manus_amd.engine import Trainer
    from manus_amd.exposure import ExposureRefiner
    from manus_amd.validation import psnr_from_sums
    ds, _ = capture
    hc = build(ds)
    plain = Trainer(build(ds), V, **KW).validate([2, 0, 1], group=3)
    ref = ExposureRefiner(["a", "b"], device=DEV)
    ref.E.copy_(R.table(2, seed=4).float())
    ref.attach(hc, [1, -1, 0])
    tr = Trainer(hc, V, exposure=ref, exposure_from_iter=100, **KW)
    ids = [2, 0, 1]
    hc.exposure_on = False                     # the training schedule's switch: validation does not ask it, and leaves it
    res = tr.validate(ids, group=3, exposure=True)
    assert hc.exposure_on is False
    with torch.no_grad():
        img = hc.forward_views(ids)[0]
    tgt = hc.targets[ids].contiguous()
    corr = ops.exposure_forward(img, ref.E, [0, 1, -1])
    assert torch.equal(corr[2], img[2]) and not torch.equal(corr[0], img[0])       # a view with id -1 is taken as it is
    sq, ss, gmax = ops.eval_views(corr, tgt, None)
    n = float(img[0].numel())
    assert res["psnr"] == psnr_from_sums(sq, n).cpu().tolist() and res["ssim"] == (ss / n).cpu().tolist()
    assert torch.equal(res["images"], ops.eval_triptych(corr, tgt, gmax))
    # without the keyword: as without a table
    again = tr.validate(ids, group=3)
    assert again["psnr"] == plain["psnr"] and again["ssim"] == plain["ssim"] and torch.equal(again["images"], plain["images"])
    assert again["psnr"] != res["psnr"]
    with pytest.raises(ValueError, match="no exposure table"):
        Trainer(build(ds), V, **KW).validate(ids, exposure=True)


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: planted per-camera gains
# ---------------------------------------------------------------------------------------------------------------------------
GAINS = (1.0, 0.8, 1.25)
E2E_STEPS = 60


@functools.lru_cache(maxsize=None)
def gain_scene():
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=2000, kind="hand", seed=6, grid_res=24, n_cameras=V, width=64, height=48, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device=DEV)
    ct = camera_table(sc["cameras"], DEV)
    with torch.no_grad():
        img = HipViewCompute(sc, torch.zeros((V, 3, 48, 64), device=DEV), ct).forward_views(IDS)[0]
    gains = torch.tensor(GAINS, device=DEV)[:, None, None, None]
    return sc, ct, (img * gains).contiguous()


def test_planted_gains_end_to_end():
    """Targets rendered from the scene itself and multiplied per camera by planted gains, camera 0 frozen.  Two orderings, no
    threshold: the run with the table ends at a lower loss than the run without, and every unfrozen camera's diagonal ends
    nearer its planted gain than it started.  Measured figures: DESIGN.md section 6."""
    from manus_amd.engine import HipViewCompute, Trainer
    from manus_amd.exposure import ExposureRefiner
    sc, ct, tg = gain_scene()
    finals = {}
    for with_table in (False, True):
        hc = HipViewCompute(sc, tg, ct, loss="l1")
        kw = dict(KW, bg_white=False)
        ref = ExposureRefiner(["c0", "c1", "c2"], frozen=("c0",), device=DEV)
        tr = Trainer(hc, V, exposure=ref, **kw) if with_table else Trainer(hc, V, **kw)
        losses = [tr.train_step()["loss"].detach().clone() for _ in range(E2E_STEPS)]
        finals[with_table] = float(torch.stack(losses[-5:]).mean())
        if with_table:
            diag = torch.stack([ref.E[:, c, c] for c in range(3)]).mean(0).cpu().tolist()
            print("diagonals (mean over the channels) %s, planted %s" % (["%.4f" % d for d in diag], GAINS))
            assert diag[0] == 1.0
            for k in (1, 2):
                assert abs(diag[k] - GAINS[k]) < abs(1.0 - GAINS[k]), (k, diag[k])
    print("loss (mean of the last 5 of %d steps): without the table %.5e, with it %.5e" % (E2E_STEPS, finals[False], finals[True]))
    assert finals[True] < finals[False]

"""GPU: `engine.Trainer(pose=...)` with a `pose.KinematicPoseRefiner` -- the Trainer is duck-typed on the refiner's surface
(`frames_of`, `apply`, `hold`, `step`, `steps`, `last_prior`) -- against hand-written loops, bit for bit (the step is
bit-reproducible at this size: DESIGN.md section 6, frame ingest).

Set-up of tests/test_gpu_pose_prior_trainer.py: a synthetic capture of 3 frames x 4 cameras at 64x48, 2000 Gaussians, l1+ssim step
with pose_grad on both routes, 3 views per step, densification and pruning off through `opts` except in the test that crosses
one.  The refiner starts at the dataset's own angles with the hand's mask (both global rows free) and joint limits."""
import os

import pytest
import torch

from test_gpu_frames import BASE
from test_gpu_pose_trainer import KW, OPTS

from manus_amd import dataset as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, IDS, STEPS, SEED = 3, [0, 1, 2], 6, 2
FROM, EVERY = 2, 2
HAND = ["bone_%d" % i for i in range(20)]
POSE_STATE = ("theta", "m", "v")


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    from manus_amd.frames import FrameStore
    path = str(tmp_path_factory.mktemp("fk_trainer"))
    D.write_tree(os.path.join(path, "grasp_1.npz"), D.synthetic_sequence(33, n_frames=3, n_cams=4, width=64, height=48))
    ds = D.SequenceDataset(path, dict(BASE, width=64, height=48, resize_factor=1.0), "train")
    return ds, FrameStore.from_dataset(ds, device=DEV)


def build(ds, fused=True, skin_grid_grad=False):
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table
    scene, targets = D.hand_scene_from_batch(ds.view_batch(IDS), ds[0]["bones_rest"], 2000, grid_res=24, seed=1, device=DEV)
    return HipViewCompute(scene, targets, camera_table(scene["cameras"], DEV), loss="l1+ssim", fused=fused, pose_grad=True,
                          skin_grid_grad=skin_grid_grad)


def refiner(ds, hc):
    from manus_amd.pose import KinematicPoseRefiner, dof_mask, joint_limits, theta_from_bones
    first = {}
    for i, k in enumerate(ds.index_list):
        first.setdefault((k[0], k[1]), i)
    bones = [ds[i]["bones_posed"] for i in first.values()]
    return KinematicPoseRefiner(ds.index_list, hc.s["rest"], bones[0].kintree, theta_from_bones(bones), 2e-3, 1e-3,
                                mask=dof_mask(HAND, True, True), limits=joint_limits(HAND), device=DEV)


def schedule(store):
    from manus_amd.engine import FrameSchedule
    return FrameSchedule(store, V, seed=SEED)


def snapshot(hc, ref, grid=False):
    out = {k: v.detach().clone() for k, v in hc.params.items()}
    out.update({k: getattr(ref, k).clone() for k in POSE_STATE if getattr(ref, k) is not None})
    if grid:
        out["grid"] = hc.grid.data.clone()
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


def trainer_run(capture, fused=True, steps=STEPS, on_step=None, skin=False, **trainer_kw):
    """Trainer(frames=, pose=, pose_from_iter=FROM, pose_every=EVERY, **trainer_kw) -> (log, compute, trainer)"""
    from manus_amd.engine import Trainer
    from manus_amd.optim import SkinGridRefiner
    ds, store = capture
    hc = build(ds, fused, skin_grid_grad=skin)
    ref = refiner(ds, hc)
    if skin:
        trainer_kw = dict(trainer_kw, skin_grid=SkinGridRefiner(hc.grid, lr=2e-3, prior_weight=0.5), skin_grid_from_iter=1, skin_grid_every=2)
    tr = Trainer(hc, V, frames=schedule(store), pose=ref, pose_from_iter=FROM, pose_every=EVERY, **dict(KW, **trainer_kw))
    log = []
    for gs in range(steps):
        if on_step is not None:
            on_step(gs, tr, hc)
        out = tr.train_step()
        assert out["changed"] is False and "loss_pose_prior" not in out and tr.pose.last_prior is None
        log.append(dict(loss=out["loss"].detach().clone(), state=snapshot(hc, tr.pose, grid=skin), steps=tr.pose.steps))
    return log, hc, tr


def hand_loop(capture, fused=True, steps=STEPS, hold=False, skin=False):
    """The same steps written out: items, load_step, apply (or hold), the step, the Gaussians' optimizer, the angles' step, the
    grid's step."""
    from manus_amd.optim import GaussianOptimizer, SkinGridRefiner
    ds, store = capture
    hc = build(ds, fused, skin_grid_grad=skin)
    ref = refiner(ds, hc)
    sched = schedule(store)
    grid_ref = SkinGridRefiner(hc.grid, lr=2e-3, prior_weight=0.5) if skin else None
    opt = GaussianOptimizer(hc.params, opts=OPTS, spatial_lr_scale=0.05, adopt=True)
    log = []
    for gs in range(steps):
        items = sched.items(gs)
        store.load_step(hc, items, masks=hc.mask_targets is not None, lpips_rects=hc.lpips_rects is not None, scene_masks=True)
        rows = ref.frames_of(store, items)
        due = gs >= FROM and (gs - FROM) % EVERY == 0
        if due:
            ref.apply(hc, IDS, rows)
        elif hold and gs >= FROM:
            ref.hold(hc, IDS, rows)
        out = hc(IDS, 1.0 / V)
        rec = dict(loss=out["loss"].detach().clone())
        opt.update_learning_rate(gs)
        opt.step(out["grads"])
        hc.mark_params_changed()
        if due:
            ref.step(out["d_transforms"], IDS, rows)
        if skin and gs >= 1 and (gs - 1) % 2 == 0:
            grid_ref.step(out["d_skin_grid"])
        rec.update(state=snapshot(hc, ref, grid=skin), steps=ref.steps)
        log.append(rec)
    return log


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_equals_the_hand_written_loop(capture, fused):
    a = trainer_run(capture, fused)[0]
    compare(a, hand_loop(capture, fused), "fused=%s" % fused)
    assert [r["steps"] for r in a] == [0, 0, 1, 1, 2, 2]
    assert "m" not in a[1]["state"] and "m" in a[2]["state"]
    assert torch.equal(a[1]["state"]["theta"], a[0]["state"]["theta"]) and not torch.equal(a[2]["state"]["theta"], a[1]["state"]["theta"])
    # only free entries of the frames a step showed have moved, and they lie inside the limits
    ds, _ = capture
    ref = refiner(ds, build(ds, fused))
    moved = (a[-1]["state"]["theta"] != ref.theta)
    assert bool(moved.any()) and not bool(moved[:, ref.mask == 0].any())
    assert bool((a[-1]["state"]["theta"][moved] >= ref.lo.expand_as(moved)[moved]).all())
    assert bool((a[-1]["state"]["theta"][moved] <= ref.hi.expand_as(moved)[moved]).all())


@pytest.mark.parametrize("fused", [True, False])
def test_pose_hold_equals_the_hand_loop_that_holds(capture, fused):
    held = trainer_run(capture, fused, pose_hold=True)[0]
    compare(held, hand_loop(capture, fused, hold=True), "pose_hold=True, fused=%s" % fused)       # (hold at steps 3 and 5)
    loose = trainer_run(capture, fused)[0]
    for gs in range(3):
        same(held[gs]["state"], loose[gs]["state"], "before the first held step, %d" % gs)
    assert [r["steps"] for r in held] == [r["steps"] for r in loose] == [0, 0, 1, 1, 2, 2]
    leaves = [k for k in held[0]["state"] if k not in POSE_STATE]
    assert not torch.equal(held[3]["loss"], loose[3]["loss"])
    assert any(not torch.equal(held[3]["state"][k], loose[3]["state"][k]) for k in leaves)


def test_together_with_skin_grid_refinement(capture):
    a = trainer_run(capture, skin=True, pose_hold=True)[0]
    compare(a, hand_loop(capture, skin=True, hold=True), "with skin_grid")
    assert not torch.equal(a[0]["state"]["grid"], a[1]["state"]["grid"]) and torch.equal(a[1]["state"]["grid"], a[2]["state"]["grid"])


def test_state_through_a_checkpoint_resumes_bit_for_bit(capture, tmp_path):
    """Before step 4 (one step of the angles behind it) the refiner's state goes through `save_checkpoint(extra_state=)` /
    `load_checkpoint` into a FRESH refiner, which takes the old one's place: the run is the uninterrupted one."""
    from manus_amd import checkpoint
    ds, _ = capture
    a = trainer_run(capture, pose_hold=True)[0]
    swapped = []

    def swap(gs, tr, hc):
        if gs != 4:
            return
        path = checkpoint.save_checkpoint(str(tmp_path), hc.params, 0, gs, 0.0, extra_state={"pose_refiner": tr.pose.state_dict()})
        state = checkpoint.load_checkpoint(path, return_checkpoint=True)[2]["pose_refiner"]
        assert sorted(state) == sorted(["frame_keys", "steps", "theta", "m", "v"])
        fresh = refiner(ds, hc)
        assert fresh.steps == 0 and fresh.m is None and not torch.equal(fresh.theta, tr.pose.theta)
        fresh.load_state_dict(state)
        assert fresh.steps == 1 and torch.equal(fresh.theta, tr.pose.theta)
        swapped.append((tr.pose, fresh))
        tr.pose = fresh

    log, hc, tr = trainer_run(capture, pose_hold=True, on_step=swap)
    assert len(swapped) == 1 and tr.pose is swapped[0][1] and swapped[0][0].steps == 1 and tr.pose.steps == 2
    compare(a, log, "through a checkpoint")


def test_across_a_densification_that_changes_n(capture):
    """Fixed views with pose_frames = [0, 2, 0], densification on: Trainer(pose=) against a Trainer without it and apply / step
    by hand around train_step."""
    from manus_amd.engine import Trainer
    ds, _ = capture
    opts = dict(OPTS, densify_from_step=0, densify_until_step=100, densification_interval=2, min_opacity_threshold=0.3)
    rows, logs = [0, 2, 0], []
    for by_hand in (False, True):
        torch.manual_seed(0)                       # (the split noise of a densification)
        hc = build(ds)
        ref = refiner(ds, hc)
        start = ref.theta.clone()
        kw = dict(KW, opts=opts)
        tr = Trainer(hc, V, **kw) if by_hand else Trainer(hc, V, pose=ref, pose_frames=rows, **kw)
        log = []
        for gs in range(5):
            if by_hand:
                ref.apply(hc, IDS, rows)
            out = tr.train_step()
            if by_hand:
                ref.step(out["d_transforms"], IDS, rows)
            log.append(dict(loss=out["loss"].detach().clone(), state=snapshot(tr.compute, ref), steps=ref.steps, N=tr.opt.N))
        logs.append(log)
    compare(logs[0], logs[1], "across a densification")
    ns = [r["N"] for r in logs[0]]
    assert ns == [r["N"] for r in logs[1]] and len(set(ns)) > 1, ns
    assert [r["steps"] for r in logs[0]] == [1, 2, 3, 4, 5]
    last = logs[0][-1]["state"]["theta"]
    assert torch.equal(last[1], start[1]) and not torch.equal(last[0], start[0]) and not torch.equal(last[2], start[2])


def test_world_size_above_one_is_refused(capture):
    from manus_amd.engine import Trainer
    ds, store = capture
    hc = build(ds)
    ref = refiner(ds, hc)
    with pytest.raises(ValueError, match="world_size"):
        Trainer(hc, V, frames=schedule(store), pose=ref, world_size=2, **KW)
    with pytest.raises(ValueError, match="world_size"):
        Trainer(hc, V, pose=ref, pose_frames=[0, 0, 0], world_size=2, **KW)

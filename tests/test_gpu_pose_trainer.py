"""GPU: `engine.Trainer(frames=..., pose=...)` -- views drawn from a `FrameStore` by a `FrameSchedule`, a `pose.PoseRefiner`
scheduled around the step -- against a hand-written loop of the same seven steps, bit for bit (the step is bit-reproducible at
this size: DESIGN.md section 6, frame ingest).

Set-up: a synthetic capture of 3 frames x 4 cameras at 64x48, 2000 Gaussians, fused l1+ssim step with pose_grad, 3 views per
step, densification and pruning off through `opts`."""
import os

import numpy as np
import pytest
import torch

from test_gpu_frames import BASE

from manus_amd import dataset as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, IDS, STEPS, SEED = 3, [0, 1, 2], 5, 2
OPTS = dict(densify_from_step=100000, densify_until_step=0, opacity_reset_interval=100000, remove_seg_end=0)
KW = dict(extent=0.3, opts=OPTS, spatial_lr_scale=0.05)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    from manus_amd.frames import FrameStore
    path = str(tmp_path_factory.mktemp("pose_trainer"))
    D.write_tree(os.path.join(path, "grasp_1.npz"), D.synthetic_sequence(33, n_frames=3, n_cams=4, width=64, height=48))
    ds = D.SequenceDataset(path, dict(BASE, width=64, height=48, resize_factor=1.0), "train")
    assert len(ds) == 12
    return ds, FrameStore.from_dataset(ds, device=DEV)


def build(ds, fused=True, pose_grad=True):
    """A compute object on a scene of its own (load_step writes into the scene's tables)."""
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table
    scene, targets = D.hand_scene_from_batch(ds.view_batch(IDS), ds[0]["bones_rest"], 2000, grid_res=24, seed=1, device=DEV)
    return HipViewCompute(scene, targets, camera_table(scene["cameras"], DEV), loss="l1+ssim", fused=fused, pose_grad=pose_grad)


def refiner(ds, hc):
    from manus_amd.pose import PoseRefiner
    return PoseRefiner(ds.index_list, hc.s["rest"].shape[0], hc.s["rest"], 2e-3, 1e-3, device=DEV)


def schedule(store):
    from manus_amd.engine import FrameSchedule
    return FrameSchedule(store, V, seed=SEED)


def snapshot(hc, ref=None):
    out = {k: v.detach().clone() for k, v in hc.params.items()}
    if ref is not None:
        out.update({k: getattr(ref, k).clone() for k in ("rotvec", "trans", "m_r", "v_r", "m_t", "v_t") if getattr(ref, k) is not None})
    return out


def same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module")
def trained(capture):
    """Trainer(frames=, pose=, pose_from_iter=2) over five steps: per step the items, the loss and a snapshot of the state."""
    from manus_amd.engine import Trainer
    ds, store = capture
    hc = build(ds)
    ref = refiner(ds, hc)
    sched = schedule(store)
    tr = Trainer(hc, V, frames=sched, pose=ref, pose_from_iter=2, **KW)
    log = []
    for k in range(STEPS):
        out = tr.train_step()
        assert out["changed"] is False and "d_transforms" in out
        log.append(dict(items=list(tr.last_items), loss=out["loss"].detach().clone(), state=snapshot(hc, ref), steps=ref.steps))
    assert tr.global_step == STEPS
    return log


def test_trainer_equals_the_hand_written_loop(capture, trained):
    from manus_amd.optim import GaussianOptimizer
    ds, store = capture
    hc = build(ds)
    ref = refiner(ds, hc)
    sched = schedule(store)
    opt = GaussianOptimizer(hc.params, opts=OPTS, spatial_lr_scale=0.05, adopt=True)
    for gs in range(STEPS):
        items = sched.items(gs)                                                                         # 1
        store.load_step(hc, items, masks=hc.mask_targets is not None, lpips_rects=hc.lpips_rects is not None, scene_masks=True)    # 2
        rows = None
        if gs >= 2:                                                                                     # 3
            rows = ref.frames_of(store, items)
            ref.apply(hc, IDS, rows)
        out = hc(IDS, 1.0 / V)                                                                          # 4
        loss = out["loss"].detach().clone()
        opt.update_learning_rate(gs)                                                                    # 5
        opt.step(out["grads"])
        hc.mark_params_changed()
        if rows is not None:                                                                            # 6
            ref.step(out["d_transforms"], IDS, rows)
        assert items == trained[gs]["items"], gs                                                        # 7: the next step
        assert torch.equal(loss, trained[gs]["loss"]), gs
        same(snapshot(hc, ref), trained[gs]["state"], "step %d" % gs)
    assert ref.steps == trained[-1]["steps"] == STEPS - 2
    assert float(ref.rotvec.abs().max()) > 0.0 and float(ref.trans.abs().max()) > 0.0
    assert not torch.equal(trained[0]["loss"], trained[1]["loss"])


def test_items_follow_the_schedule_and_pose_starts_at_its_step(capture, trained):
    from manus_amd.engine import Trainer
    ds, store = capture
    sched = schedule(store)
    for k, rec in enumerate(trained):
        assert rec["items"] == sched.items(k), k
        assert rec["steps"] == max(0, k - 1)                          # the corrections step at k = 2, 3, 4
    assert "m_r" not in trained[1]["state"] and "m_r" in trained[2]["state"]
    assert float(trained[1]["state"]["rotvec"].abs().max()) == 0.0
    # up to step 2: the trainer without a refiner
    hc = build(ds)
    tr = Trainer(hc, V, frames=schedule(store), **KW)
    for k in range(2):
        out = tr.train_step()
        assert torch.equal(out["loss"], trained[k]["loss"]), k
        same(snapshot(hc), {n: t for n, t in trained[k]["state"].items() if n in hc.params}, "no refiner, step %d" % k)


def test_constructor_refusals(capture):
    from manus_amd.engine import FrameSchedule, Trainer
    ds, store = capture
    hc = build(ds)
    ref = refiner(ds, hc)
    with pytest.raises(ValueError, match="pose_grad"):
        Trainer(build(ds, pose_grad=False), V, frames=schedule(store), pose=ref, **KW)
    with pytest.raises(ValueError, match="world_size"):
        Trainer(hc, V, frames=schedule(store), pose=ref, world_size=2, **KW)
    with pytest.raises(ValueError, match="world_size"):
        Trainer(hc, V, pose=ref, pose_frames=[0, 0, 0], world_size=2, **KW)
    with pytest.raises(ValueError, match="world_size"):
        Trainer(hc, V, frames=schedule(store), world_size=2, **KW)
    with pytest.raises(ValueError, match="pose_frames"):
        Trainer(hc, V, pose=ref, **KW)
    with pytest.raises(ValueError, match="n_views"):
        Trainer(hc, V, frames=FrameSchedule(store, 4), **KW)


def test_fixed_views_with_pose_frames_and_pose_every(capture):
    """Without a schedule: pose_frames names the frame of each fixed view; pose_every = 2 refines every other step."""
    from manus_amd.engine import Trainer
    ds, store = capture
    hc = build(ds)
    ref = refiner(ds, hc)
    rows = ref.frames_of(store, IDS)
    assert rows == [0, 0, 0]                                          # items 0..2: the cameras of the first frame
    tr = Trainer(hc, V, pose=ref, pose_frames=rows, pose_every=2, **KW)
    for k in range(3):
        tr.train_step()
        assert ref.steps == k // 2 + 1, k
    assert float(ref.rotvec[0].abs().max()) > 0.0 and float(ref.rotvec[1:].abs().max()) == 0.0


def test_modular_route_passes_d_transforms_through(capture):
    from manus_amd.engine import Trainer
    ds, _ = capture
    hc = build(ds, fused=False)
    out = Trainer(hc, V, **KW).train_step()
    assert out["d_transforms"].shape == (V, hc.s["transforms"].shape[1], 4, 4) and float(out["d_transforms"].abs().max()) > 0.0


def test_pruning_inputs_follow_the_drawn_items(capture):
    """Trainer(frames=) on a compute object WITHOUT a mask table, the mask pruning test on (remove_seg_end > 0, the default
    schedule's first 1000 steps): the masks, cameras and keypoints `prune_views` hands the pruning tests are those of the items
    the step drew -- bit for bit the dataset's host batch of `last_items` --, and the mask loss term stays off."""
    from manus_amd.engine import Trainer
    ds, store = capture
    hc = build(ds)
    assert hc.mask_targets is None and torch.is_tensor(hc.s["masks"])
    first = hc.s["masks"].clone()
    tr = Trainer(hc, V, frames=schedule(store), extent=0.3, spatial_lr_scale=0.05,
                 opts=dict(OPTS, remove_seg_end=1000))
    moved = False
    for k in range(3):
        out = tr.train_step()
        assert "loss_mask" not in out and hc.mask_targets is None
        batch = ds.view_batch(tr.last_items)
        want = batch["masks"].to(DEV)
        views = hc.prune_views(IDS)
        for j, view in enumerate(views):
            assert torch.equal(view["mask"].to(want.dtype), want[j]), (k, j)
            assert torch.equal(view["keypoints"].float().cpu(), batch["keypoints"][j].float().cpu()), (k, j)
            for name, val in batch["cameras"][j].items():
                val = np.asarray(val.cpu() if torch.is_tensor(val) else val)
                if val.dtype.kind in "fiu":
                    got = view["camera"][name]
                    assert np.array_equal(np.asarray(got.cpu() if torch.is_tensor(got) else got), val), (k, j, name)
        moved = moved or not torch.equal(hc.s["masks"], first)
    assert moved                      # (the drawn items are not the three the scene was built from)

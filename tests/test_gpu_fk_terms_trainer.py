"""GPU: `engine.Trainer(pose=...)` with a `pose.KinematicPoseRefiner` that carries the terms on its angles (deviation, smoothness,
3-D keypoints from the store) against hand-written loops, bit for bit -- leaves, theta, moments, losses and `loss_pose_prior`.

Set-up of tests/test_gpu_fk_trainer.py: a synthetic capture of 3 frames x 4 cameras at 64x48, 2000 Gaussians, l1+ssim step with
pose_grad on both routes, 3 views per step, refiner from step 2 on every second step."""
import pytest
import torch

from test_gpu_fk_trainer import EVERY, FROM, HAND, IDS, STEPS, V, build, capture, compare, schedule, snapshot, same  # noqa: F401
from test_gpu_pose_trainer import KW, OPTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TERMS = dict(w_dev_rot=0.5, w_smooth_rot=0.25, w_dev_trans=2.0, w_smooth_trans=1.0, w_kp=10.0)


def refiner(ds, store, hc, terms=TERMS, keypoints=True):
    """The refiner of test_gpu_fk_trainer.py plus the terms: theta_ref = theta0, the store's keypoints as targets in the dataset's
    convention, fingertips weighted twice."""
    from manus_amd.pose import KinematicPoseRefiner, dof_mask, joint_limits, keypoint_offsets, keypoints_of_store, theta_from_bones
    first = {}
    for i, k in enumerate(ds.index_list):
        first.setdefault((k[0], k[1]), i)
    bones = [ds[i]["bones_posed"] for i in first.values()]
    ref = KinematicPoseRefiner(ds.index_list, hc.s["rest"], bones[0].kintree, theta_from_bones(bones), 2e-3, 1e-3,
                               mask=dof_mask(HAND, True, True), limits=joint_limits(HAND), device=DEV, **(terms or {}))
    if keypoints:
        rest = ds[0]["bones_rest"]
        b, o = keypoint_offsets(rest.transforms, rest.heads, rest.tails)
        c = torch.ones(21)
        c[[4, 8, 12, 16, 20]] = 2.0
        ref.set_keypoints(b, o, keypoints_of_store(store, ds.index_list), c)
    return ref


def trainer_run(cap, fused=True, steps=STEPS, on_step=None, skin=False, terms=TERMS, keypoints=True, **trainer_kw):
    from manus_amd.engine import Trainer
    from manus_amd.optim import SkinGridRefiner
    ds, store = cap
    hc = build(ds, fused, skin_grid_grad=skin)
    ref = refiner(ds, store, hc, terms, keypoints)
    if skin:
        trainer_kw = dict(trainer_kw, skin_grid=SkinGridRefiner(hc.grid, lr=2e-3, prior_weight=0.5), skin_grid_from_iter=1, skin_grid_every=2)
    tr = Trainer(hc, V, frames=schedule(store), pose=ref, pose_from_iter=FROM, pose_every=EVERY, **dict(KW, **trainer_kw))
    log = []
    for gs in range(steps):
        if on_step is not None:
            on_step(gs, tr, hc)
        out = tr.train_step()
        assert out["changed"] is False
        prior = out.get("loss_pose_prior")
        log.append(dict(loss=out["loss"].detach().clone(), state=snapshot(hc, tr.pose, grid=skin), steps=tr.pose.steps,
                        prior=None if prior is None else prior.detach().clone(),
                        terms=None if prior is None else tr.pose.last_terms.clone()))
    return log, hc, tr


def hand_loop(cap, fused=True, steps=STEPS, hold=False, skin=False, terms=TERMS, keypoints=True):
    from manus_amd.optim import GaussianOptimizer, SkinGridRefiner
    ds, store = cap
    hc = build(ds, fused, skin_grid_grad=skin)
    ref = refiner(ds, store, hc, terms, keypoints)
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
        rec = dict(loss=out["loss"].detach().clone(), prior=None, terms=None)
        opt.update_learning_rate(gs)
        opt.step(out["grads"])
        hc.mark_params_changed()
        if due:
            ref.step(out["d_transforms"], IDS, rows)
            if ref.last_prior is not None:
                rec.update(prior=ref.last_prior.clone(), terms=ref.last_terms.clone())
        if skin and gs >= 1 and (gs - 1) % 2 == 0:
            grid_ref.step(out["d_skin_grid"])
        rec.update(state=snapshot(hc, ref, grid=skin), steps=ref.steps)
        log.append(rec)
    return log


def compare_all(a, b, what):
    compare(a, b, what)
    for gs, (x, y) in enumerate(zip(a, b)):
        assert (x["prior"] is None) == (y["prior"] is None), (what, gs)
        if x["prior"] is not None:
            assert torch.equal(x["prior"], y["prior"]) and torch.equal(x["terms"], y["terms"]), (what, gs)


def priors_at(log):
    return [gs for gs, r in enumerate(log) if r["prior"] is not None]


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_equals_the_hand_written_loop(capture, fused):
    a = trainer_run(capture, fused)[0]
    compare_all(a, hand_loop(capture, fused), "fused=%s" % fused)
    assert [r["steps"] for r in a] == [0, 0, 1, 1, 2, 2] and priors_at(a) == [2, 4]
    for gs in (2, 4):
        p, t = a[gs]["prior"], a[gs]["terms"]
        assert p.dtype == torch.float64 and p.dim() == 0 and p.is_cuda and bool(torch.isfinite(t).all())
        assert float(p) == float(t[3]) == (float(t[0]) + float(t[1])) + float(t[2])
    # step 2 is the first step of the angles: theta = theta_ref, so E_dev is exactly 0 there
    assert float(a[2]["terms"][0]) == 0.0 and float(a[2]["terms"][1]) > 0.0 and float(a[2]["terms"][2]) >= 0.0
    # the terms move the angles: another run than the refiner without them
    plain = trainer_run(capture, fused, terms=None, keypoints=False)[0]
    assert priors_at(plain) == [] and not torch.equal(plain[2]["state"]["theta"], a[2]["state"]["theta"])
    same(plain[1]["state"], a[1]["state"], "before the first step of the angles")


@pytest.mark.parametrize("fused", [True, False])
def test_zero_weights_equal_a_refiner_without_the_keywords(capture, fused):
    zero = trainer_run(capture, fused, terms=dict.fromkeys(TERMS, 0.0))[0]
    plain = trainer_run(capture, fused, terms=None, keypoints=False)[0]
    compare_all(zero, plain, "zero weights, fused=%s" % fused)
    assert priors_at(zero) == []


@pytest.mark.parametrize("fused", [True, False])
def test_pose_hold_equals_the_hand_loop_that_holds(capture, fused):
    held = trainer_run(capture, fused, pose_hold=True)[0]
    compare_all(held, hand_loop(capture, fused, hold=True), "pose_hold=True, fused=%s" % fused)
    assert priors_at(held) == [2, 4]


def test_together_with_skin_grid_refinement(capture):
    a = trainer_run(capture, skin=True, pose_hold=True)[0]
    compare_all(a, hand_loop(capture, skin=True, hold=True), "with skin_grid")
    assert priors_at(a) == [2, 4]


def test_state_through_a_checkpoint_resumes_bit_for_bit(capture, tmp_path):
    """Before step 4 the refiner's state goes through `save_checkpoint(extra_state=)` / `load_checkpoint` into a FRESH refiner
    configured alike (weights, reference and keypoints are configuration): the run is the uninterrupted one."""
    from manus_amd import checkpoint
    ds, store = capture
    a = trainer_run(capture, pose_hold=True)[0]
    swapped = []

    def swap(gs, tr, hc):
        if gs != 4:
            return
        path = checkpoint.save_checkpoint(str(tmp_path), hc.params, 0, gs, 0.0, extra_state={"pose_refiner": tr.pose.state_dict()})
        state = checkpoint.load_checkpoint(path, return_checkpoint=True)[2]["pose_refiner"]
        assert sorted(state) == sorted(["frame_keys", "steps", "theta", "m", "v"])
        fresh = refiner(ds, store, hc)
        assert fresh.steps == 0 and fresh.m is None and torch.equal(fresh.theta_ref, tr.pose.theta_ref)
        fresh.load_state_dict(state)
        assert fresh.steps == 1 and torch.equal(fresh.theta, tr.pose.theta) and not torch.equal(fresh.theta, fresh.theta_ref)
        swapped.append(fresh)
        tr.pose = fresh

    log, hc, tr = trainer_run(capture, pose_hold=True, on_step=swap)
    assert len(swapped) == 1 and tr.pose is swapped[0] and tr.pose.steps == 2
    compare_all(a, log, "through a checkpoint")


def test_across_a_densification_that_changes_n(capture):
    """Fixed views with pose_frames = [0, 2, 0], densification on: Trainer(pose=) against a Trainer without it and apply / step by
    hand around train_step.  Frame 1 is never listed: it is read as a neighbour and stays."""
    from manus_amd.engine import Trainer
    ds, store = capture
    opts = dict(OPTS, densify_from_step=0, densify_until_step=100, densification_interval=2, min_opacity_threshold=0.3)
    rows, logs = [0, 2, 0], []
    for by_hand in (False, True):
        torch.manual_seed(0)                       # (the split noise of a densification)
        hc = build(ds)
        ref = refiner(ds, store, hc)
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
                prior = ref.last_prior
            else:
                prior = out["loss_pose_prior"]
            log.append(dict(loss=out["loss"].detach().clone(), state=snapshot(tr.compute, ref), steps=ref.steps, N=tr.opt.N,
                            prior=prior.clone(), terms=ref.last_terms.clone()))
        logs.append(log)
    compare_all(logs[0], logs[1], "across a densification")
    ns = [r["N"] for r in logs[0]]
    assert ns == [r["N"] for r in logs[1]] and len(set(ns)) > 1, ns
    last = logs[0][-1]["state"]["theta"]
    assert torch.equal(last[1], start[1]) and not torch.equal(last[0], start[0]) and not torch.equal(last[2], start[2])

"""GPU: `engine.Trainer(skin_grid=...)` -- an `optim.SkinGridRefiner` scheduled behind the Gaussians' optimizer step (and the
pose corrections') -- against a second Trainer without the argument plus `refiner.step(out["d_skin_grid"])` by hand on the
scheduled steps, bit for bit.

Set-up: the hand scene of tests/test_gpu_skin_grid_grad.py (`_hand_scene`: 3000 Gaussians, 3 views of 96x64), l1+ssim step with
skin_grid_grad, the Trainer keywords of tests/test_gpu_pose_trainer.py (densification and pruning off through `opts`, except in
the test that crosses one)."""
import pytest
import torch

from test_gpu_pose_trainer import KW, OPTS
from test_gpu_skin_grid_grad import _hand_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 3


def build(fused=True, pose_grad=False, skin_grid_grad=True):
    """A compute object on a scene of its own: every call gives the same scene, targets and grid."""
    from manus_amd.engine import HipViewCompute
    sc, ct = _hand_scene(n=3000, views=V)
    tg = torch.rand((V, 3, 64, 96), device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    return HipViewCompute(sc, tg, ct, loss="l1+ssim", fused=fused, skin_grid_grad=skin_grid_grad, pose_grad=pose_grad)


def refiner(hc, **kw):
    from manus_amd.optim import SkinGridRefiner
    return SkinGridRefiner(hc.grid, **dict(dict(lr=2e-3, prior_weight=0.5), **kw))


def pose_refiner(hc):
    from manus_amd.pose import PoseRefiner
    rest = hc.s["rest"]
    return PoseRefiner([("a", k) for k in range(V)], rest.shape[0], rest, 2e-3, 1e-3, device=DEV)


def snapshot(hc, ref, pose=None):
    out = {k: v.detach().clone() for k, v in hc.params.items()}
    out["grid"] = hc.grid.data.clone()
    out.update({k: getattr(ref, k).clone() for k in ("exp_avg", "exp_avg_sq") if getattr(ref, k) is not None})
    if pose is not None:
        out.update({k: getattr(pose, k).clone() for k in ("rotvec", "trans", "m_r", "v_r") if getattr(pose, k) is not None})
    return out


def same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def run(steps, scheduled, by_hand, fused=True, pose=False, opts=OPTS, seed=0, on_step=None, **ref_kw):
    """`steps` train_steps.  by_hand False: Trainer(skin_grid=, **scheduled); True: a Trainer without the argument, and the
    refiner's step by hand behind train_step on the steps the schedule names.  -> (log, compute, refiner, trainer)"""
    from manus_amd.engine import Trainer
    torch.manual_seed(seed)                       # (the split noise of a densification)
    hc = build(fused=fused, pose_grad=pose)
    ref = refiner(hc, **ref_kw)
    pref = pose_refiner(hc) if pose else None
    kw = dict(dict(KW, opts=opts), **(dict(pose=pref, pose_frames=list(range(V))) if pose else {}))
    tr = Trainer(hc, V, **kw) if by_hand else Trainer(hc, V, skin_grid=ref, **dict(kw, **scheduled))
    frm, every = scheduled.get("skin_grid_from_iter", 0), scheduled.get("skin_grid_every", 1)
    log = []
    for gs in range(steps):
        if on_step is not None:
            on_step(gs, tr, hc)
        v0 = hc.grid.version
        out = tr.train_step()
        due = gs >= frm and (gs - frm) % every == 0
        if by_hand:
            assert "loss_skin_prior" not in out
            if due:
                ref.step(out["d_skin_grid"])
                out["loss_skin_prior"] = ref.last_prior
        assert ("loss_skin_prior" in out) == due, gs
        assert hc.grid.version == v0 + (1 if due else 0), gs
        log.append(dict(loss=out["loss"].detach().clone(), prior=out["loss_skin_prior"].clone() if due else None,
                        state=snapshot(tr.compute, ref, pref), N=tr.opt.N, steps=ref.steps))
    return log, hc, ref, tr


def compare(a, b, what):
    assert len(a) == len(b)
    for gs, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x["loss"], y["loss"]), (what, gs)
        assert (x["prior"] is None) == (y["prior"] is None) and (x["prior"] is None or torch.equal(x["prior"], y["prior"])), (what, gs)
        assert x["N"] == y["N"] and x["steps"] == y["steps"], (what, gs)
        same(x["state"], y["state"], "%s, step %d" % (what, gs))


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_equals_the_hand_stepped_loop(fused):
    sched = dict(skin_grid_from_iter=2, skin_grid_every=2)
    a = run(6, sched, False, fused=fused)[0]
    b = run(6, sched, True, fused=fused)[0]
    compare(a, b, "fused=%s" % fused)
    assert [r["steps"] for r in a] == [0, 0, 1, 1, 2, 2]                     # the grid steps at 2 and 4, nowhere else
    assert "exp_avg" not in a[1]["state"] and "exp_avg" in a[2]["state"]
    assert torch.equal(a[0]["state"]["grid"], a[1]["state"]["grid"]) and not torch.equal(a[1]["state"]["grid"], a[2]["state"]["grid"])
    assert torch.equal(a[2]["state"]["grid"], a[3]["state"]["grid"]) and not torch.equal(a[3]["state"]["grid"], a[4]["state"]["grid"])
    assert float(a[2]["prior"]) == 0.0 and float(a[4]["prior"]) > 0.0         # the value is that of the grid BEFORE the step
    assert not torch.equal(a[0]["loss"], a[5]["loss"])


def test_together_with_pose_refinement_on_fixed_views():
    sched = dict(skin_grid_from_iter=1, skin_grid_every=2)
    a = run(4, sched, False, pose=True)[0]
    b = run(4, sched, True, pose=True)[0]
    compare(a, b, "with pose")
    assert [r["steps"] for r in a] == [0, 1, 1, 2]
    assert float(a[-1]["state"]["rotvec"].abs().max()) > 0.0 and "m_r" in a[-1]["state"]


def test_steps_across_a_densification_that_changes_n():
    opts = dict(OPTS, densify_from_step=0, densify_until_step=100, densification_interval=2, min_opacity_threshold=0.3)
    a = run(5, {}, False, opts=opts)[0]
    b = run(5, {}, True, opts=opts)[0]
    compare(a, b, "across a prune")
    assert a[2]["N"] != a[1]["N"], [r["N"] for r in a]      # the leaves were replaced at step 2
    assert [r["steps"] for r in a] == [1, 2, 3, 4, 5]                             # and the grid stepped there too
    assert not torch.equal(a[1]["state"]["grid"], a[2]["state"]["grid"]) and not torch.equal(a[2]["state"]["grid"], a[3]["state"]["grid"])


def test_constructor_refusals():
    from manus_amd import ops
    from manus_amd.engine import Trainer
    hc = build()
    ref = refiner(hc)
    with pytest.raises(ValueError, match="skin_grid_grad"):
        plain = build(skin_grid_grad=False)
        Trainer(plain, V, skin_grid=refiner(plain), **KW)
    with pytest.raises(ValueError, match="compute.grid"):
        Trainer(hc, V, skin_grid=refiner(build()), **KW)
    with pytest.raises(ValueError, match="compute.grid"):
        from manus_amd.optim import SkinGridRefiner
        Trainer(hc, V, skin_grid=SkinGridRefiner(ops.SkinGrid(hc.grid.dense(), DEV), lr=1e-3), **KW)
    with pytest.raises(ValueError, match="world_size"):
        Trainer(hc, V, skin_grid=ref, world_size=2, **KW)
    for every in (0, -1):
        with pytest.raises(ValueError, match="skin_grid_every"):
            Trainer(hc, V, skin_grid=ref, skin_grid_every=every, **KW)
    Trainer(hc, V, skin_grid=ref, skin_grid_from_iter=3, skin_grid_every=5, **KW)      # and the same arguments without a fault


def test_state_through_a_checkpoint_resumes_bit_for_bit(tmp_path):
    """After two steps the refiner's state goes through `save_checkpoint(extra_state=)` / `load_checkpoint` into a FRESH refiner
    (built on the stepped grid with other hyper-parameters: the state carries moments, step count, prior target and
    hyper-parameters), which takes the old one's place: steps 2 and 3 are those of the uninterrupted run."""
    from manus_amd import checkpoint
    from manus_amd.optim import SkinGridRefiner
    a = run(4, {}, False)[0]

    def swap(gs, tr, hc):
        if gs != 2:
            return
        path = checkpoint.save_checkpoint(str(tmp_path), hc.params, 0, gs, 0.0, extra_state={"skin_grid_refiner": tr.skin_grid.state_dict()})
        state = checkpoint.load_checkpoint(path, return_checkpoint=True)[2]["skin_grid_refiner"]
        fresh = SkinGridRefiner(hc.grid, lr=0.5, prior_weight=0.0, project=False, clamp_min=None)
        assert not torch.equal(fresh.prior, tr.skin_grid.prior)                   # (built on the stepped grid)
        fresh.load_state_dict(state)
        assert fresh.steps == 2 and fresh.lr == 2e-3 and fresh.prior_weight == 0.5 and fresh.project and fresh.clamp_min == 0.0
        tr.skin_grid = fresh
        swapped.append(fresh)

    swapped = []
    log, hc, old, tr = run(4, {}, False, on_step=swap)
    assert len(swapped) == 1 and tr.skin_grid is swapped[0] and old.steps == 2 and swapped[0].steps == 4
    for gs in range(4):
        assert torch.equal(a[gs]["loss"], log[gs]["loss"]), gs
        assert torch.equal(a[gs]["prior"], log[gs]["prior"]), gs
        assert torch.equal(a[gs]["state"]["grid"], log[gs]["state"]["grid"]), gs
        same({k: v for k, v in a[gs]["state"].items() if k in hc.params}, {k: v for k, v in log[gs]["state"].items() if k in hc.params}, "step %d" % gs)
    assert torch.equal(swapped[0].exp_avg, a[-1]["state"]["exp_avg"]) and torch.equal(swapped[0].exp_avg_sq, a[-1]["state"]["exp_avg_sq"])
    assert float(a[3]["prior"]) > 0.0


def test_none_is_the_trainer_without_the_keyword():
    from manus_amd.engine import Trainer
    outs = []
    for kw in ({}, dict(skin_grid=None, skin_grid_from_iter=1, skin_grid_every=3)):
        hc = build()
        tr = Trainer(hc, V, **dict(KW, **kw))
        v0 = hc.grid.version
        rec = []
        for _ in range(3):
            out = tr.train_step()
            assert "loss_skin_prior" not in out and "d_skin_grid" in out
            rec.append(dict({k: v.detach().clone() for k, v in hc.params.items()}, loss=out["loss"].detach().clone(), grid=hc.grid.data.clone()))
        assert hc.grid.version == v0
        outs.append(rec)
    for x, y in zip(*outs):
        same(x, y, "skin_grid=None")

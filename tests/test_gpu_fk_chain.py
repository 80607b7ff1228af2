"""GPU: the device kinematic chain -- mgr_fk_apply / mgr_fk_backward / mgr_fk_adam (csrc/fk.hip) and `pose.KinematicPoseRefiner`
on top of them.

Checker: tests/fk_chain_ref.py, the chain as host torch on `transforms.euler_angles_to_armature_space` in fp64 and fp32 on the
CPU.  Tolerance where one is needed: e_kernel <= 8 * max(e32, 2^-23) in `row_rel_err` (check_rows), per (view, bone) or
(frame, row) row.  Cases: J = 1, one chain of 4, the golden's 20-bone hand, one chain of 32, a root with three children; F = 6,
V = 9, frames [0,1,1,3,-1,0,5,3,1] (2 and 4 are never viewed; 2 is listed), bone 0 of frame 5 at e_1 = pi/2."""
import functools
import os

import pytest
import torch

import fk_chain_ref as R
from fk_chain_ref import F32, F64, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case and their references, computed once and shared (left unchanged by the tests)."""
    inp = R.chain_inputs(name)
    return inp, R.host_chain(inp, F64), R.host_chain(inp, F32)


def apply(inp, frames=None, theta=None):
    """-> transforms (n_all,J+1,4,4), gathered (V,J+1,4,4), posed_out (V,J,4,4), all over a NaN fill."""
    from manus_amd._lib import check, lib, ptr, stream
    J, V = inp["J"], inp["V"]
    table = torch.full((inp["n_all"], J + 1, 4, 4), NAN, device=DEV)
    g = torch.full((V, J + 1, 4, 4), NAN, device=DEV)
    po = torch.full((V, J, 4, 4), NAN, device=DEV)
    args = [_i32(inp["rows"]), _i32(inp["frames"] if frames is None else frames), _dev(inp["posed"]), _dev(inp["rest"]), _dev(inp["local"]),
            _i32(inp["parents"]), _dev(inp["base"]), _dev(inp["theta"] if theta is None else theta)]      # (kept alive over the call)
    check(lib().mgr_fk_apply(V, J, inp["F"], *[ptr(t) for t in args], ptr(table), ptr(g), ptr(po), stream()), "mgr_fk_apply")
    return table, g, po


def backward(inp, listed, pad_rows=1, dT=None, frames=None):
    """-> d_theta (U + pad_rows, J+2, 3) over a NaN fill: the rows behind U are not the kernel's to write."""
    from manus_amd._lib import check, lib, ptr, stream
    J, V, U = inp["J"], inp["V"], len(listed)
    out = torch.full((U + pad_rows, J + 2, 3), NAN, device=DEV)
    args = [_i32(listed), _i32(inp["rows"]), _i32(inp["frames"] if frames is None else frames), _dev(inp["rest"]), _dev(inp["local"]),
            _i32(inp["parents"]), _dev(inp["base"]), _dev(inp["theta"]), _dev(inp["mask"]), _dev(inp["dT"] if dT is None else dT)]
    check(lib().mgr_fk_backward(V, J, inp["F"], U, *[ptr(t) for t in args], ptr(out), stream()), "mgr_fk_backward")
    return out


# =================================================================================================================
# apply
# =================================================================================================================
@pytest.mark.parametrize("name", R.CASES)
def test_apply(name):
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.transforms import bone_transforms
    inp, (T64, M64, _), (T32, M32, _) = case(name)
    J, V = inp["J"], inp["V"]
    table, g, po = apply(inp)
    assert torch.equal(g, table[inp["rows"]])                                             # gathered = the table's rows
    others = [v for v in range(inp["n_all"]) if v not in inp["rows"]]
    assert bool(torch.isnan(table[others]).all())                                         # views not listed are not touched
    rows = lambda x: x[:, :J].reshape(V * J, 16)
    check_rows("fk apply T %s" % name, rows(g), rows(T64), rows(T32))
    check_rows("fk apply M %s" % name, po.reshape(V * J, 16), M64.reshape(V * J, 16), M32.reshape(V * J, 16))
    # the view without a frame: the bits of mgr_bone_transforms on its posed row, which posed_out hands through
    posed, rest = _dev(inp["posed"]), _dev(inp["rest"])
    k = inp["frames"].index(-1)
    v = inp["rows"][k]
    assert torch.equal(g[k], bone_transforms(posed[v], rest)) and torch.equal(po[k], posed[v])
    for frames in ([-1] * V, [inp["F"]] * V):                                            # every view without a frame, or past the table
        t2, g2, po2 = apply(inp, frames=frames)
        want = torch.stack([bone_transforms(posed[v], rest) for v in inp["rows"]])
        assert torch.equal(g2, want) and torch.equal(t2[inp["rows"]], want) and torch.equal(po2, posed[inp["rows"]])
    # the background row: mgr_pose_apply's
    zero = torch.zeros((inp["F"], J, 3), device=DEV)
    pt = torch.full((inp["n_all"], J + 1, 4, 4), NAN, device=DEV)
    pg = torch.full((V, J + 1, 4, 4), NAN, device=DEV)
    keep = [_i32(inp["rows"]), _i32(inp["frames"])]
    check(lib().mgr_pose_apply(V, J, inp["F"], ptr(keep[0]), ptr(keep[1]), ptr(posed), ptr(rest), ptr(zero), ptr(zero), ptr(pt), ptr(pg), stream()),
          "mgr_pose_apply")
    assert torch.equal(g[:, J], pg[:, J]) and torch.equal(table[inp["rows"]][:, J], pt[inp["rows"]][:, J])
    assert torch.equal(g[:, J], torch.eye(4, device=DEV).expand(V, 4, 4))
    # without the optional outputs
    J1 = torch.full((inp["n_all"], J + 1, 4, 4), NAN, device=DEV)
    args = [_i32(inp["rows"]), _i32(inp["frames"]), posed, rest, _dev(inp["local"]), _i32(inp["parents"]), _dev(inp["base"]), _dev(inp["theta"])]
    check(lib().mgr_fk_apply(V, J, inp["F"], *[ptr(t) for t in args], ptr(J1), None, None, stream()), "mgr_fk_apply")
    assert torch.equal(J1[inp["rows"]], table[inp["rows"]])


# =================================================================================================================
# backward
# =================================================================================================================
@pytest.mark.parametrize("name", R.CASES)
def test_backward(name):
    inp, (_, _, g64), (_, _, g32) = case(name)
    J, F, listed = inp["J"], inp["F"], inp["listed"]
    U = len(listed)
    got = backward(inp, listed)
    rows = lambda x: x.reshape(-1, 3)
    check_rows("fk backward d_theta %s" % name, rows(got[:U]), rows(g64[listed]), rows(g32[listed]))
    off = _dev(inp["mask"]) == 0
    assert bool(off.any()) and bool((got[:U][:, off] == 0.0).all())                       # masked entries: exactly 0
    assert bool((got[listed.index(2)] == 0.0).all())                                       # listed, never viewed: zeros
    assert bool(torch.isnan(got[U:]).all())                                                # rows behind U are untouched
    # the gimbal frame: finite, and within the bound on its own
    u = listed.index(R.GIMBAL_FRAME)
    assert bool(torch.isfinite(got[u]).all())
    check_rows("fk backward gimbal frame %s" % name, got[u], g64[R.GIMBAL_FRAME], g32[R.GIMBAL_FRAME])
    # two runs: equal bits; a permuted list: equal bits per frame, nothing else written
    assert torch.equal(backward(inp, listed)[:U], got[:U])
    perm = [3, 5, 0, 2, 1]
    p = backward(inp, perm, pad_rows=2)
    for u2, f in enumerate(perm):
        assert torch.equal(p[u2], got[listed.index(f)]), f
    assert bool(torch.isnan(p[U:]).all())
    part = backward(inp, [5, 1], pad_rows=3)
    assert torch.equal(part[0], got[listed.index(5)]) and torch.equal(part[1], got[listed.index(1)]) and bool(torch.isnan(part[2:]).all())
    outside = backward(inp, [inp["F"], -1, 4])                                             # outside the table, and the unviewed frame 4
    assert bool((outside[:3] == 0.0).all())
    # a NaN in one view's d_transforms stays in that frame's rows
    k = 3
    f_bad = inp["frames"][k]
    dT = inp["dT"].clone()
    dT[k, 0, 1, 2] = NAN
    bad = backward(inp, listed, dT=dT)
    for u2, f in enumerate(listed):
        if f == f_bad:
            assert bool(torch.isnan(bad[u2]).any())
            assert bool((bad[u2][off] == 0.0).all())                                       # (masked entries stay exactly 0 even there)
        else:
            assert torch.equal(bad[u2], got[u2]), f
    # views without a frame contribute nothing: the chain over the remaining positions
    fewer = [-1 if q % 3 == 0 else f for q, f in enumerate(inp["frames"])]
    _, _, f64 = R.host_chain(inp, F64, frames=fewer)
    _, _, f32 = R.host_chain(inp, F32, frames=fewer)
    check_rows("fk backward, fewer views %s" % name, rows(backward(inp, listed, frames=fewer)[:U]), rows(f64[listed]), rows(f32[listed]))
    assert bool((backward(inp, listed, frames=[-1] * inp["V"])[:U] == 0.0).all())


# =================================================================================================================
# Adam
# =================================================================================================================
ADAM_LISTS = ([0, 1, 3], [1, 2, 3, 5], [0, 5])          # of F = 6: frame 4 is never listed
ADAM_LR = (0.01, 0.003)


def adam_inputs(inp, limits):
    J, F = inp["J"], inp["F"]
    g = torch.Generator().manual_seed(700 + J)
    grads = [R.rounded(torch.randn((len(l), J + 2, 3), generator=g, dtype=F64) * 10.0 ** float(k - 1)) for k, l in enumerate(ADAM_LISTS)]
    inf = torch.full((J + 2, 3), float("inf"), dtype=F64)
    if not limits:
        return grads, -inf, inf
    # about a third of the entries get a range so narrow around the start of frame 0 that steps run into it
    narrow = torch.rand((J + 2, 3), generator=g) < 0.33
    centre = inp["theta"][0]
    lo, hi = torch.where(narrow, centre - 0.004, -inf), torch.where(narrow, centre + 0.004, inf)
    return grads, R.rounded(lo), R.rounded(hi)


def run_adam(inp, grads, mask, lo, hi):
    from manus_amd._lib import check, lib, ptr, stream
    J = inp["J"]
    x = _dev(inp["theta"])
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    keep = [_dev(mask), _dev(lo), _dev(hi)]
    for step, (l, g) in enumerate(zip(ADAM_LISTS, grads), 1):
        lt, gd = _i32(l), _dev(g)
        check(lib().mgr_fk_adam(len(l), J, ptr(lt), ptr(gd), ptr(x), ptr(m), ptr(v), *[ptr(t) for t in keep], ADAM_LR[0], ADAM_LR[1], 0.9, 0.999,
                                1e-8, step, stream()), "mgr_fk_adam")
    return x, m, v


def checker_adam(inp, grads, mask, lo, hi, dtype):
    th = inp["theta"].to(dtype)
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    for step, (l, g) in enumerate(zip(ADAM_LISTS, grads), 1):
        th, m, v = R.adam_step(th, m, v, g, l, mask, lo, hi, ADAM_LR[0], ADAM_LR[1], step)
    return th, m, v


@pytest.mark.parametrize("name", R.CASES)
def test_adam_against_the_restatement(name):
    inp = case(name)[0]
    J, F = inp["J"], inp["F"]
    grads, lo, hi = adam_inputs(inp, limits=True)
    got = run_adam(inp, grads, inp["mask"], lo, hi)
    r64, r32 = checker_adam(inp, grads, inp["mask"], lo, hi, F64), checker_adam(inp, grads, inp["mask"], lo, hi, F32)
    rows = lambda t: t.reshape(F * (J + 2), 3)
    for what, k in (("theta", 0), ("exp_avg", 1), ("exp_avg_sq", 2)):
        check_rows("fk adam %s %s" % (what, name), rows(got[k]), rows(r64[k]), rows(r32[k]))
    start = _dev(inp["theta"])
    off = _dev(inp["mask"]) == 0
    assert torch.equal(got[0][:, off], start[:, off]) and bool((got[1][:, off] == 0).all()) and bool((got[2][:, off] == 0).all())
    assert torch.equal(got[0][4], start[4]) and bool((got[1][4] == 0).all()) and bool((got[2][4] == 0).all())      # never listed
    assert not torch.equal(got[0][0], start[0])
    # inside the limits wherever it moved, and on them exactly where the fp64 run ends on them
    lo_d, hi_d = _dev(lo), _dev(hi)
    moved = [0, 1, 2, 3, 5]
    on = ~off
    assert bool((got[0][moved][:, on] >= lo_d[on]).all()) and bool((got[0][moved][:, on] <= hi_d[on]).all())
    at_hi = (r64[0][moved] == hi) & inp["mask"].bool()
    at_lo = (r64[0][moved] == lo) & inp["mask"].bool()
    if name != "one":
        assert bool(at_hi.any()) and bool(at_lo.any())
    assert torch.equal(got[0][moved][at_hi.to(DEV)], hi_d.expand(len(moved), -1, -1)[at_hi.to(DEV)])
    assert torch.equal(got[0][moved][at_lo.to(DEV)], lo_d.expand(len(moved), -1, -1)[at_lo.to(DEV)])


def test_adam_steps_across_hi_and_lands_on_it():
    inp = case("chain4")[0]
    J = inp["J"]
    ones = torch.ones_like(inp["mask"])
    inf = torch.full_like(inp["mask"], float("inf"))
    hi = R.rounded(inp["theta"][0] + 0.002)                      # the first Adam step moves every entry by lr = 0.01 / 0.003
    grads = [-torch.ones((len(l), J + 2, 3), dtype=F64) for l in ADAM_LISTS]
    x, _, _ = run_adam(inp, grads, ones, -inf, hi)
    assert torch.equal(x[0], _dev(hi))
    lo = R.rounded(inp["theta"][0] - 0.002)
    x, _, _ = run_adam(inp, [-g for g in grads], ones, lo, inf)
    assert torch.equal(x[0], _dev(lo))


@pytest.mark.parametrize("name", ["one", "chain4", "hand"])
def test_adam_without_limits_equals_pose_adam(name):
    """Infinite limits, an all-ones mask: the bits of mgr_pose_adam on the same values split into its two tables -- rows 0..J as
    a rotvec table of J + 1 rows (the rotations' rate), row J+1 as a trans table of one row (the translations' rate)."""
    from manus_amd._lib import check, lib, ptr, stream
    inp = case(name)[0]
    J = inp["J"]
    grads, lo, hi = adam_inputs(inp, limits=False)
    ones = torch.ones_like(inp["mask"])
    got = run_adam(inp, grads, ones, lo, hi)
    start = _dev(inp["theta"])
    for B, sl, which in ((J + 1, slice(0, J + 1), 0), (1, slice(J + 1, J + 2), 1)):
        x = [start[:, sl].clone().contiguous(), start[:, sl].clone().contiguous()]              # rotvec, trans
        m = [torch.zeros_like(x[0]) for _ in range(2)]
        v = [torch.zeros_like(x[0]) for _ in range(2)]
        for step, (l, g) in enumerate(zip(ADAM_LISTS, grads), 1):
            lt, gd = _i32(l), _dev(g)[:, sl].contiguous()
            check(lib().mgr_pose_adam(len(l), B, ptr(lt), ptr(gd), ptr(gd), ptr(x[0]), ptr(x[1]), ptr(m[0]), ptr(v[0]), ptr(m[1]), ptr(v[1]),
                                      ADAM_LR[0], ADAM_LR[1], 0.9, 0.999, 1e-8, step, stream()), "mgr_pose_adam")
        for k, t in enumerate((x, m, v)):
            assert torch.equal(got[k][:, sl], t[which]), (name, B, k)


# =================================================================================================================
# the refiner: residual, posed, and recovery end to end
# =================================================================================================================
HAND = ["bone_%d" % i for i in range(20)]
IDS = [0, 1, 2]
BENT = (6, 2)                    # bone_6 (a PIP joint: `dataset.DOF_X`, `pose.LIMITS_X`), angle 2
STEPS, LR = 60, 5e-3
# The bar for the device loop's final free angles against the fp32 host loop's: twice the difference between the host loop run
# in fp32 and in fp64, which is the restatement's own spread over these 60 Adam steps.  Measured on an MI355X: host fp32 - host
# fp64 2.731e-03 rad, device - host fp32 2.212e-03 rad.
DEV_HOST_BAR = 5.5e-3


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    from test_gpu_frames import BASE
    from manus_amd import dataset as D
    path = str(tmp_path_factory.mktemp("fk_chain"))
    D.write_tree(os.path.join(path, "grasp_1.npz"), D.synthetic_sequence(33, n_frames=3, n_cams=4, width=64, height=48))
    return D.SequenceDataset(path, dict(BASE, width=64, height=48, resize_factor=1.0), "train")


def _compute(ds):
    from manus_amd import dataset as D
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table
    scene, targets = D.hand_scene_from_batch(ds.view_batch(IDS), ds[0]["bones_rest"], 2000, grid_res=24, seed=1, device=DEV)
    return HipViewCompute(scene, targets, camera_table(scene["cameras"], DEV), loss="l1+ssim", fused=True, pose_grad=True)


def _refiner(ds, hc, theta0, **kw):
    from manus_amd.pose import KinematicPoseRefiner, dof_mask, joint_limits
    return KinematicPoseRefiner(ds.index_list, hc.s["rest"], ds[0]["bones_posed"].kintree, theta0, LR, LR, mask=dof_mask(HAND),
                                limits=joint_limits(HAND), device=DEV, **kw)


def _frame_bones(ds):
    """The `bones_posed` record of every frame row, in the refiner's order of rows (first seen first)."""
    first = {}
    for i, k in enumerate(ds.index_list):
        first.setdefault((k[0], k[1]), i)
    return [ds[i]["bones_posed"] for i in first.values()]


def _theta0(ds):
    """The dataset's angles of its three frames, the free ones moved inside the joint limits (the synthetic capture draws
    them without regard to the limits, and the first step would clamp them), the bent angle at -0.3."""
    from manus_amd.pose import dof_mask, joint_limits, theta_from_bones
    th = theta_from_bones(_frame_bones(ds))
    lo, hi = joint_limits(HAND)
    th = torch.where(dof_mask(HAND) != 0, torch.minimum(torch.maximum(th, lo + 0.05), hi - 0.05), th)
    th[:, 1 + BENT[0], BENT[1]] = -0.3
    return th


def test_residual_and_posed(capture):
    from manus_amd.pose import theta_from_bones
    ds = capture
    hc = _compute(ds)
    bones = _frame_bones(ds)
    assert len(bones) == 3
    ref = _refiner(ds, hc, theta_from_bones(bones))
    # items 0..2 are three cameras of the first frame: FK at the dataset's angles reproduces the dataset's matrices
    res = ref.residual(hc, IDS, [0, 0, 0])
    print("FIGURE fk residual at the dataset's angles: %.3e" % res)
    assert res <= 1e-6
    assert ref.residual(hc, IDS, [1, 1, 1]) > 1e-3                                          # another frame's angles do not
    M = ref.posed(IDS, [0, -1, 2], compute=hc)
    assert torch.equal(M[1], hc.s["posed"][1]) and float((M[0] - hc.s["posed"][0]).abs().max()) <= 1e-6
    assert float((M[2].double().cpu() - ref.fk_host()[2]).abs().max()) <= 1e-6
    # a base off the identity shows as a residual, and fit_base removes it
    g = torch.Generator().manual_seed(5)
    ref.base.copy_(R.rigid(g, 3).to(F32).to(DEV))
    assert ref.residual(hc, IDS, [0, 0, 0]) > 1e-2
    ref.fit_base(torch.stack([b.transforms for b in bones]))
    assert ref.residual(hc, IDS, [0, 0, 0]) <= 2e-6


def test_recovery_with_the_kinematic_refiner(capture):
    """2 000 Gaussians, 64x48, three cameras of one frame, the Gaussians frozen.  Targets: the fused forward at theta0 with one
    PIP angle (bone_6, angle 2) bent by 0.2 rad, -0.3 -> -0.5; start: theta0, the hand's mask and limits; 60 steps at 5e-3.
    The device loop runs beside the same loop driven by the host restatement (tests/fk_chain_ref.py, fp32 and fp64 on the CPU)
    on the device's own d_transforms.  Asserted: the loss falls; the bent angle's error ends below half its start (measured: 0.2000 -> 0.0345 rad, ratio 0.173; host loops 0.0367 / 0.0350); every
    non-root bone's head stays at its rest distance from its parent's to 1e-5 (the free-form PoseRefiner has no such property);
    the device's final angles lie within DEV_HOST_BAR of the fp32 host loop's."""
    ds = capture
    hc = _compute(ds)
    rest = hc.s["rest"]
    J, rows = 20, [0, 0, 0]
    th0 = _theta0(ds)
    th_true = th0.clone()
    th_true[0, 1 + BENT[0], BENT[1]] -= 0.2
    truth = _refiner(ds, hc, th_true)
    truth.apply(hc, IDS, rows)
    with torch.no_grad():
        hc.targets = hc.forward_views_fused(IDS)[0].clone()
    err = lambda th: abs(float(th[0, 1 + BENT[0], BENT[1]]) - float(th_true[0, 1 + BENT[0], BENT[1]]))
    # -- the device loop
    ref = _refiner(ds, hc, th0)
    dev_losses = []
    for _ in range(STEPS):
        ref.apply(hc, IDS, rows)
        out = hc(IDS, 1.0 / 3)
        dev_losses.append(float(out["loss"]))
        ref.step(out["d_transforms"], IDS, rows)
    assert ref.steps == STEPS
    dev_theta = ref.theta.cpu()
    # bone lengths: heads of the refined pose (column 3 of T_i applied to the rest heads) against the rest skeleton
    ref.apply(hc, IDS, rows)
    T = hc.s["transforms"][0, :J].double().cpu()
    rest64 = rest.double().cpu()
    heads = (T @ torch.cat([rest64[:, :3, 3], torch.ones((J, 1), dtype=F64)], 1)[..., None])[:, :3, 0]
    parents = ref.parents_host
    kids = [i for i in range(J) if parents[i] >= 0]
    d_pose = torch.stack([(heads[i] - heads[parents[i]]).norm() for i in kids])
    d_rest = torch.stack([(rest64[i, :3, 3] - rest64[parents[i], :3, 3]).norm() for i in kids])
    print("FIGURE fk recovery, bone lengths: max |d_pose - d_rest| %.3e" % float((d_pose - d_rest).abs().max()))
    assert float((d_pose - d_rest).abs().max()) <= 1e-5
    # -- the host loops on the device's own d_transforms
    lo, hi = ref.lo.cpu().double(), ref.hi.cpu().double()
    inp = dict(parents=parents, rest=rest64, base=torch.eye(4, dtype=F64)[None], mask=ref.mask.cpu().double(), posed=None)
    finals, host_losses = {}, {}
    for dtype in (F32, F64):
        th = th0[:1].to(dtype).clone()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        losses = []
        for step in range(1, STEPS + 1):
            leaf = th.clone().requires_grad_(True)
            M = R.fk(leaf, rest64.to(dtype), parents, inp["base"])[0]
            Tm = M @ torch.linalg.inv(rest64.to(dtype))
            with torch.no_grad():
                hc.s["transforms"][IDS, :J] = Tm.detach().to(F32).to(DEV).expand(3, J, 4, 4)
            out = hc(IDS, 1.0 / 3)
            losses.append(float(out["loss"]))
            dT = out["d_transforms"][:, :J].sum(0).to(dtype).cpu()
            grad, = torch.autograd.grad((Tm * dT).sum(), leaf)
            th, m, v = R.adam_step(th, m, v, (grad * inp["mask"].to(dtype)), [0], inp["mask"], lo, hi, LR, LR, step)
        finals[dtype], host_losses[dtype] = th, losses
    free = ref.mask.cpu() != 0
    d_dev = float((dev_theta[0].double() - finals[F32][0].double())[free].abs().max())
    d_host = float((finals[F32][0].double() - finals[F64][0])[free].abs().max())
    print("FIGURE fk recovery, device loop: loss %.6f -> %.6f, bent angle error %.4f -> %.4f rad (ratio %.3f)"
          % (dev_losses[0], dev_losses[-1], err(th0), err(dev_theta), err(dev_theta) / err(th0)))
    print("FIGURE fk recovery, host loop fp32: loss %.6f -> %.6f, bent angle error -> %.4f rad" % (host_losses[F32][0], host_losses[F32][-1], err(finals[F32])))
    print("FIGURE fk recovery, host loop fp64: loss %.6f -> %.6f, bent angle error -> %.4f rad" % (host_losses[F64][0], host_losses[F64][-1], err(finals[F64])))
    print("FIGURE fk recovery, final free angles: device - host fp32 %.3e, host fp32 - host fp64 %.3e" % (d_dev, d_host))
    assert dev_losses[-1] < dev_losses[0]
    assert err(dev_theta) < 0.5 * err(th0)
    assert bool((dev_theta[0][~free] == th0[0][~free]).all()) and torch.equal(dev_theta[1:], th0[1:])
    assert bool((dev_theta[0] >= ref.lo.cpu()).all()) and bool((dev_theta[0] <= ref.hi.cpu()).all())
    assert d_dev <= DEV_HOST_BAR

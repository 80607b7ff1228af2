"""No GPU: the kinematic pose chain (mgr_fk_apply / mgr_fk_backward / mgr_fk_adam, manus_amd.pose.KinematicPoseRefiner) --
the ABI in header, binding and built library; the refusals, all decided before anything touches a device; `dof_mask`,
`joint_limits`, `theta_from_bones` and the validation of `parents`; the checker's gradient (tests/fk_chain_ref.py) against
central differences in fp64; `fit_base`; the refiner's state on CPU tensors; and the fp32 error of the checker itself, which
sets the GPU tests' tolerance."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import fk_chain_ref as R
from fk_chain_ref import F32, F64
from util import row_rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_fk_apply": 15, "mgr_fk_backward": 16, "mgr_fk_adam": 17}
HAND = ["bone_%d" % i for i in range(20)]


def _declared_args(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in NEW_ENTRIES.items():
        args = _declared_args(header, name)
        assert len(args) == arity and args[-1] == "void* stream", (name, args)
        res, bound = _lib.SIGNATURES[name]
        assert len(bound) == arity and res is ctypes.c_int, (name, len(bound))
        assert hasattr(so, name), "%s is not exported by the built library" % name
    assert "fk.hip" in build.SOURCES and "pose_adam.h" in build.HEADERS
    assert _declared_args(header, "mgr_fk_apply")[:3] == ["int V", "int J", "int F"]
    assert _declared_args(header, "mgr_fk_backward")[:5] == ["int V", "int J", "int F", "int U", "const int32_t* frames_listed"]
    assert _lib.SIGNATURES["mgr_fk_adam"][1][10:15] == [ctypes.c_double] * 5


P = ctypes.c_void_p(0x1000)          # a fake pointer: a refusal never dereferences it


def _refused(L, rc, entry, text=None):
    from manus_amd._lib import MGR_EINVAL
    err = L.mgr_last_error()
    assert rc == MGR_EINVAL, (rc, err)
    assert entry in err, err
    if text:
        assert text in err, err


def test_apply_refusals_before_the_device():
    from manus_amd._lib import lib
    L = lib()
    names = ("view_rows", "frame_of_view", "posed", "rest", "local", "parents", "base", "theta", "transforms")

    def call(V=3, J=20, F=4, **null):
        assert set(null) <= set(names)
        return L.mgr_fk_apply(V, J, F, *[(None if null.get(k) else P) for k in names], None, None, None)
    for k in names:
        _refused(L, call(**{k: True}), b"mgr_fk_apply", b"null pointer")
    for kw in (dict(V=0), dict(V=-2), dict(J=0), dict(J=-1), dict(J=33), dict(F=0), dict(F=-1)):
        _refused(L, call(**kw), b"mgr_fk_apply")


def test_backward_refusals_before_the_device():
    from manus_amd._lib import lib
    L = lib()
    names = ("frames_listed", "view_rows", "frame_of_view", "rest", "local", "parents", "base", "theta", "mask", "d_transforms", "d_theta")

    def call(V=3, J=20, F=4, U=2, **null):
        assert set(null) <= set(names)
        return L.mgr_fk_backward(V, J, F, U, *[(None if null.get(k) else P) for k in names], None)
    for k in names:
        _refused(L, call(**{k: True}), b"mgr_fk_backward", b"null pointer")
    for kw in (dict(V=0), dict(V=-2), dict(J=0), dict(J=33), dict(F=0), dict(F=-3), dict(U=0), dict(U=-1)):
        _refused(L, call(**kw), b"mgr_fk_backward")


def test_adam_refusals_before_the_device():
    from manus_amd._lib import lib
    L = lib()
    names = ("frames_listed", "d_theta", "theta", "m", "v", "mask", "lo", "hi")

    def call(U=2, J=20, step=1, lr_rot=1e-3, lr_trans=1e-3, **null):
        assert set(null) <= set(names)
        return L.mgr_fk_adam(U, J, *[(None if null.get(k) else P) for k in names], lr_rot, lr_trans, 0.9, 0.999, 1e-8, step, None)
    for k in names:
        _refused(L, call(**{k: True}), b"mgr_fk_adam", b"null pointer")
    for kw in (dict(U=0), dict(U=-1), dict(J=0), dict(J=-4), dict(J=33), dict(step=0)):
        _refused(L, call(**kw), b"mgr_fk_adam")
    for kw in (dict(lr_rot=float("nan")), dict(lr_rot=float("inf")), dict(lr_trans=float("nan")), dict(lr_trans=-float("inf"))):
        _refused(L, call(**kw), b"mgr_fk_adam", b"finite")


# =================================================================================================================
# host helpers
# =================================================================================================================
def test_dof_mask_frees_the_23_constrained_angles():
    from manus_amd.dataset import DOF_X, DOF_XZ, apply_constraints_to_poses
    from manus_amd.pose import dof_mask
    mask = dof_mask(HAND)
    assert mask.shape == (22, 3) and mask.dtype == torch.float32
    assert float(mask.sum()) == 23.0 and float(mask[0].sum()) == 0.0 and float(mask[-1].sum()) == 0.0
    for i, bn in enumerate(HAND):
        want = [1.0, 0.0, 1.0] if bn in DOF_XZ else ([0.0, 0.0, 1.0] if bn in DOF_X else [0.0, 0.0, 0.0])
        assert mask[1 + i].tolist() == want, bn
    assert float(dof_mask(HAND, optimize_global_R=True).sum()) == 26.0
    assert float(dof_mask(HAND, optimize_global_T=True)[-1].sum()) == 3.0
    both = dof_mask(HAND, True, True)
    assert float(both.sum()) == 29.0 and torch.equal(both[1:-1], mask[1:-1])
    # masking the angles loses nothing the constrained vector keeps
    e = np.random.default_rng(0).normal(0, 1, (5, 20, 3)).astype(np.float32)
    masked = e * mask[1:-1].numpy()[None]
    assert np.array_equal(apply_constraints_to_poses(masked, HAND), apply_constraints_to_poses(e, HAND))
    assert apply_constraints_to_poses(e, HAND).shape == (5, 23)


def test_joint_limits_values():
    from manus_amd.pose import LIMITS_X, LIMITS_XZ, joint_limits
    lo, hi = joint_limits(HAND)
    assert lo.shape == hi.shape == (22, 3) and lo.dtype == torch.float32
    pi = torch.tensor(math.pi, dtype=torch.float32)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    for i, bn in enumerate(HAND):
        row = (lo[1 + i].tolist(), hi[1 + i].tolist())
        if bn in LIMITS_XZ:
            assert row == ([f32(-math.pi / 6), float(-pi), f32(-math.pi / 2)], [f32(math.pi / 6), float(pi), f32(math.pi / 9)]), bn
        elif bn in LIMITS_X:
            assert row == ([float(-pi), float(-pi), f32(-math.pi / 2)], [float(pi), float(pi), 0.0]), bn
        else:
            assert row == ([float(-pi)] * 3, [float(pi)] * 3), bn
    assert LIMITS_XZ == ("bone_5", "bone_9", "bone_13", "bone_17") and len(LIMITS_X) == 8 and "bone_3" not in LIMITS_X
    assert lo[0].tolist() == [float(-pi)] * 3 and hi[0].tolist() == [float(pi)] * 3
    assert bool(torch.isinf(lo[-1]).all()) and bool(torch.isinf(hi[-1]).all()) and bool((lo[-1] < 0).all()) and bool((hi[-1] > 0).all())


def test_theta_from_bones():
    from manus_amd.pose import theta_from_bones
    g = np.random.default_rng(1)
    recs = [dict(eulers=g.normal(size=(20, 3)).astype(np.float32), root_rotation=g.normal(size=3).astype(np.float32),
                 root_translation=g.normal(size=3).astype(np.float32)) for _ in range(3)]

    class Rec:
        def __init__(self, d):
            self.__dict__.update(d)
    for wrap in (lambda d: d, Rec):
        th = theta_from_bones([wrap(r) for r in recs])
        assert th.shape == (3, 22, 3) and th.dtype == torch.float32
        for f, r in enumerate(recs):
            assert np.array_equal(th[f, 0].numpy(), r["root_rotation"]) and np.array_equal(th[f, 1:21].numpy(), r["eulers"])
            assert np.array_equal(th[f, 21].numpy(), r["root_translation"])
    with pytest.raises(ValueError):
        theta_from_bones([])


def _cpu_refiner(case="hand", base=None, **kw):
    from manus_amd.pose import KinematicPoseRefiner
    inp = R.chain_inputs(case)
    keys = [("take", f, "cam0") for f in range(inp["F"])]
    ref = KinematicPoseRefiner(keys, inp["rest"], inp["parents"], inp["theta"], 1e-3, 2e-3, base=base, device="cpu", **kw)
    return inp, ref


def test_parents_are_validated_on_the_host():
    from manus_amd.pose import KinematicPoseRefiner, check_parents
    from manus_amd.transforms import build_kintree
    rest = torch.eye(4).repeat(4, 1, 1)
    th = torch.zeros((1, 6, 3))
    mk = lambda parents: KinematicPoseRefiner([("a", 0)], rest, parents, th, 1e-3, 1e-3, device="cpu")
    assert mk([-1, 0, 1, 2]).parents_host == [-1, 0, 1, 2]
    assert mk([-1, -1, 0, 0]).parents_host == [-1, -1, 0, 0]                     # several roots
    assert mk(torch.tensor([-1, 0, 0, 2], dtype=torch.int32)).parents_host == [-1, 0, 0, 2]
    assert mk(build_kintree(["a", "b", "c", "d"], ["None", "a", "b", "c"])).parents_host == [-1, 0, 1, 2]
    for bad in ([-1, 2, 0, 1], [-1, 1, 0, 2], [0, 0, 1, 2], [-1, 0, 1, 3], [-2, 0, 1, 2], [-1, 0, 1, 4], [-1, 0, 1]):
        with pytest.raises(ValueError):
            mk(bad)
    with pytest.raises(ValueError):
        check_parents([-1, 1], 2)                                                  # a self-parent
    with pytest.raises(ValueError):
        KinematicPoseRefiner([("a", 0)], torch.eye(4).repeat(33, 1, 1), [-1] * 33, torch.zeros((1, 35, 3)), 1e-3, 1e-3, device="cpu")
    with pytest.raises(ValueError):
        KinematicPoseRefiner([("a", 0)], rest, [-1, 0, 1, 2], th, float("nan"), 1e-3, device="cpu")
    with pytest.raises(ValueError):
        KinematicPoseRefiner([("a", 0)], rest, [-1, 0, 1, 2], th, 1e-3, 1e-3, mask=torch.full((6, 3), 0.5), device="cpu")


# =================================================================================================================
# the checker's gradient against central differences
# =================================================================================================================
@pytest.mark.parametrize("case", ["one", "chain4", "hand"])
def test_restatement_gradient_equals_central_differences(case):
    """fp64, base != I, every entry of theta of every frame: the five-point central difference at h = 1e-3 (truncation h^4 / 30
    times a fifth derivative, roundoff 1e-16 / h times the loss: both below 1e-10 of the largest gradient) against autograd
    through `euler_angles_to_armature_space`, relative to the largest entry of the frame's gradient; the bound is 1e-8."""
    inp = R.chain_inputs(case)
    J, F = inp["J"], inp["F"]
    ones = dict(inp, mask=torch.ones_like(inp["mask"]))
    _, _, grad = R.host_chain(ones, F64)
    assert not torch.equal(inp["base"], torch.eye(4, dtype=F64).expand(F, 4, 4))
    inv = torch.linalg.inv(inp["rest"])
    P, h = (J + 2) * 3, 1e-3
    worst = 0.0
    for f in range(F):
        shown = [k for k, ff in enumerate(inp["frames"]) if ff == f]
        if not shown:
            assert float(grad[f].abs().max()) == 0.0
            continue
        dT = inp["dT"][shown][:, :J].sum(0)
        steps = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=F64) * h
        th = inp["theta"][f].reshape(1, 1, P).repeat(4, P, 1)
        th = th + steps[:, None, None] * torch.eye(P, dtype=F64)[None]
        M = R.fk(th.reshape(4 * P, J + 2, 3), inp["rest"], inp["parents"], inp["base"][f][None].expand(4 * P, 4, 4))
        loss = ((M @ inv) * dT).sum((-1, -2, -3)).reshape(4, P)
        num = (loss[0] - 8.0 * loss[1] + 8.0 * loss[2] - loss[3]) / (12.0 * h)
        err = float((num - grad[f].reshape(P)).abs().max() / grad[f].abs().max())
        worst = max(worst, err)
    print("restatement against central differences, %s: %.3e" % (case, worst))
    assert worst <= 1e-8
    # the mask only zeroes entries
    _, _, masked = R.host_chain(inp, F64)
    assert torch.equal(masked, grad * inp["mask"])


# =================================================================================================================
# the refiner on CPU tensors
# =================================================================================================================
def test_fit_base_recovers_a_planted_transform():
    inp, ref = _cpu_refiner("hand")
    planted = R.fk(inp["theta"], inp["rest"], inp["parents"], inp["base"])              # fp64, at the planted base
    assert float((ref.fk_host() - planted).abs().max()) > 1e-2                          # base = identity does not fit
    got = ref.fit_base(planted)
    assert got.dtype == F64 and float((got - inp["base"]).abs().max()) <= 1e-12
    assert torch.equal(ref.base, got.to(F32))
    assert float((ref.fk_host() - planted).abs().max()) <= 1e-6                          # the residual at the fp32 base
    with pytest.raises(ValueError):
        ref.fit_base(planted[:, :3])


def test_refiner_state_round_trips_on_cpu():
    from manus_amd.pose import joint_limits, dof_mask
    inp, a = _cpu_refiner("hand", mask=dof_mask(HAND), limits=joint_limits(HAND))
    assert a.frame_keys == [("take", f) for f in range(6)] and a.theta.shape == (6, 22, 3) and a.m is None and a.steps == 0
    assert a.last_prior is None and a.last_grad is None
    assert torch.equal(a.theta, inp["theta"].to(F32)) and torch.equal(a.local, inp["local"].to(F32))
    empty = a.state_dict()
    assert sorted(empty) == ["frame_keys", "m", "steps", "theta", "v"] and empty["m"] is None
    g = torch.Generator().manual_seed(1)
    a.theta.copy_(torch.randn(a.theta.shape, generator=g))
    a.m, a.v = torch.randn(a.theta.shape, generator=g), torch.rand(a.theta.shape, generator=g)
    a.steps = 17
    state = a.state_dict()
    a.theta.zero_()                                                  # the state is a copy, not a view
    assert float(state["theta"].abs().max()) > 0.0
    _, b = _cpu_refiner("hand")
    b.load_state_dict(state)
    again = b.state_dict()
    assert again["steps"] == 17 and again["frame_keys"] == state["frame_keys"]
    for k in ("theta", "m", "v"):
        assert torch.equal(again[k], state[k]), k
    b.load_state_dict(empty)
    assert b.m is None and b.steps == 0 and torch.equal(b.theta, inp["theta"].to(F32))
    from manus_amd.pose import KinematicPoseRefiner
    other = KinematicPoseRefiner([("take", f) for f in range(5)], inp["rest"], inp["parents"], inp["theta"][:5], 1e-3, 1e-3, device="cpu")
    with pytest.raises(ValueError):
        other.load_state_dict(state)
    with pytest.raises(ValueError):
        b.step(torch.zeros((1, 21, 4, 4)), [0], [0])                 # before apply


# =================================================================================================================
# the checker's own conditions
# =================================================================================================================
@pytest.mark.parametrize("case", R.CASES)
def test_checker_fp32_error_is_small(case):
    """e32 of the restatement on every committed case is at most 1e-4 per row, in the norm and over the rows the GPU tests judge:
    their bound is 8 * max(e32, 2^-23), and this keeps it below 1e-3."""
    inp = R.chain_inputs(case)
    J, V, F = inp["J"], inp["V"], inp["F"]
    T64, M64, g64 = R.host_chain(inp, F64)
    T32, M32, g32 = R.host_chain(inp, F32)
    for tag, a, b in (("T", T32[:, :J].reshape(V * J, 16), T64[:, :J].reshape(V * J, 16)), ("M", M32.reshape(V * J, 16), M64.reshape(V * J, 16)),
                      ("d_theta", g32.reshape(F * (J + 2), 3), g64.reshape(F * (J + 2), 3))):
        e32 = row_rel_err(a, b)
        print("e32 %-9s %-8s %.3e" % (case, tag, e32))
        assert e32 <= 1e-4, (case, tag, e32)
    for f in range(F):
        if f not in inp["frames"]:
            assert float(g64[f].abs().max()) == 0.0
    assert bool(torch.isfinite(g64).all()) and float(g64[R.GIMBAL_FRAME, 1].abs().max()) > 0.0
    assert float(inp["theta"][R.GIMBAL_FRAME, 1, 1]) == float(torch.tensor(math.pi / 2, dtype=F32))
    assert bool((g64[:, inp["mask"] == 0] == 0).all())
    # the Adam restatement
    lo, hi = torch.full_like(inp["mask"], -0.5), torch.full_like(inp["mask"], 0.5)
    m0 = torch.zeros_like(inp["theta"])
    for dt in (F64, F32):
        th, m, v = R.adam_step(inp["theta"].to(dt), m0.to(dt), m0.to(dt), g64[inp["listed"]], inp["listed"], inp["mask"], lo, hi, 0.3, 0.1, 1)
        off = inp["mask"] == 0
        assert torch.equal(th[:, off], inp["theta"].to(dt)[:, off]) and torch.equal(th[4], inp["theta"].to(dt)[4])
        assert float(th[inp["listed"]][:, ~off].abs().max()) <= 0.5 and float(m[4].abs().max()) == 0.0

"""No GPU: the ABI of the device pose chain (mgr_pose_apply / mgr_pose_backward / mgr_pose_adam) -- header, binding, built
library --, its refusals, which are all decided before anything touches a device, the analytic Rodrigues vector-Jacobian
product of the backward kernel against fp64 autograd, `engine.FrameSchedule`, `PoseRefiner`'s state on CPU tensors, and the
fp32 error of the checker itself (tests/pose_chain_ref.py), which sets the GPU tests' tolerance."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_chain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_pose_apply": 12, "mgr_pose_backward": 15, "mgr_pose_adam": 18}


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
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, bound = _lib.SIGNATURES[name]
        assert len(bound) == arity and res is ctypes.c_int, (name, len(bound))
        assert hasattr(so, name), "%s is not exported by the built library" % name
    assert "pose.hip" in build.SOURCES and "bone_math.h" in build.HEADERS
    assert _declared_args(header, "mgr_pose_apply")[:3] == ["int V", "int B", "int F"]
    assert _declared_args(header, "mgr_pose_backward")[:5] == ["int V", "int B", "int F", "int U", "const int32_t* frames_listed"]
    # the five hyper-parameters travel as doubles, like mgr_skin_grid_adam's
    assert _lib.SIGNATURES["mgr_pose_adam"][1][11:16] == [ctypes.c_double] * 5


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
    names = ("view_rows", "frame_of_view", "posed", "rest", "rotvec", "trans", "transforms")

    def call(V=3, B=20, F=4, **null):
        assert set(null) <= set(names)
        return L.mgr_pose_apply(V, B, F, *[(None if null.get(k) else P) for k in names], None, None)
    for k in names:
        _refused(L, call(**{k: True}), b"mgr_pose_apply", b"null pointer")
    for kw in (dict(V=0), dict(V=-2), dict(B=0), dict(B=-1), dict(B=33), dict(F=0), dict(F=-1)):
        _refused(L, call(**kw), b"mgr_pose_apply")


def test_backward_refusals_before_the_device():
    from manus_amd._lib import lib
    L = lib()
    names = ("frames_listed", "view_rows", "frame_of_view", "posed", "rest", "rotvec", "trans", "d_transforms", "d_rotvec", "d_trans")

    def call(V=3, B=20, F=4, U=2, **null):
        assert set(null) <= set(names)
        return L.mgr_pose_backward(V, B, F, U, *[(None if null.get(k) else P) for k in names], None)
    for k in names:
        _refused(L, call(**{k: True}), b"mgr_pose_backward", b"null pointer")
    for kw in (dict(V=0), dict(V=-2), dict(B=0), dict(B=33), dict(F=0), dict(F=-3), dict(U=0), dict(U=-1)):
        _refused(L, call(**kw), b"mgr_pose_backward")


def test_adam_refusals_before_the_device():
    from manus_amd._lib import lib
    L = lib()
    names = ("frames_listed", "d_rotvec", "d_trans", "rotvec", "trans", "m_r", "v_r", "m_t", "v_t")

    def call(U=2, B=20, step=1, **null):
        assert set(null) <= set(names)
        return L.mgr_pose_adam(U, B, *[(None if null.get(k) else P) for k in names], 1e-3, 1e-3, 0.9, 0.999, 1e-8, step, None)
    for k in names:
        _refused(L, call(**{k: True}), b"mgr_pose_adam", b"null pointer")
    for kw in (dict(U=0), dict(U=-1), dict(B=0), dict(B=-4), dict(B=33), dict(step=0)):
        _refused(L, call(**kw), b"mgr_pose_adam")


@pytest.mark.parametrize("norm", [0.0, 9.99e-4, 1.001e-3, 0.5])
def test_analytic_rodrigues_vjp_equals_fp64_autograd(norm):
    """r = 0 exactly, |r|^2 just below and just above the series threshold 1e-6, and |r| = 0.5: the closed form the backward
    kernel evaluates against fp64 autograd of pose._exp_so3.  Both are fp64 evaluations of the same derivative; the bound is
    fp64 roundoff amplified by the cancellation of the closed-form coefficients near the threshold (eps64 / |r|^2 ~ 2e-10)."""
    from manus_amd.pose import _exp_so3
    g = torch.Generator().manual_seed(5)
    d = torch.randn(3, generator=g, dtype=torch.float64)
    r = (norm * d / d.norm()).requires_grad_(True)
    t = float((r.detach() * r.detach()).sum())
    assert (t < R.SMALL) == (norm < 1e-3)
    G = torch.randn((3, 3), generator=g, dtype=torch.float64)
    (_exp_so3(r) * G).sum().backward()
    got = R.rodrigues_vjp(r.detach().numpy(), G.numpy())
    err = np.abs(got - r.grad.numpy()).max() / np.abs(r.grad.numpy()).max()
    print("|r| = %g: analytic against autograd %.3e" % (norm, err))
    assert err <= 1e-9


class _Store:
    def __init__(self, n):
        self.items = list(range(100, 100 + n))


def test_frame_schedule():
    from manus_amd.engine import FrameSchedule
    st = _Store(11)
    a, b = FrameSchedule(st, 3, seed=4), FrameSchedule(st, 3, seed=4)
    assert a.steps_per_epoch == 3
    epochs = []
    for e in range(3):
        got = [a.items(e * 3 + k) for k in range(3)]
        flat = [i for part in got for i in part]
        assert all(len(part) == 3 for part in got)
        assert len(set(flat)) == 9 and set(flat) <= set(st.items)              # every item once, a tail of two dropped
        assert set(st.items) - set(flat) == set(a.epoch(e)[9:])
        epochs.append(flat)
    assert epochs[0] != epochs[1] and epochs[1] != epochs[2]                     # another permutation per epoch
    assert [b.items(s) for s in (7, 0, 4, 7)] == [a.items(s) for s in (7, 0, 4, 7)]      # a pure function of (seed, step)
    assert [FrameSchedule(st, 3, seed=5).items(s) for s in range(3)] != [a.items(s) for s in range(3)]
    seq = FrameSchedule(st, 4, order="sequential")
    assert seq.items(0) == [100, 101, 102, 103] and seq.items(1) == [104, 105, 106, 107] and seq.items(2) == seq.items(0)
    FrameSchedule(st, 11)
    with pytest.raises(ValueError):
        FrameSchedule(st, 12)
    with pytest.raises(ValueError):
        FrameSchedule(st, 3, order="random")


def test_pose_refiner_state_round_trips_on_cpu():
    from manus_amd.pose import PoseCorrection, PoseRefiner
    keys = [("grasp_1", 8, "cam00"), ("grasp_1", 8, "cam01"), ("grasp_1", 11, "cam00"), ("wave", 8, "cam00")]
    rest = torch.eye(4).repeat(5, 1, 1)
    a = PoseRefiner(keys, 5, rest, 1e-3, 2e-3, device="cpu")
    assert a.frame_keys == [("grasp_1", 8), ("grasp_1", 11), ("wave", 8)] and a.rotvec.shape == (3, 5, 3) and a.m_r is None
    assert float(a.rotvec.abs().max()) == 0.0 and float(a.trans.abs().max()) == 0.0 and a.steps == 0
    empty = a.state_dict()
    assert empty["m_r"] is None and empty["steps"] == 0
    g = torch.Generator().manual_seed(1)
    a.rotvec.copy_(torch.randn(a.rotvec.shape, generator=g))
    a.trans.copy_(torch.randn(a.trans.shape, generator=g))
    a.m_r, a.v_r, a.m_t, a.v_t = (torch.randn(a.rotvec.shape, generator=g) for _ in range(4))
    a.steps = 17
    state = a.state_dict()
    a.rotvec.zero_()                                             # the state is a copy, not a view
    assert float(state["rotvec"].abs().max()) > 0.0
    b = PoseRefiner(keys, 5, rest, 1e-3, 2e-3, device="cpu")
    b.load_state_dict(state)
    again = b.state_dict()
    assert again["steps"] == 17 and again["frame_keys"] == state["frame_keys"]
    for k in ("rotvec", "trans", "m_r", "v_r", "m_t", "v_t"):
        assert torch.equal(again[k], state[k]), k
    b.load_state_dict(empty)
    assert b.m_r is None and b.steps == 0 and float(b.rotvec.abs().max()) == 0.0
    with pytest.raises(ValueError):
        PoseRefiner(keys[:2], 5, rest, 1e-3, 2e-3, device="cpu").load_state_dict(state)
    # as_module: a PoseCorrection on the same storage
    b.load_state_dict(state)
    m = b.as_module()
    assert isinstance(m, PoseCorrection) and m.rotvec.data_ptr() == b.rotvec.data_ptr() and m.trans.data_ptr() == b.trans.data_ptr()
    with pytest.raises(ValueError):
        PoseRefiner(keys, 33, torch.eye(4).repeat(33, 1, 1), 1e-3, 1e-3, device="cpu")


@pytest.mark.parametrize("B", R.BONES)
def test_checker_fp32_error_is_small(B):
    """e32 of the host chain on the committed seeds is at most 1e-5 (measured on the CPU: T at most 2.1e-7, d_trans 4.2e-7,
    d_rotvec 7.5e-6 -- the row just above the series threshold, pose_chain_ref.chain_inputs; every other row below 8e-7): the
    GPU tests' bound is 8 * max(e32, 2^-23), and this keeps it from widening unnoticed."""
    for V in R.VIEWS:
        inp = R.chain_inputs(B, V)
        T64, dr64, dt64 = R.host_chain(inp, R.F64)
        T32, dr32, dt32 = R.host_chain(inp, R.F32)
        rows = lambda x, w: x.reshape(-1, w)
        for tag, a, b, w in (("T", T32, T64, 16), ("d_rotvec", dr32, dr64, 3), ("d_trans", dt32, dt64, 3)):
            e32 = R.row_rel_err(rows(a, w), rows(b, w))
            print("e32 B %2d V %d %-8s %.3e" % (B, V, tag, e32))
            assert e32 <= 1e-5, (B, V, tag, e32)
        # frame 2 is never viewed: no gradient at all
        assert float(dr64[2].abs().max()) == 0.0 and float(dt64[2].abs().max()) == 0.0
        # the checker's analytic product against its own autograd: dC = posed^T dT inv(rest)^T summed over the frame's positions
        inv = torch.linalg.inv(inp["rest"])
        for f in sorted(set(inp["frames"])):
            for b_ in range(min(B, 3)):
                dC = sum(inp["posed"][v, b_].T @ inp["dT"][k, b_] @ inv[b_].T for k, (v, ff) in enumerate(zip(inp["rows"], inp["frames"])) if ff == f)
                got = R.rodrigues_vjp(inp["rotvec"][f, b_].numpy(), dC[:3, :3].numpy())
                want = dr64[f, b_].numpy()
                assert np.abs(got - want).max() <= 1e-9 * max(np.abs(want).max(), np.abs(dC.numpy()).max()), (B, V, f, b_)
                assert np.abs(dC[:3, 3].numpy() - dt64[f, b_].numpy()).max() <= 1e-12 * np.abs(dC.numpy()).max()

"""No GPU: the terms on the kinematic refiner's angles (mgr_fk_backward_terms, `KinematicPoseRefiner(w_dev_* / w_smooth_* / w_kp)`)
-- the ABI in header, binding and built library; every refusal, decided before anything touches a device; the restatement's
gradient (tests/fk_terms_ref.py) against central differences in fp64; the count-once rule of the values; `keypoint_offsets` on
the reference's golden skeleton; `keypoints_of_store`; the refiner's new arguments; the recovery fixture's own condition; and
the fp32 error of the restatement, which sets the GPU tests' tolerance."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import fk_chain_ref as R
import fk_terms_ref as T
from fk_chain_ref import F32, F64
from util import row_rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["bone_%d" % i for i in range(20)]
P = ctypes.c_void_p(0x1000)          # a fake pointer: a refusal never dereferences it


def test_new_entries_are_declared_bound_and_exported():
    """The declaration of the issue has 31 parameters (mgr_fk_backward's 15 + theta_ref, neighbours, four weights, K, four keypoint
    pointers, w_kp, values, workspace, workspace_bytes + stream)."""
    from manus_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bint\s+mgr_fk_backward_terms\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, "include/manus_hip.h does not declare mgr_fk_backward_terms"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 31 and args[-1] == "void* stream" and args[:4] == ["int V", "int J", "int F", "int U"], args
    assert args[15:17] == ["const float* theta_ref", "const int32_t* neighbours"] and args[21] == "int K" and args[26] == "double w_kp"
    assert args[27:30] == ["double* values", "void* workspace", "size_t workspace_bytes"]
    res, bound = _lib.SIGNATURES["mgr_fk_backward_terms"]
    assert res is ctypes.c_int and len(bound) == 31
    assert bound[17:21] == [ctypes.c_double] * 4 and bound[21] is ctypes.c_int and bound[26] is ctypes.c_double and bound[29] is ctypes.c_size_t
    m = re.search(r"\bsize_t\s+mgr_fk_terms_workspace_bytes\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["int U", "int J", "int K"]
    res, bound = _lib.SIGNATURES["mgr_fk_terms_workspace_bytes"]
    assert res is ctypes.c_size_t and len(bound) == 3
    assert hasattr(so, "mgr_fk_backward_terms") and hasattr(so, "mgr_fk_terms_workspace_bytes")
    assert re.search(r"#define\s+MGR_FK_MAX_KEYPOINTS\s+64\b", header) and _lib.MGR_FK_MAX_KEYPOINTS == 64
    L = _lib.lib()
    assert L.mgr_fk_terms_workspace_bytes(5, 20, 21) >= 5 * 3 * 8 and L.mgr_fk_terms_workspace_bytes(0, 20, 21) == 0


CHAIN = ("frames_listed", "view_rows", "frame_of_view", "rest", "local", "parents", "base", "theta", "mask", "d_transforms", "d_theta")
EXTRA = ("theta_ref", "neighbours", "kp_bone", "kp_offset", "kp_target", "kp_weight", "values", "workspace")


def _call(L, V=3, J=20, F=4, U=2, K=21, w=(0.5, 0.25, 2.0, 1.0, 10.0), ws_bytes=1 << 20, **null):
    assert set(null) <= set(CHAIN + EXTRA)
    p = {k: (None if null.get(k) else P) for k in CHAIN + EXTRA}
    return L.mgr_fk_backward_terms(V, J, F, U, *[p[k] for k in CHAIN], p["theta_ref"], p["neighbours"], w[0], w[1], w[2], w[3], K,
                                   p["kp_bone"], p["kp_offset"], p["kp_target"], p["kp_weight"], w[4], p["values"], p["workspace"], ws_bytes, None)


def _refused(L, rc, text=None, code=None):
    from manus_amd._lib import MGR_EINVAL
    err = L.mgr_last_error()
    assert rc == (MGR_EINVAL if code is None else code) and rc != 0, (rc, err)
    assert b"mgr_fk_backward_terms" in err, err
    if text:
        assert text in err, err


def test_refusals_before_the_device():
    from manus_amd._lib import MGR_ENOMEM, lib
    L = lib()
    zero = (0.0,) * 5
    # mgr_fk_backward's own conditions: with every weight zero all of them, d_transforms and the view lists included
    for k in CHAIN:
        _refused(L, _call(L, w=zero, **{k: True}), b"null pointer")
    for kw in (dict(V=0), dict(V=-2), dict(J=0), dict(J=33), dict(F=0), dict(F=-3), dict(U=0), dict(U=-1)):
        _refused(L, _call(L, w=zero, **kw))
        if kw != dict(V=0):
            _refused(L, _call(L, **kw))
    # with a weight on: every pointer but d_transforms / the view lists (those only together with d_transforms)
    for k in CHAIN:
        if k not in ("d_transforms", "view_rows", "frame_of_view"):
            _refused(L, _call(L, **{k: True}), b"null pointer")
    _refused(L, _call(L, view_rows=True), b"null pointer")
    _refused(L, _call(L, frame_of_view=True), b"null pointer")
    _refused(L, _call(L, V=0), None)                                   # V = 0 with d_transforms given
    _refused(L, _call(L, V=-1, d_transforms=True, view_rows=True, frame_of_view=True))
    # the weights
    for i in range(5):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            w = [0.5, 0.25, 2.0, 1.0, 10.0]
            w[i] = bad
            _refused(L, _call(L, w=tuple(w)), b"finite")
    # what a term needs
    _refused(L, _call(L, theta_ref=True), b"theta_ref")
    _refused(L, _call(L, w=(0.0, 0.0, 2.0, 0.0, 0.0), theta_ref=True), b"theta_ref")
    _refused(L, _call(L, neighbours=True), b"neighbour")
    _refused(L, _call(L, w=(0.0, 0.0, 0.0, 1.0, 0.0), neighbours=True), b"neighbour")
    for K in (0, -1, 65):
        _refused(L, _call(L, K=K), b"MGR_FK_MAX_KEYPOINTS")
    for k in ("kp_bone", "kp_offset", "kp_target", "kp_weight"):
        _refused(L, _call(L, **{k: True}), b"keypoint")
    for one in ((0.5, 0, 0, 0, 0), (0, 0.25, 0, 0, 0), (0, 0, 2.0, 0, 0), (0, 0, 0, 1.0, 0), (0, 0, 0, 0, 10.0)):
        w = tuple(float(x) for x in one)
        _refused(L, _call(L, w=w, values=True), b"values")
        _refused(L, _call(L, w=w, workspace=True), b"workspace")
        need = L.mgr_fk_terms_workspace_bytes(2, 20, 21)
        _refused(L, _call(L, w=w, ws_bytes=need - 1), b"workspace too small", code=MGR_ENOMEM)
        _refused(L, _call(L, w=w, ws_bytes=0), b"workspace too small", code=MGR_ENOMEM)


# =================================================================================================================
# the restatement
# =================================================================================================================
@pytest.mark.parametrize("combo", list(T.COMBOS))
@pytest.mark.parametrize("case", ["one", "chain4", "hand"])
def test_restatement_gradient_equals_central_differences(case, combo):
    """fp64, every entry of theta of every frame, all rows counted: the five-point central difference at h = 1e-3 of the full E
    (truncation h^4 / 30 times a fifth derivative, roundoff 1e-16 / h times E: both below 1e-10 of the largest gradient)
    against autograd through the restatement, relative to the largest entry of the frame's gradient; the bound is 1e-8, the bar
    test_fk_chain_cpu.py uses for the chain."""
    inp = T.terms_inputs(case)
    ones = dict(inp, mask=torch.ones_like(inp["mask"]))
    w = T.COMBOS[combo]
    J, F = inp["J"], inp["F"]
    _, grad = T.host_terms(ones, F64, w, chain=False)

    def value(theta):
        M = R.fk(theta, inp["rest"], inp["parents"], inp["base"])
        return float(sum(T.terms(ones, theta, M, w)))
    h, worst = 1e-3, 0.0
    for f in range(F):
        num = torch.zeros((J + 2, 3), dtype=F64)
        for r in range(J + 2):
            for c in range(3):
                vals = []
                for s in (-2.0, -1.0, 1.0, 2.0):
                    th = inp["theta"].clone()
                    th[f, r, c] += s * h
                    vals.append(value(th))
                num[r, c] = (vals[0] - 8.0 * vals[1] + 8.0 * vals[2] - vals[3]) / (12.0 * h)
        assert float(grad[f].abs().max()) > 0.0
        worst = max(worst, float((num - grad[f]).abs().max() / grad[f].abs().max()))
    print("terms restatement against central differences, %s / %s: %.3e" % (case, combo, worst))
    assert worst <= 1e-8
    # the mask only zeroes entries of the gradient and removes its elements from the priors' values
    _, masked = T.host_terms(inp, F64, w, chain=False)
    assert bool((masked[:, inp["mask"] == 0] == 0).all())


@pytest.mark.parametrize("case", ["chain4", "hand"])
def test_values_count_every_term_once(case):
    """The value on all rows is the full E; on a list it is the part that touches the list: for disjoint lists that share no edge
    the parts add up to the whole, and a list's part never exceeds the whole.  A skipped keypoint (c = 0, NaN target) adds 0."""
    inp = T.terms_inputs(case)
    w = T.WEIGHTS
    full, _ = T.host_terms(inp, F64, w, chain=False)
    every, _ = T.host_terms(inp, F64, w, listed=list(range(inp["F"])), chain=False)
    assert torch.equal(full, every) and bool(torch.isfinite(full).all()) and float(full[:3].min()) > 0.0
    assert abs(float(full[3] - full[:3].sum())) <= 1e-15 * float(full[3])
    parts = {name: T.host_terms(inp, F64, w, listed=l, chain=False)[0] for name, l in T.LISTS.items()}
    for name, v in parts.items():
        assert bool((v <= full * (1 + 1e-12)).all()), name
    # take a = rows 0..3: {0} and {2, 3} share no edge only if edge (0,1) and (1,2) are counted once each: {0} u {2} u take b
    a = T.host_terms(inp, F64, w, listed=[0], chain=False)[0]                  # dev 0, kp 0, edge (0,1)
    b = T.host_terms(inp, F64, w, listed=[2, 3], chain=False)[0]               # dev 2 3, kp 2 3, edges (1,2) (2,3)
    c = T.host_terms(inp, F64, w, listed=[4, 5], chain=False)[0]               # take b whole
    one = T.host_terms(inp, F64, w, listed=[1], chain=False)[0]                # dev 1, kp 1, edges (0,1) (1,2)
    only_dev_kp_1 = T.host_terms(inp, F64, dict(w, w_smooth_rot=0.0, w_smooth_trans=0.0), listed=[1], chain=False)[0]
    assert float(((a + b + c + only_dev_kp_1)[3] - full[3]).abs()) <= 1e-12 * float(full[3])
    assert float(one[1]) > 0.0 and float(one[3]) > float(only_dev_kp_1[3])
    # adjacent rows: the edge between them once
    adj, i1, i2 = parts["adjacent"], one, parts["interior"]
    sm = lambda l: float(T.host_terms(inp, F64, T.COMBOS["smooth"], listed=l, chain=False)[0][1])
    e12 = sm([1]) + sm([2]) - sm([1, 2])                                       # the shared edge (1,2)
    th = inp["theta"]
    ws = torch.full((inp["J"] + 2, 1), 0.25, dtype=F64)
    ws[-1] = 1.0
    want = float((ws * (inp["mask"] != 0) * (th[1] - th[2]) ** 2).sum())
    assert abs(e12 - want) <= 1e-12 * want
    assert float(adj[0]) == pytest.approx(float(i1[0] + i2[0]), rel=1e-14)


@pytest.mark.parametrize("case", R.CASES)
def test_checker_fp32_error_is_small(case):
    """e32 of the restatement on every committed case and list is at most 1e-4 per row: the GPU tests' bound is
    8 * max(e32, 2^-23), and this keeps it below 1e-3."""
    inp = T.terms_inputs(case)
    J = inp["J"]
    for combo, w in T.COMBOS.items():
        for chain in (True, False):
            v64, g64 = T.host_terms(inp, F64, w, listed=T.LISTS["listed"], chain=chain)
            v32, g32 = T.host_terms(inp, F32, w, listed=T.LISTS["listed"], chain=chain)
            l = T.LISTS["listed"]
            e32 = row_rel_err(g32[l].reshape(-1, 3), g64[l].reshape(-1, 3))
            print("e32 %-9s %-6s chain=%-5s %.3e" % (case, combo, chain, e32))
            assert e32 <= 1e-4, (case, combo, chain, e32)
            assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(v64).all())
            assert float((v32.double() - v64).abs().max()) <= 1e-4 * max(float(v64[3]), 1e-30)


# =================================================================================================================
# host helpers
# =================================================================================================================
def test_keypoint_offsets_on_the_golden_skeleton():
    """world_pose_matrixs . offsets(world_rest_matrixs, world_rest_heads, world_rest_tails) reproduces world_pose_tails and
    world_pose_heads[:, 0] to 1e-6 absolute (coordinates up to 0.19), and the offsets are (0, length, 0)."""
    from manus_amd.pose import keypoint_offsets
    d = np.load(R.GOLDEN)
    bones, off = keypoint_offsets(d["world_rest_matrixs"], d["world_rest_heads"], d["world_rest_tails"])
    assert bones.dtype == torch.int32 and bones.tolist() == [0] + list(range(20)) and off.shape == (21, 3) and off.dtype == F32
    M = torch.tensor(d["world_pose_matrixs"], dtype=F64)
    p = T.keypoints_of(M, bones.tolist(), off.to(F64))
    want = torch.cat([torch.tensor(d["world_pose_heads"], dtype=F64)[:, :1], torch.tensor(d["world_pose_tails"], dtype=F64)], 1)
    err = float((p - want).abs().max())
    length = torch.tensor(np.linalg.norm(d["world_rest_tails"] - d["world_rest_heads"], axis=1), dtype=F64)
    shape = torch.zeros((21, 3), dtype=F64)
    shape[1:, 1] = length
    dev = float((off.double() - shape).abs().max())
    print("keypoint_offsets on the golden: posed keypoints %.3e, offsets against (0, length, 0) %.3e" % (err, dev))
    assert err <= 1e-6 and dev <= 1e-7
    with pytest.raises(ValueError):
        keypoint_offsets(d["world_rest_matrixs"], d["world_rest_heads"][:5], d["world_rest_tails"])


def test_keypoints_of_store_takes_the_first_item_of_every_frame():
    from manus_amd.pose import keypoints_of_store
    keys = [("a", "3"), ("a", "3"), ("a", "4"), ("b", "3"), ("a", "4")]
    kp = torch.arange(5 * 3 * 3, dtype=F32).reshape(5, 3, 3)
    store = types.SimpleNamespace(frame_keys=keys, keypoints=kp)
    got = keypoints_of_store(store, [("b", "3", "cam0"), ("a", "4", "cam1"), ("a", "3", "cam0"), ("b", "3", "cam1")])
    assert torch.equal(got, kp[[3, 2, 0]])
    with pytest.raises(ValueError, match="no item"):
        keypoints_of_store(store, [("a", "3"), ("c", "0")])
    with pytest.raises(ValueError):
        keypoints_of_store(types.SimpleNamespace(frame_keys=None, keypoints=None), keys)


def _cpu_refiner(case="hand", **kw):
    from manus_amd.pose import KinematicPoseRefiner
    inp = T.terms_inputs(case)
    return inp, KinematicPoseRefiner(inp["frame_keys"], inp["rest"], inp["parents"], inp["theta"], 1e-3, 2e-3, device="cpu", **kw)


def test_refiner_arguments():
    inp, plain = _cpu_refiner()
    assert plain.last_prior is None and plain.last_terms is None and plain.has_terms is False and plain.kp is None
    assert plain.weights == (0.0, 0.0, 0.0, 0.0) and plain.w_kp == 0.0
    assert sorted(plain.state_dict()) == ["frame_keys", "m", "steps", "theta", "v"]
    _, ref = _cpu_refiner(**T.WEIGHTS)
    assert ref.has_terms and ref.weights == (0.5, 0.25, 2.0, 1.0) and ref.w_kp == 10.0 and ref.last_prior is None
    assert sorted(ref.state_dict()) == ["frame_keys", "m", "steps", "theta", "v"]
    assert torch.equal(ref.theta_ref, ref.theta) and ref.theta_ref.data_ptr() != ref.theta.data_ptr()
    assert torch.equal(ref.neighbours, T.neighbours()) and ref.neighbours.dtype == torch.int32
    assert ref.neighbours.tolist() == [[-1, 1], [0, 2], [1, 3], [2, -1], [-1, 5], [4, -1]]
    _, cut = _cpu_refiner(w_smooth_rot=1.0, max_gap=0)
    assert bool((cut.neighbours == -1).all())
    for name in T.NAMES:
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                _cpu_refiner(**{name: bad})
    # set_reference
    ref.theta.add_(1.0)
    ref.set_reference()
    assert torch.equal(ref.theta_ref, ref.theta)
    ref.set_reference(inp["theta_ref"])
    assert torch.equal(ref.theta_ref, inp["theta_ref"].to(F32))
    with pytest.raises(ValueError):
        ref.set_reference(inp["theta_ref"][:2])
    # set_keypoints
    J, F, K = inp["J"], inp["F"], inp["K"]
    b, o, y, c = inp["kp_bone"], inp["kp_offset"], inp["kp_target"], inp["kp_weight"]
    ref.set_keypoints(b, o, y)
    assert ref.kp[0].dtype == torch.int32 and ref.kp[0].tolist() == b and torch.equal(ref.kp[3], torch.ones((F, K)))
    ref.set_keypoints(torch.tensor(b), o, y, c)
    assert torch.equal(ref.kp[3], c.to(F32)) and ref.kp[2].shape == (F, K, 3) and ref.kp[1].dtype == F32
    ref.set_keypoints(b, o, y, c[0])
    assert torch.equal(ref.kp[3], c[0].to(F32).expand(F, K))
    for bad in (dict(bones=b[:-1]), dict(bones=[J] + b[1:]), dict(bones=[-1] + b[1:]), dict(offsets=o[:, :2]), dict(targets=y[:, :-1]),
                dict(targets=y[:-1]), dict(weights=c[:, :-1]), dict(weights=c[:-1]), dict(bones=[0.0] * K), dict(bones=[]),
                dict(bones=torch.tensor(b)[None])):
        args = dict(bones=b, offsets=o, targets=y, weights=c)
        args.update(bad)
        with pytest.raises(ValueError):
            ref.set_keypoints(**args)
    from manus_amd.pose import KinematicPoseRefiner
    big = KinematicPoseRefiner([("a", 0)], torch.eye(4).repeat(2, 1, 1), [-1, 0], torch.zeros((1, 4, 3)), 1e-3, 1e-3, device="cpu", w_kp=1.0)
    big.set_keypoints([0] * 64, torch.zeros((64, 3)), torch.zeros((1, 64, 3)))
    with pytest.raises(ValueError):
        big.set_keypoints([0] * 65, torch.zeros((65, 3)), torch.zeros((1, 65, 3)))
    # w_kp without keypoints raises at the step, before any entry is called
    _, bare = _cpu_refiner(w_kp=1.0)
    bare._posed = torch.zeros((1, J, 4, 4))
    with pytest.raises(ValueError, match="set_keypoints"):
        bare.step(torch.zeros((1, J + 1, 4, 4)), [0], [0])
    with pytest.raises(ValueError, match="set_keypoints"):
        bare.fit_keypoints(1)
    with pytest.raises(ValueError, match="set_keypoints"):
        bare.keypoints([0], [0])
    with pytest.raises(ValueError):
        plain.fit_keypoints(1)


def test_the_recovery_fixture_recovers_in_fp64():
    """The fixture of the GPU recovery test, on the host: the fp64 Adam loop's E_kp after 100 steps is below 1 % of its start,
    and the fp32 host loop stays close to it."""
    fx = T.recovery_inputs()
    cfg = T.RECOVERY
    listed = list(range(fx["F"]))
    assert float(fx["mask"].sum()) == 29.0 and float(fx["theta_true"][:, fx["mask"] == 0].abs().max()) == 0.0
    assert float(fx["theta_true"][:, -1].abs().max()) <= 0.02 and float(fx["theta_true"][:, :-1].abs().max()) > 0.3
    th64, h64 = T.adam_loop(fx, F64, cfg["w"], cfg["steps"], listed, cfg["lr_rot"], cfg["lr_trans"])
    th32, h32 = T.adam_loop(fx, F32, cfg["w"], cfg["steps"], listed, cfg["lr_rot"], cfg["lr_trans"])
    last64 = float(T.host_terms(fx, F64, cfg["w"], chain=False, theta=th64)[0][2])
    last32 = float(T.host_terms(fx, F64, cfg["w"], chain=False, theta=th32.double())[0][2])
    start = float(h64[0, 2])
    print("recovery fixture: E_kp %.4e -> %.4e (%.4f %%), host fp32 loop -> %.4e (%.2e relative)"
          % (start, last64, 100 * last64 / start, last32, abs(last32 - last64) / last64))
    assert last64 < 0.01 * start
    assert bool((h64[1:, 2] < start).all())

"""No GPU: the multi-view 2-D keypoint term of the kinematic refiner (mgr_fk_backward_terms2d, `KinematicPoseRefiner(w_kp2d=...)`) --
the ABI in header, binding and built library; every refusal, decided before anything touches a device; the restatement's gradient
(tests/fk_kp2d_ref.py) against central differences in fp64; the fixture's own conditions (depth margins, detections inside and
outside delta, the planted ones); the host helpers; `set_keypoints_2d`; the new keywords; and the recovery fixture in fp64."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import fk_chain_ref as R
import fk_kp2d_ref as Q
import fk_terms_ref as T
from fk_chain_ref import F32, F64
from util import row_rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)          # a fake pointer: a refusal never dereferences it


@functools.lru_cache(maxsize=None)
def case(row):
    return Q.kp2d_inputs(row)


def test_new_entries_are_declared_bound_and_exported():
    """mgr_fk_backward_terms2d: mgr_fk_backward_terms' 31 parameters with C, three pointers, three doubles and kp2d_dist behind w_kp:
    39.  mgr_fk_backward_terms keeps its 31."""
    from manus_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    old = re.search(r"\bint\s+mgr_fk_backward_terms\s*\(([^;]*?)\)\s*;", header, re.S)
    new = re.search(r"\bint\s+mgr_fk_backward_terms2d\s*\(([^;]*?)\)\s*;", header, re.S)
    assert old and new, "include/manus_hip.h does not declare both entries"
    a_old, a_new = ([a.strip() for a in m.group(1).split(",")] for m in (old, new))
    assert len(a_old) == 31 and len(_lib.SIGNATURES["mgr_fk_backward_terms"][1]) == 31
    assert len(a_new) == 39 and a_new[:27] == a_old[:27] and a_new[35:] == a_old[27:]
    assert a_new[27:35] == ["int C", "const float* kp2d_proj", "const float* kp2d_target", "const float* kp2d_weight", "double w_kp2d",
                            "double delta", "double z_min", "float* kp2d_dist"]
    res, bound = _lib.SIGNATURES["mgr_fk_backward_terms2d"]
    assert res is ctypes.c_int and len(bound) == 39 and bound[:27] == _lib.SIGNATURES["mgr_fk_backward_terms"][1][:27]
    assert bound[27] is ctypes.c_int and bound[31:34] == [ctypes.c_double] * 3 and bound[37] is ctypes.c_size_t
    m = re.search(r"\bsize_t\s+mgr_fk_terms2d_workspace_bytes\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["int U", "int J", "int K", "int C"]
    res, bound = _lib.SIGNATURES["mgr_fk_terms2d_workspace_bytes"]
    assert res is ctypes.c_size_t and len(bound) == 4
    assert hasattr(so, "mgr_fk_backward_terms2d") and hasattr(so, "mgr_fk_terms2d_workspace_bytes")
    L = _lib.lib()
    assert L.mgr_fk_terms2d_workspace_bytes(5, 20, 21, 8) >= 5 * 4 * 8 and L.mgr_fk_terms2d_workspace_bytes(0, 20, 21, 8) == 0
    assert L.mgr_fk_terms2d_workspace_bytes(5, 20, 21, 8) >= L.mgr_fk_terms_workspace_bytes(5, 20, 21)


CHAIN = ("frames_listed", "view_rows", "frame_of_view", "rest", "local", "parents", "base", "theta", "mask", "d_transforms", "d_theta")
EXTRA = ("theta_ref", "neighbours", "kp_bone", "kp_offset", "kp_target", "kp_weight", "kp2d_proj", "kp2d_target", "kp2d_weight", "kp2d_dist",
         "values", "workspace")


def _call(L, V=3, J=20, F=4, U=2, K=21, C=5, w=(0.5, 0.25, 2.0, 1.0, 10.0), w2d=0.01, delta=4.0, zmin=0.01, ws_bytes=1 << 20, **null):
    assert set(null) <= set(CHAIN + EXTRA)
    p = {k: (None if null.get(k) else P) for k in CHAIN + EXTRA}
    return L.mgr_fk_backward_terms2d(V, J, F, U, *[p[k] for k in CHAIN], p["theta_ref"], p["neighbours"], w[0], w[1], w[2], w[3], K,
                                     p["kp_bone"], p["kp_offset"], p["kp_target"], p["kp_weight"], w[4], C, p["kp2d_proj"], p["kp2d_target"],
                                     p["kp2d_weight"], w2d, delta, zmin, p["kp2d_dist"], p["values"], p["workspace"], ws_bytes, None)


def _refused(L, rc, text=None, code=None, name=b"mgr_fk_backward_terms2d"):
    from manus_amd._lib import MGR_EINVAL
    err = L.mgr_last_error()
    assert rc == (MGR_EINVAL if code is None else code) and rc != 0, (rc, err)
    assert name in err, err
    if text:
        assert text in err, err


def test_refusals_before_the_device():
    """Every call here passes fake pointers: a refusal that came after a launch, or wrote anything, would fault the process."""
    from manus_amd._lib import MGR_ENOMEM, lib
    L = lib()
    zero = (0.0,) * 5
    bads = (-1.0, float("nan"), float("inf"), -float("inf"))
    # the new scalars, whether the term is on or off
    for w2d in (0.01, 0.0):
        for bad in bads:
            _refused(L, _call(L, w2d=w2d, delta=bad), b"delta")
        for bad in bads + (0.0,):
            _refused(L, _call(L, w2d=w2d, zmin=bad), b"z_min")
    for bad in bads:
        _refused(L, _call(L, w2d=bad), b"w_kp2d")
    # the term on: mgr_fk_backward_terms' conditions for a call with a term on
    for k in CHAIN:
        if k not in ("d_transforms", "view_rows", "frame_of_view"):
            _refused(L, _call(L, **{k: True}), b"null pointer")
    _refused(L, _call(L, view_rows=True), b"null pointer")
    _refused(L, _call(L, frame_of_view=True), b"null pointer")
    for kw in (dict(V=0), dict(V=-2), dict(J=0), dict(J=33), dict(F=0), dict(F=-3), dict(U=0), dict(U=-1)):
        _refused(L, _call(L, **kw))
        _refused(L, _call(L, w=zero, **kw))
    _refused(L, _call(L, V=-1, d_transforms=True, view_rows=True, frame_of_view=True))
    for i in range(5):
        for bad in bads:
            w = [0.5, 0.25, 2.0, 1.0, 10.0]
            w[i] = bad
            _refused(L, _call(L, w=tuple(w)), b"finite")
    _refused(L, _call(L, theta_ref=True), b"theta_ref")
    _refused(L, _call(L, neighbours=True), b"neighbour")
    # what the 2-D term needs, with and without the other terms
    for w in ((0.5, 0.25, 2.0, 1.0, 10.0), zero):
        for C in (0, -1):
            _refused(L, _call(L, w=w, C=C), b"C >= 1")
        for K in (0, -1, 65):
            _refused(L, _call(L, w=w, K=K), b"MGR_FK_MAX_KEYPOINTS")
        for k in ("kp_bone", "kp_offset", "kp2d_proj", "kp2d_target", "kp2d_weight"):
            _refused(L, _call(L, w=w, **{k: True}), b"2-D keypoint term needs")
        _refused(L, _call(L, w=w, values=True), b"values")
        _refused(L, _call(L, w=w, workspace=True), b"workspace")
        need = L.mgr_fk_terms2d_workspace_bytes(2, 20, 21, 5)
        _refused(L, _call(L, w=w, ws_bytes=need - 1), b"workspace too small", code=MGR_ENOMEM)
        _refused(L, _call(L, w=w, ws_bytes=0), b"workspace too small", code=MGR_ENOMEM)
    for k in ("kp_target", "kp_weight"):
        _refused(L, _call(L, **{k: True}), b"3-D keypoint term needs")
    # the term off: mgr_fk_backward_terms' own refusals, under its own name, the 2-D pointers NULL or not
    nul2d = dict(kp2d_proj=True, kp2d_target=True, kp2d_weight=True, kp2d_dist=True)
    old = b"mgr_fk_backward_terms:"
    for k in CHAIN:
        _refused(L, _call(L, w2d=0.0, w=zero, **{k: True}), b"null pointer", name=old)
    _refused(L, _call(L, w2d=0.0, K=65, **nul2d), b"MGR_FK_MAX_KEYPOINTS", name=old)
    _refused(L, _call(L, w2d=0.0, kp_target=True, **nul2d), b"keypoint", name=old)
    _refused(L, _call(L, w2d=0.0, theta_ref=True, C=0, **nul2d), b"theta_ref", name=old)
    _refused(L, _call(L, w2d=0.0, ws_bytes=L.mgr_fk_terms_workspace_bytes(2, 20, 21) - 1, **nul2d), b"workspace too small", code=MGR_ENOMEM, name=old)


# =================================================================================================================
# the fixture and the restatement
# =================================================================================================================
@pytest.mark.parametrize("row", list(Q.ROWS))
def test_fixture_conditions(row):
    """The depth skip is the term's only discontinuous decision: every active detection has fp64 q_z >= 4 z_min and every one
    skipped by depth q_z <= z_min / 4, so fp32 and fp64 decide alike.  Per case at least one active detection inside delta and one
    outside, in a listed frame; and the planted ones are where the docstring says."""
    inp = case(row)
    K, C, F = inp["K"], inp["C"], inp["F"]
    assert (inp["case"], K, C) == Q.ROWS[row] and inp["kp2d_target"].shape == (F, C, K, 2) and inp["kp2d_proj"].shape == (C, 3, 4)
    for name in ("kp2d_proj", "kp2d_target", "kp2d_weight", "kp_offset"):
        x = inp[name]
        assert torch.equal(torch.nan_to_num(x.to(F32).to(F64)), torch.nan_to_num(x)), name      # fp32-representable
    M = R.fk(inp["theta"], inp["rest"], inp["parents"], inp["base"])
    qz = Q.project(inp["kp2d_proj"], T.keypoints_of(M, inp["kp_bone"], inp["kp_offset"]))[..., 2]
    s = inp["kp2d_weight"]
    weighted = s > 0
    active = weighted & (qz > Q.Z_MIN)
    assert bool((qz[active] >= 4.0 * Q.Z_MIN).all()) and bool((qz[weighted & ~active] <= Q.Z_MIN / 4.0).all())
    per, dist, live = Q.term2d(inp, M, Q.DELTA, Q.Z_MIN)
    assert torch.equal(live, active) and bool(torch.isfinite(dist[active]).all()) and bool(torch.isnan(dist[~active]).all())
    _, d32, live32 = Q.term2d(inp, M.to(F32), Q.DELTA, Q.Z_MIN)
    assert torch.equal(live32, active)
    listed = R.LISTED
    d_l, a_l = dist[listed], active[listed]
    inside, outside = int((d_l[a_l] <= Q.DELTA).sum()), int((d_l[a_l] > 3.0 * Q.DELTA).sum())
    print("fixture %-9s K %2d C %2d: %d detections, %d active (%d listed inside delta, %d several delta outside), depth of the active %.3g .. %.3g"
          % (row, K, C, s.numel(), int(active.sum()), inside, outside, float(qz[active].min()), float(qz[active].max())))
    assert inside >= 1 and outside >= 1
    f, c, k = Q.NEAR
    assert s[f, c, k] > 0 and 0.0 < float(qz[f, c, k]) <= Q.Z_MIN / 4.0                    # between 0 and z_min
    f, c, k = Q.BEHIND
    assert s[f, c, k] > 0 and float(qz[f, c, k]) < 0.0                                     # behind its camera
    assert float(s[2, C - 1, 0]) == 0.0 and bool(torch.isnan(inp["kp2d_target"][2, C - 1, 0]).all())
    assert int(torch.isnan(s).sum()) == 1 and int(torch.isnan(inp["kp2d_target"]).sum()) == 2
    if C * K > 1:
        assert bool(torch.isnan(s[5, C - 1, K - 1]))
    assert bool(torch.isfinite(per).all())
    if row == "chain4":
        assert inp["kp_bone"] == [1, 1]
    if row == "fan65":
        assert C > 64 and (C * K) % 64 != 0


@pytest.mark.parametrize("delta", [0.0, Q.DELTA])
@pytest.mark.parametrize("combo", ["2d", "all"])
@pytest.mark.parametrize("row", ["one", "chain4", "hand"])
def test_restatement_gradient_equals_central_differences(row, combo, delta):
    """fp64, every entry of theta of every frame, all rows counted: the five-point central difference of the full E against
    autograd through the restatement, relative to the largest entry of the frame's gradient; the bound is 1e-8, the bar
    test_fk_terms_cpu.py uses for f23's terms.  h = 2.5e-4: a pixel coordinate moves by up to 500 pixels per radian, and the
    truncation h^4 / 30 times the fifth derivative of |r| at |r| of a few pixels needs the smaller step (at 1e-3 it is 7e-8);
    roundoff, 1e-16 / h times E, stays below 1e-10 of the largest gradient.  Huber's rho is C^1, not C^2: the fixture's
    distances keep 20 % of delta away from delta and the stencil moves them by a fraction of a pixel, so none crosses."""
    inp = case(row)
    ones = dict(inp, mask=torch.ones_like(inp["mask"]))
    w = Q.COMBOS[combo]
    J, F = inp["J"], inp["F"]
    _, grad, _ = Q.host_terms2d(ones, F64, w, delta, chain=False)

    def value(theta):
        with torch.no_grad():
            return float(Q.host_values(ones, theta, w, delta))
    h, worst, largest = 2.5e-4, 0.0, float(grad.abs().max())
    for f in range(F):
        num = torch.zeros((J + 2, 3), dtype=F64)
        for r in range(J + 2):
            for c in range(3):
                vals = []
                for sgn in (-2.0, -1.0, 1.0, 2.0):
                    th = inp["theta"].clone()
                    th[f, r, c] += sgn * h
                    vals.append(value(th))
                num[r, c] = (vals[0] - 8.0 * vals[1] + 8.0 * vals[2] - vals[3]) / (12.0 * h)
        if float(grad[f].abs().max()) == 0.0:                                              # a frame whose detections are all skipped
            assert combo == "2d" and float(num.abs().max()) <= 1e-10 * largest
            continue
        worst = max(worst, float((num - grad[f]).abs().max() / grad[f].abs().max()))
    assert largest > 0.0
    print("kp2d restatement against central differences, %s / %s / delta %g: %.3e" % (row, combo, delta, worst))
    assert worst <= 1e-8
    _, masked, _ = Q.host_terms2d(inp, F64, w, delta, chain=False)
    assert bool((masked[:, inp["mask"] == 0] == 0).all())


@pytest.mark.parametrize("row", list(Q.ROWS))
def test_checker_fp32_error_is_small(row):
    """e32 of the restatement per row, every combination: printed, and kept below 1e-3 so the GPU bound 8 e32 stays a check."""
    inp = case(row)
    l = T.LISTS["listed"]
    for combo, w in Q.COMBOS.items():
        for delta in (0.0, Q.DELTA):
            v64, g64, _ = Q.host_terms2d(inp, F64, w, delta, listed=l, chain=False)
            v32, g32, _ = Q.host_terms2d(inp, F32, w, delta, listed=l, chain=False)
            e32 = row_rel_err(g32[l].reshape(-1, 3), g64[l].reshape(-1, 3))
            print("e32 %-9s %-8s delta %g: %.3e, E_kp2d %.4e (fp32 %.1e relative)"
                  % (row, combo, delta, e32, float(v64[4]), abs(float(v32[4]) - float(v64[4])) / float(v64[4])))
            assert e32 <= 1e-3 and bool(torch.isfinite(g64).all()) and bool(torch.isfinite(v64).all()) and float(v64[4]) > 0.0
            assert float(v64[3]) == float(((v64[0] + v64[1]) + v64[2]) + v64[4])


# =================================================================================================================
# host helpers and the refiner's surface
# =================================================================================================================
def test_projection_helpers_on_the_golden_skeleton():
    """`projection_matrices` / `project_keypoints` against mgr_project_points' convention written out, uv = (K (E [x; 1]))[:2] / z, in
    fp64 on the golden skeleton's posed tails: P keeps fp32's 2^-24 per entry, the pixels follow to 1e-3 of a pixel."""
    from manus_amd.pose import project_keypoints, projection_matrices
    d = np.load(R.GOLDEN)
    x = torch.tensor(d["world_pose_tails"], dtype=F64)                                       # (frames, 20, 3)
    g = torch.Generator().manual_seed(77)
    centre = x.reshape(-1, 3).mean(0)
    ext = torch.stack([Q.look_at(centre + 0.8 * v, -v) for v in Q.sphere(3, g)])
    Kin = torch.tensor([[[600.0, 0.5, 300.0], [0.0, 590.0, 250.0], [0.0, 0.0, 1.0]]], dtype=F64).repeat(3, 1, 1)
    P = projection_matrices(Kin, ext)
    assert P.shape == (3, 3, 4) and P.dtype == F32
    e44 = torch.eye(4, dtype=F64).repeat(3, 1, 1)
    e44[:, :3] = ext
    assert torch.equal(projection_matrices(Kin.float(), e44.float()), projection_matrices(Kin.float().double(), ext.float().double()))
    want = Kin @ ext
    assert float(((P.double() - want).abs() / want.abs().clamp_min(1.0)).max()) <= 2.0 ** -24
    uv = project_keypoints(P, x)
    assert uv.shape == (x.shape[0], 3, 20, 2) and uv.dtype == F64
    hom = torch.cat([x, torch.ones_like(x[..., :1])], -1)
    for c in range(3):
        cam = torch.einsum("ij,fkj->fki", ext[c], hom)
        q = torch.einsum("ij,fkj->fki", Kin[c], cam)
        err = float((q[..., :2] / q[..., 2:] - uv[:, c]).abs().max())
        assert bool((q[..., 2] > 0.3).all()) and err <= 1e-3, err
    assert project_keypoints(P, x[0]).shape == (3, 20, 2)
    for bad in ((Kin[:2], ext), (Kin, ext[:, :, :3]), (Kin[0], ext)):
        with pytest.raises(ValueError):
            projection_matrices(*bad)
    with pytest.raises(ValueError):
        project_keypoints(P[0], x)


def _cpu_refiner(row="hand", **kw):
    from manus_amd.pose import KinematicPoseRefiner
    inp = case(row)
    return inp, KinematicPoseRefiner(inp["frame_keys"], inp["rest"], inp["parents"], inp["theta"], 1e-3, 2e-3, device="cpu", **kw)


def test_refiner_keywords_and_set_keypoints_2d():
    inp, plain = _cpu_refiner()
    assert plain.has_terms is False and plain.last_terms is None and plain.last_prior is None and plain.last_kp2d is None
    assert plain.w_kp2d == 0.0 and plain.kp2d_delta == 0.0 and plain.kp2d_zmin == 1e-2 and plain.kp2d is None
    assert sorted(plain.state_dict()) == ["frame_keys", "m", "steps", "theta", "v"]
    _, ref = _cpu_refiner(w_kp2d=0.5, kp2d_delta=4.0, kp2d_zmin=0.02)
    assert ref.has_terms is True and (ref.w_kp2d, ref.kp2d_delta, ref.kp2d_zmin) == (0.5, 4.0, 0.02) and ref.last_kp2d is None
    assert ref.weights == (0.0, 0.0, 0.0, 0.0) and ref.w_kp == 0.0 and sorted(ref.state_dict()) == ["frame_keys", "m", "steps", "theta", "v"]
    for name in ("w_kp2d", "kp2d_delta"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                _cpu_refiner(**{name: bad})
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kp2d_zmin"):
            _cpu_refiner(kp2d_zmin=bad)
    J, F, K, C = inp["J"], inp["F"], inp["K"], inp["C"]
    b, o, P, t, s = inp["kp_bone"], inp["kp_offset"], inp["kp2d_proj"], inp["kp2d_target"], inp["kp2d_weight"]
    # the term on without detections raises at the step, before any entry is called
    ref._posed = torch.zeros((1, J, 4, 4))
    for call in (lambda: ref.step(torch.zeros((1, J + 1, 4, 4)), [0], [0]), lambda: ref.fit_keypoints(1), lambda: ref.reprojection_error()):
        with pytest.raises(ValueError, match="set_keypoints_2d"):
            call()
    with pytest.raises(ValueError, match="bones and offsets"):
        ref.set_keypoints_2d(P, t, s)
    ref.set_keypoints_2d(P, t, bones=b, offsets=o)
    assert torch.equal(ref.kp2d[2], torch.ones((F, C, K))) and ref.kp2d[0].dtype == F32 and ref.kp2d[1].shape == (F, C, K, 2)
    assert ref._kp_geom[0].dtype == torch.int32 and ref._kp_geom[0].tolist() == b and ref.kp is None
    ref.set_keypoints_2d(P, t, s)                                                           # bones / offsets are kept
    assert torch.equal(torch.nan_to_num(ref.kp2d[2]), torch.nan_to_num(s.to(F32)))
    ref.set_keypoints_2d(P, t, s[0], bones=torch.tensor(b), offsets=o)                      # (C,K) and (K,) broadcast
    assert torch.equal(torch.nan_to_num(ref.kp2d[2]), torch.nan_to_num(s[0].to(F32).expand(F, C, K)))
    ref.set_keypoints_2d(P, t, torch.arange(K, dtype=F32))
    assert torch.equal(ref.kp2d[2], torch.arange(K, dtype=F32).expand(F, C, K))
    args = dict(proj=P, targets=t, weights=s, bones=b, offsets=o)
    for bad in (dict(proj=P[:, :, :3]), dict(proj=P[0]), dict(targets=t[..., :1]), dict(targets=t[:, :-1]), dict(targets=t[:-1]),
                dict(weights=s[:, :, :-1]), dict(weights=s[:-1]), dict(weights=s[0, :-1]), dict(bones=None), dict(offsets=None),
                dict(bones=[J] + b[1:]), dict(bones=[0.0] * K), dict(bones=b[:-1], offsets=o[:-1])):
        with pytest.raises(ValueError):
            ref.set_keypoints_2d(**dict(args, **bad))
    # both setters name one set of keypoints
    y3, c3 = inp["kp_target"], inp["kp_weight"]
    ref.set_keypoints(b, o, y3, c3)
    ref.set_keypoints_2d(P, t, s, bones=b, offsets=o)
    with pytest.raises(ValueError, match="share"):
        ref.set_keypoints_2d(P, t, s, bones=b[:1] + [3] + b[2:], offsets=o)
    with pytest.raises(ValueError, match="share"):
        ref.set_keypoints_2d(P, t, s, bones=b, offsets=o + 1.0)
    with pytest.raises(ValueError, match="share"):
        ref.set_keypoints([b[0]] + [2] + b[2:], o, y3, c3)
    with pytest.raises(ValueError):
        ref.set_keypoints(b[:-1], o[:-1], y3[:, :-1], c3[:, :-1])
    assert ref.kp[0].tolist() == b                                                           # a refused call changes nothing
    _, first3d = _cpu_refiner(w_kp=1.0, w_kp2d=1.0)
    first3d.set_keypoints(b, o, y3, c3)
    first3d.set_keypoints_2d(P, t)
    assert first3d._kp_geom[0] is first3d.kp[0]


def test_the_recovery_fixture_prefers_huber_in_fp64():
    """The fixture of the GPU recovery test, on the host in fp64: with camera 1 wrong about the bent finger by 50 pixels, the Huber
    fit ends nearer theta_true than the plain-square fit, and both reduce the term."""
    fx, cfg = Q.recovery_inputs(), Q.RECOVERY
    listed = list(range(fx["F"]))
    assert float(fx["mask"].sum()) == 23.0 and int((fx["theta_true"] != 0).sum()) == 3
    M = R.fk(fx["theta_true"], fx["rest"], fx["parents"], fx["base"])
    _, dist, live = Q.term2d(fx, M, cfg["delta"], Q.Z_MIN)
    assert bool(live.all()) and int((dist > 1.0).sum()) == 3 * len(cfg["finger"]) and abs(float(dist.max()) - 50.0) < 1e-3
    err = {}
    for name, delta in (("huber", cfg["delta"]), ("square", 0.0)):
        th, hist = Q.adam_loop(fx, F64, cfg["w"], delta, cfg["steps"], listed, cfg["lr_rot"], cfg["lr_trans"])
        err[name] = float((th - fx["theta_true"]).abs().max())
        last = float(Q.host_terms2d(fx, F64, cfg["w"], delta, chain=False, theta=th)[0][4])
        print("recovery fixture %-6s: E_kp2d %.4e -> %.4e, max |theta - true| %.4f rad" % (name, float(hist[0, 4]), last, err[name]))
        assert last < float(hist[0, 4])
    assert err["huber"] < 0.5 * err["square"]

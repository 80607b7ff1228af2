"""No GPU: the robust multi-view triangulation (mgr_triangulate, `pose.triangulate_keypoints`, `KinematicPoseRefiner.triangulate`)
-- the ABI in header, binding and built library; every refusal, decided before anything touches a device; the restatement
(tests/triangulate_ref.py) on noise-free detections and its Gauss-Newton gradient against central differences; the fixture
conditions that let test_gpu_triangulate.py judge EVERY problem against the fp64 run, none left out; the argument checks of the
two Python calls and the refiner's weight bookkeeping; and the recovery pipeline of test_gpu_triangulate_refiner.py as a host
fp64 loop on the restatements."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import triangulate_ref as Q
from triangulate_ref import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)          # a fake pointer: a refusal never dereferences it
VARIANTS = [s + (inv,) for s in Q.SHAPES for inv in ((False, True) if s[0] >= Q.RICH and s[1] * s[2] >= 6 else (False,))]


def test_the_entry_is_declared_bound_and_exported():
    from manus_amd import _lib
    text = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mgr_triangulate\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, "include/manus_hip.h does not declare mgr_triangulate"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["int F", "int C", "int K", "const float* proj", "const float* targets", "const float* weights", "double tau",
                    "double min_conf", "int min_views", "double z_min", "double det_min", "int refit_rounds", "int gn_iters", "float* xyz",
                    "float* conf", "int32_t* n_inliers", "uint8_t* inliers", "float* dist", "void* stream"]
    assert re.search(r"#define\s+MGR_TRI_MAX_CAMERAS\s+64\b", header) and _lib.MGR_TRI_MAX_CAMERAS == 64
    res, bound = _lib.SIGNATURES["mgr_triangulate"]
    d, i, p = ctypes.c_double, ctypes.c_int, ctypes.c_void_p
    assert res is ctypes.c_int and bound == [i, i, i, p, p, p, d, d, i, d, d, i, i, p, p, p, p, p, p]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mgr_triangulate")
    from manus_amd import build
    assert "triangulate.hip" in build.SOURCES


REQUIRED = ("proj", "targets", "weights", "xyz", "conf", "n_inliers")


def _call(L, F=4, C=8, K=21, tau=25.0, min_conf=0.1, min_views=3, z_min=1e-2, det_min=1e-6, refit_rounds=2, gn_iters=2, **null):
    assert set(null) <= set(REQUIRED + ("inliers", "dist"))
    p = {k: (None if null.get(k) else P) for k in REQUIRED + ("inliers", "dist")}
    return L.mgr_triangulate(F, C, K, p["proj"], p["targets"], p["weights"], tau, min_conf, min_views, z_min, det_min, refit_rounds, gn_iters,
                             p["xyz"], p["conf"], p["n_inliers"], p["inliers"], p["dist"], None)


def test_refusals_before_the_device():
    """Every call here passes fake pointers: a refusal that came after a launch, or wrote anything, would fault the process."""
    from manus_amd._lib import MGR_EINVAL, lib
    L = lib()

    def refused(rc, text):
        err = L.mgr_last_error()
        assert rc == MGR_EINVAL and rc != 0 and b"mgr_triangulate" in err and text in err, (rc, err)
    for kw in (dict(F=0), dict(F=-1), dict(C=0), dict(C=-3), dict(K=0), dict(K=-2)):
        refused(_call(L, **kw), b"at least 1")
    for C in (65, 66, 1 << 20):
        refused(_call(L, C=C), b"MGR_TRI_MAX_CAMERAS")
    for k in REQUIRED:
        refused(_call(L, **{k: True}), b"null pointer")
    bads = (0.0, -1.0, float("nan"), float("inf"), -float("inf"))
    for name in ("tau", "z_min", "det_min"):
        for bad in bads:
            refused(_call(L, **{name: bad}), name.encode())
    for bad in bads[1:]:
        refused(_call(L, min_conf=bad), b"min_conf")
    for bad in (1, 0, -1):
        refused(_call(L, min_views=bad), b"min_views")
    for bad in (0, -1):
        refused(_call(L, refit_rounds=bad), b"refit_rounds")
    for bad in (-1, -5):
        refused(_call(L, gn_iters=bad), b"gn_iters")
    refused(_call(L, F=1 << 20, K=(1 << 10) + 1), b"2^30")
    # the first of several faults is reported; C = 64 with NULL inliers / dist would pass the checks (not called: it would launch)
    refused(_call(L, C=65, inliers=True, dist=True), b"MGR_TRI_MAX_CAMERAS")


# =================================================================================================================
# the restatement
# =================================================================================================================
@pytest.mark.parametrize("C", [2, 3, 8, 53])
def test_noise_free_detections_give_the_planted_point(C):
    """fp64, exact fp64 projections as targets, all weights 1 (the rigs' looking-away camera and copy of camera 0 included): the planted point to
    1e-9 m, with every refit / polish setting, every ring camera an inlier and its distance below 1e-6 px."""
    g = np.random.default_rng(31 + C)
    proj = Q.ring(C)
    pts = (g.random((6, 3)) - 0.5) * Q.BOX
    t = Q.project(proj, pts)
    away = C - 1 if C >= Q.RICH else None
    for par in (dict(), dict(gn_iters=0), dict(refit_rounds=1), dict(refit_rounds=1, gn_iters=0), dict(refit_rounds=3, gn_iters=4)):
        for x, tx in zip(pts, t):
            p = Q.problem(proj, tx, np.ones(C), F64, min_views=2, **par)
            assert p["valid"] and float(np.abs(p["X"] - x).max()) <= 1e-9, (C, par, p["X"], x)
            assert p["n"] == C - (away is not None) and (away is None or (not p["S"][away] and np.isnan(p["dist"][away])))
            assert float(np.nanmax(p["dist"])) <= 1e-6 and p["conf"] == 1.0


def test_gauss_newton_gradient_equals_central_differences():
    """g = sum_S s J^T r of the polish is the gradient of E = sum_S s |u(X) - t|^2 / 2: five-point central differences in fp64 at a
    point 5 mm off the fit, relative to the largest entry; the bound is 1e-8 (h = 1e-4 m: truncation h^4 / 30 times the fifth
    derivative of a projection at 1 m, roundoff 1e-16 E / h)."""
    fx = Q.case(8, 1, 21)
    r64 = Q.reference(8, 1, 21)[0]
    worst = 0.0
    for k in (0, 5, 20):
        p = r64["problems"][0][k]
        assert p["valid"]
        Pm, t, s = fx["proj"], fx["targets"][0, :, k], fx["weights"][0, :, k]
        t = np.where(p["S"][:, None], t, 0.0)
        X = p["X"] + np.array([0.005, -0.003, 0.004])
        g, _ = Q.reprojection_gradient(Pm, t, s, p["S"], X)
        h, num = 1e-4, np.zeros(3)
        for i in range(3):
            v = []
            for sgn in (-2.0, -1.0, 1.0, 2.0):
                Y = X.copy()
                Y[i] += sgn * h
                v.append(Q.reprojection_gradient(Pm, t, s, p["S"], Y)[1])
            num[i] = (v[0] - 8.0 * v[1] + 8.0 * v[2] - v[3]) / (12.0 * h)
        worst = max(worst, float(np.abs(num - g).max() / np.abs(g).max()))
    print("triangulation: Gauss-Newton gradient against central differences %.3e" % worst)
    assert worst <= 1e-8


# =================================================================================================================
# the fixtures: what lets the GPU test judge every problem
# =================================================================================================================
def _margins(fx, r64, r32):
    """-> (the nearest any classified distance of either run comes to tau, as a fraction of tau; the seeds within one of the best
    count; how many of them end in another final set than the best one), over every problem of a fixture."""
    par = fx["par"]
    tau = par["tau"]
    F, K = fx["F"], fx["K"]
    margin, seeds, changed = np.inf, 0, 0
    for f in range(F):
        for k in range(K):
            p64, p32 = r64["problems"][f][k], r32["problems"][f][k]
            assert np.array_equal(p64["active"], p32["active"]) and np.array_equal(p64["counts"] >= 0, p32["counts"] >= 0)
            for p in (p64, p32):
                for d in p["rounds"]:
                    d = d[np.isfinite(d)].astype(F64)
                    if d.size:
                        margin = min(margin, float(np.abs(d / tau - 1.0).min()))
            if p64["seed"] < 0:
                continue
            best = int(p64["counts"].max())
            near = np.flatnonzero(p64["counts"] >= max(best - 1, 0))
            # what follows a seed depends on it through inliers(X_ab) alone: one run per distinct first set
            _, first, weight = np.unique(p64["sets"][near], axis=0, return_index=True, return_counts=True)
            for i, n_same in zip(near[first], weight):
                q = Q.from_point(p64, fx["proj"], p64["points"][i], **par)
                seeds += int(n_same)
                changed += int(n_same) * int(q["valid"] != p64["valid"] or not np.array_equal(q["S"], p64["S"]))
    return margin, seeds, changed


@pytest.mark.parametrize("C,F,K,seed,invalid", VARIANTS)
def test_fixture_conditions(C, F, K, seed, invalid):
    """(a) the fp32 and the fp64 run end in identical inlier sets (and agree on which problems are valid);
    (b) no distance classified in any refit round or for the final set lies within tau (1 +- 1e-3), in either run;
    (c) every seed pair whose count is at least best - 1 leads to the same final set (fp64): a seed the fp32 kernel picks differently
        cannot change the answer;
    (d) the twin problem's determinant ratio det / m^3 is below det_min / 8 in both runs;
    and what the docstring of `fixture` plants is there."""
    fx = Q.case(C, F, K, seed, invalid)
    r64, r32 = Q.reference(C, F, K, seed, invalid)
    par = fx["par"]
    tau = par["tau"]
    t, s = fx["targets"], fx["weights"]
    assert t.dtype == F32 and s.dtype == F32 and fx["proj"].dtype == F32 and t.shape == (F, C, K, 2) and s.shape == (F, C, K)
    assert np.array_equal(r64["inliers"], r32["inliers"]) and np.array_equal(r64["n_inliers"], r32["n_inliers"])          # (a)
    assert np.array_equal(np.isnan(r64["dist"]), np.isnan(r32["dist"])) and np.array_equal(np.isnan(r64["xyz"]), np.isnan(r32["xyz"]))
    margin, seeds, changed = _margins(fx, r64, r32)
    valid = ~np.isnan(r64["xyz"][..., 0])
    print("fixture C %2d F %d K %2d %s: %d of %d problems valid, inliers %s .. %d, nearest classified distance to tau %.3g of tau, "
          "%d seeds within one of the best, %d of them end elsewhere" % (C, F, K, "invalid" if invalid else "plain", int(valid.sum()), valid.size,
                                                                         r64["n_inliers"][valid].min() if valid.any() else "-", int(r64["n_inliers"].max()), margin, seeds, changed))
    assert margin > 1e-3                                                                                                      # (b)
    assert changed == 0 and seeds >= int(valid.sum())                                                                        # (c)
    assert valid.any()
    err = np.linalg.norm(r64["xyz"] - fx["points"], axis=-1)[valid]
    assert float(err.max()) <= 3e-3              # 0.5 px at 1.2 m and focal 500 is 1.2 mm per camera
    if C >= Q.RICH:
        assert not r64["inliers"][:, [Q.DEAD, C - 1]].any()
        assert int((s[:, Q.DEAD] != 0).sum()) == (2 if invalid else 0)                       # the copy of camera 0 is off but in twin and behind
        assert bool(np.isnan(t[0, 2, 0]).all()) and s[0, 2, 0] > par["min_conf"] and int(np.isnan(t).sum()) == 2
        assert bool(np.isnan(r64["dist"][:, C - 1]).all()) and bool((s[:, C - 1] > par["min_conf"]).sum() >= F * K - 4)  # behind, confident
        if F * K > 1:
            assert bool(((s > 0) & (s < par["min_conf"])).any())
            clean = Q.project(fx["proj"], fx["points"])                                         # (F,K,C,2)
            off = np.linalg.norm(np.moveaxis(clean, 1, 2) - t, axis=-1)
            planted = (off > 10.0) & (s > par["min_conf"])
            planted[:, C - 1] = False
            assert planted.any() and float(off[planted].min()) >= Q.OUTLIER[0] - 1.0
    if invalid:
        pl = fx["invalid"]
        assert sorted(pl) == ["behind", "few1", "few2", "twin"]
        for name, (f, k) in pl.items():
            p64, p32 = r64["problems"][f][k], r32["problems"][f][k]
            assert not p64["valid"] and not p32["valid"] and r64["n_inliers"][f, k] == 0 and bool(np.isnan(r64["dist"][f, :, k]).all()), name
        assert int(r64["problems"][0][1]["active"].sum()) == 1
        few2 = r64["problems"][0][2]
        assert int(few2["active"].sum()) == 2 and few2["counts"].tolist() == [2] and len(few2["rounds"]) == par["refit_rounds"] + 1
        for p in (r64["problems"][0][3], r32["problems"][0][3]):                                                             # (d)
            assert p["pairs"].tolist() == [[0, Q.DEAD]] and p["counts"].tolist() == [-1]
            assert float(p["ratios"][0]) < par["det_min"] / 8.0, float(p["ratios"][0])
        behind = r64["problems"][0][4]
        assert int(behind["active"].sum()) == C - 1 and bool((behind["counts"] == -1).all())
        # the other problems are those of the fixture without the planted ones
        base = Q.case(C, F, K, seed, False)
        other = np.ones((F, K), bool)
        for f, k in pl.values():
            other[f, k] = False
        sel = np.broadcast_to(other[:, None, :], s.shape)
        assert np.array_equal(base["weights"][sel], s[sel]) and np.array_equal(np.nan_to_num(base["targets"][sel]), np.nan_to_num(t[sel]))
    if C == 3 and K > 1:
        assert r64["n_inliers"][0, K - 1] == 0 and len(r64["problems"][0][K - 1]["rounds"]) == par["refit_rounds"] + 1


@pytest.mark.parametrize("C,F,K", Q.ROGUE_SHAPES)
def test_a_rogue_camera_fixture(C, F, K):
    """Camera 4 displaced in every problem: never an inlier, in either run, and the fixture keeps conditions (a) to (c)."""
    fx = Q.case(C, F, K, 0, False, Q.ROGUE)
    r64, r32 = Q.reference(C, F, K, 0, False, Q.ROGUE)
    assert not r64["inliers"][:, Q.ROGUE].any() and not r32["inliers"][:, Q.ROGUE].any() and np.array_equal(r64["inliers"], r32["inliers"])
    assert float(np.nanmin(r64["dist"][:, Q.ROGUE])) >= Q.OUTLIER[0] - 5.0 and not np.isnan(r64["xyz"]).any()
    margin, seeds, changed = _margins(fx, r64, r32)
    assert margin > 1e-3 and changed == 0 and seeds >= F * K


# =================================================================================================================
# the Python surface
# =================================================================================================================
def test_triangulate_keypoints_argument_checks():
    from manus_amd.pose import Triangulation, triangulate_keypoints
    assert Triangulation._fields == ("xyz", "conf", "n_inliers", "inliers", "dist")
    fx = Q.case(8, 1, 21)
    Pm, t, s = (torch.tensor(fx[k]) for k in ("proj", "targets", "weights"))
    good = dict(proj=Pm, targets=t, weights=s)
    bads = [dict(proj=Pm[0]), dict(proj=Pm[:, :, :3]), dict(proj=Pm[:0]), dict(proj=Pm.repeat(9, 1, 1)), dict(targets=t[..., :1]), dict(targets=t[0]),
            dict(targets=t[:, :-1]), dict(targets=t[:0]), dict(weights=s[:, :-1]), dict(weights=s[:, :, :-1]), dict(weights=s[0, 0, :-1]),
            dict(weights=s[..., None])]
    for name in ("tau", "z_min", "det_min"):
        bads += [{name: bad} for bad in (0.0, -1.0, float("nan"), float("inf"))]
    bads += [dict(min_conf=bad) for bad in (-0.1, float("nan"), float("inf"))]
    bads += [dict(min_views=1), dict(min_views=2.5), dict(refit_rounds=0), dict(gn_iters=-1), dict(gn_iters=1.5)]
    for bad in bads:
        with pytest.raises(ValueError, match="triangulate_keypoints"):
            triangulate_keypoints(**dict(good, **bad))


def _cpu_refiner():
    import fk_kp2d_ref as K2
    from manus_amd.pose import KinematicPoseRefiner
    inp = K2.kp2d_inputs("hand")
    return inp, KinematicPoseRefiner(inp["frame_keys"], inp["rest"], inp["parents"], inp["theta"], 1e-3, 2e-3, device="cpu")


def test_refiner_triangulate_refusal_and_bookkeeping():
    """Without `set_keypoints_2d` the call raises before anything else; `_adopt`, the bookkeeping behind the kernel call, on host
    tensors: the 3-D tables become (shared bones, shared offsets, xyz, conf), the 2-D weights are multiplied by the flags, and each
    switch leaves the other table alone."""
    from manus_amd.pose import Triangulation
    inp, ref = _cpu_refiner()
    with pytest.raises(ValueError, match="set_keypoints_2d"):
        ref.triangulate()
    F, C, K = inp["F"], inp["C"], inp["K"]
    ref.set_keypoints_2d(inp["kp2d_proj"], inp["kp2d_target"], inp["kp2d_weight"], bones=inp["kp_bone"], offsets=inp["kp_offset"])
    g = torch.Generator().manual_seed(3)
    xyz = torch.randn((F, K, 3), generator=g)
    xyz[1, 2] = float("nan")
    conf = torch.rand((F, K), generator=g)
    conf[1, 2] = 0.0
    flags = torch.rand((F, C, K), generator=g) < 0.7
    res = Triangulation(xyz, conf, flags.sum(1).int(), flags, torch.zeros((F, C, K)))
    P0, t0, w0 = ref.kp2d
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))
    ref._adopt(res, True, False)
    assert ref.kp[0] is ref._kp_geom[0] and ref.kp[1] is ref._kp_geom[1] and same(ref.kp[2], xyz) and torch.equal(ref.kp[3], conf)
    assert ref.kp2d[2] is w0 and ref.kp[0].tolist() == inp["kp_bone"]
    ref.kp = None
    ref._adopt(res, False, True)
    assert ref.kp is None and ref.kp2d[0] is P0 and ref.kp2d[1] is t0
    want = w0 * flags.float()
    assert same(ref.kp2d[2], want) and bool((ref.kp2d[2][~flags & ~torch.isnan(w0)] == 0).all()) and same(ref.kp2d[2][flags], w0[flags])
    assert int(torch.isnan(w0).sum()) == 1                                                    # the fixture's NaN weight stays NaN: still skipped
    ref._adopt(res, False, False)
    assert ref.kp is None and same(ref.kp2d[2], want)
    for bad in (res._replace(xyz=xyz[:, :-1]), res._replace(conf=conf[:-1]), res._replace(inliers=flags[:, :-1])):
        with pytest.raises(ValueError, match="triangulate"):
            ref._adopt(bad, True, True)
    assert sorted(ref.state_dict()) == ["frame_keys", "m", "steps", "theta", "v"]


def test_the_recovery_pipeline_in_fp64():
    """The host loop test_gpu_triangulate_refiner.py draws its line from: detections only, a start 0.25 m and 0.6 rad off, two wrong
    cameras per frame.  The triangulation flags exactly the wrong cameras' detections and lands within 2 mm of the true keypoints (0.5 px
    at four hand radii and focal 500 is below 1 mm per camera); the fit with w_kp and w_kp2d on the triangulated tables then brings the mean
    keypoint error from 0.24 m to below 2 mm."""
    fx, r = Q.hand_inputs(), Q.hand_recovery()
    tri = r["tri"]
    wrong = fx["wrong"].numpy()
    assert int(wrong.sum(1).min()) == 2 and int(wrong.sum(1).max()) == 2
    assert not tri["inliers"][wrong].any() and tri["inliers"][~wrong].all() and bool((tri["n_inliers"] == fx["C"] - 2).all())
    assert float(np.nanmin(tri["dist"][wrong])) >= Q.OUTLIER[0] - 5.0
    err3d = np.linalg.norm(tri["xyz"] - fx["points"].numpy(), axis=-1)
    print("hand fixture: triangulated keypoints within %.3f mm; host fp64 fit: mean keypoint error %.4f m -> %.3f mm" % (1e3 * err3d.max(), r["start"], 1e3 * r["final"]))
    assert float(err3d.max()) <= 2e-3 and r["start"] >= 0.2 and r["final"] <= 2e-3
    assert float(fx["theta_true"][:, 0].norm(dim=1).min()) > 0.59 and float(fx["theta_true"][:, -1].norm(dim=1).min()) > 0.249
    assert "kp_target" not in fx and bool((r["fx"]["kp2d_weight"][fx["wrong"]] == 0).all())

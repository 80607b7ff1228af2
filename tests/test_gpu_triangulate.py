"""GPU: the robust multi-view triangulation -- mgr_triangulate (csrc/triangulate.hip) and `pose.triangulate_keypoints`.

Checker: tests/triangulate_ref.py, the algorithm of the entry's header comment as numpy in fp64 and in fp32.  `inliers`, `n_inliers`,
the NaN positions of `dist` and which problems are invalid are compared EXACTLY with the fp64 run, for every problem of every
fixture: test_triangulate_cpu.py asserts the margins (fp32 and fp64 runs agree, no classified distance within 1e-3 of tau, every
seed within one of the best ends in the same set, the twin pair's determinant ratio well below det_min) that make that fair.
Tolerance where one is needed: `check_rows`, e_kernel <= 8 * max(e32, 2^-23) in `row_rel_err` against the fp64 run, e32 the fp32
run's own error -- `xyz` per (f, k) row, `conf` per problem, `dist` over its finite entries.  Shapes: C = 2 (min_views = 2), 3, 8, 53
and 64 cameras; F * K = 1, 21 and 5 * 21 problems, the last two ending in a partial workgroup."""
import numpy as np
import pytest
import torch

import triangulate_ref as Q
from pose_chain_ref import check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
VARIANTS = [s + (inv,) for s in Q.SHAPES for inv in ((False, True) if s[0] >= Q.RICH and s[1] * s[2] >= 6 else (False,))]


def run(proj, targets, weights, par, null=(), C=None, fill=7.0):
    """One raw call over prefilled outputs -> (rc, dict of the five outputs as they are afterwards)."""
    from manus_amd._lib import lib, ptr, stream
    proj, targets, weights = (torch.as_tensor(np.array(x)).float().to(DEV).contiguous() for x in (proj, targets, weights))
    F, Cw, K = weights.shape
    C = Cw if C is None else C
    out = dict(xyz=torch.full((F, K, 3), fill, device=DEV), conf=torch.full((F, K), fill, device=DEV),
               n_inliers=torch.full((F, K), -5, dtype=torch.int32, device=DEV), inliers=torch.full((F, Cw, K), 9, dtype=torch.uint8, device=DEV),
               dist=torch.full((F, Cw, K), fill, device=DEV))
    p = {k: (None if k in null else ptr(v)) for k, v in out.items()}
    par = dict(Q.DEFAULTS, **par)
    rc = lib().mgr_triangulate(F, C, K, ptr(proj), ptr(targets), ptr(weights), par["tau"], par["min_conf"], par["min_views"], par["z_min"],
                               par["det_min"], par["refit_rounds"], par["gn_iters"], p["xyz"], p["conf"], p["n_inliers"], p["inliers"], p["dist"],
                               stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in out.items()}


def ok(res):
    from manus_amd._lib import check
    check(res[0], "mgr_triangulate")
    return res[1]


def same_bits(a, b, keys=("xyz", "conf", "n_inliers", "inliers", "dist"), at=None):
    """Equal bits, NaN equal to NaN; `at`: a boolean (F,K) of the problems to compare."""
    for k in keys:
        x, y = a[k], b[k]
        if at is not None:
            x, y = (v.movedim(1, 2)[at] if v.dim() == 3 and k in ("inliers", "dist") else v[at] for v in (x, y))
        if x.dtype.is_floating_point:
            if not (torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))):
                return False
        elif not torch.equal(x, y):
            return False
    return True


def judge(tag, got, r64, r32):
    """Every problem of a call against the two runs of the restatement."""
    valid = ~np.isnan(r64["xyz"][..., 0])
    assert np.array_equal(got["inliers"].numpy().astype(bool), r64["inliers"]) and int(got["inliers"].max()) <= 1, tag
    assert np.array_equal(got["n_inliers"].numpy(), r64["n_inliers"]), tag
    xyz, conf, dist = (got[k].double().numpy() for k in ("xyz", "conf", "dist"))
    assert np.array_equal(np.isnan(dist), np.isnan(r64["dist"])) and np.array_equal(np.isnan(xyz), np.isnan(r64["xyz"])), tag
    # invalid problems: exactly as specified
    assert bool((conf[~valid] == 0.0).all()) and bool((got["n_inliers"].numpy()[~valid] == 0).all()), tag
    inv_cols = np.broadcast_to(~valid[:, None, :], dist.shape)
    assert bool(np.isnan(dist[inv_cols]).all()) and not got["inliers"].numpy()[inv_cols].any(), tag
    if not valid.any():
        return 0.0
    worst = 0.0
    for name, g, a, b in (("xyz", xyz[valid], r64["xyz"][valid], r32["xyz"][valid]), ("conf", conf[valid], r64["conf"][valid], r32["conf"][valid])):
        ek, e32 = check_rows("triangulate %s %s" % (tag, name), torch.tensor(g), torch.tensor(a), torch.tensor(b.astype(np.float64)))
        worst = max(worst, ek / max(e32, 2.0 ** -23))
    live = ~np.isnan(r64["dist"])
    assert np.array_equal(np.isnan(r32["dist"]), ~live)
    ek, e32 = check_rows("triangulate %s dist" % tag, torch.tensor(dist[live]), torch.tensor(r64["dist"][live]), torch.tensor(r32["dist"][live].astype(np.float64)))
    return max(worst, ek / max(e32, 2.0 ** -23))


@pytest.mark.parametrize("C,F,K,seed,invalid", VARIANTS)
def test_against_the_restatement(C, F, K, seed, invalid):
    fx = Q.case(C, F, K, seed, invalid)
    got = ok(run(fx["proj"], fx["targets"], fx["weights"], fx["par"]))
    worst = judge("C%d F%d K%d%s" % (C, F, K, " invalid" if invalid else ""), got, *Q.reference(C, F, K, seed, invalid))
    print("FIGURE triangulate C %2d F %d K %2d %s: worst ratio %.2f" % (C, F, K, "invalid" if invalid else "plain", worst))
    again = ok(run(fx["proj"], fx["targets"], fx["weights"], fx["par"]))
    assert same_bits(again, got)                                                             # two runs: equal bits
    if invalid:
        # the planted problems are invalid, and the other problems keep the bits of the call without them
        base = Q.case(C, F, K, seed, False)
        plain = ok(run(base["proj"], base["targets"], base["weights"], base["par"]))
        other = torch.ones((F, K), dtype=torch.bool)
        for f, k in fx["invalid"].values():
            other[f, k] = False
            assert bool(torch.isnan(got["xyz"][f, k]).all()) and float(got["conf"][f, k]) == 0.0 and int(got["n_inliers"][f, k]) == 0
            assert not bool(got["inliers"][f, :, k].any()) and bool(torch.isnan(got["dist"][f, :, k]).all())
            assert int(plain["n_inliers"][f, k]) >= 3
        assert same_bits(got, plain, at=other)


@pytest.mark.parametrize("C,F,K", [(8, 5, 21), (53, 1, 21)])
def test_a_problem_alone_has_the_bits_it_has_in_the_batch(C, F, K):
    fx = Q.case(C, F, K, 0, True)
    got = ok(run(fx["proj"], fx["targets"], fx["weights"], fx["par"]))
    for f, k in [(0, 0), (0, 3), (0, 4), (F - 1, K - 1), (F - 1, 7)]:
        alone = ok(run(fx["proj"], fx["targets"][f:f + 1, :, k:k + 1], fx["weights"][f:f + 1, :, k:k + 1], fx["par"]))
        part = {key: (v[f:f + 1, :, k:k + 1] if key in ("inliers", "dist") else v[f:f + 1, k:k + 1]) for key, v in got.items()}
        assert same_bits(alone, part), (f, k)


@pytest.mark.parametrize("C,F,K", [(8, 1, 21), (64, 1, 21)])
def test_null_inliers_and_dist_change_nothing_else(C, F, K):
    fx = Q.case(C, F, K, 0, True)
    got = ok(run(fx["proj"], fx["targets"], fx["weights"], fx["par"]))
    for null in (("inliers",), ("dist",), ("inliers", "dist")):
        part = ok(run(fx["proj"], fx["targets"], fx["weights"], fx["par"], null=null))
        assert same_bits(part, got, keys=[k for k in got if k not in null]), null
        for k in null:                                                                       # the prefill: nothing was written
            assert bool((part[k] == (9 if k == "inliers" else 7.0)).all())


def test_65_cameras_are_refused_over_untouched_outputs():
    from manus_amd._lib import MGR_EINVAL, lib
    fx = Q.case(64, 1, 21)
    proj = np.concatenate([fx["proj"], fx["proj"][:1]])
    t, s = np.concatenate([fx["targets"], fx["targets"][:, :1]], 1), np.concatenate([fx["weights"], fx["weights"][:, :1]], 1)
    rc, out = run(proj, t, s, fx["par"], fill=NAN)
    assert rc == MGR_EINVAL and b"mgr_triangulate" in lib().mgr_last_error() and b"MGR_TRI_MAX_CAMERAS" in lib().mgr_last_error()
    assert bool(torch.isnan(out["xyz"]).all()) and bool(torch.isnan(out["conf"]).all()) and bool((out["n_inliers"] == -5).all())
    assert bool((out["inliers"] == 9).all()) and bool(torch.isnan(out["dist"]).all())
    from manus_amd.pose import triangulate_keypoints
    with pytest.raises(ValueError, match="64"):
        triangulate_keypoints(proj, t, s)


@pytest.mark.parametrize("par", [dict(gn_iters=0), dict(refit_rounds=1), dict(refit_rounds=1, gn_iters=0), dict(refit_rounds=3, gn_iters=4)])
@pytest.mark.parametrize("C,F,K", [(8, 1, 21), (53, 1, 21)])
def test_other_round_counts_follow_the_restatement(C, F, K, par):
    fx = Q.case(C, F, K, 0, True)
    ref = Q.reference(C, F, K, 0, True, refit_rounds=par.get("refit_rounds"), gn_iters=par.get("gn_iters"))
    got = ok(run(fx["proj"], fx["targets"], fx["weights"], dict(fx["par"], **par)))
    judge("C%d %s" % (C, par), got, *ref)
    if par.get("gn_iters") == 0:
        # without the polish dist is taken at the point that classified the set: an inlier's is below tau, every other live one not
        d, inl = got["dist"], got["inliers"].bool()
        assert bool((d[inl] < 25.0).all()) and bool((d[~inl & ~torch.isnan(d)] >= 25.0).all())


@pytest.mark.parametrize("C,F,K", Q.ROGUE_SHAPES)
def test_a_rogue_camera_is_flagged_and_changes_nothing(C, F, K):
    """Camera 4 is displaced by 80 px and more in every problem: flagged everywhere, its distance reported, and the point is the
    one triangulated WITHOUT that camera, to the bound (the restatement run on the other C - 1 cameras)."""
    rogue = Q.ROGUE
    fx = Q.case(C, F, K, 0, False, rogue)
    got = ok(run(fx["proj"], fx["targets"], fx["weights"], fx["par"]))
    judge("C%d rogue" % C, got, *Q.reference(C, F, K, 0, False, rogue))
    assert not bool(got["inliers"][:, rogue].any()) and float(got["dist"][:, rogue].min()) >= Q.OUTLIER[0] - 5.0
    keep = [c for c in range(C) if c != rogue]
    without = [Q.triangulate(fx["proj"][keep], fx["targets"][:, keep], fx["weights"][:, keep], dt, **fx["par"]) for dt in (Q.F64, Q.F32)]
    valid = ~np.isnan(without[0]["xyz"][..., 0])
    assert valid.all() and np.array_equal(got["n_inliers"].numpy(), without[0]["n_inliers"])
    check_rows("triangulate C%d without the rogue camera" % C, got["xyz"].reshape(-1, 3), torch.tensor(without[0]["xyz"]).reshape(-1, 3),
               torch.tensor(without[1]["xyz"].astype(np.float64)).reshape(-1, 3))
    less = ok(run(fx["proj"][keep], fx["targets"][:, keep], fx["weights"][:, keep], fx["par"]))
    assert torch.equal(less["inliers"], got["inliers"][:, keep]) and torch.equal(less["n_inliers"], got["n_inliers"])


def test_triangulate_keypoints_is_the_entry():
    """The Python call against the raw one: equal bits, `inliers` as bool, everything on the device; (K,) and (C,K) weights broadcast;
    tensors already on the device are taken as they are."""
    from manus_amd.pose import Triangulation, triangulate_keypoints
    fx = Q.case(8, 5, 21, 0, True)
    got = ok(run(fx["proj"], fx["targets"], fx["weights"], fx["par"]))
    res = triangulate_keypoints(fx["proj"], fx["targets"], fx["weights"], device=DEV)
    assert isinstance(res, Triangulation) and res.inliers.dtype == torch.bool and res.n_inliers.dtype == torch.int32
    assert all(t.device == torch.device(DEV) for t in res)
    mine = dict(xyz=res.xyz.cpu(), conf=res.conf.cpu(), n_inliers=res.n_inliers.cpu(), inliers=res.inliers.cpu().to(torch.uint8), dist=res.dist.cpu())
    assert same_bits(mine, got)
    dev = [torch.tensor(fx[k]).to(DEV) for k in ("proj", "targets", "weights")]
    res2 = triangulate_keypoints(*dev)
    assert torch.equal(res2.inliers, res.inliers) and torch.equal(torch.nan_to_num(res2.xyz), torch.nan_to_num(res.xyz)) and res2.xyz.device == dev[0].device
    for w in (fx["weights"][0], fx["weights"][0, 0], None):
        full = np.ones_like(fx["weights"]) if w is None else np.broadcast_to(w, fx["weights"].shape)
        a = triangulate_keypoints(fx["proj"], fx["targets"], w, device=DEV, min_views=4, gn_iters=1)
        b = ok(run(fx["proj"], fx["targets"], full, dict(min_views=4, gn_iters=1)))
        assert torch.equal(a.n_inliers.cpu(), b["n_inliers"]) and torch.equal(torch.nan_to_num(a.xyz.cpu()), torch.nan_to_num(b["xyz"]))

"""GPU: the multi-view 2-D keypoint term on the kinematic refiner's angles -- mgr_fk_backward_terms2d (csrc/fk.hip) and
`pose.KinematicPoseRefiner` with w_kp2d / kp2d_delta / kp2d_zmin, `set_keypoints_2d`, `reprojection_error`, `fit_keypoints`.

Checker: tests/fk_kp2d_ref.py, the term as host torch on `fk_terms_ref.terms` / `fk_chain_ref.fk` in fp64 and fp32 on the CPU.
Tolerance where one is needed: e_kernel <= 8 * max(e32, 2^-23) in `row_rel_err` per (frame, row) (check_rows); a scalar against
fp64 within `bound_of` of the fp32 restatement's own relative error.  Cases: the six rows of `fk_kp2d_ref.ROWS` -- K = 1 / C = 1,
two keypoints on one bone with two cameras, the hand's 21 with 5, 64 keypoints on 32 bones with 3, 3 keypoints with 65 cameras,
7 with 9 --, F = 6 in two takes of 4 + 2, V = 9, frames [0,1,1,3,-1,0,5,3,1]."""
import functools

import pytest
import torch

import fk_chain_ref as R
import fk_kp2d_ref as Q
import fk_terms_ref as T
from fk_chain_ref import F32, F64, bound_of, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ROWS = list(Q.ROWS)


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def case(row):
    return Q.kp2d_inputs(row)


@functools.lru_cache(maxsize=None)
def reference(row, combo, delta, lname, chain=True):
    """(values64, grad64, dist64, values32, grad32, dist32) of one row, weight combination, delta and list: computed once, shared,
    left unchanged."""
    inp, w, listed = case(row), Q.COMBOS[combo], T.LISTS[lname]
    return Q.host_terms2d(inp, F64, w, delta, listed, chain=chain) + Q.host_terms2d(inp, F32, w, delta, listed, chain=chain)


def run(inp, listed, w, delta=Q.DELTA, chain=True, pad_rows=1, short=0, null2d=False, null3d=False, dist=True, proj=None, target=None,
        weight=None, zmin=Q.Z_MIN):
    """-> (rc, d_theta (U + pad_rows, J+2, 3), values (5,), dist (U + pad_rows, C, K)), all over a NaN fill (dist over a fill of 7)."""
    from manus_amd._lib import lib, ptr, stream
    J, V, F, U, K = inp["J"], inp["V"], inp["F"], len(listed), inp["K"]
    proj = inp["kp2d_proj"] if proj is None else proj
    C = proj.shape[0]
    L = lib()
    out = torch.full((U + pad_rows, J + 2, 3), NAN, device=DEV)
    values = torch.full((5,), NAN, dtype=F64, device=DEV)
    d = torch.full((U + pad_rows, C, K), 7.0, device=DEV)
    ws = torch.empty(int(L.mgr_fk_terms2d_workspace_bytes(U, J, K, C)), dtype=torch.uint8, device=DEV)
    a = [_i32(listed), _i32(inp["rows"]), _i32(inp["frames"]), _dev(inp["rest"]), _dev(inp["local"]), _i32(inp["parents"]), _dev(inp["base"]),
         _dev(inp["theta"]), _dev(inp["mask"]), _dev(inp["dT"])]
    e = [_dev(inp["theta_ref"]), inp["neighbours"].to(DEV), _i32(inp["kp_bone"]), _dev(inp["kp_offset"]), _dev(inp["kp_target"]), _dev(inp["kp_weight"])]
    e2 = [_dev(proj), _dev(inp["kp2d_target"] if target is None else target), _dev(inp["kp2d_weight"] if weight is None else weight)]
    ap, ep, e2p = [ptr(t) for t in a], [ptr(t) for t in e], [ptr(t) for t in e2]
    if not chain:
        ap[1] = ap[2] = ap[9] = None
    if null3d:
        ep[4] = ep[5] = None
    if null2d:
        e2p = [None] * 3
    rc = L.mgr_fk_backward_terms2d(V if chain else 0, J, F, U, *ap, ptr(out), ep[0], ep[1], w["w_dev_rot"], w["w_smooth_rot"], w["w_dev_trans"],
                                   w["w_smooth_trans"], K, ep[2], ep[3], ep[4], ep[5], w["w_kp"], C, e2p[0], e2p[1], e2p[2], w["w_kp2d"],
                                   float(delta), float(zmin), ptr(d) if dist else None, ptr(values), ptr(ws), ws.numel() - short, stream())
    torch.cuda.synchronize()
    return rc, out, values, d


def ok(res):
    from manus_amd._lib import check
    check(res[0], "mgr_fk_backward_terms2d")
    return res[1:]


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def same_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


# =================================================================================================================
# gradient, values and distances against the restatement
# =================================================================================================================
@pytest.mark.parametrize("delta", [0.0, Q.DELTA])
@pytest.mark.parametrize("combo", ["2d", "2d3d", "2dpriors", "all"])
@pytest.mark.parametrize("row", ROWS)
def test_against_the_restatement(row, combo, delta):
    """`2d`, `2d3d` and `2dpriors` run without the chain part on the unviewed frame only; every combination runs with d_transforms
    ("2-D + chain"), so each list checks viewed and unviewed rows."""
    inp, w = case(row), Q.COMBOS[combo]
    off = _dev(inp["mask"]) == 0
    rows = lambda x: x.reshape(-1, 3)
    for lname, listed in T.LISTS.items():
        v64, g64, d64, v32, g32, d32 = reference(row, combo, delta, lname)
        U = len(listed)
        got, values, dist = ok(run(inp, listed, w, delta))
        check_rows("fk kp2d d_theta %s %s %g %s" % (row, combo, delta, lname), rows(got[:U]), rows(g64[listed]), rows(g32[listed]))
        assert bool(off.any()) and bool((got[:U][:, off] == 0.0).all())                   # masked entries: exactly 0
        assert bool(torch.isnan(got[U:]).all()) and bool((dist[U:] == 7.0).all())          # rows behind U are untouched
        vals = values.cpu().tolist()
        e32 = rel(float(v32[4]), float(v64[4])) if float(v64[4]) != 0.0 else 0.0
        print("VALUES %-9s %-8s %g %-8s kp2d %.6e (%.1e; fp32 restatement %.1e) kp %.3e" % (row, combo, delta, lname, vals[4],
              rel(vals[4], float(v64[4])) if float(v64[4]) else 0.0, e32, vals[2]))
        if float(v64[4]) == 0.0:
            assert vals[4] == 0.0                                                           # every detection of the list skipped
        else:
            assert rel(vals[4], float(v64[4])) <= bound_of(e32)
        assert vals[3] == ((vals[0] + vals[1]) + vals[2]) + vals[4]
        if w["w_kp"] > 0:
            assert rel(vals[2], float(v64[2])) <= bound_of(rel(float(v32[2]), float(v64[2])))
        else:
            assert vals[2] == 0.0
        # the distances: NaN exactly where the restatement skips, the others within the bound of the fp32 restatement's own error
        want, want32, have = d64[listed], d32[listed].double(), dist[:U].cpu().double()
        assert torch.equal(torch.isnan(have), torch.isnan(want)) and torch.equal(torch.isnan(want32), torch.isnan(want))
        live = ~torch.isnan(want)
        if bool(live.any()):
            ed = ((have - want).abs() / want)[live].max()
            ed32 = ((want32 - want).abs() / want)[live].max()
            assert float(ed) <= bound_of(float(ed32)), (row, lname, float(ed), float(ed32))
    outside, values, dist = ok(run(inp, [inp["F"], -1], w, delta))
    assert bool((outside[:2] == 0.0).all()) and bool((values == 0.0).all()) and bool(torch.isnan(dist[:2]).all())


@pytest.mark.parametrize("row", ROWS)
def test_the_term_alone_needs_no_view(row):
    """Only w_kp2d on, d_transforms / the view lists / the 3-D tables NULL, V = 0: the term's gradient on every listed row, the
    unviewed frame 2 included; the other four values exactly 0; kp2d_dist = NULL changes nothing."""
    inp, w = case(row), Q.COMBOS["2d"]
    listed = T.LISTS["listed"]
    v64, g64, d64, v32, g32, d32 = reference(row, "2d", Q.DELTA, "listed", False)
    got, values, dist = ok(run(inp, listed, w, chain=False, null3d=True))
    U = len(listed)
    check_rows("fk kp2d alone %s" % row, got[:U].reshape(-1, 3), g64[listed].reshape(-1, 3), g32[listed].reshape(-1, 3))
    vals = values.tolist()
    assert vals[0] == 0.0 and vals[1] == 0.0 and vals[2] == 0.0 and vals[3] == vals[4] and vals[4] > 0.0
    assert bool(torch.isfinite(dist[listed.index(2)]).any()) or row == "one"               # written for a frame no view shows
    again, values2, _ = ok(run(inp, listed, w, chain=False, null3d=True, dist=False))
    assert torch.equal(again[:U], got[:U]) and torch.equal(values2, values)
    with_chain = ok(run(inp, listed, w))
    assert torch.equal(with_chain[1], values) and same_nan(with_chain[2], dist)            # values and distances do not depend on views


# =================================================================================================================
# exact properties
# =================================================================================================================
@pytest.mark.parametrize("combo", ["all", "kp", "zero"])
@pytest.mark.parametrize("row", ["one", "hand", "chain_max"])
def test_zero_weight_is_the_terms_entry(row, combo):
    """w_kp2d == 0: d_theta and values[:4] are `torch.equal` to mgr_fk_backward_terms', values[4] = 0, kp2d_dist all NaN, with the 2-D
    pointers given or NULL."""
    from test_gpu_fk_terms import ok as ok3, run as run3
    inp = case(row)
    w3 = dict(T.ZERO) if combo == "zero" else T.COMBOS[combo]
    listed = T.LISTS["listed"]
    U = len(listed)
    plain, pv = ok3(run3(inp, listed, w3))
    for null in (False, True):
        got, values, dist = ok(run(inp, listed, dict(w3, w_kp2d=0.0), null2d=null))
        assert torch.equal(got[:U], plain[:U]) and bool(torch.isnan(got[U:]).all())
        assert torch.equal(values[:4], pv) and float(values[4]) == 0.0
        assert bool(torch.isnan(dist[:U]).all()) and bool((dist[U:] == 7.0).all())


@pytest.mark.parametrize("row", ["chain4", "hand", "fan65"])
def test_bits_do_not_depend_on_the_list_or_the_run(row):
    inp, w = case(row), Q.COMBOS["all"]
    listed = T.LISTS["listed"]
    got, values, dist = ok(run(inp, listed, w))
    again = ok(run(inp, listed, w))
    assert torch.equal(again[0][:5], got[:5]) and torch.equal(again[1], values) and same_nan(again[2], dist)      # two runs
    perm = [3, 5, 0, 2, 1]
    p, pv, pd = ok(run(inp, perm, w, pad_rows=2))
    for u, f in enumerate(perm):
        assert torch.equal(p[u], got[listed.index(f)]) and same_nan(pd[u], dist[listed.index(f)]), f
    assert bool(torch.isnan(p[len(perm):]).all())
    for a, b in zip(pv.tolist(), values.tolist()):
        assert rel(a, b) <= 1e-12
    # a frame listed alone has the bits it has in the full list (only the 2-D and 3-D terms: a smoothness edge's VALUE is counted
    # by the list, its gradient is not)
    for f in listed:
        alone, av, ad = ok(run(inp, [f], w))
        assert torch.equal(alone[0], got[listed.index(f)]) and same_nan(ad[0], dist[listed.index(f)]), f


@pytest.mark.parametrize("row", ["one", "hand", "fan9"])
def test_a_skipped_detection_is_never_read_into_a_result(row):
    """The targets of every skipped detection -- weight 0, NaN weight, behind the camera, nearer than z_min -- set to NaN, inf and
    1e30: no bit changes."""
    inp, w = case(row), Q.COMBOS["2d3d"]
    listed = T.LISTS["listed"]
    ref = ok(run(inp, listed, w))
    skipped = torch.isnan(reference(row, "2d3d", Q.DELTA, "listed")[2])
    assert bool(skipped[Q.NEAR]) and bool(skipped[Q.BEHIND]) and int(skipped.sum()) >= 4
    for bad in (NAN, float("inf"), 1e30):
        t = inp["kp2d_target"].clone()
        t[skipped] = bad
        got = ok(run(inp, listed, w, target=t))
        assert torch.equal(got[0][:5], ref[0][:5]) and torch.equal(got[1], ref[1]) and same_nan(got[2], ref[2]), bad


@pytest.mark.parametrize("row", ["hand", "fan65"])
def test_camera_order_and_camera_split_change_rounding_only(row):
    """A permuted camera order, judged with `check_rows` against the same reference (the sum over cameras is taken in another
    order); and, with 65 cameras, the call on cameras 0..63 plus the call on camera 64 against the call on all."""
    inp, w = case(row), Q.COMBOS["2d"]
    listed = T.LISTS["listed"]
    U, C = len(listed), inp["C"]
    _, g64, _, _, g32, _ = reference(row, "2d", Q.DELTA, "listed", False)
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(5)).tolist()
    kw = lambda idx: dict(proj=inp["kp2d_proj"][idx], target=inp["kp2d_target"][:, idx], weight=inp["kp2d_weight"][:, idx])
    got, values, dist = ok(run(inp, listed, w, chain=False))
    p, pv, pd = ok(run(inp, listed, w, chain=False, **kw(perm)))
    check_rows("fk kp2d permuted cameras %s" % row, p[:U].reshape(-1, 3), g64[listed].reshape(-1, 3), g32[listed].reshape(-1, 3))
    assert same_nan(pd[:U], dist[:U][:, perm]) and rel(float(pv[4]), float(values[4])) <= 1e-12
    if C > 64:
        a, av, _ = ok(run(inp, listed, w, chain=False, **kw(list(range(64)))))
        b, bv, _ = ok(run(inp, listed, w, chain=False, **kw([64])))
        check_rows("fk kp2d cameras 0..63 + camera 64 %s" % row, (a[:U] + b[:U]).reshape(-1, 3), g64[listed].reshape(-1, 3), g32[listed].reshape(-1, 3))
        assert rel(float(av[4] + bv[4]), float(values[4])) <= 1e-12 and float(bv[4]) > 0.0


def test_a_nan_target_stays_in_its_frame():
    inp, w = case("hand"), Q.COMBOS["all"]
    listed = T.LISTS["listed"]
    got, values, dist = ok(run(inp, listed, w))
    live = ~torch.isnan(reference("hand", "all", Q.DELTA, "listed")[2])
    f = 3
    c, k = [int(i) for i in live[f].nonzero()[0]]
    t = inp["kp2d_target"].clone()
    t[f, c, k, 1] = NAN
    bad, bv, bd = ok(run(inp, listed, w, target=t))
    for u, fr in enumerate(listed):
        if fr == f:
            assert bool(torch.isnan(bad[u]).any()) and bool(torch.isnan(bd[u, c, k]))
        else:
            assert torch.equal(bad[u], got[u]) and same_nan(bd[u], dist[u]), fr
    assert bool(torch.isnan(bv[4])) and torch.equal(bv[:3], values[:3])


def test_a_short_workspace_is_refused_over_untouched_outputs():
    from manus_amd._lib import MGR_ENOMEM, lib
    inp = case("hand")
    rc, out, values, dist = run(inp, T.LISTS["listed"], Q.COMBOS["all"], short=1)
    assert rc == MGR_ENOMEM and b"mgr_fk_backward_terms2d" in lib().mgr_last_error()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(values).all()) and bool((dist == 7.0).all())


def test_projection_helpers_against_mgr_project_points():
    """`pose.project_keypoints(pose.projection_matrices(K, E), x)` against the device's own projection `ops.project_points(x, K, E)`
    on the golden skeleton's posed tails: pixel coordinates up to 640 in magnitude from about sixteen fp32 roundings on the device,
    16 * 2^-24 * 640 = 6e-4 pixels, plus 1.5e-4 from the helper's fp32 storage of P (four products of up to 480 at 2^-24, over a depth
    of 0.8); the bound is 1e-3."""
    import numpy as np
    from manus_amd.ops import project_points
    from manus_amd.pose import project_keypoints, projection_matrices
    x = torch.tensor(np.load(R.GOLDEN)["world_pose_tails"], dtype=F64)
    g = torch.Generator().manual_seed(77)
    centre = x.reshape(-1, 3).mean(0)
    ext = torch.stack([Q.look_at(centre + 0.8 * v, -v) for v in Q.sphere(3, g)]).to(F32)
    Kin = torch.tensor([[[600.0, 0.5, 300.0], [0.0, 590.0, 250.0], [0.0, 0.0, 1.0]]]).repeat(3, 1, 1)
    uv = project_keypoints(projection_matrices(Kin, ext), x)
    worst = 0.0
    for c in range(3):
        dev = project_points(x.to(F32).to(DEV), Kin[c].to(DEV), ext[c].to(DEV)).cpu().double()
        assert dev.shape == uv[:, c].shape and float(uv[:, c].abs().max()) <= 640.0
        worst = max(worst, float((dev - uv[:, c]).abs().max()))
    print("FIGURE projection helpers against mgr_project_points: %.3e pixels" % worst)
    assert worst <= 1e-3


# =================================================================================================================
# the refiner
# =================================================================================================================
def make_refiner(inp, w, delta=Q.DELTA, lr=(0.01, 0.003), keypoints3d=True):
    from manus_amd.pose import KinematicPoseRefiner
    ref = KinematicPoseRefiner(inp["frame_keys"], inp["rest"], inp["parents"], inp["theta"], lr[0], lr[1], mask=inp["mask"], base=inp["base"],
                               device=DEV, kp2d_delta=delta, kp2d_zmin=inp["kp2d_zmin"], **w)
    ref.set_reference(inp["theta_ref"])
    if keypoints3d:
        ref.set_keypoints(inp["kp_bone"], inp["kp_offset"], inp["kp_target"], inp["kp_weight"])
        ref.set_keypoints_2d(inp["kp2d_proj"], inp["kp2d_target"], inp["kp2d_weight"])
    else:
        ref.set_keypoints_2d(inp["kp2d_proj"], inp["kp2d_target"], inp["kp2d_weight"], bones=inp["kp_bone"], offsets=inp["kp_offset"])
    return ref


@pytest.mark.parametrize("combo", ["2d", "all"])
def test_step_equals_the_direct_calls(combo):
    """Two steps through `KinematicPoseRefiner.step` against mgr_fk_backward_terms2d + mgr_fk_adam called by hand, bit for bit."""
    from manus_amd._lib import check, lib, ptr, stream
    from test_gpu_fk_terms import Tables
    inp, w = case("hand"), Q.COMBOS[combo]
    J = inp["J"]
    ref = make_refiner(inp, w, keypoints3d=combo == "all")
    tables = Tables(inp)
    listed = sorted({f for f in inp["frames"] if f >= 0})
    theta = _dev(inp["theta"])
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    inf = torch.full((J + 2, 3), float("inf"), device=DEV)
    keep = [_i32(listed), _dev(inp["mask"]), -inf, inf]
    for step in (1, 2):
        ref.apply(tables, inp["rows"], inp["frames"])
        ref.step(_dev(inp["dT"]), inp["rows"], inp["frames"])
        g, values, _ = ok(run(dict(inp, theta=theta.cpu().double()), listed, w, pad_rows=0))
        check(lib().mgr_fk_adam(len(listed), J, ptr(keep[0]), ptr(g), ptr(theta), ptr(m), ptr(v), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), 0.01,
                                0.003, 0.9, 0.999, 1e-8, step, stream()), "mgr_fk_adam")
        assert ref.last_grad[0] == listed and torch.equal(ref.last_grad[1], g)
        assert torch.equal(ref.theta, theta) and torch.equal(ref.m, m) and torch.equal(ref.v, v) and ref.steps == step
        assert torch.equal(ref.last_terms, values[:4]) and torch.equal(ref.last_kp2d, values[4]) and ref.last_terms.shape == (4,)
        assert ref.last_prior.data_ptr() == ref.last_terms[3:].data_ptr()                  # views of one buffer
        assert ref.last_kp2d.data_ptr() == ref.last_prior.data_ptr() + 8 and float(ref.last_kp2d) > 0.0


def test_reprojection_error_is_kp2d_dist_and_disturbs_nothing():
    from test_gpu_fk_terms import Tables
    inp, w = case("hand"), Q.COMBOS["all"]
    ref = make_refiner(inp, w)
    ref.apply(Tables(inp), inp["rows"], inp["frames"])
    ref.step(_dev(inp["dT"]), inp["rows"], inp["frames"])
    keep = dict(theta=ref.theta.clone(), m=ref.m.clone(), v=ref.v.clone(), terms=ref.last_terms.clone(), kp2d=ref.last_kp2d.clone())
    ptrs = (ref.last_terms.data_ptr(), ref.last_prior.data_ptr(), ref.last_kp2d.data_ptr())
    frames = [4, 0, 3]
    err = ref.reprojection_error(frames)
    direct = ok(run(dict(inp, theta=ref.theta.cpu().double()), frames, Q.COMBOS["2d"], chain=False, pad_rows=0))[2]
    assert err.shape == (3, inp["C"], inp["K"]) and err.dtype == F32 and same_nan(err, direct) and bool(torch.isfinite(err).any())
    assert same_nan(ref.reprojection_error(), ok(run(dict(inp, theta=ref.theta.cpu().double()), range(inp["F"]), Q.COMBOS["2d"], chain=False, pad_rows=0))[2])
    assert torch.equal(ref.theta, keep["theta"]) and torch.equal(ref.m, keep["m"]) and torch.equal(ref.v, keep["v"]) and ref.steps == 1
    assert torch.equal(ref.last_terms, keep["terms"]) and torch.equal(ref.last_kp2d, keep["kp2d"])
    assert ptrs == (ref.last_terms.data_ptr(), ref.last_prior.data_ptr(), ref.last_kp2d.data_ptr())
    # a refiner with the term off still measures its detections
    off = make_refiner(inp, dict(Q.ZERO))
    off.theta.copy_(ref.theta)
    assert same_nan(off.reprojection_error(frames), err) and off.last_terms is None and off.last_kp2d is None


def margin(v32, v64):
    """10 x the host fp32 loop's own deviation from the fp64 loop, floor 1e-3 relative (test_gpu_fk_terms.py)."""
    return max(10.0 * abs(v32 - v64), 1e-3 * abs(v64))


def test_recovery_with_fit_keypoints_prefers_huber():
    """`fit_keypoints` with the 2-D term alone on the fixture test_fk_kp2d_cpu.py checks on the host: the final E_kp2d and the final
    angle error against the fp64 loop's, in the tolerance form of f23's recovery test; the Huber run ends nearer the truth."""
    from manus_amd.pose import KinematicPoseRefiner
    fx, cfg = Q.recovery_inputs(), Q.RECOVERY
    listed = list(range(fx["F"]))
    err = {}
    for name, delta in (("huber", cfg["delta"]), ("square", 0.0)):
        ref = KinematicPoseRefiner(fx["frame_keys"], fx["rest"], fx["parents"], fx["theta"], cfg["lr_rot"], cfg["lr_trans"], mask=fx["mask"],
                                   device=DEV, kp2d_delta=delta, **cfg["w"])
        ref.set_keypoints_2d(fx["kp2d_proj"], fx["kp2d_target"], fx["kp2d_weight"], bones=fx["kp_bone"], offsets=fx["kp_offset"])
        ref.fit_keypoints(cfg["steps"])
        assert ref.m is None and ref.v is None and ref.steps == 0 and ref.last_grad is None
        moved = ref.theta.clone()
        ref.fit_keypoints(1, lr_rot=0.0, lr_trans=0.0)                                     # the values at the final angles; nothing moves
        assert torch.equal(ref.theta, moved)
        e_dev = float(ref.last_kp2d)
        assert float(ref.last_prior) == e_dev and bool((ref.last_terms[:3] == 0.0).all())
        th64, h64 = Q.adam_loop(fx, F64, cfg["w"], delta, cfg["steps"], listed, cfg["lr_rot"], cfg["lr_trans"])
        th32, _ = Q.adam_loop(fx, F32, cfg["w"], delta, cfg["steps"], listed, cfg["lr_rot"], cfg["lr_trans"])
        e64 = float(Q.host_terms2d(fx, F64, cfg["w"], delta, chain=False, theta=th64)[0][4])
        e32 = float(Q.host_terms2d(fx, F64, cfg["w"], delta, chain=False, theta=th32.double())[0][4])
        a_dev, a64, a32 = (float((t.cpu().double() - fx["theta_true"]).abs().max()) for t in (moved, th64, th32))
        print("FIGURE fk kp2d recovery %-6s: E_kp2d %.4e -> device %.6e, fp64 loop %.6e, fp32 loop %.6e (|device - fp64| %.2e, margin %.2e); "
              "max |theta - true| device %.6f, fp64 loop %.6f, fp32 loop %.6f (|device - fp64| %.2e, margin %.2e)"
              % (name, float(h64[0, 4]), e_dev, e64, e32, abs(e_dev - e64), margin(e32, e64), a_dev, a64, a32, abs(a_dev - a64), margin(a32, a64)))
        assert e_dev < float(h64[0, 4])
        assert abs(e_dev - e64) <= margin(e32, e64) and abs(a_dev - a64) <= margin(a32, a64)
        free = fx["mask"] != 0
        assert bool((moved.cpu()[:, ~free] == 0.0).all())
        err[name] = a_dev
    assert err["huber"] < err["square"]

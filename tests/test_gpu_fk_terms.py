"""GPU: the terms on the kinematic refiner's angles -- mgr_fk_backward_terms (csrc/fk.hip) and `pose.KinematicPoseRefiner` with
w_dev_* / w_smooth_* / w_kp, `set_keypoints`, `fit_keypoints`, `keypoints`.

Checker: tests/fk_terms_ref.py, the three terms as host torch on `fk_chain_ref.fk` in fp64 and fp32 on the CPU.  Tolerance where
one is needed: e_kernel <= 8 * max(e32, 2^-23) in `row_rel_err` per (frame, row) (check_rows).  Cases: those of
test_gpu_fk_chain.py with K = 1 (one), two keypoints on one bone and a bone with none (chain4), the dataset's 21 (hand), 64 on
32 bones (chain_max), 7 (fan); F = 6 in two takes of 4 + 2, V = 9, frames [0,1,1,3,-1,0,5,3,1]."""
import functools

import pytest
import torch

import fk_chain_ref as R
import fk_terms_ref as T
from fk_chain_ref import EPS32, F32, F64, bound_of, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def case(name):
    return T.terms_inputs(name)


@functools.lru_cache(maxsize=None)
def reference(name, combo, lname, chain=True):
    """(values64, grad64, values32, grad32) of one case, weight combination and list: computed once, shared, left unchanged."""
    inp = case(name)
    return T.host_terms(inp, F64, T.COMBOS[combo], T.LISTS[lname], chain=chain) + T.host_terms(inp, F32, T.COMBOS[combo], T.LISTS[lname], chain=chain)


def run(inp, listed, w, chain=True, dT=None, theta=None, kp_weight=None, kp_target=None, pad_rows=1, short=0, null_extras=False):
    """-> (rc, d_theta (U + pad_rows, J+2, 3), values (4,)), both over a NaN fill."""
    from manus_amd._lib import lib, ptr, stream
    J, V, F, U, K = inp["J"], inp["V"], inp["F"], len(listed), inp["K"]
    L = lib()
    out = torch.full((U + pad_rows, J + 2, 3), NAN, device=DEV)
    values = torch.full((4,), NAN, dtype=F64, device=DEV)
    ws = torch.empty(int(L.mgr_fk_terms_workspace_bytes(U, J, K)), dtype=torch.uint8, device=DEV)
    a = [_i32(listed), _i32(inp["rows"]), _i32(inp["frames"]), _dev(inp["rest"]), _dev(inp["local"]), _i32(inp["parents"]), _dev(inp["base"]),
         _dev(inp["theta"] if theta is None else theta), _dev(inp["mask"]), _dev(inp["dT"] if dT is None else dT)]
    e = [_dev(inp["theta_ref"]), inp["neighbours"].to(DEV), _i32(inp["kp_bone"]), _dev(inp["kp_offset"]),
         _dev(inp["kp_target"] if kp_target is None else kp_target), _dev(inp["kp_weight"] if kp_weight is None else kp_weight)]
    ap = [ptr(t) for t in a]
    ep = [None] * 6 if null_extras else [ptr(t) for t in e]
    if not chain:
        ap[1] = ap[2] = ap[9] = None
    rc = L.mgr_fk_backward_terms(V if chain else 0, J, F, U, *ap, ptr(out), ep[0], ep[1], w["w_dev_rot"], w["w_smooth_rot"], w["w_dev_trans"],
                                 w["w_smooth_trans"], K, ep[2], ep[3], ep[4], ep[5], w["w_kp"], ptr(values),
                                 None if null_extras else ptr(ws), 0 if null_extras else ws.numel() - short, stream())
    torch.cuda.synchronize()
    return rc, out, values


def ok(res):
    from manus_amd._lib import check
    check(res[0], "mgr_fk_backward_terms")
    return res[1], res[2]


def prior_values_fp32(inp, w, listed):
    """E_dev and E_smooth on the rows `listed` as the fp64 sum of the fp32 differences of the fp32 tables."""
    th, ref, on = inp["theta"].to(F32), inp["theta_ref"].to(F32), (inp["mask"] != 0).to(F64)
    J = inp["J"]
    wd = torch.full((J + 2, 1), w["w_dev_rot"], dtype=F64)
    ws = torch.full((J + 2, 1), w["w_smooth_rot"], dtype=F64)
    wd[-1], ws[-1] = w["w_dev_trans"], w["w_smooth_trans"]
    dev = sum(float((wd * on * (th[f] - ref[f]).double() ** 2).sum()) for f in listed)
    smooth = sum(float((ws * on * (th[f] - th[n]).double() ** 2).sum()) for f, (_, n) in enumerate(inp["neighbours"].tolist())
                 if n >= 0 and (f in listed or n in listed))
    return dev, smooth


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# =================================================================================================================
# gradient and values against the restatement
# =================================================================================================================
@pytest.mark.parametrize("combo", list(T.COMBOS))
@pytest.mark.parametrize("name", R.CASES)
def test_terms_against_the_restatement(name, combo):
    inp, w = case(name), T.COMBOS[combo]
    off = _dev(inp["mask"]) == 0
    rows = lambda x: x.reshape(-1, 3)
    for lname, listed in T.LISTS.items():
        v64, g64, v32, g32 = reference(name, combo, lname)
        U = len(listed)
        got, values = ok(run(inp, listed, w))
        check_rows("fk terms d_theta %s %s %s" % (name, combo, lname), rows(got[:U]), rows(g64[listed]), rows(g32[listed]))
        assert bool(off.any()) and bool((got[:U][:, off] == 0.0).all())                   # masked entries: exactly 0
        assert bool(torch.isnan(got[U:]).all())                                            # rows behind U are untouched
        again, values2 = ok(run(inp, listed, w))
        assert torch.equal(again[:U], got[:U]) and torch.equal(values2, values)           # two runs: equal bits
        vals = values.cpu().tolist()
        dev, smooth = prior_values_fp32(inp, w, listed)
        print("VALUES %-9s %-6s %-8s dev %.3e (%.1e) smooth %.3e (%.1e) kp %.3e (%.1e; fp32 restatement %.1e)"
              % (name, combo, lname, vals[0], rel(vals[0], dev), vals[1], rel(vals[1], smooth), vals[2], rel(vals[2], float(v64[2])),
                 rel(float(v32[2]), float(v64[2]))))
        assert rel(vals[0], dev) <= 1e-10 and rel(vals[1], smooth) <= 1e-10
        assert (vals[0] > 0) == (w["w_dev_rot"] > 0) and (vals[1] > 0) == (w["w_smooth_rot"] > 0)
        if w["w_kp"] > 0:
            assert rel(vals[2], float(v64[2])) <= bound_of(rel(float(v32[2]), float(v64[2])))
        else:
            assert vals[2] == 0.0
        assert vals[3] == (vals[0] + vals[1]) + vals[2]
        # a listed frame that no view shows (2): the terms alone
        if 2 in listed:
            _, t64, _, t32 = reference(name, combo, lname, False)
            u = listed.index(2)
            check_rows("fk terms unviewed frame %s %s %s" % (name, combo, lname), got[u], t64[2], t32[2])
            assert bool((got[u] != 0).any())
    outside, values = ok(run(inp, [inp["F"], -1], w))
    assert bool((outside[:2] == 0.0).all()) and bool((values == 0.0).all())              # outside the table: zeros


@pytest.mark.parametrize("name", R.CASES)
def test_without_d_transforms(name):
    """d_transforms = NULL, the view lists NULL, V = 0: the terms' gradient alone."""
    inp = case(name)
    listed = T.LISTS["listed"]
    v64, g64, v32, g32 = reference(name, "all", "listed", False)
    got, values = ok(run(inp, listed, T.WEIGHTS, chain=False))
    check_rows("fk terms alone %s" % name, got[:len(listed)].reshape(-1, 3), g64[listed].reshape(-1, 3), g32[listed].reshape(-1, 3))
    with_chain = ok(run(inp, listed, T.WEIGHTS))[1]
    assert torch.equal(values, with_chain)                                                 # the values do not depend on views


@pytest.mark.parametrize("name", ["one", "hand", "chain_max"])
def test_zero_weights_are_the_plain_entry(name):
    from test_gpu_fk_chain import backward
    inp = case(name)
    listed = T.LISTS["listed"]
    plain = backward(inp, listed)
    for null in (False, True):
        got, values = ok(run(inp, listed, T.ZERO, null_extras=null))
        assert torch.equal(got[:len(listed)], plain[:len(listed)]) and bool(torch.isnan(got[len(listed):]).all())
        assert bool((values == 0.0).all())


@pytest.mark.parametrize("name", ["one", "chain4", "hand"])
def test_every_keypoint_skipped(name):
    """w_kp on, every weight zero, negative or NaN and every target NaN: the chain gradient alone, and E_kp exactly 0."""
    inp = case(name)
    listed = T.LISTS["listed"]
    _, _, g64 = R.host_chain(inp, F64)
    _, _, g32 = R.host_chain(inp, F32)
    c = torch.zeros_like(inp["kp_weight"])
    c[1::3] = -1.0
    c[2::3] = NAN
    got, values = ok(run(inp, listed, T.COMBOS["kp"], kp_weight=c, kp_target=torch.full_like(inp["kp_target"], NAN)))
    assert bool(torch.isfinite(got[:len(listed)]).all())
    check_rows("fk terms, every keypoint skipped %s" % name, got[:len(listed)].reshape(-1, 3), g64[listed].reshape(-1, 3), g32[listed].reshape(-1, 3))
    assert float(values[2]) == 0.0 and float(values[3]) == 0.0


@pytest.mark.parametrize("name", ["chain4", "hand"])
def test_jacobi_unlisted_rows_and_permutations(name):
    from manus_amd._lib import check, lib, ptr, stream
    inp, w = case(name), T.WEIGHTS
    J, F = inp["J"], inp["F"]
    # two adjacent listed rows = two calls of one row each from the same tables
    both, _ = ok(run(inp, [1, 2], w))
    assert torch.equal(both[0], ok(run(inp, [1], w))[0][0]) and torch.equal(both[1], ok(run(inp, [2], w))[0][0])
    # a permuted list: equal bits per row, values within 1e-12
    listed = T.LISTS["listed"]
    got, values = ok(run(inp, listed, w))
    perm = [3, 5, 0, 2, 1]
    p, pv = ok(run(inp, perm, w, pad_rows=2))
    for u, f in enumerate(perm):
        assert torch.equal(p[u], got[listed.index(f)]), f
    assert bool(torch.isnan(p[len(perm):]).all())
    for a, b in zip(pv.tolist(), values.tolist()):
        assert rel(a, b) <= 1e-12
    # behind mgr_fk_adam only the listed rows of theta have moved; the tables the entry read are untouched
    theta = _dev(inp["theta"])
    start = theta.clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    inf = torch.full((J + 2, 3), float("inf"), device=DEV)
    keep = [_i32([1, 2]), _dev(inp["mask"]), -inf, inf]
    check(lib().mgr_fk_adam(2, J, ptr(keep[0]), ptr(both), ptr(theta), ptr(m), ptr(v), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), 0.01, 0.003, 0.9,
                            0.999, 1e-8, 1, stream()), "mgr_fk_adam")
    for f in range(F):
        assert torch.equal(theta[f], start[f]) == (f not in (1, 2)), f
    # a NaN in one view's d_transforms stays in that frame's row; the values keep their bits
    k = 3
    dT = inp["dT"].clone()
    dT[k, 0, 1, 2] = NAN
    bad, bv = ok(run(inp, listed, w, dT=dT))
    for u, f in enumerate(listed):
        if f == inp["frames"][k]:
            assert bool(torch.isnan(bad[u]).any())
        else:
            assert torch.equal(bad[u], got[u]), f
    assert torch.equal(bv, values)


def test_a_short_workspace_is_refused_over_untouched_outputs():
    from manus_amd._lib import MGR_ENOMEM, lib
    inp = case("hand")
    rc, out, values = run(inp, T.LISTS["listed"], T.WEIGHTS, short=1)
    assert rc == MGR_ENOMEM and b"mgr_fk_backward_terms" in lib().mgr_last_error()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(values).all())


# =================================================================================================================
# the refiner
# =================================================================================================================
class Tables:
    """What `KinematicPoseRefiner.apply` needs of a compute object: the posed and transforms tables."""

    def __init__(self, inp):
        self.s = dict(posed=_dev(inp["posed"]), transforms=torch.zeros((inp["n_all"], inp["J"] + 1, 4, 4), device=DEV))

    def gathered_transforms(self, view_ids):
        return None

    def transforms_changed(self, written=None):
        pass


def margin(v32, v64):
    """10 x the host fp32 loop's own deviation from the fp64 loop, floor 1e-3 relative."""
    return max(10.0 * abs(v32 - v64), 1e-3 * abs(v64))


DESCENT_STEPS, DESCENT_LR = 40, (0.01, 0.003)


def test_descent_through_the_refiner_step():
    """40 steps of the terms alone (zero d_transforms) through `KinematicPoseRefiner.step` on the hand: E on the listed rows, last
    over first, against the fp64 host loop's fraction.  Measured on an MI355X: see DESIGN.md section 6, row f23."""
    from manus_amd.pose import KinematicPoseRefiner
    inp = case("hand")
    ref = KinematicPoseRefiner(inp["frame_keys"], inp["rest"], inp["parents"], inp["theta"], DESCENT_LR[0], DESCENT_LR[1], mask=inp["mask"],
                               base=inp["base"], device=DEV, **T.WEIGHTS)
    ref.set_reference(inp["theta_ref"])
    ref.set_keypoints(inp["kp_bone"], inp["kp_offset"], inp["kp_target"], inp["kp_weight"])
    tables = Tables(inp)
    zero = torch.zeros((inp["V"], inp["J"] + 1, 4, 4), device=DEV)
    history = []
    for _ in range(DESCENT_STEPS):
        ref.apply(tables, inp["rows"], inp["frames"])
        ref.step(zero, inp["rows"], inp["frames"])
        history.append(ref.last_terms)
        assert ref.last_prior.data_ptr() == ref.last_terms[3:].data_ptr()
    listed = sorted({f for f in inp["frames"] if f >= 0})
    assert ref.steps == DESCENT_STEPS and ref.last_grad[0] == listed
    e = torch.stack(history).cpu()[:, 3]
    h64 = T.adam_loop(inp, F64, T.WEIGHTS, DESCENT_STEPS, listed, *DESCENT_LR)[1][:, 3]
    h32 = T.adam_loop(inp, F32, T.WEIGHTS, DESCENT_STEPS, listed, *DESCENT_LR)[1][:, 3]
    frac, f64, f32 = float(e[-1] / e[0]), float(h64[-1] / h64[0]), float(h32[-1] / h32[0])
    print("FIGURE fk terms descent: E %.6e -> %.6e, fraction %.6f; fp64 loop %.6e -> %.6e, fraction %.6f; fp32 loop fraction %.6f; "
          "|device - fp64| %.2e, margin %.2e" % (float(e[0]), float(e[-1]), frac, float(h64[0]), float(h64[-1]), f64, f32, abs(frac - f64),
                                                margin(f32, f64)))
    assert frac < 1.0 and abs(frac - f64) <= margin(f32, f64)
    unlisted = [f for f in range(inp["F"]) if f not in listed]
    assert torch.equal(ref.theta[unlisted], _dev(inp["theta"])[unlisted])


def test_recovery_with_fit_keypoints():
    """`fit_keypoints(100)` on the fixture test_fk_terms_cpu.py checks on the host: E_kp at the end against the fp64 loop's, the
    training state untouched, and the `keypoints()` residual against `last_terms[2]`."""
    from manus_amd.pose import KinematicPoseRefiner
    fx, cfg = T.recovery_inputs(), T.RECOVERY
    F, J = fx["F"], fx["J"]
    ref = KinematicPoseRefiner(fx["frame_keys"], fx["rest"], fx["parents"], fx["theta"], cfg["lr_rot"], cfg["lr_trans"], mask=fx["mask"],
                               device=DEV, **cfg["w"])
    ref.set_keypoints(fx["kp_bone"], fx["kp_offset"], fx["kp_target"], fx["kp_weight"])
    ref.fit_keypoints(cfg["steps"])
    assert ref.m is None and ref.v is None and ref.steps == 0 and ref.last_grad is None
    moved = ref.theta.clone()
    ref.fit_keypoints(1, lr_rot=0.0, lr_trans=0.0)                                       # the values at the final angles; nothing moves
    assert torch.equal(ref.theta, moved) and ref.m is None and ref.steps == 0
    e_dev = float(ref.last_terms[2])
    assert float(ref.last_terms[0]) == 0.0 and float(ref.last_terms[1]) == 0.0 and float(ref.last_prior) == e_dev
    listed = list(range(F))
    w = cfg["w"]
    th64, h64 = T.adam_loop(fx, F64, w, cfg["steps"], listed, cfg["lr_rot"], cfg["lr_trans"])
    th32, _ = T.adam_loop(fx, F32, w, cfg["steps"], listed, cfg["lr_rot"], cfg["lr_trans"])
    e64 = float(T.host_terms(fx, F64, w, chain=False, theta=th64)[0][2])
    e32 = float(T.host_terms(fx, F64, w, chain=False, theta=th32.double())[0][2])
    print("FIGURE fk terms recovery: E_kp %.4e -> device %.6e, fp64 loop %.6e, fp32 loop %.6e; |device - fp64| %.2e, margin %.2e"
          % (float(h64[0, 2]), e_dev, e64, e32, abs(e_dev - e64), margin(e32, e64)))
    assert e_dev < 0.01 * float(h64[0, 2])
    assert abs(e_dev - e64) <= margin(e32, e64)
    free = fx["mask"] != 0
    assert bool((moved.cpu()[:, ~free] == 0.0).all()) and bool((moved.cpu()[:, free] != 0.0).any())
    # keypoints(): E_kp from the posed keypoints.  Each coordinate of p carries at most delta = 8 * 2^-23 * max|y| of fp32 error in
    # either evaluation, and |dE| <= 2 delta sqrt(3 w_kp sum(c)) sqrt(E) (Cauchy-Schwarz over E = w_kp sum c r^2)
    p = ref.keypoints(list(range(F)), listed).double().cpu()
    assert p.shape == (F, J + 1, 3)
    e_host = float(w["w_kp"] * (fx["kp_weight"] * ((p - fx["kp_target"]) ** 2).sum(-1)).sum())
    delta = 8.0 * EPS32 * float(fx["kp_target"].abs().max())
    tol = 2.0 * (2.0 * delta) * (3.0 * w["w_kp"] * float(fx["kp_weight"].sum())) ** 0.5 * e_dev ** 0.5
    print("FIGURE fk terms recovery: keypoints() residual %.6e against last_terms[2] %.6e (|diff| %.2e, tolerance %.2e)" % (e_host, e_dev, abs(e_host - e_dev), tol))
    assert abs(e_host - e_dev) <= tol

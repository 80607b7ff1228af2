"""GPU: the priors on the pose corrections -- mgr_pose_backward_prior (csrc/pose.hip) in front of the unchanged mgr_pose_adam, and
`pose.PoseRefiner` with w_mag_* / w_smooth_*.

Checker: tests/pose_prior_ref.py (fp64 restatement and its own fp32 run).  Tolerance where one is needed: the project's
`check_rows`, e_kernel <= 8 * max(e32, 2^-23) in `row_rel_err` per (frame, bone) row.  Shapes: B = 1, 20, 32; F = 6 in two takes
(4 + 2); V = 9 positions that show every frame; lists of one interior row, a first and a last row of a take, two adjacent rows and
all rows; an F = 1 table; and F = 12 with B = 32, where the (u, bone) threads of the backward itself span two workgroups."""
import functools

import pytest
import torch

import pose_chain_ref as R
import pose_prior_ref as P
from pose_chain_ref import F32, F64, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB = P.neighbours_of(P.KEYS)
LISTS = {"interior": [1], "first": [0], "last": [3], "first of the short take": [4], "adjacent": [1, 2], "all": [0, 1, 2, 3, 4, 5]}
MODES = {"all four": P.WEIGHTS, "magnitude": P.ONLY_MAG, "smoothness": P.ONLY_SMOOTH}
NAMES = ("rotvec", "trans", "m_r", "v_r", "m_t", "v_t")


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _nb(nb):
    return torch.tensor([list(p) for p in nb], dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def case(B, V=9, keys=tuple(P.KEYS)):
    nb = P.neighbours_of(list(keys))
    return P.chain_case(B, V, nb), nb


def backward_prior(inp, nb, listed, w, pad_rows=1, ws_bytes=None, neighbours=True, value=True, dT=None, tables=None):
    """The raw entry -> (rc, d_rotvec, d_trans (U + pad_rows,B,3) NaN-filled, prior_value: a NaN-filled double scalar or None)."""
    from manus_amd._lib import lib, ptr, stream
    B, V, U = inp["B"], inp["V"], len(listed)
    L = lib()
    g_r = torch.full((U + pad_rows, B, 3), float("nan"), device=DEV)
    g_t = torch.full((U + pad_rows, B, 3), float("nan"), device=DEV)
    val = torch.full((), float("nan"), dtype=F64, device=DEV) if value else None
    need = int(L.mgr_pose_prior_workspace_bytes(U, B))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=DEV)
    rv, tr = tables if tables is not None else (_dev(inp["rotvec"]), _dev(inp["trans"]))
    args = [_i32(listed), _i32(inp["rows"]), _i32(inp["frames"]), _dev(inp["posed"]), _dev(inp["rest"]), rv, tr,
            _dev(inp["dT"]) if dT is None else dT]
    nbt = _nb(nb) if neighbours else None
    rc = L.mgr_pose_backward_prior(V, B, inp["F"], U, *[ptr(t) for t in args], ptr(g_r), ptr(g_t), ptr(nbt), *[float(x) for x in w], ptr(val),
                                   ptr(ws), need if ws_bytes is None else ws_bytes, stream())
    torch.cuda.synchronize()
    return rc, g_r, g_t, val


def adam(B, listed, g_r, g_t, state, step=1, lr=P.LR):
    from manus_amd._lib import check, lib, ptr, stream
    lt = _i32(listed)
    check(lib().mgr_pose_adam(len(listed), B, ptr(lt), ptr(g_r), ptr(g_t), *[ptr(state[k]) for k in NAMES], lr[0], lr[1], P.BETAS[0], P.BETAS[1],
                              P.EPS, step, stream()), "mgr_pose_adam")
    torch.cuda.synchronize()


def fresh_state(inp, moments=None):
    st = dict(rotvec=_dev(inp["rotvec"]), trans=_dev(inp["trans"]))
    for k in NAMES[2:]:
        st[k] = torch.zeros_like(st["rotvec"]) if moments is None else _dev(moments[k])
    return st


def full_step(inp, nb, listed, w, moments=None, dT=None):
    """backward_prior on the tables of `inp`, then mgr_pose_adam -> (state after, g_r, g_t, value)."""
    from manus_amd._lib import MGR_OK
    st = fresh_state(inp, moments)
    rc, g_r, g_t, val = backward_prior(inp, nb, listed, w, dT=dT, tables=(st["rotvec"], st["trans"]))
    assert rc == MGR_OK
    U = len(listed)
    assert bool(torch.isnan(g_r[U:]).all()) and bool(torch.isnan(g_t[U:]).all())           # rows behind U are not the kernel's
    adam(inp["B"], listed, g_r, g_t, st)
    return st, g_r[:U], g_t[:U], val


# =================================================================================================================
# 1. weights zero: today's path, bit for bit
# =================================================================================================================
@pytest.mark.parametrize("B", R.BONES)
@pytest.mark.parametrize("V", R.VIEWS)
def test_zero_weights_are_pose_backward_bit_for_bit(B, V):
    from manus_amd._lib import MGR_OK, check, lib, ptr, stream
    inp = R.chain_inputs(B, V)
    nb = [(-1, 1), (0, 2), (1, 3), (2, -1)]
    listed = sorted(set(inp["frames"])) + [2]             # (frame 2 is never viewed)
    U = len(listed)
    g_r = torch.full((U, B, 3), float("nan"), device=DEV)
    g_t = torch.full((U, B, 3), float("nan"), device=DEV)
    args = [_i32(listed), _i32(inp["rows"]), _i32(inp["frames"])] + [_dev(inp[k]) for k in ("posed", "rest", "rotvec", "trans", "dT")]
    check(lib().mgr_pose_backward(V, B, inp["F"], U, *[ptr(t) for t in args], ptr(g_r), ptr(g_t), stream()), "mgr_pose_backward")
    want = fresh_state(inp)
    adam(B, listed, g_r, g_t, want)
    for kw in (dict(), dict(neighbours=False, value=False)):
        rc, p_r, p_t, val = backward_prior(inp, nb, listed, (0.0, 0.0, 0.0, 0.0), pad_rows=0, **kw)
        assert rc == MGR_OK
        assert torch.equal(p_r, g_r) and torch.equal(p_t, g_t), kw
        assert val is None or float(val) == 0.0
        got = fresh_state(inp)
        adam(B, listed, p_r, p_t, got)
        for k in NAMES:
            assert torch.equal(got[k], want[k]), (kw, k)


def test_refiner_without_weights_takes_todays_two_entries(monkeypatch):
    """`PoseRefiner` with all weights zero never reaches the new entry, keeps `last_prior` None and today's state dict."""
    from manus_amd import _lib
    from manus_amd.pose import PoseRefiner
    inp = R.chain_inputs(20, 3)
    called = []
    real = _lib.lib()

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(real, name)
    import manus_amd.pose as pose_mod
    monkeypatch.setattr(pose_mod, "lib", lambda: Spy())
    ref = PoseRefiner([("a", k) for k in range(4)], 20, inp["rest"], 1e-3, 1e-3, device=DEV)
    ref.rotvec.copy_(_dev(inp["rotvec"]))
    ref._posed = _dev(inp["posed"])
    ref.step(_dev(inp["dT"]), inp["rows"], inp["frames"])
    assert called == ["mgr_pose_backward", "mgr_pose_adam"] and ref.last_prior is None
    assert sorted(ref.state_dict()) == sorted(["frame_keys", "steps", "rotvec", "trans", "m_r", "v_r", "m_t", "v_t"])
    del called[:]
    pri = PoseRefiner([("a", k) for k in range(4)], 20, inp["rest"], 1e-3, 1e-3, device=DEV, w_mag_trans=0.5)
    pri._posed = ref._posed
    pri.step(_dev(inp["dT"]), inp["rows"], inp["frames"])
    assert called == ["mgr_pose_prior_workspace_bytes", "mgr_pose_backward_prior", "mgr_pose_adam"]
    assert pri.last_prior.dtype == F64 and pri.last_prior.device.type == "cuda" and float(pri.last_prior) == 0.0      # zero tables
    assert sorted(pri.state_dict()) == sorted(ref.state_dict())


# =================================================================================================================
# 2. the full chain per (frame, bone) row against the restatement
# =================================================================================================================
def _check_step(tag, inp, nb, listed, w):
    st, g_r, g_t, val = full_step(inp, nb, listed, w)
    r64, r32 = P.regularised_step(inp, nb, listed, w, F64), P.regularised_step(inp, nb, listed, w, F32)
    rows = lambda t: t.reshape(-1, 3)
    check_rows("%s d_rotvec" % tag, rows(g_r), rows(r64["g_r"]), rows(r32["g_r"]))
    check_rows("%s d_trans" % tag, rows(g_t), rows(r64["g_t"]), rows(r32["g_t"]))
    for k in NAMES:
        check_rows("%s %s" % (tag, k), rows(st[k][listed]), rows(r64[k][listed]), rows(r32[k][listed]))
    want = P.total_listed_value(inp["rotvec"], inp["trans"], nb, listed, w, diff_dtype=F32)
    assert abs(float(val) - want) <= 1e-10 * max(want, 1e-300), (tag, float(val), want)
    return st


@pytest.mark.parametrize("B", R.BONES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_regularised_step_against_the_restatement(B, mode):
    inp, nb = case(B)
    assert set(inp["frames"]) == set(range(P.F))              # every frame is shown
    for name, listed in LISTS.items():
        _check_step("B=%d %s, %s" % (B, mode, name), inp, nb, listed, MODES[mode])


@pytest.mark.parametrize("B", R.BONES)
def test_a_take_of_one_frame(B):
    """F = 1: no neighbour at all; the smoothness weights change nothing, the magnitude terms act."""
    inp, nb = case(B, 3, (("solo", 5),))
    assert nb == [(-1, -1)] and inp["frames"] == [0, 0, 0]
    _check_step("B=%d F=1" % B, inp, nb, [0], P.WEIGHTS)
    a = full_step(inp, nb, [0], P.ONLY_SMOOTH)
    b = full_step(inp, nb, [0], (0.0, 7.0, 0.0, 0.25))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and float(a[3]) == 0.0 and float(b[3]) == 0.0


def test_threads_over_two_workgroups():
    """F = 12 in three takes (7 + 4 + 1), B = 32, all rows listed: 384 (u, bone) threads, two workgroups of the backward (and five
    of the Adam behind it)."""
    keys = tuple([("a", i) for i in range(7)] + [("b", 2 * i) for i in range(4)] + [("c", 0)])
    inp, nb = case(32, 9, keys)
    _check_step("B=32 F=12, all rows", inp, nb, list(range(12)), P.WEIGHTS)
    _check_step("B=32 F=12, the rows on either side of the workgroup border", inp, nb, [6, 7, 8], P.WEIGHTS)


# =================================================================================================================
# 3. Jacobi   4. unlisted rows   5. permuted lists
# =================================================================================================================
def _moments(B, seed=1):
    g = torch.Generator().manual_seed(77 + B + seed)
    m = {k: R.rounded(0.1 * torch.randn((P.F, B, 3), generator=g, dtype=F64)) for k in ("m_r", "m_t")}
    m.update({k: R.rounded(0.01 * torch.rand((P.F, B, 3), generator=g, dtype=F64)) for k in ("v_r", "v_t")})
    return m


@pytest.mark.parametrize("B", R.BONES)
def test_adjacent_listed_rows_see_the_tables_before_the_step(B):
    inp, nb = case(B)
    both = full_step(inp, nb, [1, 2], P.WEIGHTS, moments=_moments(B))
    one = full_step(inp, nb, [1], P.WEIGHTS, moments=_moments(B))
    two = full_step(inp, nb, [2], P.WEIGHTS, moments=_moments(B))
    assert torch.equal(both[1][0], one[1][0]) and torch.equal(both[2][0], one[2][0])       # the gradients
    assert torch.equal(both[1][1], two[1][0]) and torch.equal(both[2][1], two[2][0])
    for k in NAMES:
        assert torch.equal(both[0][k][1], one[0][k][1]), k
        assert torch.equal(both[0][k][2], two[0][k][2]), k
    assert not torch.equal(both[0]["rotvec"][1], _dev(inp["rotvec"])[1])                     # (and the rows did move)


@pytest.mark.parametrize("B", R.BONES)
def test_rows_never_listed_keep_their_bits(B):
    inp, nb = case(B)
    mom = _moments(B)
    start = fresh_state(inp, mom)
    for listed in ([1], [0, 3], [1, 2], [4]):
        st = full_step(inp, nb, listed, P.WEIGHTS, moments=mom)[0]
        for f in range(P.F):
            for k in NAMES:
                assert torch.equal(st[k][f], start[k][f]) == (f not in listed), (listed, f, k)


def test_a_permuted_list_gives_the_same_rows():
    inp, nb = case(32)
    mom = _moments(32)
    base = full_step(inp, nb, [0, 1, 2, 3, 4, 5], P.WEIGHTS, moments=mom)
    for listed in ([3, 0, 5, 1, 4, 2], [5, 4, 3, 2, 1, 0]):
        st, g_r, g_t, val = full_step(inp, nb, listed, P.WEIGHTS, moments=mom)
        for k in NAMES:
            assert torch.equal(st[k], base[0][k]), (listed, k)
        for u, f in enumerate(listed):
            assert torch.equal(g_r[u], base[1][f]) and torch.equal(g_t[u], base[2][f]), (listed, f)
        assert abs(float(val) - float(base[3])) <= 1e-12 * float(base[3]), (listed, float(val), float(base[3]))
    part = full_step(inp, nb, [1, 3, 4], P.WEIGHTS, moments=mom)             # a partial list: the prev-is-listed search in any order
    st, _, _, val = full_step(inp, nb, [4, 1, 3], P.WEIGHTS, moments=mom)
    for k in NAMES:
        assert torch.equal(st[k], part[0][k]), k
    assert abs(float(val) - float(part[3])) <= 1e-12 * float(part[3])


# =================================================================================================================
# 6. NaN in one view's d_transforms
# =================================================================================================================
@pytest.mark.parametrize("B", R.BONES)
def test_nan_stays_in_the_frame_that_view_shows(B):
    inp, nb = case(B)
    listed = [0, 1, 2, 3, 4, 5]
    clean = full_step(inp, nb, listed, P.WEIGHTS)
    dT = _dev(inp["dT"])
    k = 5                                                    # position 5 shows frame 2, and is the only one that does
    assert inp["frames"][k] == 2 and inp["frames"].count(2) == 1
    dT[k] = float("nan")
    st, g_r, g_t, val = full_step(inp, nb, listed, P.WEIGHTS, dT=dT)
    assert bool(torch.isnan(g_r[2]).all()) and bool(torch.isnan(g_t[2]).all())
    for name in NAMES:
        assert bool(torch.isnan(st[name][2]).all()), name
        for f in (0, 1, 3, 4, 5):
            assert torch.equal(st[name][f], clean[0][name][f]), (name, f)
    for f in (0, 1, 3, 4, 5):
        assert torch.equal(g_r[f], clean[1][f]) and torch.equal(g_t[f], clean[2][f]), f
    assert bool(torch.isfinite(val)) and torch.equal(val, clean[3])


# =================================================================================================================
# 7. the value
# =================================================================================================================
@pytest.mark.parametrize("B", R.BONES)
def test_value_counts_once_is_reproducible_and_a_short_workspace_is_refused(B):
    from manus_amd._lib import MGR_ENOMEM, MGR_OK, lib
    inp, nb = case(B)
    for name, listed in LISTS.items():
        for mode, w in MODES.items():
            rc, _, _, val = backward_prior(inp, nb, listed, w)
            assert rc == MGR_OK
            want = P.total_listed_value(inp["rotvec"], inp["trans"], nb, listed, w, diff_dtype=F32)
            rel = abs(float(val) - want) / want
            print("FIGURE value B=%d %s, %s: %.12e, relative to the fp64 sum of the fp32 differences %.2e" % (B, name, mode, float(val), rel))
            assert rel <= 1e-10, (name, mode, float(val), want)
            again = backward_prior(inp, nb, listed, w)[3]
            assert torch.equal(again, val), (name, mode)
    # all rows: E of the whole tables (the differences in fp32: relative 2^-23 on each, so 1e-6 on E)
    E = float(P.total_energy(inp["rotvec"], inp["trans"], nb, P.WEIGHTS))
    assert abs(float(backward_prior(inp, nb, LISTS["all"], P.WEIGHTS)[3]) - E) <= 1e-6 * E
    # a short workspace: refused with nothing written
    need = int(lib().mgr_pose_prior_workspace_bytes(2, B))
    rc, g_r, g_t, val = backward_prior(inp, nb, [1, 2], P.WEIGHTS, ws_bytes=need - 1)
    assert rc == MGR_ENOMEM and b"mgr_pose_backward_prior" in lib().mgr_last_error()
    assert bool(torch.isnan(g_r).all()) and bool(torch.isnan(g_t).all()) and bool(torch.isnan(val))


# =================================================================================================================
# 8. pure-prior descent
# =================================================================================================================
def test_pure_prior_descent():
    """Zero d_transforms, random tables, all rows listed, the steps and rates of pose_prior_ref (test_pose_prior_cpu.py asserts
    that the fp64 loop brings E below DESCENT_FRACTION of its start): the device loop ends below that line times DESCENT_MARGIN."""
    from manus_amd._lib import MGR_OK
    B = P.DESCENT_B
    inp, nb = case(B)
    inp = dict(inp)
    inp["rotvec"], inp["trans"] = P.tables(B, 5, P.F)          # the tables of pose_prior_ref.descent
    listed = list(range(P.F))
    st = fresh_state(inp)
    dT = torch.zeros((inp["V"], B + 1, 4, 4), device=DEV)
    e0 = float(P.total_energy(inp["rotvec"], inp["trans"], nb, P.WEIGHTS))
    for s in range(1, P.DESCENT_STEPS + 1):
        rc, g_r, g_t, _ = backward_prior(inp, nb, listed, P.WEIGHTS, pad_rows=0, dT=dT, tables=(st["rotvec"], st["trans"]))
        assert rc == MGR_OK
        adam(B, listed, g_r, g_t, st, step=s, lr=P.DESCENT_LR)
    e1 = float(P.total_energy(st["rotvec"].cpu().double(), st["trans"].cpu().double(), nb, P.WEIGHTS))
    print("FIGURE pure-prior descent on the device: E %.6e -> %.6e (fraction %.4e; the line %.4e)" % (e0, e1, e1 / e0, P.DESCENT_FRACTION * P.DESCENT_MARGIN))
    assert e1 <= P.DESCENT_FRACTION * P.DESCENT_MARGIN * e0


# =================================================================================================================
# 9. recovery, end to end: the set-up of test_gpu_pose_chain.py::test_pose_recovery_with_the_refiner
# =================================================================================================================
RECOVERY_W_MAG = 0.05


def test_recovery_with_a_magnitude_prior():
    """Hand scene, n = 3000, 3 views, 96x64, targets = the fused forward at the true pose, three bones turned by 0.05 rad; 50 steps
    at lr 1e-3, the Gaussians frozen -- once without a prior and once with w_mag_rot = w_mag_trans = RECOVERY_W_MAG.  Direction
    only: the regularised run ends with the smaller |rotvec|, and its image loss still ends below its start.
    The weight: the image gradient's largest d_rotvec element at the first step is 3.5e-3 (the chain without a prior, printed
    below); at the true correction, 0.05 rad, the prior's gradient 2 w 0.05 = 5e-3 is of that size, so the prior holds the
    rotations well short of 0.05 without drowning the image term.  Measured: |rotvec| 0.078 without, 0.013 with; loss
    6.5e-4 -> 4.4e-4 without, -> 4.6e-4 with."""
    from test_gpu_pose_grad import _scene
    from manus_amd.engine import HipViewCompute
    from manus_amd.pose import PoseRefiner, _exp_so3
    views, ids, steps = 3, [0, 1, 2], 50
    sc, ct = _scene("hand", 3000, views)
    rest, nb = sc["rest"], sc["rest"].shape[0]
    posed_true = sc["posed"].clone()
    hc = HipViewCompute(sc, torch.zeros((views, 3, 64, 96), device=DEV), ct, fused=True, pose_grad=True, loss="l1+ssim")
    with torch.no_grad():
        hc.targets = hc.forward_views_fused(ids)[0].clone()
    bones = [3, 7, 12]
    delta = torch.eye(4, device=DEV).repeat(nb, 1, 1)
    delta[bones, :3, :3] = _exp_so3(0.05 * torch.eye(3, device=DEV))
    sc["posed"].copy_((posed_true @ delta).contiguous())
    res = {}
    for w in (0.0, RECOVERY_W_MAG):
        ref = PoseRefiner([("capture", v) for v in ids], nb, rest, 1e-3, 1e-3, device=DEV, w_mag_rot=w, w_mag_trans=w)
        losses, g0 = [], None
        for _ in range(steps):
            ref.apply(hc, ids, ids)
            out = hc(ids, 1.0 / views)
            losses.append(float(out["loss"]))
            ref.step(out["d_transforms"], ids, ids)
            g0 = float(ref.last_grad[1].abs().max()) if g0 is None else g0
        print("FIGURE recovery w_mag %.3g: largest |d_rotvec| element of the first step %.3e" % (w, g0))
        res[w] = (losses[0], losses[-1], float(ref.rotvec.norm()), float(ref.trans.norm()), None if ref.last_prior is None else float(ref.last_prior))
        print("FIGURE recovery w_mag %.3g: loss %.6f -> %.6f, |rotvec| %.5f, |trans| %.5f, prior %s" % ((w,) + res[w]))
    assert res[0.0][4] is None and res[RECOVERY_W_MAG][4] > 0.0
    assert res[RECOVERY_W_MAG][2] < res[0.0][2]
    assert res[RECOVERY_W_MAG][1] < res[RECOVERY_W_MAG][0]

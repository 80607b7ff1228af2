"""No GPU: the ABI of mgr_pose_backward_prior / mgr_pose_prior_workspace_bytes -- header, binding, built library --, its refusals,
which are all decided before anything touches a device, `pose.neighbour_table`, `PoseRefiner`'s new arguments, and the checker
of the GPU tests (tests/pose_prior_ref.py) against itself: gradient against central differences of E, the count-once rule of the
listed value, the fp64 reassociation bound of a permuted list, and the descent line of the pure-prior loop."""
import ctypes
import itertools
import os
import random
import re

import pytest
import torch

import pose_prior_ref as P
from pose_prior_ref import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)


def _declared(header, result, name):
    m = re.search(r"\b%s\s+%s\s*\(([^;]*?)\)\s*;" % (re.escape(result), re.escape(name)), header, re.S)
    assert m, "include/manus_hip.h does not declare %s %s" % (result, name)
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib
    header = _header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    args = _declared(header, "int", "mgr_pose_backward_prior")
    old = _declared(header, "int", "mgr_pose_backward")
    assert args[:14] == old[:14], "the first fourteen arguments are mgr_pose_backward's"
    assert args[14:] == ["const int32_t* neighbours", "double w_mag_rot", "double w_smooth_rot", "double w_mag_trans", "double w_smooth_trans",
                         "double* prior_value", "void* workspace", "size_t workspace_bytes", "void* stream"]
    assert _declared(header, "size_t", "mgr_pose_prior_workspace_bytes") == ["int U", "int B"]
    for name, res, arity in (("mgr_pose_backward_prior", ctypes.c_int, 23), ("mgr_pose_prior_workspace_bytes", ctypes.c_size_t, 2)):
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        got_res, bound = _lib.SIGNATURES[name]
        assert got_res is res and len(bound) == arity, (name, got_res, len(bound))
        assert hasattr(so, name), "%s is not exported by the built library" % name
    assert _lib.SIGNATURES["mgr_pose_backward_prior"][1][15:19] == [ctypes.c_double] * 4
    L = _lib.lib()
    assert L.mgr_pose_prior_workspace_bytes(6, 32) >= 6 * 32 * 8
    assert L.mgr_pose_prior_workspace_bytes(0, 32) == 0 and L.mgr_pose_prior_workspace_bytes(3, 0) == 0


# =================================================================================================================
# refusals: a fake pointer is never dereferenced, and nothing is launched (there is no device here)
# =================================================================================================================
PTR = ctypes.c_void_p(0x1000)
NAMES = ("frames_listed", "view_rows", "frame_of_view", "posed", "rest", "rotvec", "trans", "d_transforms", "d_rotvec", "d_trans")


def _call(L, V=3, B=20, F=4, U=2, w=(0.5, 0.25, 0.125, 1.0), neighbours=True, value=True, ws=True, ws_bytes=None, **null):
    assert set(null) <= set(NAMES)
    need = L.mgr_pose_prior_workspace_bytes(max(U, 0), max(B, 0))
    return L.mgr_pose_backward_prior(V, B, F, U, *[(None if null.get(k) else PTR) for k in NAMES], PTR if neighbours else None, *w,
                                     PTR if value else None, PTR if ws else None, need if ws_bytes is None else ws_bytes, None)


def _refused(L, rc, code, text=None):
    err = L.mgr_last_error()
    assert rc == code, (rc, err)
    assert b"mgr_pose_backward_prior" in err, err
    if text:
        assert text in err, err


def test_every_condition_of_pose_backward_is_refused():
    from manus_amd._lib import MGR_EINVAL, lib
    L = lib()
    for k in NAMES:
        _refused(L, _call(L, **{k: True}), MGR_EINVAL, b"null pointer")
        _refused(L, _call(L, w=(0, 0, 0, 0), neighbours=False, value=False, ws=False, **{k: True}), MGR_EINVAL, b"null pointer")
    for kw in (dict(V=0), dict(V=-2), dict(B=0), dict(B=33), dict(F=0), dict(F=-3), dict(U=0), dict(U=-1)):
        _refused(L, _call(L, **kw), MGR_EINVAL)
    _refused(L, _call(L, V=(1 << 24) // 21 + 1), MGR_EINVAL, b"2^24")


def test_weight_pointer_and_workspace_refusals():
    from manus_amd._lib import MGR_EINVAL, MGR_ENOMEM, lib
    L = lib()
    for k in range(4):
        for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            w = [0.5, 0.25, 0.125, 1.0]
            w[k] = bad
            _refused(L, _call(L, w=tuple(w)), MGR_EINVAL, b"weights")
            w = [0.0] * 4
            w[k] = bad
            _refused(L, _call(L, w=tuple(w)), MGR_EINVAL, b"weights")
    # a smoothness weight without the table
    _refused(L, _call(L, w=(0, 0.5, 0, 0), neighbours=False), MGR_EINVAL, b"neighbour")
    _refused(L, _call(L, w=(0, 0, 0, 0.5), neighbours=False), MGR_EINVAL, b"neighbour")
    # any weight without the value or the workspace
    for k in range(4):
        w = [0.0] * 4
        w[k] = 0.5
        _refused(L, _call(L, w=tuple(w), value=False), MGR_EINVAL, b"prior_value")
        _refused(L, _call(L, w=tuple(w), ws=False), MGR_EINVAL, b"workspace")
        _refused(L, _call(L, w=tuple(w), ws_bytes=2 * 20 * 8 - 1), MGR_ENOMEM, b"workspace too small")
        _refused(L, _call(L, w=tuple(w), ws_bytes=0), MGR_ENOMEM, b"workspace too small")


# =================================================================================================================
# the restatement against itself
# =================================================================================================================
SHAPES = {"F5": [("a", 0), ("a", 1), ("a", 2), ("b", 0), ("b", 1)], "F1": [("a", 7)], "F2": [("a", 0), ("a", 1)]}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gradient_equals_central_differences_of_e(shape):
    """dE/dx_f of the restatement against (E(x + h e) - E(x - h e)) / 2h in fp64, every element of every row.  E is quadratic, so
    the central difference is exact up to rounding: E ~ 1, h = 1e-4 -> eps64 * E / h ~ 2e-12 absolute."""
    nb = P.neighbours_of(SHAPES[shape])
    Fn, B, h = len(nb), 3, 1e-4
    rv, tr = P.tables(B, seed=1, n_frames=Fn)
    worst = 0.0
    for which, x, (wm, ws) in (("rotvec", rv, P.WEIGHTS[:2]), ("trans", tr * 30.0, P.WEIGHTS[2:])):
        for f in range(Fn):
            got = P.prior_grad(x, nb, f, wm, ws)
            for b, c in itertools.product(range(B), range(3)):
                hi, lo = x.clone(), x.clone()
                hi[f, b, c] += h
                lo[f, b, c] -= h
                want = float(P.energy(hi, nb, wm, ws) - P.energy(lo, nb, wm, ws)) / (2 * h)
                worst = max(worst, abs(float(got[b, c]) - want))
    print("FIGURE %s: prior gradient against central differences, worst absolute %.3e" % (shape, worst))
    assert worst <= 1e-10
    if shape == "F1":
        assert nb == [(-1, -1)]
        assert torch.equal(P.prior_grad(rv, nb, 0, 0.0, 5.0), torch.zeros_like(rv[0]))       # no edge: smoothness alone is flat


def _independent_partitions(nb):
    """Partitions of all rows into lists in which no two rows are neighbours: odd / even positions along every take."""
    colour = {}
    for f, (p, _) in enumerate(nb):
        if p < 0:
            k, g = f, 0
            while k >= 0:
                colour[k] = g % 2
                k, g = nb[k][1], g + 1
    return [[f for f in range(len(nb)) if colour[f] == c] for c in (0, 1)]


@pytest.mark.parametrize("shape", sorted(SHAPES) + ["F6"])
def test_listed_value_counts_every_term_once(shape):
    """The count-once rule inside ONE list: with all rows listed the value is E; over a partition of the rows into whole takes
    (lists that share no edge) the values add up to E; a single interior row carries its magnitude and both edges, two adjacent
    rows the edge between them once.
    A partition into lists in which no two rows are neighbours (odd / even rows of every take) does NOT add up to E under the
    rule: each edge has one end in either list, the list of its first row counts it as (f, next(f)) and the list of its second row
    as (prev(f), f) with prev(f) not listed there, as the rule tells each call to.  The sum over such a partition is the
    magnitude terms once and every edge twice, E + the edge terms, and that identity is what is asserted for it."""
    nb = P.neighbours_of(P.KEYS if shape == "F6" else SHAPES[shape])
    Fn, B = len(nb), 4
    rv, tr = P.tables(B, seed=2, n_frames=Fn)
    E = float(P.total_energy(rv, tr, nb, P.WEIGHTS))
    every = P.total_listed_value(rv, tr, nb, list(range(Fn)), P.WEIGHTS)
    assert abs(every - E) <= 1e-13 * E, (every, E)
    parts = [l for l in _independent_partitions(nb) if l]
    for l in parts:
        assert all(nb[f][0] not in l and nb[f][1] not in l for f in l)
    edges = float(P.total_energy(rv, tr, nb, (0.0, P.WEIGHTS[1], 0.0, P.WEIGHTS[3])))
    total = sum(P.total_listed_value(rv, tr, nb, l, P.WEIGHTS) for l in parts)
    mags = sum(P.total_listed_value(rv, tr, nb, l, P.ONLY_MAG) for l in parts)
    assert abs(mags - (E - edges)) <= 1e-13 * E
    # an edge is counted once by every list that holds an end of it
    ends = sum(1 for l in parts for f in l if nb[f][1] >= 0) + sum(1 for l in parts for f in l if nb[f][0] >= 0 and nb[f][0] not in l)
    n_edges = sum(1 for f in range(Fn) if nb[f][1] >= 0)
    assert ends == 2 * n_edges
    assert abs(total - (E + edges)) <= 1e-13 * max(E, 1e-300), (total, E, edges)
    # a partition into whole takes shares no edge: the sum is E
    takes = {}
    for f, k in enumerate(P.KEYS if shape == "F6" else SHAPES[shape]):
        takes.setdefault(k[0], []).append(f)
    whole = sum(P.total_listed_value(rv, tr, nb, l, P.WEIGHTS) for l in takes.values())
    assert abs(whole - E) <= 1e-13 * E, (whole, E)
    # a single interior row: its magnitude and both of its edges
    if shape == "F6":
        one = P.listed_value(rv, nb, [1], 0.7, 0.45)
        want = 0.7 * float((rv[1] ** 2).sum()) + 0.45 * float(((rv[1] - rv[0]) ** 2).sum() + ((rv[1] - rv[2]) ** 2).sum())
        assert abs(one - want) <= 1e-14 * want
        two = P.listed_value(rv, nb, [1, 2], 0.7, 0.45)       # adjacent rows: the edge between them once
        want2 = 0.7 * float((rv[1] ** 2).sum() + (rv[2] ** 2).sum()) + 0.45 * float(((rv[1] - rv[0]) ** 2).sum() + ((rv[1] - rv[2]) ** 2).sum()
                                                                                  + ((rv[2] - rv[3]) ** 2).sum())
        assert abs(two - want2) <= 1e-14 * want2


def test_value_of_a_permuted_list_is_within_fp64_reassociation():
    """The terms are the same whatever the order of the list; only the fp64 sums are reassociated: relative 1e-12 (the bound the GPU
    test asserts for the entry; about 200 positive terms of eps64 each)."""
    nb = P.neighbours_of(P.KEYS)
    rv, tr = P.tables(32, seed=3)
    base = P.total_listed_value(rv, tr, nb, [0, 1, 2, 3, 4, 5], P.WEIGHTS, diff_dtype=F32)
    rng = random.Random(4)
    for _ in range(10):
        l = list(range(6))
        rng.shuffle(l)
        assert abs(P.total_listed_value(rv, tr, nb, l, P.WEIGHTS, diff_dtype=F32) - base) <= 1e-12 * base
    part = P.total_listed_value(rv, tr, nb, [5, 0, 2], P.WEIGHTS, diff_dtype=F32)
    assert abs(P.total_listed_value(rv, tr, nb, [0, 2, 5], P.WEIGHTS, diff_dtype=F32) - part) <= 1e-12 * part


# =================================================================================================================
# neighbour_table
# =================================================================================================================
def _table(keys, max_gap=None):
    from manus_amd.pose import neighbour_table
    t = neighbour_table(keys, max_gap)
    assert t.dtype == torch.int32 and t.device.type == "cpu" and tuple(t.shape) == (len(dict.fromkeys((k[0], k[1]) for k in keys)), 2)
    return [tuple(r) for r in t.tolist()]


def test_neighbour_table_equals_the_brute_force_restatement():
    rng = random.Random(11)
    shuffled = [("grasp", i) for i in range(7)] + [("wave", i) for i in range(4)] + [("solo", 3)]
    rng.shuffle(shuffled)
    strided = [("a", i) for i in range(0, 40, 5)] + [("b", i) for i in (3, 4, 9, 10, 30)]
    rng.shuffle(strided)
    strings = [("a", "0010"), ("a", "2"), ("a", "007"), ("b", "x1"), ("b", "3"), ("b", "x0"), ("c", "5")]
    triples = [(a, f, "cam%02d" % c) for (a, f) in shuffled for c in range(2)]
    for keys, gaps in ((shuffled, (None, 1, 3)), (strided, (None, 1, 4, 5, 6, 20)), (strings, (None, 4, 5)), (triples, (None,)),
                       ([("only", 0)], (None, 1)), ([("a", 1), ("b", 1), ("c", 1)], (None,))):
        for gap in gaps:
            got, want = _table(keys, gap), P.neighbours_of(keys, gap)
            assert got == want, (keys, gap, got, want)
            for f, (p, n) in enumerate(got):              # symmetric, and inside the action
                assert n < 0 or got[n][0] == f
                assert p < 0 or got[p][1] == f
    # spelled out
    assert _table([("a", 2), ("a", 0), ("a", 1)]) == [(2, -1), (-1, 2), (1, 0)]
    assert _table([("a", 0), ("a", 5), ("a", 6)], max_gap=1) == [(-1, -1), (-1, 2), (1, -1)]
    assert _table([("a", "10"), ("a", "9")]) == [(1, -1), (-1, 0)]                          # by number, not by string
    assert _table([("b", "x1"), ("b", "3"), ("b", "x0")], max_gap=1) == [(-1, 1), (0, 2), (1, -1)]   # first-seen order, no gap to cut
    assert _table([("a", 1), ("b", 2)]) == [(-1, -1), (-1, -1)]
    assert _table(P.KEYS) == [(-1, 1), (0, 2), (1, 3), (2, -1), (-1, 5), (4, -1)]


def test_pose_refiner_arguments():
    from manus_amd.pose import PoseRefiner
    rest = torch.eye(4).repeat(5, 1, 1)
    keys = [("grasp_1", 8, "cam00"), ("grasp_1", 8, "cam01"), ("grasp_1", 11, "cam00"), ("wave", 8, "cam00")]
    plain = PoseRefiner(keys, 5, rest, 1e-3, 2e-3, device="cpu")
    assert plain.has_prior is False and plain.last_prior is None and plain.weights == (0.0, 0.0, 0.0, 0.0)
    assert sorted(plain.state_dict()) == sorted(["frame_keys", "steps", "rotvec", "trans", "m_r", "v_r", "m_t", "v_t"])
    assert plain.neighbours.tolist() == [[-1, 1], [0, -1], [-1, -1]]
    cut = PoseRefiner(keys, 5, rest, 1e-3, 2e-3, device="cpu", w_smooth_rot=0.5, max_gap=2)
    assert cut.has_prior and cut.neighbours.tolist() == [[-1, -1]] * 3 and cut.last_prior is None
    assert sorted(cut.state_dict()) == sorted(plain.state_dict())          # the weights are configuration, not state
    for name in ("w_mag_rot", "w_smooth_rot", "w_mag_trans", "w_smooth_trans"):
        for bad in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                PoseRefiner(keys, 5, rest, 1e-3, 2e-3, device="cpu", **{name: bad})
        assert PoseRefiner(keys, 5, rest, 1e-3, 2e-3, device="cpu", **{name: 0.25}).has_prior
    for bad in (-1, float("nan")):
        with pytest.raises(ValueError, match="max_gap"):
            PoseRefiner(keys, 5, rest, 1e-3, 2e-3, device="cpu", max_gap=bad)
    assert callable(plain.hold)


# =================================================================================================================
# the restatement's own fp32 error and the descent line
# =================================================================================================================
@pytest.mark.parametrize("B", (1, 20, 32))
def test_checker_fp32_error_is_small(B):
    """e32 of one regularised step on the committed inputs stays at fp32 rounding (no planted threshold row here: |rotvec| is
    0.03 .. 0.3), which keeps the GPU tests' bound 8 * max(e32, 2^-23) tight."""
    import pose_chain_ref as R
    nb = P.neighbours_of(P.KEYS)
    inp = P.chain_case(B, 9, nb)
    listed = list(range(P.F))
    a, b = P.regularised_step(inp, nb, listed, P.WEIGHTS, F64), P.regularised_step(inp, nb, listed, P.WEIGHTS, F32)
    for k in ("g_r", "g_t", "rotvec", "trans"):
        e32 = R.row_rel_err(b[k].reshape(-1, 3), a[k].reshape(-1, 3))
        print("e32 B %2d %-6s %.3e" % (B, k, e32))
        assert e32 <= 2e-6, (B, k, e32)


def test_pure_prior_descent_of_the_restatement_clears_its_line():
    """Zero d_transforms, all rows listed, DESCENT_STEPS steps at DESCENT_LR: the fp64 loop brings E below DESCENT_FRACTION of its
    start -- the line the GPU test holds the device loop to with the margin DESCENT_MARGIN -- and the fp32 run of the same loop
    stays inside that margin too."""
    nb = P.neighbours_of(P.KEYS)
    for B in (P.DESCENT_B,):
        e0, e1 = P.descent(B, nb, P.WEIGHTS, F64)
        f0, f1 = P.descent(B, nb, P.WEIGHTS, F32)
        print("FIGURE descent B %d: fp64 E %.6e -> %.6e (fraction %.4e), fp32 %.6e -> %.6e (fraction %.4e)" % (B, e0, e1, e1 / e0, f0, f1, f1 / f0))
        assert e0 > 0.0 and e1 / e0 <= P.DESCENT_FRACTION < 1.0 / P.DESCENT_MARGIN
        assert f1 <= P.DESCENT_FRACTION * P.DESCENT_MARGIN * f0


def test_refiner_state_goes_through_a_checkpoint(tmp_path):
    """`save_checkpoint(extra_state=)` / `load_checkpoint` under the safe unpickler carry the refiner's state (string frame ids as
    the dataset gives them) into a fresh refiner with the same weights."""
    from manus_amd import checkpoint
    from manus_amd.pose import PoseRefiner
    keys = [("grasp_1", "8", "cam00"), ("grasp_1", "11", "cam00"), ("grasp_1", "14", "cam01"), ("wave", "3", "cam00")]
    rest = torch.eye(4).repeat(5, 1, 1)
    kw = dict(device="cpu", w_mag_rot=0.5, w_smooth_trans=0.25)
    a = PoseRefiner(keys, 5, rest, 1e-3, 2e-3, **kw)
    assert a.neighbours.tolist() == [[-1, 1], [0, 2], [1, -1], [-1, -1]]
    g = torch.Generator().manual_seed(1)
    a.rotvec.copy_(torch.randn(a.rotvec.shape, generator=g))
    a.trans.copy_(torch.randn(a.trans.shape, generator=g))
    a.m_r, a.v_r, a.m_t, a.v_t = (torch.randn(a.rotvec.shape, generator=g) for _ in range(4))
    a.steps = 9
    params = {k[len("model."):]: torch.zeros((4, 3)) for k in checkpoint.LEAF_KEYS}
    path = checkpoint.save_checkpoint(str(tmp_path), params, 0, 9, 0.0, extra_state={"pose_refiner": a.state_dict()})
    state = checkpoint.load_checkpoint(path, return_checkpoint=True)[2]["pose_refiner"]
    b = PoseRefiner(keys, 5, rest, 1e-3, 2e-3, **kw)
    b.load_state_dict(state)
    assert b.steps == 9 and b.weights == a.weights and torch.equal(b.neighbours, a.neighbours)
    for k in ("rotvec", "trans", "m_r", "v_r", "m_t", "v_t"):
        assert torch.equal(getattr(b, k), getattr(a, k)), k

"""GPU: mgr_knn_self and mgr_outlier_scores (csrc/knn_k.hip, manus_amd.outliers) against tests/outlier_ref.py.

The search is exact: indices, squared distances and counts must be `torch.equal` to the numpy restatement (same fp32
arithmetic, same key order) on the smallest shapes at which a wave-per-query select can go wrong.  Everything after d2 is
judged by the project's row rule, e_kernel <= 8 * max(e32, 2^-23) in `util.row_rel_err` against the fp64 run, with e32 the
restatement's own fp32 run; the masks must equal the fp64 run's exactly at each fixture's `prob`, whose distance from every
score test_outliers_cpu.py asserts to be at least 1000 x the fp32 / fp64 distance of the scores."""
import ctypes

import numpy as np
import pytest
import torch

import outlier_ref as R
from util import row_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
FACTOR = 8.0


def bound_of(e32):
    return FACTOR * max(e32, EPS32)


def check_rows(tag, got, ref64, ref32, rows=None):
    """e_kernel <= 8 * max(e32, 2^-23), both in `row_rel_err` against the fp64 run, over the rows `rows` (boolean mask or
    None = all).  Prints the figures before it asserts."""
    got, ref64, ref32 = (x.detach().cpu().double() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, np.float64)) for x in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    if rows is not None:
        rows = torch.as_tensor(rows).reshape(-1)
        got, ref64, ref32 = got[rows], ref64[rows], ref32[rows]
    e32, ek = row_rel_err(ref32, ref64), row_rel_err(got, ref64)
    ratio = ek / max(e32, EPS32)
    print("RATIO %-44s e_kernel %.3e  e32 %.3e  ratio %.2f" % (tag, ek, e32, ratio))
    assert ek <= bound_of(e32), "%s: e_kernel %.3e  e32 %.3e  ratio %.2f > %g" % (tag, ek, e32, ratio, FACTOR)
    return ek, e32


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def sigma_of(d2, n, dt):
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(np.isfinite(d2), d2.astype(np.float64), 0.0).sum(1)
        return np.sqrt((S / n).astype(dt)).astype(dt)


def check_search(tag, x, k, include_self):
    from manus_amd.outliers import knn_self
    idx, d2, n = R.knn_self_ref(x, k, include_self)
    got = knn_self(dev(x), k, include_self=include_self, want_d2=True, want_idx=True)
    torch.cuda.synchronize()
    assert got.idx.shape == (x.shape[0], k) and got.idx.dtype == torch.int32 and got.count.dtype == torch.int32
    assert torch.equal(got.count.cpu(), torch.as_tensor(n)), (tag, "count")
    bad = (got.idx.cpu() != torch.as_tensor(idx)).any(1).nonzero().reshape(-1)
    assert bad.numel() == 0, (tag, "idx rows differ", bad[:5].tolist(), got.idx[bad[:1]].cpu(), idx[bad[:1].numpy()])
    assert torch.equal(got.d2.cpu(), torch.as_tensor(d2)), (tag, "d2")
    ok = n > 0
    s = got.sigma.cpu().numpy()
    assert np.isnan(s[~ok]).all(), (tag, "sigma of rows without neighbours")
    if ok.any():
        check_rows(tag + " sigma", s, sigma_of(d2, n, np.float64), sigma_of(d2, n, np.float32), rows=ok)
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_self", [True, False])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128, 511, 512])
def test_knn_k_values(k, include_self):
    check_search("N700 k%d self%d" % (k, include_self), R.random_points(700, seed=11), k, include_self)


@pytest.mark.parametrize("include_self", [True, False])
@pytest.mark.parametrize("N", [63, 64, 65, 1])
def test_knn_n_around_k(N, include_self):
    check_search("N%d k64 self%d" % (N, include_self), R.random_points(N, seed=12), 64, include_self)


def test_knn_empty():
    from manus_amd.outliers import knn_self, outlier_scores
    got = knn_self(torch.zeros((0, 3), device=DEV), 64, want_d2=True, want_idx=True)
    assert got.idx.shape == (0, 64) and got.d2.shape == (0, 64) and got.sigma.shape == (0,) and got.count.shape == (0,)
    s = outlier_scores(torch.zeros((0, 3), device=DEV), 64, prob=0.5)
    torch.cuda.synchronize()
    assert s.score.shape == (0,) and s.mask.shape == (0,) and s.stats.cpu().tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("include_self", [True, False])
@pytest.mark.parametrize("k", [27, 33])
def test_knn_lattice_ties(k, include_self):
    """9 x 9 x 9 integer lattice: exact ties at the k-th key everywhere; the lower index wins."""
    check_search("lattice k%d self%d" % (k, include_self), R.lattice(9), k, include_self)


@pytest.mark.parametrize("include_self", [True, False])
def test_knn_coincident_beyond_the_buffer(include_self):
    """3000 coincident points (one cell, far beyond the 384-entry buffer of k = 128) plus 50 others."""
    x = np.concatenate([np.full((3000, 3), 0.25, np.float32), R.random_points(50, seed=5)])
    x = x[np.random.default_rng(2).permutation(len(x))]
    check_search("coincident self%d" % include_self, x, 128, include_self)


def test_knn_plane_and_far_point():
    x = R.random_points(600, seed=13)
    x[:, 2] = 0.5                                         # one grid dimension of a single cell
    check_search("plane", x, 40, True)
    y = np.concatenate([R.random_points(500, seed=14) * np.float32(0.05), np.array([[1e4, 0, 0]], np.float32)])
    check_search("far point", y, 20, True)                # the bbox coarsens the grid
    check_search("far point, no self", y, 20, False)


@pytest.mark.parametrize("include_self", [True, False])
def test_knn_non_finite_rows(include_self):
    x = R.random_points(400, seed=15)
    x[7, 0] = np.nan
    x[100] = np.nan
    x[201, 2] = np.inf
    x[399, 1] = -np.inf
    got = check_search("non-finite self%d" % include_self, x, 33, include_self)
    bad = [7, 100, 201, 399]
    assert (got.count[bad] == 0).all() and (got.idx[bad] == -1).all() and torch.isinf(got.d2[bad]).all()
    assert not torch.isin(got.idx, torch.tensor(bad, device=DEV, dtype=torch.int32)).any()


def test_knn_two_runs_equal_bits():
    from manus_amd.outliers import knn_self
    x = dev(np.concatenate([R.random_points(2000, seed=16), np.full((500, 3), 0.1, np.float32)]))
    a = knn_self(x, 100, want_d2=True, want_idx=True)
    b = knn_self(x, 100, want_d2=True, want_idx=True)
    assert torch.equal(a.idx, b.idx) and torch.equal(a.d2, b.d2) and torch.equal(a.count, b.count)
    assert torch.equal(a.sigma.view(torch.int32), b.sigma.view(torch.int32))


def test_knn_short_workspace_is_refused_and_outputs_untouched():
    from manus_amd._lib import MGR_EINVAL, MGR_ENOMEM, lib, ptr, stream
    L = lib()
    N, k = 300, 16
    x = dev(R.random_points(N, seed=17))
    d2 = torch.full((N, k), float("nan"), device=DEV)
    sg = torch.full((N,), float("nan"), device=DEV)
    idx = torch.full((N, k), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    need = int(L.mgr_knn_self_workspace_bytes(N, k))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert L.mgr_knn_self(N, ptr(x), k, 1, ptr(d2), ptr(idx), ptr(sg), ptr(cnt), ptr(ws), need - 1, stream()) == MGR_ENOMEM
    assert L.mgr_knn_self(N, ptr(x), 513, 1, ptr(d2), ptr(idx), ptr(sg), ptr(cnt), ptr(ws), need, stream()) == MGR_EINVAL
    sc = torch.full((N,), float("nan"), device=DEV)
    need2 = int(L.mgr_outlier_scores_workspace_bytes(N, k))
    ws2 = torch.empty(need2, dtype=torch.uint8, device=DEV)
    assert L.mgr_outlier_scores(N, ptr(x), k, 1, 0.5, ptr(sc), None, ptr(sg), None, None, ptr(ws2), need2 - 1, stream()) == MGR_ENOMEM
    torch.cuda.synchronize()
    assert torch.isnan(d2).all() and torch.isnan(sg).all() and torch.isnan(sc).all() and (idx == -7).all() and (cnt == -7).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the scores
# ---------------------------------------------------------------------------------------------------------------------------
def run_scores(x, k, prob, include_self=True):
    from manus_amd.outliers import outlier_scores
    out = outlier_scores(dev(x), k=k, include_self=include_self, prob=prob)
    torch.cuda.synchronize()
    return out


def check_scores(tag, x, k):
    r64 = R.cached((tag, k, 64), lambda: R.loop_ref(x, k))
    r32 = R.cached((tag, k, 32), lambda: R.loop_ref(x, k, dt=np.float32))
    prob, half = R.fixture_prob(r64["score"])
    dist = float(np.abs(r32["score"].astype(np.float64) - r64["score"]).max())
    print("%s: prob %.6f  half gap %.3e  max|score32 - score64| %.3e" % (tag, prob, half, dist))
    assert half >= 1000.0 * dist                          # a condition on the fixture, not a tolerance
    out = run_scores(x, k, prob)
    for name, got in (("sigma", out.sigma), ("plof", out.plof), ("score", out.score)):
        check_rows("%s %s" % (tag, name), got, r64[name], r32[name])
    e32 = abs(float(r32["nplof"]) - float(r64["nplof"]))
    ek = abs(float(out.nplof) - float(r64["nplof"]))
    print("RATIO %-44s e_kernel %.3e  e32 %.3e" % (tag + " nplof", ek, e32))
    assert ek <= FACTOR * max(e32, EPS32 * float(r64["nplof"]))
    want = torch.as_tensor(r64["score"] > prob)
    assert out.mask.dtype == torch.bool and torch.equal(out.mask.cpu(), want), (tag, (out.mask.cpu() != want).nonzero().reshape(-1))
    stats = out.stats.cpu().tolist()
    assert stats[0] == float(out.nplof) and stats[1] == len(x) and stats[2] == float(out.mask.sum())
    assert torch.equal(out.mask, out.score > np.float32(prob))
    return out, want


@pytest.mark.parametrize("seed,n,nout,k", R.PLANTED)
def test_scores_planted_floaters(seed, n, nout, k):
    out, want = check_scores("planted %d/%d seed %d" % (n, nout, seed), R.planted(seed, n, nout), k)
    assert out.mask[n:].all()                              # every planted floater is flagged


@pytest.mark.parametrize("k", [27, 33])
def test_scores_lattice(k):
    check_scores("lattice", R.lattice(9), k)


def test_scores_all_coincident():
    out = run_scores(np.full((500, 3), 0.5, np.float32), 64, 0.5)
    assert (out.score == 0).all() and not out.mask.any() and (out.plof == 0).all() and (out.sigma == 0).all()
    assert out.stats.cpu().tolist() == [0.0, 500.0, 0.0]


def test_scores_nan_row_is_inert():
    """A NaN row keeps a NaN score and mask 0, and every other row's bits are those of a run without that row."""
    x = R.planted(0, 700, 9)
    k = 33
    base = run_scores(x, k, 0.8)
    y = np.concatenate([x[:350], np.full((1, 3), np.nan, np.float32), x[350:]])
    out = run_scores(y, k, 0.8)
    keep = np.arange(len(y)) != 350
    assert torch.isnan(out.score[350]) and torch.isnan(out.sigma[350]) and torch.isnan(out.plof[350]) and not out.mask[350]
    for name in ("score", "sigma", "plof"):
        assert torch.equal(getattr(out, name)[keep].view(torch.int32), getattr(base, name).view(torch.int32)), name
    assert torch.equal(out.mask[keep], base.mask)
    so, sb = out.stats.cpu().tolist(), base.stats.cpu().tolist()
    assert so[1:] == sb[1:] and abs(so[0] - sb[0]) <= 1e-14 * sb[0]      # (the fp64 fold's blocks moved by one row)


def test_scores_permutation_and_repeat():
    """Tie-free rows: a permutation of the rows gives the permuted outputs bit for bit; two runs give equal bits."""
    x = R.tie_free_points()
    k = 33
    perm = np.random.default_rng(4).permutation(len(x))
    a, b, c = run_scores(x, k, 0.7), run_scores(x[perm], k, 0.7), run_scores(x, k, 0.7)
    p = torch.as_tensor(perm, device=DEV)
    for name in ("score", "sigma", "plof"):
        assert torch.equal(getattr(a, name)[p].view(torch.int32), getattr(b, name).view(torch.int32)), name
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(c, name).view(torch.int32)), name
    assert torch.equal(a.mask[p], b.mask) and torch.equal(a.mask, c.mask)
    sa, sb, sc = (t.stats.cpu().tolist() for t in (a, b, c))
    assert sa == sc and sa[1:] == sb[1:] and abs(sa[0] - sb[0]) <= 1e-14 * sa[0]      # (the fp64 fold runs in row order)


def test_reference_named_entry():
    from manus_amd.outliers import outlier_mask, update_mask_based_on_outliers
    x = dev(R.planted(0, 1500, 12))
    got = update_mask_based_on_outliers(x)
    assert got.dtype == torch.bool and got.is_cuda and torch.equal(got, outlier_mask(x, prob=0.5, neighbors=128))

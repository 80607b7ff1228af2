"""numpy restatement of mgr_knn_self and mgr_outlier_scores (include/manus_hip.h), and the fixtures their tests share.

The search is fp32 with exactly the stated arithmetic -- d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded to fp32 -- and
the stated key order (d2, index), on a full distance matrix (sizes here are at most a few thousand).  Everything after d2
runs in fp64 (`dt=np.float64`: the reference) or in fp32 (`dt=np.float32`: the measure e32 of what fp32 arithmetic costs).
"""
import numpy as np
from scipy.special import erf

F32 = np.float32


def knn_self_ref(xyz, k, include_self=True):
    """(idx (N,k) int32, d2 (N,k) float32, count (N,) int32): rows in ascending key order, -1 / +inf beyond count."""
    x = np.asarray(xyz, F32).reshape(-1, 3)
    N = x.shape[0]
    idx = np.full((N, k), -1, np.int32)
    d2o = np.full((N, k), np.inf, F32)
    count = np.zeros((N,), np.int32)
    if N == 0:
        return idx, d2o, count
    fin = np.isfinite(x).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = (x[None, :, 0] - x[:, None, 0]).astype(F32)
        dy = (x[None, :, 1] - x[:, None, 1]).astype(F32)
        dz = (x[None, :, 2] - x[:, None, 2]).astype(F32)
        d2 = (((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32) + (dz * dz).astype(F32)).astype(F32)
    cand = np.broadcast_to(fin[None, :], (N, N)).copy()
    cand[~fin, :] = False
    if not include_self:
        cand[np.arange(N), np.arange(N)] = False
    key = np.where(cand, d2, np.inf).astype(F32)
    # stable argsort on d2 keeps the lower index first among equal distances; non-candidates (inf) go last but a candidate at
    # d2 = +inf would tie with them, so candidates are ranked first explicitly
    order = np.lexsort((np.broadcast_to(np.arange(N), (N, N)), key, ~cand), axis=1)
    n = np.minimum(k, cand.sum(1)).astype(np.int32)
    kk = min(k, N)
    top = order[:, :kk]
    dd = np.take_along_axis(d2, top, 1)
    valid = np.arange(kk)[None, :] < n[:, None]
    idx[:, :kk] = np.where(valid, top, -1)
    d2o[:, :kk] = np.where(valid, dd, np.inf)
    return idx, d2o, n


def loop_ref(xyz, k, include_self=True, dt=np.float64):
    """dict(idx, d2, count, sigma, plof, nplof, score) by the definition above mgr_outlier_scores; sums in fp64 and the
    rest in `dt`.  Points with count 0 carry NaN sigma / plof / score and are left out of nplof."""
    idx, d2, n = knn_self_ref(xyz, k, include_self)
    N = idx.shape[0]
    valid = idx >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(valid, d2.astype(np.float64), 0.0).sum(1)
        sigma = np.sqrt((S / n).astype(dt)).astype(dt)          # NaN where n == 0
        sj = np.where(valid, sigma[np.where(valid, idx, 0)].astype(np.float64), 0.0).sum(1)
        den = (sj / n).astype(dt)
        plof = np.where(den == 0, dt(0), sigma / np.where(den == 0, dt(1), den) - dt(1)).astype(dt)
        plof = np.where(n > 0, plof, dt(np.nan)).astype(dt)
        ok = n > 0
        nplof = np.sqrt((plof[ok].astype(np.float64) ** 2).mean()) if ok.any() else 0.0
        nplof = dt(nplof)
        if nplof == 0:
            score = np.where(ok, dt(0), dt(np.nan)).astype(dt)
        else:
            arg = (plof / (nplof * dt(np.sqrt(dt(2))))).astype(dt)
            score = np.maximum(dt(0), erf(arg).astype(dt)).astype(dt)
            score = np.where(ok, score, dt(np.nan)).astype(dt)
    return dict(idx=idx, d2=d2, count=n, sigma=sigma, plof=plof, nplof=nplof, score=score)


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------------
# planted floaters: (seed, blob points, floaters, k) -- a Gaussian blob with anisotropic sigmas of 4 / 3 / 1 cm and uniform
# floaters above it.  Seeds chosen so that every planted floater is flagged at the fixture's own `prob` (fixture_prob) and the
# gap around it is at least 1000 x the fp32 / fp64 distance of the scores (tests/test_outliers_cpu.py asserts both).
PLANTED = ((1, 300, 6, 8), (0, 700, 9, 33), (0, 1500, 12, 64), (0, 1500, 12, 128))


def planted(seed, n, nout):
    rng = np.random.default_rng(seed)
    body = rng.normal(size=(n, 3)) * np.array([0.04, 0.03, 0.01])
    out = rng.uniform(-0.3, 0.3, size=(nout, 3))
    out[:, 2] += 0.25
    return np.concatenate([body, out]).astype(F32)


def fixture_prob(score64, lo=0.5, hi=0.95):
    """(prob, half gap): the midpoint of the widest gap between neighbouring fp64 scores inside [lo, hi] (the interval's
    ends count as neighbours, so an empty interval gives its middle)."""
    s = np.asarray(score64, np.float64)
    s = np.sort(s[np.isfinite(s) & (s > lo) & (s < hi)])
    edges = np.concatenate([[lo], s, [hi]])
    gaps = np.diff(edges)
    j = int(np.argmax(gaps))
    return float(0.5 * (edges[j] + edges[j + 1])), float(0.5 * gaps[j])


def lattice(n=9):
    g = np.arange(n, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)


def random_points(n, seed=0):
    return np.random.default_rng(seed).normal(size=(n, 3)).astype(F32)


TIE_FREE_SEED = 7      # smallest relative gap 1.4e-5 (seeds 0 .. 11 give 4.9e-7 .. 1.5e-5)


def tie_free_points(n=300):
    """Random points whose 35 smallest distances per row differ by more than 2e-6 relative (tests/test_outliers_cpu.py asserts
    it): the neighbour sets up to k = 33 do not depend on fp32 rounding or on the index order."""
    return random_points(n, seed=TIE_FREE_SEED)


_CACHE = {}


def cached(name, fn):
    """A reference computed once and shared among the tests that need it (callers must not modify it)."""
    if name not in _CACHE:
        _CACHE[name] = fn()
    return _CACHE[name]

"""No GPU: outlier pruning (mgr_knn_self / mgr_outlier_scores / mgr_prune_tests, manus_amd.outliers) -- the ABI in header,
binding and built library; the refusals decided before anything touches a device; the restatement's neighbour sets
(tests/outlier_ref.py) against scipy's kd-tree; the planted-floater fixtures' own conditions, which make the GPU tests' exact
mask comparison meaningful; and the documents that used to say "not built"."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.spatial import cKDTree

import outlier_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_knn_self": (11, ctypes.c_int), "mgr_outlier_scores": (13, ctypes.c_int), "mgr_prune_tests": (8, ctypes.c_int),
               "mgr_knn_self_workspace_bytes": (2, ctypes.c_size_t), "mgr_outlier_scores_workspace_bytes": (2, ctypes.c_size_t)}
P = ctypes.c_void_p(0x1000)          # a fake pointer: a refusal never dereferences it
TIE_FREE = 2e-6                      # relative distance gap that fp32 rounding of d2 (about 2e-7) cannot close


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib, build
    raw = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, (arity, res) in NEW_ENTRIES.items():
        args = _declared_args(header, name)
        assert len(args) == arity, (name, args)
        got_res, bound = _lib.SIGNATURES[name]
        assert len(bound) == arity and got_res is res, (name, len(bound))
        assert hasattr(so, name), "%s is not exported by the built library" % name
    assert "knn_k.hip" in build.SOURCES
    assert _declared_args(header, "mgr_knn_self")[:4] == ["int N", "const float* xyz", "int k", "int include_self"]
    assert _declared_args(header, "mgr_outlier_scores")[:5] == ["int N", "const float* xyz", "int k", "int include_self", "float prob"]
    assert re.search(r"#define\s+MGR_KNN_MAX_K\s+512\b", header) and _lib.MGR_KNN_MAX_K == 512
    assert re.search(r"#define\s+MGR_VERSION\s+100\b", header)
    # the definition stands in full above the entry
    for word in ("Local Outlier Probability", "plof_i", "nplof", "erff", "lambda", "lower\n * index wins a tie"):
        assert word in raw, word


def _err(L):
    return L.mgr_last_error()


def test_knn_self_refusals_before_the_device():
    from manus_amd._lib import MGR_EINVAL, MGR_ENOMEM, MGR_OK, lib
    L = lib()
    need = L.mgr_knn_self_workspace_bytes(1000, 64)
    assert need >= 1000 * 16

    def call(N=1000, xyz=P, k=64, ws=P, nbytes=None):
        return L.mgr_knn_self(N, xyz, k, 1, P, P, P, P, ws, need if nbytes is None else nbytes, None)
    for kw in (dict(k=0), dict(k=-1), dict(k=513), dict(N=-1), dict(xyz=None)):
        assert call(**kw) == MGR_EINVAL and b"mgr_knn_self" in _err(L), kw
    for kw in (dict(nbytes=need - 1), dict(nbytes=0), dict(ws=None)):
        assert call(**kw) == MGR_ENOMEM and b"workspace" in _err(L), kw
    assert call(N=0, xyz=None, ws=None, nbytes=0) == MGR_OK          # N = 0 is valid and launches nothing
    assert call(N=0, k=513) == MGR_EINVAL                            # ... but k is still checked
    assert L.mgr_knn_self_workspace_bytes(0, 1) > 0


def test_outlier_scores_refusals_before_the_device():
    from manus_amd._lib import MGR_EINVAL, MGR_ENOMEM, lib
    L = lib()
    need = L.mgr_outlier_scores_workspace_bytes(1000, 64)
    assert need >= L.mgr_knn_self_workspace_bytes(1000, 64) + 1000 * 64 * 4 + 1000 * 12

    def call(N=1000, xyz=P, k=64, score=P, ws=P, nbytes=None):
        return L.mgr_outlier_scores(N, xyz, k, 1, 0.8, score, P, P, P, P, ws, need if nbytes is None else nbytes, None)
    for kw in (dict(k=0), dict(k=513), dict(N=-1), dict(xyz=None), dict(score=None)):
        assert call(**kw) == MGR_EINVAL and b"mgr_outlier_scores" in _err(L), kw
    for kw in (dict(nbytes=need - 1), dict(ws=None)):
        assert call(**kw) == MGR_ENOMEM and b"workspace" in _err(L), kw
    assert L.mgr_prune_tests(-1, P, P, 0.005, 1.0, 0.0, P, None) == MGR_EINVAL
    assert L.mgr_prune_tests(5, None, P, 0.005, 1.0, 0.0, P, None) == MGR_EINVAL


def test_python_surface_refuses_cpu_tensors_and_bad_k():
    import torch
    from manus_amd import outliers
    from manus_amd._lib import ManusHipError
    x = torch.zeros((10, 3))
    for fn in (lambda: outliers.knn_self(x, 4), lambda: outliers.outlier_scores(x, 4), lambda: outliers.outlier_mask(x),
               lambda: outliers.update_mask_based_on_outliers(x)):
        with pytest.raises(ManusHipError):
            fn()
    import inspect
    sig = inspect.signature(outliers.update_mask_based_on_outliers)
    assert sig.parameters["prob"].default == 0.5 and sig.parameters["neighbors"].default == 128
    sig = inspect.signature(outliers.outlier_mask)
    assert sig.parameters["prob"].default == 0.8 and sig.parameters["neighbors"].default == 512


@pytest.mark.parametrize("k", [1, 8, 33])
@pytest.mark.parametrize("include_self", [True, False])
def test_restatement_neighbours_match_a_kd_tree(k, include_self):
    """Tie-free fixture: random fp32 points, whose pairwise distances differ far beyond the fp32 rounding of d2 at the k-th rank
    (asserted), so the fp32 search and an fp64 kd-tree must pick the same ordered sets."""
    x = R.tie_free_points()
    idx, d2, n = R.knn_self_ref(x, k, include_self)
    x64 = x.astype(np.float64)
    dd, ii = cKDTree(x64).query(x64, k=k + 1)
    ii = ii[:, :k] if include_self else ii[:, 1:]
    dd = dd[:, :k] if include_self else dd[:, 1:]
    full = np.sort(((x64[:, None] - x64[None]) ** 2).sum(-1), 1)[:, :k + 2]      # column 0 is the point itself
    assert (np.diff(full, axis=1) > TIE_FREE * full[:, 1:]).all(), "the fixture has near ties"
    assert (n == k).all()
    assert np.array_equal(idx, ii.reshape(idx.shape).astype(np.int32))
    assert np.allclose(d2, dd.reshape(d2.shape) ** 2, rtol=1e-5, atol=0)


def test_restatement_edge_rows():
    x = R.random_points(10, seed=1)
    x[3, 1] = np.nan
    x[7, 0] = np.inf
    idx, d2, n = R.knn_self_ref(x, 4, include_self=True)
    assert n[3] == 0 and n[7] == 0 and (idx[3] == -1).all() and np.isinf(d2[7]).all()
    assert not np.isin(idx, [3, 7]).any()
    idx, d2, n = R.knn_self_ref(x, 12, include_self=False)
    ok = np.isfinite(x).all(1)
    assert (n[ok] == 7).all() and (idx[ok][:, 7:] == -1).all() and (idx[ok][:, :7] >= 0).all()
    # ties go to the lower index
    lat = R.lattice(3)
    idx, d2, n = R.knn_self_ref(lat, 4, include_self=True)
    centre = 13
    assert idx[centre, 0] == centre and list(idx[centre, 1:]) == [4, 10, 12] and (d2[centre, 1:] == 1).all()
    r = R.loop_ref(np.zeros((20, 3), np.float32), 5)
    assert (r["score"] == 0).all() and r["nplof"] == 0


@pytest.mark.parametrize("seed,n,nout,k", R.PLANTED)
def test_planted_fixture_conditions(seed, n, nout, k):
    """The conditions on the INPUTS that let the GPU test demand the fp64 mask exactly: at the fixture's `prob` (the midpoint
    of the widest gap between neighbouring fp64 scores inside [0.5, 0.95]) half the gap is at least 1000 x the largest
    |score32 - score64| of the restatement's own two runs, and every planted floater is flagged."""
    x = R.planted(seed, n, nout)
    r64 = R.cached(("loop", seed, n, nout, k, 64), lambda: R.loop_ref(x, k))
    r32 = R.cached(("loop", seed, n, nout, k, 32), lambda: R.loop_ref(x, k, dt=np.float32))
    assert np.array_equal(r64["idx"], r32["idx"])
    prob, half = R.fixture_prob(r64["score"])
    dev = float(np.abs(r32["score"].astype(np.float64) - r64["score"]).max())
    print("fixture %d/%d k=%d seed %d: prob %.6f half gap %.3e max|s32-s64| %.3e" % (n, nout, k, seed, prob, half, dev))
    assert 0.5 <= prob <= 0.95
    assert half >= 1000.0 * dev, (half, dev)
    mask = r64["score"] > prob
    assert mask[n:].all(), "planted floaters missed: %s" % np.nonzero(~mask[n:])[0]
    assert mask[:n].sum() < n // 4                        # and the blob is not flagged wholesale
    assert np.array_equal(r32["score"] > np.float32(prob), mask)


def test_documents_no_longer_say_not_built():
    from manus_amd.optim import OUTLIER_NEIGHBORS, OUTLIER_PROB, GaussianOptimizer
    doc = GaussianOptimizer.densify_and_prune.__doc__
    assert "not built" not in doc and "LocalOutlierFactor" not in doc and "Local Outlier Probability" in doc
    assert (OUTLIER_PROB, OUTLIER_NEIGHBORS) == (0.8, 512)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [l for l in integ.splitlines() if "remove_outliers" in l]
    assert rows and not any("not built" in l or "not supported" in l or "unsupported" in l.lower() for l in rows), rows

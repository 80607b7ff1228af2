"""Outlier pruning on the device: exact k-nearest search and Local Outlier Probability scores (`csrc/knn_k.hip`).

The reference's `update_mask_based_on_outliers` (src/utils/gaussian_utils.py:557-568) dumps the Gaussian centres to a .ply,
loads them into pymeshlab and calls `compute_selection_point_cloud_outliers(propthreshold, knearest)`: MeshLab's "select
outliers", the Local Outlier Probability of Kriegel, Kroeger, Schubert and Zimek (2009).  Here the same quantity is computed
on the GPU with the definition written out in include/manus_hip.h (`mgr_outlier_scores`); MeshLab's own constants (its erf
approximation, whether it counts the query point) cannot be pinned without MeshLab, so each is an argument or a named
constant.  GPU tensors only; there is no CPU or PyTorch fallback.
"""
import collections

import torch

from ._lib import MGR_KNN_MAX_K, ManusHipError, check, f32c, lib, ptr, stream

KnnSelf = collections.namedtuple("KnnSelf", "sigma count d2 idx")
OutlierScores = collections.namedtuple("OutlierScores", "score sigma plof nplof stats mask")


def _points(xyz, k):
    if not torch.is_tensor(xyz) or not xyz.is_cuda:
        raise ManusHipError("manus_amd.outliers needs a GPU tensor; there is no CPU fallback")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ManusHipError("outliers: xyz must be (N, 3)")
    k = int(k)
    if not 1 <= k <= MGR_KNN_MAX_K:
        raise ManusHipError("outliers: k must lie in 1 .. %d" % MGR_KNN_MAX_K)
    return f32c(xyz.detach()), k


def knn_self(xyz, k, include_self=True, want_d2=False, want_idx=False):
    """The exact k nearest of every row of xyz (N,3) among the rows themselves (`mgr_knn_self`): keys (d2, index), the lower
    index wins a tie; include_self keeps the row itself (d2 = 0), else it is excluded by index.  Returns
    KnnSelf(sigma (N,), count (N,) int32, d2 (N,k) or None, idx (N,k) int32 or None): rows in ascending key order, -1 / +inf
    beyond count; sigma = sqrt(mean d2 of the row), NaN where count is 0 (a row with a non-finite coordinate)."""
    xyz, k = _points(xyz, k)
    N, dev = xyz.shape[0], xyz.device
    sigma = torch.empty((N,), dtype=torch.float32, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    d2 = torch.empty((N, k), dtype=torch.float32, device=dev) if want_d2 else None
    idx = torch.empty((N, k), dtype=torch.int32, device=dev) if want_idx else None
    nbytes = int(lib().mgr_knn_self_workspace_bytes(N, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().mgr_knn_self(N, ptr(xyz), k, int(bool(include_self)), ptr(d2), ptr(idx), ptr(sigma), ptr(count), ptr(ws), nbytes,
                             stream()), "mgr_knn_self")
    return KnnSelf(sigma, count, d2, idx)


def outlier_scores(xyz, k=512, include_self=True, prob=None):
    """LoOP of every row of xyz (N,3) on its k nearest (`mgr_outlier_scores`, lambda = 1).  Returns OutlierScores with
    score, sigma, plof (N,), nplof (0-d float64 device tensor), stats = [nplof, n_valid, n_flagged] (3,) float64 on the
    device, and mask (N,) bool = score > prob when `prob` is given (else None).  Nothing is read back to the host."""
    xyz, k = _points(xyz, k)
    N, dev = xyz.shape[0], xyz.device
    score, sigma, plof = (torch.empty((N,), dtype=torch.float32, device=dev) for _ in range(3))
    mask = torch.empty((N,), dtype=torch.uint8, device=dev) if prob is not None else None
    stats = torch.empty((3,), dtype=torch.float64, device=dev)
    nbytes = int(lib().mgr_outlier_scores_workspace_bytes(N, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().mgr_outlier_scores(N, ptr(xyz), k, int(bool(include_self)), float(prob if prob is not None else 2.0), ptr(score),
                                   ptr(mask), ptr(sigma), ptr(plof), ptr(stats), ptr(ws), nbytes, stream()), "mgr_outlier_scores")
    return OutlierScores(score, sigma, plof, stats[0], stats, mask.bool() if mask is not None else None)


def outlier_mask(xyz, prob=0.8, neighbors=512, include_self=True):
    """(N,) device bool: LoOP score above `prob` on `neighbors` nearest.  The defaults are those densify_and_prune passes
    (src/models/gaussian.py:324)."""
    return outlier_scores(xyz, k=neighbors, include_self=include_self, prob=prob).mask


def update_mask_based_on_outliers(xyz, prob=0.5, neighbors=128):
    """The reference's name and defaults (src/utils/gaussian_utils.py:557): a device bool tensor, True = outlier."""
    return outlier_mask(xyz, prob=prob, neighbors=neighbors)

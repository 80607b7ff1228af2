"""CPU restatements (numpy, float32) of the contact-map contract, shared by test_contact_render_cpu.py and
test_gpu_contact_render.py.  Nothing here touches the GPU or the package under test."""
import numpy as np

from oracle import torch_ref as tr


def nearest_nan_safe(pt1, pt2, chunk=256):
    """The reference loop of get_contact_dist (gaussian_utils.py:537-547) with NaN coordinates defined the way the loop
    defines them: `dist < min_dist` is false for a NaN distance, so a NaN point is never anybody's nearest point and a NaN
    query keeps min_dist = 1e9 (index 0 here, as in oracle.torch_ref.contact_dist, which uses argmin and therefore does not
    define NaN).  fp32, (dx^2 + dy^2) + dz^2, rooted, first minimum."""
    a, b = np.asarray(pt1, np.float32).reshape(-1, 3), np.asarray(pt2, np.float32).reshape(-1, 3)
    n1, n2 = a.shape[0], b.shape[0]
    dist = np.full(n1, 1e9, np.float32)
    idx = np.zeros(n1, np.int64)
    if n2 == 0:
        return dist, idx
    with np.errstate(all="ignore"):
        for s in range(0, n1, chunk):
            d = a[s:s + chunk, None, :] - b[None, :, :]
            d2 = d[..., 0] * d[..., 0]
            d2 = d2 + d[..., 1] * d[..., 1]
            d2 = d2 + d[..., 2] * d[..., 2]
            r = np.sqrt(d2)
            r = np.where(np.isnan(r), np.float32(np.inf), r)        # never '<' anything
            j = np.argmin(r, axis=1)
            m = r[np.arange(r.shape[0]), j]
            ok = m < np.float32(1e9)
            dist[s:s + chunk] = np.where(ok, m, np.float32(1e9))
            idx[s:s + chunk] = np.where(ok, j, 0)
    return dist, idx


def value_formula(dist, c_thresh=0.004):
    """get_cmap lines 573-574 in float32: 1 - clamp(dist, 0, c) / c."""
    c = np.float32(c_thresh)
    d = np.asarray(dist, np.float32)
    return (np.float32(1) - np.minimum(np.maximum(d, np.float32(0)), c) / c).astype(np.float32)


def near_reference(pt1, pt2, c_thresh=0.004, nearest=tr.contact_dist):
    """The contract of mgr_contact_near from a brute-force search: value for every point; index and distance where
    value > 0, -1 and 1e9 elsewhere."""
    dist, idx = nearest(pt1, pt2)
    value = value_formula(dist, c_thresh)
    hit = value > 0
    return value, np.where(hit, idx, -1).astype(np.int64), np.where(hit, dist, np.float32(1e9)).astype(np.float32)


def lut_index(values):
    """Entry of a 256-entry matplotlib map for float32 values; -1 for NaN (the 'bad' colour, black)."""
    v = np.asarray(values, np.float32)
    with np.errstate(all="ignore"):
        s = v * np.float32(256)
        k = np.where(s > 0, np.where(s >= 255, 255, np.trunc(np.where(np.isfinite(s), s, 0))), 0).astype(np.int64)
    return np.where(np.isnan(v), -1, k)


def lut_colors(values, lut):
    k = lut_index(values)
    return np.where((k < 0)[:, None], np.float32(0), np.asarray(lut, np.float32)[np.maximum(k, 0)]).astype(np.float32)


def blend(rgb, cmap, alpha):
    """rgb * alpha + (1 - alpha) * cmap in float32 with the Python-float weights rounded to float32 (what torch does), two
    rounded products and one rounded sum."""
    a, b = np.float32(alpha), np.float32(1.0 - float(alpha))
    return (np.asarray(rgb, np.float32) * a + b * np.asarray(cmap, np.float32)).astype(np.float32)


def contact_inputs(n1, n2):
    """Inputs of the near-search test: pt1 = N(0, 0.05^2), pt2 = N(0, 0.05^2) + (0.04, 0, 0), seeded like
    test_gpu_contact.py, with 20 duplicated pt2 points, 20 coincident pairs, one pt2 outlier 1e4 m away and one NaN point
    in each set planted where the sizes allow."""
    g = np.random.default_rng(n1 + n2)
    pt1 = (g.normal(size=(n1, 3)) * 0.05).astype(np.float32)
    pt2 = (g.normal(size=(n2, 3)) * 0.05 + np.array([0.04, 0.0, 0.0])).astype(np.float32).reshape(-1, 3)
    if n2 > 100 and n1 > 100:
        pt2[n2 // 2:n2 // 2 + 20] = pt2[:20]            # every one of these has an earlier duplicate
        pt1[:20] = pt2[:20]                             # coincident pairs (distance 0, tie between the duplicates)
        pt2[77] = (1e4, 0.0, 0.0)                       # far outlier: must not blow the grid up
        pt2[91, 1] = np.nan
        pt1[55, 2] = np.nan
    return pt1, pt2

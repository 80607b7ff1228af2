"""Edge-case inputs and CPU references for the geometry kernels (helper module, no tests here): the contact searches of
csrc/contact.hip (mgr_contact_near, mgr_contact_dist) and the MANO-initialisation kernels of csrc/mesh.hip
(mgr_knn_mean_rows, mgr_mesh_sdf).  Nothing here touches the GPU or the package under test.

  near search     thresholds from 1e-5 to 1 m on one input, target points on cell borders with queries at distance exactly c and
                  one fp32 either side, a 1024-bucket table under millions of cells, coordinates up to +-inf, the 2^22 table cap
  brute force     the extreme coordinates and a NaN / inf planted (1000, 1025) input
  k nearest rows  every kernel instantiation (k = 1, k = 4, generic up to k = 32) at m around k and around the 256-row LDS tile, on
                  an integer lattice (exact distances, exact ties) and on random fp32 points
  signed distance one triangle against closed forms, closed boxes at face counts around the 256-face LDS tile, points on the
                  surface, degenerate faces, an open box, a box far from the origin, no faces at all

References: oracle.torch_ref.contact_dist / contact_oracle.nearest_nan_safe / contact_oracle.near_reference for the searches,
oracle.mesh_ref in float64 for the other two.  tests/test_geometry_cases_cpu.py proves on these references alone that every
case is what it is named for; tests/test_gpu_geometry_edges.py runs the kernels."""
import functools
import itertools

import numpy as np

import contact_oracle as co
from oracle import mesh_ref as R
from oracle import torch_ref as tr

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the host arithmetic of mgr_contact_near, restated (csrc/contact.hip: cn_cells, r, h, cn_coord, cn_hash)
# ---------------------------------------------------------------------------------------------------------------------
CN_COORD_MAX = 2.0 ** 40


def cn_cells(n2):
    n = 1024
    while n < 2 * max(n2, 0) and n < (1 << 22):
        n <<= 1
    return n


def cn_r_h(c):
    """(r, h) in float64 from the fp32 threshold, the way the host code forms them: r = c * 1.0001, h = r * 1.001."""
    r = float(F32(c)) * 1.0001
    return r, r * 1.001


def cn_coord(v, c):
    """Cell coordinate of float64 values v: floor(v * (1 / h)) clamped to +-2^40, NaN in the border cell (fmax / fmin drop it)."""
    _, h = cn_r_h(c)
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(v, np.float64) * (1.0 / h))
        f = np.where(np.isnan(f), -CN_COORD_MAX, f)
        return np.clip(f, -CN_COORD_MAX, CN_COORD_MAX).astype(np.int64)


def cn_hash(cx, cy, cz, mask):
    """The kernel's hash in integer arithmetic: the low 32 bits of each coordinate times a prime, modulo 2^32, xor-ed."""
    m32 = np.int64(0xFFFFFFFF)
    h = ((cx & m32) * np.int64(73856093)) & m32
    h = h ^ (((cy & m32) * np.int64(19349663)) & m32)
    h = h ^ (((cz & m32) * np.int64(83492791)) & m32)
    return h & np.int64(mask)


def visited_buckets(pt1, n2, c):
    """(n1, 27) buckets of the cells a query visits (-1 where an axis has fewer than three cells)."""
    r, _ = cn_r_h(c)
    p = np.asarray(pt1, np.float64)
    lo, hi = cn_coord(p - r, c), np.minimum(cn_coord(p + r, c), cn_coord(p - r, c) + 2)
    mask = cn_cells(n2) - 1
    out = np.full((p.shape[0], 27), -1, np.int64)
    for s, (dz, dy, dx) in enumerate(itertools.product(range(3), repeat=3)):
        cx, cy, cz = lo[:, 0] + dx, lo[:, 1] + dy, lo[:, 2] + dz
        ok = (cx <= hi[:, 0]) & (cy <= hi[:, 1]) & (cz <= hi[:, 2])
        out[:, s] = np.where(ok, cn_hash(cx, cy, cz, mask), -1)
    return out


def dist32(p, q):
    """The reference loop's rooted fp32 distance: sqrt((dx^2 + dy^2) + dz^2), every operation rounded to fp32."""
    d = np.asarray(p, F32) - np.asarray(q, F32)
    d2 = d[..., 0] * d[..., 0]
    d2 = d2 + d[..., 1] * d[..., 1]
    d2 = d2 + d[..., 2] * d[..., 2]
    return np.sqrt(d2)


# ---------------------------------------------------------------------------------------------------------------------
# A. inputs of the near search
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_THRESHOLDS = (1e-5, 4e-4, 0.004, 0.05, 1.0)
SWEEP_N = (2000, 3000)
BORDER_C = 0.004
BORDER_MULTIPLES = (-4, -2, 0, 2, 4)     # even multiples of fl32(h): exact in fp32, and 2 h apart, so that a query at distance c
                                         # from its lattice point is farther than c (2 h - c = 1.002 c) from the next one
BELOW, EQUAL, ABOVE = 0, 1, 2


SWEEP_WIDE_FROM, SWEEP_WIDE_SCALE = 1200, 3.0


@functools.lru_cache(maxsize=None)
def sweep_inputs():
    """contact_inputs(2000, 3000) -- duplicates, coincident pairs, the outlier and the NaN rows where it plants them -- with the
    queries from row 1200 on spread three times as wide (sigma 0.15).  As contact_inputs draws them, 99.3 % of the queries lie
    within 0.05 of a target; the wide part keeps the share in contact at c = 0.05 below 95 % while all of it stays within 1.0 of
    the targets, and the narrow part keeps the share at c = 0.004 above 5 %."""
    pt1, pt2 = co.contact_inputs(*SWEEP_N)
    pt1 = pt1.copy()
    pt1[SWEEP_WIDE_FROM:] *= F32(SWEEP_WIDE_SCALE)
    return pt1, pt2


def _ulp_steps(x, u):
    """The 2 u + 1 fp32 numbers within u ulps of x (x finite, not near zero)."""
    return (np.full(2 * u + 1, x, F32).view(np.int32) + np.arange(-u, u + 1, dtype=np.int32)).view(F32)


@functools.lru_cache(maxsize=None)
def border_inputs():
    """pt2: the lattice of BORDER_MULTIPLES * fl32(h) on every axis (125 points).  pt1: each lattice point displaced by about c along
    one, two and three axes (which axes and which way round varies with the point), the displaced coordinates moved by a few ulps
    until the reference's rooted fp32 distance is exactly the fp32 below c, c, or the fp32 above c -- one query for every
    (point, number of axes, class) for which the search finds one.  -> pt1, pt2, c, class, number of axes, lattice index."""
    c32 = F32(BORDER_C)
    _, h = cn_r_h(BORDER_C)
    hf = F32(h)
    ks = np.array(BORDER_MULTIPLES, F32)
    lat = np.stack(np.meshgrid(ks * hf, ks * hf, ks * hf, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    targets = (np.nextafter(c32, F32(0)), c32, np.nextafter(c32, F32(np.inf)))
    rows, cls, ndirs, src = [], [], [], []
    for li, q in enumerate(lat):
        for nd in (1, 2, 3):
            axes = [(li + t) % 3 for t in range(nd)]
            a = float(c32) / np.sqrt(nd)
            cands = []
            for t, ax in enumerate(axes):
                sign = 1.0 if (li >> t) & 1 else -1.0
                cands.append(_ulp_steps(F32(float(q[ax]) + sign * a), {1: 8, 2: 6, 3: 4}[nd]))
            combos = np.stack(np.meshgrid(*cands, indexing="ij"), -1).reshape(-1, nd)
            p = np.repeat(q[None, :], combos.shape[0], 0)
            p[:, axes] = combos
            d = dist32(p, q[None, :])
            for k, tgt in enumerate(targets):
                hit = np.flatnonzero(d == tgt)
                if hit.size:
                    rows.append(p[hit[0]]), cls.append(k), ndirs.append(nd), src.append(li)
    return np.array(rows, F32), lat, BORDER_C, np.array(cls), np.array(ndirs), np.array(src)


SPARSE_N2, SPARSE_PLANTED, SPARSE_FREE, SPARSE_FOLDED = 500, 200, 313, 60


def folded_queries(pt1, n2, c):
    """Queries for which at least two of the visited cells share a bucket: the kernel walks that bucket twice."""
    vb = visited_buckets(pt1, n2, c)
    return np.array([len(set(r[r >= 0].tolist())) < int((r >= 0).sum()) for r in vb])


@functools.lru_cache(maxsize=None)
def sparse_inputs():
    """500 target points over a 1 m cube at c = 0.004: 1.6e7 cells fold into the 1024 buckets.  200 queries are planted within
    0.2 c .. 0.9 c of a target point, 313 more are uniform in the cube.  The hash spreads neighbouring cells well (about 3 % of
    random places have two of their 27 cells in one bucket), so the targets are chosen from a pool of 20000 places: the first
    60 planted queries are ones that visit a bucket twice, the other 140 are not.  -> pt1, pt2, c."""
    g = np.random.default_rng(500)
    pool = g.uniform(-0.5, 0.5, size=(20000, 3)).astype(F32)
    u = g.normal(size=(pool.shape[0], 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    query = (pool + u * g.uniform(0.2, 0.9, size=(pool.shape[0], 1)) * 0.004).astype(F32)
    folded = folded_queries(query, SPARSE_N2, 0.004)
    chosen = np.concatenate([np.flatnonzero(folded)[:SPARSE_FOLDED], np.flatnonzero(~folded)[:SPARSE_N2 - SPARSE_FOLDED]])
    order = g.permutation(SPARSE_N2)                       # the targets of the planted queries are not the first rows of pt2
    pt2 = np.empty((SPARSE_N2, 3), F32)
    pt2[order] = pool[chosen]
    free = g.uniform(-0.5, 0.5, size=(SPARSE_FREE, 3)).astype(F32)
    return np.concatenate([query[chosen[:SPARSE_PLANTED]], free]), pt2, 0.004


EXTREME_VALUES = (1e6, -1e6, 5e9, -5e9, 1e12, -1e12, 3e38, -3e38, np.inf, -np.inf, -0.0, np.nan)
EXTREME_DUPLICATES = ((1e6, 2.0, 3.0), (1e12, -1e12, 5.0))       # the same row in both sets: distance 0, value 1
EXTREME_THRESHOLDS = (0.004, 0.1)                                # 0.1 is above the fp32 spacing at 1e6 (0.0625), 0.004 below it


@functools.lru_cache(maxsize=None)
def extreme_inputs():
    """contact_inputs(300, 400) with rows of extreme coordinates appended to both sets: every value of EXTREME_VALUES on one
    axis, on another axis beside small coordinates, and on all three; fp32 neighbours at 1e6; the two exact duplicate pairs.
    -> pt1, pt2 (the reference is nearest_nan_safe: the sets hold NaN and inf)."""
    pt1, pt2 = co.contact_inputs(300, 400)
    a, b = [], []
    for v in EXTREME_VALUES:
        a += [(v, 0.0, 0.0), (0.0, v, 0.01), (v, v, v)]
        b += [(v, 0.001, 0.0), (0.002, v, 0.0), (v, -v, v)]
    near = np.nextafter(F32(1e6), F32(np.inf))
    a += [(1e6, 5.0, 5.0), (-1e6, 5.0, 5.0)]
    b += [(near, 5.0, 5.0), (-near, 5.0, 5.0)]
    a += list(EXTREME_DUPLICATES)
    b += list(EXTREME_DUPLICATES)
    with np.errstate(all="ignore"):
        return np.concatenate([pt1, np.array(a, F32)]), np.concatenate([pt2, np.array(b, F32)])


CAP_N1, CAP_N2, CAP_PLANTED = 64, 2300000, 32


@functools.lru_cache(maxsize=None)
def cap_inputs():
    """2.3 M target points uniform in a 2 m cube (2 * n2 > 2^22: the table stays at its cap, load factor 0.55, and its scan runs
    4096 workgroups); 32 queries planted within 0.2 c .. 0.9 c of a target point, 32 uniform.  -> pt1, pt2, c."""
    g = np.random.default_rng(23)
    pt2 = g.uniform(-1.0, 1.0, size=(CAP_N2, 3)).astype(F32)
    u = g.normal(size=(CAP_PLANTED, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    planted = pt2[g.integers(0, CAP_N2, size=CAP_PLANTED)] + u * g.uniform(0.2, 0.9, size=(CAP_PLANTED, 1)) * 0.004
    free = g.uniform(-1.0, 1.0, size=(CAP_N1 - CAP_PLANTED, 3))
    return np.concatenate([planted, free]).astype(F32), pt2, 0.004


NEAR_CASES = (["sweep@%g" % c for c in SWEEP_THRESHOLDS] + ["borders", "sparse_table"] + ["extremes@%g" % c for c in EXTREME_THRESHOLDS]
              + ["table_cap"])


def near_inputs(name):
    """-> pt1, pt2, c_thresh of a near-search case."""
    kind, _, c = name.partition("@")
    if kind == "sweep":
        return sweep_inputs() + (float(c),)
    if kind == "extremes":
        return extreme_inputs() + (float(c),)
    return {"borders": border_inputs, "sparse_table": sparse_inputs, "table_cap": cap_inputs}[kind]()[:3]


@functools.lru_cache(maxsize=None)
def nearest_of(kind):
    """nearest_nan_safe of a case's points, once for all its thresholds; 4 queries at a time against the 2.3 M points of the
    table cap (under 400 MB of temporaries)."""
    pt1, pt2 = near_inputs(kind if kind not in ("sweep", "extremes") else kind + "@1")[:2]
    return co.nearest_nan_safe(pt1, pt2, chunk=4 if kind == "table_cap" else 256)


def near_expected(name):
    """(value, index, distance) that mgr_contact_near must return, bit for bit: contact_oracle.near_reference over
    nearest_nan_safe."""
    pt1, pt2, c = near_inputs(name)
    return co.near_reference(pt1, pt2, c, nearest=lambda a, b: nearest_of(name.partition("@")[0]))


def finite_rows(p):
    return np.isfinite(p).all(1)


def nan_safe_equals_oracle(pt1, pt2, chunk=256):
    """nearest_nan_safe against oracle.torch_ref.contact_dist on the rows the oracle defines: queries and targets without NaN or
    inf (inf - inf is NaN, and the oracle's argmin does not define NaN).  -> number of rows compared."""
    ok1, ok2 = finite_rows(pt1), finite_rows(pt2)
    with np.errstate(all="ignore"):
        od, oi = tr.contact_dist(pt1[ok1], pt2[ok2], chunk=chunk)
        nd, ni = co.nearest_nan_safe(pt1[ok1], pt2[ok2], chunk=chunk)
        fd, fi = (nd, ni) if ok2.all() else co.nearest_nan_safe(pt1[ok1], pt2, chunk=chunk)
    np.testing.assert_array_equal(nd, od)
    np.testing.assert_array_equal(ni, oi)
    # the non-finite targets are nobody's nearest point: the search over all of pt2 finds the same points
    np.testing.assert_array_equal(fd, od)
    np.testing.assert_array_equal(fi, np.where(od < F32(1e9), np.flatnonzero(ok2)[oi], 0))
    return int(ok1.sum())


# ---------------------------------------------------------------------------------------------------------------------
# B. inputs of the brute-force search
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_inputs():
    """(1000, 1025) points -- two query workgroups, one LDS tile of targets and one point -- with duplicates, coincident pairs
    and NaN / inf rows in both sets: at the first and last rows, either side of the tile seam (targets 1023, 1024) and of the
    workgroup seam (queries 511, 512)."""
    n1, n2 = 1000, 1025
    g = np.random.default_rng(n1 + n2)
    pt1 = (g.normal(size=(n1, 3)) * 0.05).astype(F32)
    pt2 = (g.normal(size=(n2, 3)) * 0.05).astype(F32)
    pt2[n2 // 2:n2 // 2 + 20] = pt2[100:120]
    pt1[100:120] = pt2[100:120]
    nan, inf = np.nan, np.inf
    pt2[0] = (nan, nan, nan)
    pt2[1, 1] = nan
    pt2[2] = (inf, 0.0, 0.0)
    pt2[1023, 2] = nan
    pt2[1024] = (-inf, inf, 0.0)
    pt2[700] = (0.0, -inf, 0.0)
    pt1[0, 0] = nan
    pt1[1] = (inf, 0.0, 0.0)
    pt1[511] = (nan, nan, nan)
    pt1[512] = (0.0, 0.0, -inf)
    pt1[999, 1] = nan
    pt1[998] = (inf, inf, inf)
    return pt1, pt2


DIST_CASES = {"extremes": extreme_inputs, "nan_planted": planted_inputs}


@functools.lru_cache(maxsize=None)
def dist_expected(name):
    return co.nearest_nan_safe(*DIST_CASES[name]())


# ---------------------------------------------------------------------------------------------------------------------
# C. k nearest rows
# ---------------------------------------------------------------------------------------------------------------------
# (k, m, C, n): every k of {1, 2, 4, 5, 31, 32} (k = 1 and k = 4 have kernels of their own, the others share the generic one; 32 is
# the full scratch list), m of {1, k - 1, k, 255, 256, 257, 778}, C of {1, 3, 20, 33}, n of {1, 255, 257}; k = 1, 4 and 32 each at m = 257
KNN_CASES = [
    (1, 257, 1, 257), (4, 257, 3, 255), (32, 257, 20, 257),
    (1, 1, 1, 1), (2, 1, 33, 1), (32, 32, 33, 1),
    (4, 3, 3, 257), (4, 4, 1, 255), (5, 5, 3, 255), (5, 4, 20, 257), (31, 30, 1, 257), (31, 31, 3, 255), (32, 31, 3, 255), (2, 2, 20, 257),
    (4, 255, 20, 257), (2, 256, 33, 255), (32, 256, 1, 257), (1, 255, 3, 255), (5, 256, 1, 257),
    (5, 778, 20, 257), (31, 778, 3, 255), (1, 778, 20, 255), (4, 778, 33, 257), (32, 778, 3, 257), (2, 257, 3, 257), (31, 257, 33, 255),
]
KNN_MEAN_RTOL = 2.0 ** -22         # lattice means: the row sum is exact; one rounded reciprocal and one rounded product
KNN_NEAR_TIE = 1e-5                # random points: rows whose k-th and (k+1)-th squared distances are this close may differ


def knn_id(case):
    return "k%d-m%d-C%d-n%d" % case


@functools.lru_cache(maxsize=None)
def knn_lattice(case):
    """Integer coordinates: |x| <= 4 for most points (729 sites: duplicates and equal distances everywhere), a few at +-64;
    rows of integers in [-8, 8].  Every fp32 squared distance and every row sum is exact.  -> points, refs, rows (fp32)."""
    k, m, C, n = case
    g = np.random.default_rng(1000 * k + m + 7 * C + n)
    pts = g.integers(-4, 5, size=(n, 3))
    refs = g.integers(-4, 5, size=(m, 3))
    if n > 8:
        pts[::50] = g.integers(-64, 65, size=pts[::50].shape)
    if m > 8:
        refs[::40] = g.integers(-64, 65, size=refs[::40].shape)
    rows = g.integers(-8, 9, size=(m, C))
    return pts.astype(F32), refs.astype(F32), rows.astype(F32)


@functools.lru_cache(maxsize=None)
def knn_random(case):
    """Random fp32 points N(0, 1) and rows in [0, 1).  -> points, refs, rows."""
    k, m, C, n = case
    g = np.random.default_rng(2000 * k + m + 7 * C + n)
    return g.normal(size=(n, 3)).astype(F32), g.normal(size=(m, 3)).astype(F32), g.uniform(0, 1, size=(m, C)).astype(F32)


def knn_sorted(points, refs):
    """(stable argsort of the float64 squared distances, the sorted distances), all m columns."""
    p, r = np.asarray(points, np.float64), np.asarray(refs, np.float64)
    d2 = ((p[:, None, :] - r[None, :, :]) ** 2).sum(-1)
    order = np.argsort(d2, axis=1, kind="stable")
    return order, np.take_along_axis(d2, order, 1)


def knn_expected(points, refs, rows, k):
    """(indices (n, k) with -1 in the slots past m, float64 mean of the min(k, m) nearest rows, sorted squared distances)."""
    order, d2 = knn_sorted(points, refs)
    m = refs.shape[0]
    idx = np.full((points.shape[0], k), -1, np.int64)
    idx[:, :min(k, m)] = order[:, :k]
    return idx, np.asarray(rows, np.float64)[order[:, :k]].mean(1), d2


def knn_tie_at_k(d2, k):
    """Rows whose k-th and (k+1)-th nearest references are exactly as far (needs m > k)."""
    return d2[:, k] == d2[:, k - 1] if d2.shape[1] > k else np.zeros(d2.shape[0], bool)


def knn_near_tie_at_k(d2, k):
    return (d2[:, k] - d2[:, k - 1]) < KNN_NEAR_TIE * d2[:, k] if d2.shape[1] > k else np.zeros(d2.shape[0], bool)


def knn_clear_order(d2, k):
    """Rows in which no two neighbouring distances among the first k + 1 are within KNN_NEAR_TIE: the order itself is pinned."""
    d = d2[:, :k + 1]
    return ((d[:, 1:] - d[:, :-1]) >= KNN_NEAR_TIE * d[:, 1:]).all(1) if d.shape[1] > 1 else np.ones(d2.shape[0], bool)


def knn_random_atol(k):
    """Mean of k fp32 rows in [0, 1): k - 1 rounded additions of partial sums below k, one rounded reciprocal and one rounded
    product, each half an ulp -- at most ((k - 1) k 2^-24 + 2 k 2^-24) / k = (k + 1) 2^-24."""
    return (k + 1) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# D. signed distance
# ---------------------------------------------------------------------------------------------------------------------
def mesh_sdf_f32(points, verts, faces):
    """oracle.mesh_ref.mesh_sdf with every operation in float32 numpy (the oracle's region walk on float32 arrays, its solid
    angles restated line for line): the yardstick of what fp32 can give on these formulas.  -> (sdf, winding), float32."""
    v = np.asarray(verts, F32)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    out, wind = np.zeros(len(points), F32), np.zeros(len(points), F32)
    for i, p in enumerate(np.asarray(points, F32)):
        q = R._closest_on_triangle(p, a, b, c)
        assert q.dtype == F32
        d = np.sqrt(((p - q) ** 2).sum(-1).min())
        A, B, C = a - p, b - p, c - p
        la, lb, lc = np.sqrt((A * A).sum(-1)), np.sqrt((B * B).sum(-1)), np.sqrt((C * C).sum(-1))
        det = (A * np.cross(B, C)).sum(-1)
        den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
        w = (F32(2.0) * np.arctan2(det, den)).sum() / F32(4.0 * np.pi)
        wind[i] = w
        out[i] = d if abs(w) > 0.5 else -d
    return out, wind


def box_mesh(na, nb, nc, step=0.25):
    """The surface of the box [0, na] x [0, nb] x [0, nc] * step, every face a grid of squares cut into two triangles, oriented
    outwards: 4 (na nb + na nc + nb nc) faces, all coordinates multiples of `step`.  -> verts (fp32), faces (int64)."""
    dims = (na, nb, nc)
    index, verts, faces = {}, [], []

    def vid(ijk):
        if ijk not in index:
            index[ijk] = len(verts)
            verts.append([step * t for t in ijk])
        return index[ijk]

    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3                  # e_u x e_v = e_ax
        for side in (0, dims[ax]):
            for iu in range(dims[u]):
                for iv in range(dims[v]):
                    def corner(du, dv):
                        ijk = [0, 0, 0]
                        ijk[ax], ijk[u], ijk[v] = side, iu + du, iv + dv
                        return vid(tuple(ijk))
                    c00, c10, c11, c01 = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    tris = [(c00, c10, c11), (c00, c11, c01)]
                    faces += tris if side else [(t[0], t[2], t[1]) for t in tris]
    return np.array(verts, F32), np.array(faces, np.int64)


def split_face(verts, faces, t, e=2):
    """Face t cut in two at the midpoint of its edge e (a new vertex; the neighbour across the edge is left whole).  On a
    flat patch the surface is the same set of points, with one face more.  -> verts, faces."""
    f = faces[t]
    i, j, o = f[e], f[(e + 1) % 3], f[(e + 2) % 3]
    mid = ((verts[i].astype(np.float64) + verts[j]) / 2).astype(F32)
    assert (mid.astype(np.float64) * 2 == verts[i].astype(np.float64) + verts[j]).all()      # exactly representable
    m = len(verts)
    faces = np.concatenate([faces[:t], [[i, m, o], [m, j, o]], faces[t + 1:]])
    return np.concatenate([verts, mid[None]]), faces


# name -> (box grid, faces to split).  Closed meshes have an even number of faces; the odd counts come from adding faces on flat
# patches: each split cuts one triangle of a box face in two along the square's diagonal (edge 2 of the first triangle of a
# square, whose midpoint is the square's centre), without touching the triangle across the diagonal
BOXES = {255: ((3, 3, 9), (0, 40, 100)), 256: ((4, 4, 6), ()), 257: ((4, 4, 6), (10,)), 513: ((8, 8, 4), (6,))}
SHIFT = (10.0, -7.0, 3.0)


@functools.lru_cache(maxsize=None)
def closed_box(nf):
    dims, splits = BOXES[nf]
    verts, faces = box_mesh(*dims)
    for t in splits:
        verts, faces = split_face(verts, faces, t)
    assert faces.shape[0] == nf
    return verts, faces


def tetrahedron():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    return verts, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)


def points_around(verts, n, seed, scale=1.3):
    """n points uniform in the bounding box of the mesh scaled by `scale` about its centre."""
    g = np.random.default_rng(seed)
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * scale
    return (mid + g.uniform(-1, 1, size=(n, 3)) * half).astype(F32)


TRI = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0]], F32)
TRI_REGIONS = ("vertex_a", "vertex_b", "vertex_c", "edge_ab", "edge_bc", "edge_ca", "interior")


def triangle_points():
    """(x, y) of three points in each Voronoi region of TRI (a = origin, b = (2, 0), c = (0, 1), in the plane z = 0), each
    above and below the plane at three heights.  -> points (fp32), region name per point."""
    xy = {"vertex_a": [(-0.5, -0.25), (-2.0, -0.125), (-0.125, -3.0)],
          "vertex_b": [(3.0, -0.5), (2.5, 0.5), (4.0, 0.25)],                # beyond b: (p - b).(b - a) >= 0, (p - b).(c - b) <= 0
          "vertex_c": [(-0.5, 1.5), (0.25, 2.0), (-1.0, 1.25)],
          "edge_ab": [(0.5, -0.5), (1.0, -2.0), (1.75, -0.125)],
          "edge_bc": [(1.5, 1.0), (1.0, 0.75), (2.0, 1.5)],
          "edge_ca": [(-0.5, 0.5), (-2.0, 0.25), (-0.125, 0.875)],
          "interior": [(0.5, 0.25), (1.0, 0.25), (0.125, 0.75)]}
    pts, names = [], []
    for name in TRI_REGIONS:
        for (x, y), z in itertools.product(xy[name], (0.5, -0.5, 0.0625, -0.0625, 3.0, -3.0)):
            pts.append((x, y, z)), names.append(name)
    return np.array(pts, F32), names


def triangle_closed_form(points, names):
    """Distance of each point to TRI from its region's closed form, float64."""
    p = np.asarray(points, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    form = {"vertex_a": np.sqrt(x * x + y * y + z * z),
            "vertex_b": np.sqrt((x - 2) ** 2 + y * y + z * z),
            "vertex_c": np.sqrt(x * x + (y - 1) ** 2 + z * z),
            "edge_ab": np.sqrt(y * y + z * z),
            "edge_ca": np.sqrt(x * x + z * z),
            "edge_bc": np.sqrt((x + 2 * y - 2) ** 2 / 5 + z * z),             # the line x + 2 y = 2
            "interior": np.abs(z)}
    return np.array([form[nm][i] for i, nm in enumerate(names)])


def surface_points(verts, faces, count=64):
    """Points of the surface: the first `count` vertices, the midpoints of the first edge of `count` faces spread over the mesh
    (exact: the coordinates are multiples of the grid step) and those faces' centroids rounded to fp32 -- the faces of a box lie
    in axis planes, so the rounded centroid is still a point of the face."""
    pick = np.linspace(0, faces.shape[0] - 1, count).astype(np.int64)
    v = verts.astype(np.float64)
    a, b, c = v[faces[pick, 0]], v[faces[pick, 1]], v[faces[pick, 2]]
    mids = (a + b) / 2
    assert (mids.astype(F32).astype(np.float64) == mids).all()
    return np.concatenate([verts[:count], mids.astype(F32), ((a + b + c) / 3).astype(F32)])


@functools.lru_cache(maxsize=None)
def degenerate_box():
    """The 256-face box with six degenerate faces appended on edges at two of its corners and on an inner grid line:
    (i, i, j), (i, j, i) and (a, mid, b) with a new vertex `mid` at the exact midpoint.  Points: 193 around the box, and 64 near
    the supporting lines of those edges beyond the segment ends (0.05 .. 0.6 past the end, up to 2e-3 off the line).
    -> verts, faces (the clean faces first), number of clean faces, points."""
    verts, faces = closed_box(256)
    key = {tuple(np.round(v * 4).astype(int)): i for i, v in enumerate(verts)}
    edges = [(key[(0, 0, 0)], key[(1, 0, 0)]), (key[(4, 4, 6)], key[(4, 4, 5)]), (key[(2, 0, 3)], key[(2, 0, 4)])]
    extra, new_verts = [], []
    for i, j in edges:
        extra += [(i, i, j), (i, j, i)]
    for i, j in edges:
        mid = (verts[i] + verts[j]) / 2
        new_verts.append(mid)
        extra.append((i, len(verts) + len(new_verts) - 1, j))
    g = np.random.default_rng(4)
    near = []
    for i, j in edges:
        a, b = verts[i].astype(np.float64), verts[j].astype(np.float64)
        d = (b - a) / np.linalg.norm(b - a)
        for end, way in ((a, -d), (b, d)):
            t = g.uniform(0.05, 0.6, size=(11, 1))
            near.append(end + way * t + g.uniform(-2e-3, 2e-3, size=(11, 3)))
    near = np.concatenate(near)[:64]
    pts = np.concatenate([points_around(verts, 257 - len(near), 41), near.astype(F32)])
    return np.concatenate([verts, np.array(new_verts, F32)]), np.concatenate([faces, np.array(extra, np.int64)]), faces.shape[0], pts


def open_cube():
    """The unit cube of test_signed_distance_of_a_cube_is_analytic without its top square (faces (4, 5, 6), (4, 6, 7), z = 1):
    10 faces, 4 boundary edges.  Points: 160 around it, 97 within 0.3 of the hole's centre on either side."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], F32)
    faces = np.array([[0, 2, 1], [0, 3, 2], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5], [0, 4, 7], [0, 7, 3]], np.int64)
    g = np.random.default_rng(5)
    hole = np.array([0.5, 0.5, 1.0]) + g.uniform(-0.3, 0.3, size=(97, 3))
    return verts, faces, np.concatenate([points_around(verts, 160, 51, scale=2.0), hole.astype(F32)])


SDF_CASES = ("triangle", "tetrahedron", "box255", "box256", "box257", "box513", "surface", "surface_shifted", "degenerate", "open_cube",
             "box256_shifted")


@functools.lru_cache(maxsize=None)
def sdf_case(name):
    """-> dict(verts, faces, points) and, for `degenerate`, ref_faces: the clean mesh the oracle is run on."""
    if name == "triangle":
        return dict(verts=TRI, faces=np.array([[0, 1, 2]], np.int64), points=triangle_points()[0])
    if name == "tetrahedron":
        verts, faces = tetrahedron()
        g = np.random.default_rng(3)
        pts = np.concatenate([g.uniform(0.0, 0.6, size=(129, 3)), g.uniform(-0.3, 1.1, size=(128, 3))]).astype(F32)
        return dict(verts=verts, faces=faces, points=pts)
    if name.startswith("box") and not name.endswith("shifted"):
        verts, faces = closed_box(int(name[3:]))
        return dict(verts=verts, faces=faces, points=points_around(verts, 257, int(name[3:])))
    if name == "box256_shifted":
        c = sdf_case("box256")
        s = np.array(SHIFT, F32)
        return dict(verts=c["verts"] + s, faces=c["faces"], points=c["points"] + s)
    if name == "surface":
        verts, faces = closed_box(256)
        return dict(verts=verts, faces=faces, points=surface_points(verts, faces))
    if name == "surface_shifted":
        verts, faces = closed_box(256)
        s = np.array(SHIFT, F32)
        return dict(verts=verts + s, faces=faces, points=surface_points(verts + s, faces))
    if name == "degenerate":
        verts, faces, nclean, pts = degenerate_box()
        return dict(verts=verts, faces=faces, points=pts, ref_faces=faces[:nclean])
    if name == "open_cube":
        verts, faces, pts = open_cube()
        return dict(verts=verts, faces=faces, points=pts)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sdf_oracle(name):
    """oracle.mesh_ref.mesh_sdf (float64) of a case: (sdf, winding); on the clean mesh for `degenerate`."""
    c = sdf_case(name)
    return R.mesh_sdf(c["points"], c["verts"], c.get("ref_faces", c["faces"]))


def sdf_f32_error(name):
    """max |float32 restatement - float64 oracle| over the case's points: (of |sdf|, of the winding number)."""
    c = sdf_case(name)
    s64, w64 = sdf_oracle(name)
    s32, w32 = mesh_sdf_f32(c["points"], c["verts"], c.get("ref_faces", c["faces"]))
    return float(np.abs(np.abs(s32.astype(np.float64)) - np.abs(s64)).max()), float(np.abs(w32.astype(np.float64) - w64).max())


# Measured by sdf_f32_error on the CPU (numpy float32 against the float64 oracle, on the fp32 inputs of each case), rounded up
# to two digits: (max error of |sdf|, max error of the winding number).  tests/test_geometry_cases_cpu.py measures them again
# and fails if a value here is below the measurement or more than twice above it.  The kernel is held to SDF_FACTOR times these:
# it adds the 1 .. 513 solid angles in face order (with a compensation term; numpy sums pairwise) and contracts multiply-adds,
# so it lies about as far from the float64 result as another float32 evaluation of the same formulas does.  Never set from the
# kernel's output.
SDF_F32_ERR = {
    "triangle": (1.5e-07, 2.3e-08),          # measured 1.480e-07, 2.227e-08
    "tetrahedron": (6.9e-08, 1.9e-07),       # measured 6.830e-08, 1.897e-07
    "box255": (1.6e-08, 2.4e-07),            # measured 1.547e-08, 2.384e-07
    "box256": (1.5e-08, 5.4e-07),            # measured 1.427e-08, 5.364e-07
    "box257": (8.6e-09, 1.2e-07),            # measured 8.566e-09, 1.192e-07
    "box513": (2.7e-08, 1.9e-07),            # measured 2.601e-08, 1.897e-07
    "surface": (1.2e-07, None),              # measured 1.192e-07; on the surface the winding number jumps: not compared
    "surface_shifted": (9.6e-07, None),      # measured 9.537e-07
    "degenerate": (3.9e-08, 2.2e-06),        # measured 3.858e-08, 2.163e-06 (on the clean mesh)
    "open_cube": (4.1e-08, 3.2e-06),         # measured 4.037e-08, 3.179e-06
    "box256_shifted": (1.3e-08, 3.0e-07),    # measured 1.262e-08, 2.980e-07
}
SDF_FACTOR = 4.0
SDF_CLEAR = 1e-3          # the sign is asserted where the oracle's |winding| is this far from 1/2
SDF_EMPTY = -float(np.sqrt(F32(3.0e38)))      # nf = 0: the kernel's "no face yet" squared distance, rooted, negative (outside)


def sdf_tolerance(name):
    """(atol of |sdf|, atol of the winding number or None) for the kernel on a case."""
    s, w = SDF_F32_ERR[name]
    return SDF_FACTOR * s, None if w is None else SDF_FACTOR * w

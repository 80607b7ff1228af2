"""CPU: the input conditions of tests/test_gpu_geometry_edges.py (tests/geometry_cases.py).  Nothing here runs a kernel: these
tests prove on the references alone -- oracle.torch_ref.contact_dist, contact_oracle.nearest_nan_safe / near_reference,
oracle.mesh_ref in float64 -- that every case is what it is named for: the shares of queries in contact over the threshold sweep,
the three distance classes at the cell borders, the folded buckets of the sparse table, the clamp and the table cap, the exact ties
of the lattice kNN inputs and the near-tie shares of the random ones, the inside shares of the meshes, and the float32 yardsticks
the signed-distance tolerances are derived from."""
import numpy as np
import pytest

import contact_oracle as co
import geometry_cases as gc
from oracle import mesh_ref as R

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# A. near search
# ---------------------------------------------------------------------------------------------------------------------
def test_threshold_sweep_shares():
    pt1, pt2 = gc.sweep_inputs()
    assert pt1.shape == (2000, 3) and pt2.shape == (3000, 3)
    assert np.isnan(pt1[55]).any() and np.isnan(pt2[91]).any() and pt2[77, 0] == 1e4            # contact_inputs' plants
    assert (pt1[:20] == pt2[:20]).all() and (pt2[1500:1520] == pt2[:20]).all()
    finite = gc.finite_rows(pt1)
    assert finite.sum() == 1999
    share = {}
    for c in gc.SWEEP_THRESHOLDS:
        value, idx, dist = gc.near_expected("sweep@%g" % c)
        share[c] = float((value[finite] > 0).mean())
        assert value[55] == 0 and idx[55] == -1
        print("SWEEP c = %g: %.2f %% of the finite queries in contact" % (c, 100 * share[c]))
    assert share[1.0] == 1.0                                              # every finite query is a hit ...
    body = np.ones(3000, bool)
    body[[77, 91]] = False
    cells = {tuple(r) for r in gc.cn_coord(pt2[body], 1.0)}
    assert len(cells) <= 8, cells                                         # ... and the targets (bar the outlier and the NaN row) share 8 cells
    v = gc.near_expected("sweep@1e-05")[0]
    assert (np.flatnonzero(v > 0) == np.arange(20)).all()                 # only the coincident pairs
    assert 0.05 < share[0.004] < 0.95 and 0.05 < share[0.05] < 0.95
    assert gc.cn_cells(3000) == 8192


def test_cell_border_classes():
    pt1, pt2, c, cls, ndir, src = gc.border_inputs()
    c32 = F32(c)
    _, h = gc.cn_r_h(c)
    hf = F32(h)
    # the lattice: fp32 coordinates that are exactly integer multiples of fl32(h), negative ones and 0 included
    k = pt2.astype(np.float64) / float(hf)
    assert (k == np.round(k)).all() and set(np.unique(k).tolist()) == set(float(m) for m in gc.BORDER_MULTIPLES)
    assert (k * float(hf) == pt2.astype(np.float64)).all() and (k < 0).any() and (k == 0).any()
    # fl32(h) is not h: the lattice points lie within 1e-7 of a cell border, on either side of it
    off = gc.cn_coord(pt2, c) - k.astype(np.int64)
    print("BORDERS fl32(h) - h = %.3e; cell coordinate minus multiple: %s" % (float(hf) - h, sorted(set(off.reshape(-1).tolist()))))
    assert set(off.reshape(-1).tolist()) <= {-1, 0} and abs(float(hf) - h) < 1e-7 * h
    targets = np.array([np.nextafter(c32, F32(0)), c32, np.nextafter(c32, F32(np.inf))], F32)
    assert targets[0] < c32 < targets[2]
    for nd in (1, 2, 3):
        counts = [int(((ndir == nd) & (cls == k_)).sum()) for k_ in range(3)]
        print("BORDERS %d-axis displacements: below / equal / above = %s" % (nd, counts))
        assert min(counts) >= 20, (nd, counts)                            # all three classes in every displacement direction
        moved = (pt1[ndir == nd] != pt2[src[ndir == nd]]).sum(1)
        assert (moved == nd).all()
    dist, idx = co.nearest_nan_safe(pt1, pt2)
    assert (idx == src).all() and (dist == targets[cls]).all()           # the reference's rooted distance IS the class's
    value, ridx, rdist = gc.near_expected("borders")
    assert (value[cls == gc.BELOW] > 0).all() and (ridx[cls == gc.BELOW] == src[cls == gc.BELOW]).all()
    assert (value[cls != gc.BELOW] == 0).all() and (ridx[cls != gc.BELOW] == -1).all()
    # both ways round: queries displaced towards lower and towards higher cells
    d = pt1.astype(np.float64) - pt2[src]
    assert (d > 0).any() and (d < 0).any()


def test_sparse_table_folds_cells():
    pt1, pt2, c = gc.sparse_inputs()
    assert pt2.shape == (gc.SPARSE_N2, 3) and gc.cn_cells(gc.SPARSE_N2) == 1024
    _, h = gc.cn_r_h(c)
    assert (1.0 / h) ** 3 > 1e7                                           # cells in the 1 m cube the points are spread over
    assert (pt2.max(0) - pt2.min(0) > 0.95).all()
    occupied = {tuple(r) for r in gc.cn_coord(pt2, c)}
    assert len(occupied) >= 495                                           # next to no two points in one cell
    value, idx, dist = gc.near_expected("sparse_table")
    planted = np.arange(gc.SPARSE_PLANTED)
    assert (value[planted] > 0).all() and len(set(idx[planted].tolist())) == gc.SPARSE_PLANTED
    folded = gc.folded_queries(pt1, gc.SPARSE_N2, c)
    print("SPARSE %.1f %% of the planted contacts visit a bucket twice; %d of the other queries hit" % (100 * folded[planted].mean(), int((value[gc.SPARSE_PLANTED:] > 0).sum())))
    assert folded[planted].mean() >= 0.10
    ncell = (gc.visited_buckets(pt1, gc.SPARSE_N2, c) >= 0).sum(1)        # 2 r = 1.998 h: three cells per axis but for 0.2 % of places
    assert set(ncell.tolist()) <= {8, 12, 18, 27} and (ncell == 27).mean() > 0.95
    # the restated hash against a by-hand evaluation with Python integers
    for cx, cy, cz in ((0, 0, 0), (1, -1, 5), (-250, 124, 2 ** 40), (-2 ** 40, 3, -7)):
        want = (((cx * 73856093) & 0xFFFFFFFF) ^ ((cy * 19349663) & 0xFFFFFFFF) ^ ((cz * 83492791) & 0xFFFFFFFF)) & 1023
        assert int(gc.cn_hash(np.int64(cx), np.int64(cy), np.int64(cz), 1023)) == want


def test_extreme_coordinates_are_what_they_are_named_for():
    pt1, pt2 = gc.extreme_inputs()
    _, h = gc.cn_r_h(0.004)
    for p in (pt1, pt2):
        vals = p.reshape(-1)
        for v in gc.EXTREME_VALUES:
            if np.isnan(v):
                assert np.isnan(vals).any()
            else:
                assert (vals == F32(v)).any(), v
        assert (np.signbit(vals) & (vals == 0)).any()                     # -0.0
    assert np.spacing(F32(1e6)) > F32(0.004) and np.spacing(F32(1e6)) < F32(0.1)
    assert 5e9 / h > gc.CN_COORD_MAX and 1e6 / h < gc.CN_COORD_MAX        # 5e9 and 1e12 lie beyond the clamp, 1e6 inside it
    assert (gc.cn_coord(np.array([5e9, 1e12, 3e38, np.inf, np.nan, -5e9, -np.inf]), 0.004)
            == np.array([2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, -2 ** 40, -2 ** 40, -2 ** 40])).all()
    for c in gc.EXTREME_THRESHOLDS:
        value, idx, dist = gc.near_expected("extremes@%g" % c)
        for row in gc.EXTREME_DUPLICATES:
            i = int(np.flatnonzero((pt1 == np.array(row, F32)).all(1))[0])
            j = int(np.flatnonzero((pt2 == np.array(row, F32)).all(1))[0])
            assert value[i] == 1 and idx[i] == j and dist[i] == 0, (c, row)
        bad = ~gc.finite_rows(pt1)
        assert bad.sum() >= 9 and (value[bad] == 0).all() and (idx[bad] == -1).all()     # NaN / inf queries: no contact
        assert not np.isin(idx, np.flatnonzero(~gc.finite_rows(pt2))).any()              # NaN / inf targets: nobody's neighbour
        print("EXTREMES c = %g: %d of %d queries in contact" % (c, int((value > 0).sum()), value.shape[0]))
    # the fp32 neighbours at 1e6 are 0.0625 apart: a contact at c = 0.1 only
    i = int(np.flatnonzero((pt1 == np.array((1e6, 5.0, 5.0), F32)).all(1))[0])
    assert gc.near_expected("extremes@0.1")[0][i] > 0 and gc.near_expected("extremes@0.004")[0][i] == 0


def test_table_cap_is_reached():
    pt1, pt2, c = gc.cap_inputs()
    assert pt1.shape == (64, 3) and pt2.shape == (2300000, 3)
    assert 2 * pt2.shape[0] > (1 << 22) and gc.cn_cells(pt2.shape[0]) == 1 << 22 and gc.cn_cells(pt2.shape[0]) // 1024 == 4096
    assert gc.cn_cells(2097152) == 1 << 22 and gc.cn_cells(2097153) == 1 << 22 and gc.cn_cells(1048577) == 1 << 22
    value, idx, dist = gc.near_expected("table_cap")
    print("TABLE CAP: %d planted and %d other queries in contact" % (int((value[:gc.CAP_PLANTED] > 0).sum()), int((value[gc.CAP_PLANTED:] > 0).sum())))
    assert (value[:gc.CAP_PLANTED] > 0).all() and (value[gc.CAP_PLANTED:] == 0).sum() >= 16


@pytest.mark.parametrize("name", ["sweep", "borders", "sparse_table", "extremes", "table_cap", "nan_planted"])
def test_nan_safe_search_equals_the_oracle_where_the_oracle_is_defined(name):
    """nearest_nan_safe is the reference of every case here; on the rows without NaN or inf it must be torch_ref.contact_dist."""
    if name == "nan_planted":
        pt1, pt2 = gc.planted_inputs()
    else:
        pt1, pt2 = gc.near_inputs(name if name not in ("sweep", "extremes") else name + "@1")[:2]
    n = gc.nan_safe_equals_oracle(pt1, pt2, chunk=4 if name == "table_cap" else 256)
    assert n >= 0.9 * pt1.shape[0] or name in ("extremes", "nan_planted")
    assert n >= 0.75 * pt1.shape[0]


def test_planted_input_of_the_brute_force_search():
    pt1, pt2 = gc.planted_inputs()
    assert pt1.shape == (1000, 3) and pt2.shape == (1025, 3)
    for p, rows in ((pt2, (0, 1, 2, 700, 1023, 1024)), (pt1, (0, 1, 511, 512, 998, 999))):
        assert (~gc.finite_rows(p)).sum() == 6 and not gc.finite_rows(p)[list(rows)].any()
        assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
    dist, idx = gc.dist_expected("nan_planted")
    bad = ~gc.finite_rows(pt1)
    assert (dist[bad] == F32(1e9)).all() and (idx[bad] == 0).all()
    assert (dist[~bad] < 1).all() and not np.isin(idx[~bad], np.flatnonzero(~gc.finite_rows(pt2))).any()
    assert (dist[100:120] == 0).all() and (idx[100:120] == np.arange(100, 120)).all()       # the lower of the two duplicates


# ---------------------------------------------------------------------------------------------------------------------
# C. k nearest rows
# ---------------------------------------------------------------------------------------------------------------------
def test_knn_cases_cover_what_they_must():
    ks, ms, Cs, ns = (set(c[i] for c in gc.KNN_CASES) for i in range(4))
    assert ks == {1, 2, 4, 5, 31, 32} and Cs == {1, 3, 20, 33} and ns == {1, 255, 257}
    assert {1, 255, 256, 257, 778} <= ms
    for k in ks:
        if k > 1:
            assert (k, k - 1) in {(c[0], c[1]) for c in gc.KNN_CASES}, k           # m = k - 1
        assert (k, k) in {(c[0], c[1]) for c in gc.KNN_CASES}, k                   # m = k
    for k in (1, 4, 32):
        assert (k, 257) in {(c[0], c[1]) for c in gc.KNN_CASES}
    assert len(set(gc.KNN_CASES)) == len(gc.KNN_CASES)


@pytest.mark.parametrize("case", gc.KNN_CASES, ids=gc.knn_id)
def test_knn_lattice_is_exact_and_full_of_ties(case):
    k, m, C, n = case
    pts, refs, rows = gc.knn_lattice(case)
    assert pts.shape == (n, 3) and refs.shape == (m, 3) and rows.shape == (m, C)
    for a in (pts, refs):
        assert (a == np.round(a)).all() and np.abs(a).max() <= 64
    assert (rows == np.round(rows)).all() and np.abs(rows).max() <= 8
    idx, mean, d2 = gc.knn_expected(pts, refs, rows, k)
    d = pts[:, None, :] - refs[None, :, :]                                   # float32 throughout
    d32 = np.sort((d * d).sum(-1, dtype=F32), axis=1)
    assert d32.dtype == F32 and (d32.astype(np.float64) == d2).all() and d2.max() < 2 ** 24     # fp32 squared distances are exact
    assert (idx[:, min(k, m):] == -1).all() and (idx[:, :min(k, m)] >= 0).all()
    tie = gc.knn_tie_at_k(d2, k)
    if m > k and n >= 255:
        print("KNN lattice %s: %.1f %% of the queries tie exactly at the k-th place" % (gc.knn_id(case), 100 * tie.mean()))
        assert tie.mean() >= 0.20
    else:
        assert m <= k or n == 1


@pytest.mark.parametrize("case", gc.KNN_CASES, ids=gc.knn_id)
def test_knn_random_inputs_have_next_to_no_near_ties(case):
    k, m, C, n = case
    pts, refs, rows = gc.knn_random(case)
    _, _, d2 = gc.knn_expected(pts, refs, rows, k)
    near, clear = gc.knn_near_tie_at_k(d2, k), gc.knn_clear_order(d2, k)
    print("KNN random %s: %.2f %% near ties at the k-th place, %.1f %% of the rows with a pinned order" % (gc.knn_id(case), 100 * near.mean(), 100 * clear.mean()))
    assert near.mean() < 0.01 and clear.mean() > 0.9
    assert rows.min() >= 0 and rows.max() < 1


def test_knn_far_query_overflows_in_fp32():
    """(1e20, 0, 0) is finite, its fp32 squared distance to anything near the origin is not: no reference beats the kernel's 3e38."""
    with np.errstate(over="ignore"):
        d = F32(1e20) - F32(1.0)
        assert np.isfinite(F32(1e20)) and not (d * d < F32(3.0e38))


# ---------------------------------------------------------------------------------------------------------------------
# D. signed distance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SDF_CASES)
def test_sdf_float32_yardstick(name):
    """The constants the kernel's tolerances are 4 x of: measured again here, float32 numpy against the float64 oracle."""
    s, w = gc.sdf_f32_error(name)
    cs, cw = gc.SDF_F32_ERR[name]
    print("SDF YARDSTICK %s: float32 restatement vs float64 oracle |sdf| %.3e winding %.3e (constants %s, %s)" % (name, s, w, cs, cw))
    assert s <= cs <= 2 * s
    if cw is not None:
        assert w <= cw <= 2 * w
    assert gc.SDF_FACTOR == 4.0


def test_single_triangle_regions_follow_the_closed_forms():
    pts, names = gc.triangle_points()
    sdf, wind = gc.sdf_oracle("triangle")
    want = gc.triangle_closed_form(pts, names)
    np.testing.assert_allclose(np.abs(sdf), want, rtol=0, atol=1e-14)
    assert (sdf < 0).all() and (np.abs(wind) < 0.5).all()                 # one triangle encloses nothing
    for name in gc.TRI_REGIONS:
        z = pts[[i for i, nm in enumerate(names) if nm == name], 2]
        assert (z > 0).sum() >= 3 and (z < 0).sum() >= 3                  # above and below the plane
    assert (np.sign(wind) == -np.sign(pts[:, 2])).all() or (np.sign(wind) == np.sign(pts[:, 2])).all()
    # the regions are the ones named: the closest point of the oracle's region walk is a vertex, on an edge, or inside
    a, b, c = (gc.TRI[i].astype(np.float64)[None] for i in range(3))
    for p, nm in zip(pts.astype(np.float64), names):
        q = R._closest_on_triangle(p, a, b, c)[0]
        bary = np.array([1 - q[0] / 2 - q[1], q[0] / 2, q[1]])           # weights of a, b, c
        zero = np.abs(bary) < 1e-12
        want_zero = {"vertex_a": (0, 1, 1), "vertex_b": (1, 0, 1), "vertex_c": (1, 1, 0), "edge_ab": (0, 0, 1), "edge_bc": (1, 0, 0),
                     "edge_ca": (0, 1, 0), "interior": (0, 0, 0)}[nm]
        assert tuple(int(z_) for z_ in zero) == want_zero, (nm, p, q)


def _edge_counts(faces):
    e = {}
    for f in faces:
        for i in range(3):
            e[(int(f[i]), int(f[(i + 1) % 3]))] = e.get((int(f[i]), int(f[(i + 1) % 3])), 0) + 1
    return e


@pytest.mark.parametrize("name", ["tetrahedron", "box255", "box256", "box257", "box513", "box256_shifted"])
def test_closed_meshes_are_closed_and_the_points_lie_on_both_sides(name):
    c = gc.sdf_case(name)
    nf = c["faces"].shape[0]
    assert nf == {"tetrahedron": 4, "box255": 255, "box256": 256, "box257": 257, "box513": 513, "box256_shifted": 256}[name]
    assert c["points"].shape == (257, 3)
    sdf, wind = gc.sdf_oracle(name)
    assert np.abs(np.abs(wind) - np.round(np.abs(wind))).max() < 1e-9 and set(np.round(np.abs(wind)).tolist()) == {0.0, 1.0}
    inside = float((sdf > 0).mean())
    print("SDF %s: %d faces, %.1f %% of the points inside" % (name, nf, 100 * inside))
    assert 0.20 < inside < 0.80
    e = _edge_counts(c["faces"])
    unpaired = [k for k in e if (k[1], k[0]) not in e]
    splits = {"box255": 3, "box257": 1, "box513": 1}.get(name, 0)
    # a closed, consistently oriented mesh has every directed edge once and its opposite once; each split face leaves its cut
    # diagonal (one edge on the whole side, two halves on the split side) without a partner: 3 directed edges
    assert max(e.values()) == 1 and len(unpaired) == 3 * splits
    if name == "box256_shifted":
        base = gc.sdf_case("box256")
        assert (c["verts"].astype(np.float64) - np.array(gc.SHIFT) == base["verts"]).all()
        assert np.abs(c["points"].astype(np.float64) - np.array(gc.SHIFT) - base["points"]).max() < 1e-6
        assert np.abs(c["verts"]).max() > 10


def test_surface_points_lie_on_the_surface():
    for name in ("surface", "surface_shifted"):
        c = gc.sdf_case(name)
        sdf, _ = gc.sdf_oracle(name)
        assert c["points"].shape == (192, 3) and np.abs(sdf).max() < 1e-14, (name, np.abs(sdf).max())


def test_degenerate_faces_and_their_query_points():
    c = gc.sdf_case("degenerate")
    v, f = c["verts"].astype(np.float64), c["faces"]
    clean, extra = c["ref_faces"], f[c["ref_faces"].shape[0]:]
    assert clean.shape[0] == 256 and extra.shape[0] == 9
    area = np.linalg.norm(np.cross(v[extra[:, 1]] - v[extra[:, 0]], v[extra[:, 2]] - v[extra[:, 0]]), axis=1)
    assert (area == 0).all()
    assert sum(1 for t in extra if t[0] == t[1]) == 3 and sum(1 for t in extra if t[0] == t[2]) == 3
    ce = _edge_counts(clean)
    for t in extra[6:]:
        assert (2 * v[t[1]] == v[t[0]] + v[t[2]]).all() and t[1] > clean.max()     # an exact midpoint, a vertex of its own
        assert (int(t[0]), int(t[2])) in ce or (int(t[2]), int(t[0])) in ce         # on an existing edge
    for t in extra[:6]:
        i, j = int(t[0]), int(t[1] if t[1] != t[0] else t[2])
        assert (i, j) in ce or (j, i) in ce
    # the last 64 points: near the edges' supporting lines, beyond the segment ends
    near = c["points"][-64:].astype(np.float64)
    ok = np.zeros(64, bool)
    for t in extra[6:]:
        a, b = v[t[0]], v[t[2]]
        d = (b - a) / np.linalg.norm(b - a)
        s = (near - a) @ d
        off = np.linalg.norm(near - a - s[:, None] * d, axis=1)
        ok |= ((s < -0.04) | (s > np.linalg.norm(b - a) + 0.04)) & (off < 4e-3)
    assert ok.all()
    sdf, wind = gc.sdf_oracle("degenerate")
    assert np.isfinite(sdf).all() and np.isfinite(wind).all() and 0.2 < (sdf > 0).mean() < 0.8
    with np.errstate(all="ignore"):
        raw, _ = R.mesh_sdf(c["points"][:8], c["verts"], c["faces"])
    print("SDF degenerate: the oracle on the degenerate mesh itself gives %s" % raw[:4])   # why the reference is the clean mesh


def test_open_cube_has_a_hole_and_points_around_it():
    c = gc.sdf_case("open_cube")
    e = _edge_counts(c["faces"])
    boundary = [k for k in e if (k[1], k[0]) not in e]
    assert c["faces"].shape[0] == 10 and len(boundary) == 4 and {i for k in boundary for i in k} == {4, 5, 6, 7}
    sdf, wind = gc.sdf_oracle("open_cube")
    clear = np.abs(np.abs(wind) - 0.5) > gc.SDF_CLEAR
    near_hole = np.linalg.norm(c["points"] - np.array([0.5, 0.5, 1.0]), axis=1) < 0.55
    print("SDF open cube: %.1f %% inside, %.1f %% clear of |w| = 1/2, %d points near the hole, winding %.3f .. %.3f"
          % (100 * (sdf > 0).mean(), 100 * clear.mean(), int(near_hole.sum()), np.abs(wind).min(), np.abs(wind).max()))
    assert clear.mean() > 0.9 and near_hole.sum() >= 97 and (~near_hole).sum() >= 100
    assert 0.1 < (sdf > 0).mean() < 0.8
    assert ((np.abs(wind) > 0.05) & (np.abs(wind) < 0.95)).mean() > 0.2        # an open mesh: fractional winding numbers


def test_empty_mesh_constant():
    assert gc.SDF_EMPTY == -float(np.sqrt(F32(3.0e38))) and -1.8e19 < gc.SDF_EMPTY < -1.7e19

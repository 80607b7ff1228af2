"""GPU: the geometry kernels at thresholds, seams and k routes (tests/geometry_cases.py; the cases' conditions are proved on the
references in tests/test_geometry_cases_cpu.py).

  mgr_contact_near   bit for bit against contact_oracle.near_reference over nearest_nan_safe -- value for every row, index and
                     distance where value > 0, -1 / 1e9 elsewhere -- and the same bits from a second run: thresholds from 1e-5 to
                     1, targets on cell borders with queries at distance c and one fp32 either side, a 1024-bucket table under
                     1.6e7 cells, coordinates up to +-inf and NaN, 2.3 M targets at the 2^22 table cap
  mgr_contact_dist   bit for bit against nearest_nan_safe on the extreme coordinates and a NaN / inf planted (1000, 1025) input,
                     through get_contact_dist and get_contact_map; a CPU pt2 is rejected
  mgr_knn_mean_rows  k = 1 and k = 4 (their own kernels) and 2, 5, 31, 32 (the generic one) at m around k and around the 256-row
                     tile: exact indices and 2^-22 means on an integer lattice full of exact ties, the MANO test's near-tie rule
                     on random points; a query without any neighbour (all squared distances overflow, or m = 0) gets -1 / NaN
  mgr_mesh_sdf       one triangle against closed forms per Voronoi region, closed boxes of 255 / 256 / 257 / 513 faces and a
                     tetrahedron, points on the surface, degenerate faces, an open cube, a box at (10, -7, 3), no faces; held to 4 x
                     the distance of a float32 numpy evaluation of the oracle's formulas from the float64 oracle
                     (geometry_cases.SDF_F32_ERR, measured on the CPU)"""
import numpy as np
import pytest
import torch

import geometry_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# A. mgr_contact_near
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.NEAR_CASES)
def test_near_search_equals_the_reference_bit_for_bit(name):
    from manus_amd.contact import contact_near
    pt1, pt2, c = gc.near_inputs(name)
    ref_v, ref_i, ref_d = gc.near_expected(name)
    a, b = dev(pt1), dev(pt2)
    first, second = contact_near(a, b, c, want_dist=True), contact_near(a, b, c, want_dist=True)
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))            # run to run: the same bits
    value, idx, dist = host(first[0]), host(first[1]).astype(np.int64), host(first[2])
    hit = ref_v > 0
    print("GPU NEAR %s: %d x %d, %d queries in contact" % (name, pt1.shape[0], pt2.shape[0], int(hit.sum())))
    np.testing.assert_array_equal(bits(value), bits(ref_v))
    np.testing.assert_array_equal(idx[hit], ref_i[hit])
    np.testing.assert_array_equal(bits(dist[hit]), bits(ref_d[hit]))
    assert (idx[~hit] == -1).all() and (dist[~hit] == F32(1e9)).all()
    if name == "borders":
        cls = gc.border_inputs()[3]
        assert (value[cls == gc.BELOW] > 0).all() and (value[cls != gc.BELOW] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# B. mgr_contact_dist
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.DIST_CASES))
def test_brute_force_search_defines_nan_and_inf_like_the_loop(name):
    from manus_amd.contact import get_contact_dist, get_contact_map
    pt1, pt2 = gc.DIST_CASES[name]()
    rd, ri = gc.dist_expected(name)
    a, b = dev(pt1), dev(pt2)
    dist, idx = get_contact_dist(a, b)
    assert idx.dtype == torch.float32
    np.testing.assert_array_equal(bits(host(dist)), bits(rd))
    np.testing.assert_array_equal(host(idx).astype(np.int64), ri)
    np.testing.assert_array_equal(bits(host(get_contact_map(a, b))), bits(rd))
    print("GPU DIST %s: %d of %d queries without a nearest point (1e9, index 0)" % (name, int((rd == F32(1e9)).sum()), rd.shape[0]))


def test_brute_force_search_rejects_cpu_tensors():
    from manus_amd._lib import ManusHipError
    from manus_amd.contact import get_contact_dist, get_contact_map
    on, off = torch.zeros((4, 3), device=DEV), torch.zeros((5, 3))
    for fn in (get_contact_dist, get_contact_map):
        with pytest.raises(ManusHipError, match="no CPU fallback"):
            fn(on, off)
        with pytest.raises(ManusHipError, match="no CPU fallback"):
            fn(off, on)
        with pytest.raises(ManusHipError, match="no CPU fallback"):
            fn(on, torch.zeros((0, 3)))


# ---------------------------------------------------------------------------------------------------------------------
# C. mgr_knn_mean_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.KNN_CASES, ids=gc.knn_id)
def test_knn_on_the_integer_lattice_is_exact(case):
    """Exact distances, exact ties: the indices are the stable argsort's (the lowest index among equals, nearest first), -1 past
    m; the mean is the exact row sum times the rounded 1 / min(k, m)."""
    from manus_amd import mano_init as MI
    k, m, C, n = case
    pts, refs, rows = gc.knn_lattice(case)
    want_idx, want_mean, _ = gc.knn_expected(pts, refs, rows, k)
    out, idx = MI.knn_mean_rows(dev(pts), dev(refs), dev(rows), k, want_idx=True)
    assert tuple(out.shape) == (n, C) and tuple(idx.shape) == (n, k) and idx.dtype == torch.int32
    np.testing.assert_array_equal(host(idx).astype(np.int64), want_idx)
    err = np.abs(host(out).astype(np.float64) - want_mean)
    assert (err <= gc.KNN_MEAN_RTOL * np.abs(want_mean)).all(), float((err / np.maximum(np.abs(want_mean), 1e-300)).max())
    assert torch.equal(MI.knn_mean_rows(dev(pts), dev(refs), dev(rows), k), out)          # the same without the index output


@pytest.mark.parametrize("case", gc.KNN_CASES, ids=gc.knn_id)
def test_knn_on_random_points_follows_the_near_tie_rule(case):
    """The rule of test_nearest_vertex_weights_equal_the_reference: a row may differ only where the k-th and (k+1)-th float64
    squared distances are within a relative 1e-5; where no two neighbouring distances are that close the order is the oracle's."""
    from manus_amd import mano_init as MI
    k, m, C, n = case
    pts, refs, rows = gc.knn_random(case)
    want_idx, want_mean, d2 = gc.knn_expected(pts, refs, rows, k)
    near_tie, clear = gc.knn_near_tie_at_k(d2, k), gc.knn_clear_order(d2, k)
    out, idx = MI.knn_mean_rows(dev(pts), dev(refs), dev(rows), k, want_idx=True)
    idx = host(idx).astype(np.int64)
    off = np.abs(host(out).astype(np.float64) - want_mean).max(1) > gc.knn_random_atol(k)
    assert not (off & ~near_tie).any(), int((off & ~near_tie).sum())
    assert off.mean() < 0.01
    same = (np.sort(idx, 1) == np.sort(want_idx, 1)).all(1)
    assert not (~same & ~near_tie).any()
    assert (idx == want_idx)[clear].all()                                                 # nearest first
    assert (idx[:, min(k, m):] == -1).all()


@pytest.mark.parametrize("k", [1, 4, 5])
def test_knn_query_without_neighbours_gets_no_index_and_nan(k):
    """No neighbour -- every fp32 squared distance overflows past the kernel's 3e38, or there are no references at all --
    is what a non-finite query already is: indices -1, mean NaN (not index 0 k times / rows[0], not a finite 0).  The queries
    beside it in the workgroup are untouched."""
    from manus_amd import mano_init as MI
    case = (k, 257, 3, 257)
    pts, refs, rows = gc.knn_random(case)
    pts = pts.copy()
    pts[7] = (1e20, 0.0, 0.0)
    pts[200] = (0.0, -1e20, 1e20)
    want_idx, want_mean, _ = gc.knn_expected(pts, refs, rows, k)
    out, idx = MI.knn_mean_rows(dev(pts), dev(refs), dev(rows), k, want_idx=True)
    out, idx = host(out), host(idx).astype(np.int64)
    far = np.zeros(257, bool)
    far[[7, 200]] = True
    assert (idx[far] == -1).all(), idx[far]
    assert np.isnan(out[far]).all(), out[far]
    assert (idx[~far] == want_idx[~far]).all()
    np.testing.assert_allclose(out[~far], want_mean[~far], rtol=0, atol=gc.knn_random_atol(k))
    # m = 0
    out, idx = MI.knn_mean_rows(dev(pts[:5]), torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV), k, want_idx=True)
    assert tuple(out.shape) == (5, 3) and tuple(idx.shape) == (5, k)
    assert (host(idx) == -1).all(), host(idx)
    assert np.isnan(host(out)).all(), host(out)


# ---------------------------------------------------------------------------------------------------------------------
# D. mgr_mesh_sdf
# ---------------------------------------------------------------------------------------------------------------------
def run_sdf(name, n=None):
    from manus_amd import mano_init as MI
    c = gc.sdf_case(name)
    pts = c["points"] if n is None else c["points"][:n]
    sdf, wind = MI.mesh_sdf(dev(pts), dev(c["verts"]), torch.tensor(c["faces"], device=DEV), want_winding=True)
    return host(sdf), host(wind)


def check_against_oracle(name, sdf, wind, ref=None):
    """|sdf| and the winding number within the case's tolerance of the float64 oracle, the sign wherever the oracle's |winding| is
    clear of 1/2, nothing NaN."""
    ref_s, ref_w = gc.sdf_oracle(name)
    n = sdf.shape[0]
    ref_s, ref_w = ref_s[:n], ref_w[:n]
    want = np.abs(ref_s) if ref is None else ref[:n]
    atol_s, atol_w = gc.sdf_tolerance(name)
    es, ew = np.abs(np.abs(sdf.astype(np.float64)) - want).max(), np.abs(wind.astype(np.float64) - ref_w).max()
    print("GPU SDF %s n = %d: |sdf| error %.3e (tolerance %.3e), winding error %.3e (tolerance %.3e)" % (name, n, es, atol_s, ew, atol_w))
    assert np.isfinite(sdf).all() and np.isfinite(wind).all()
    assert es <= atol_s, (es, atol_s)
    assert ew <= atol_w, (ew, atol_w)
    clear = np.abs(np.abs(ref_w) - 0.5) > gc.SDF_CLEAR
    assert (np.sign(sdf) == np.sign(ref_s))[clear].all()


def test_sdf_single_triangle_regions_against_closed_forms():
    pts, names = gc.triangle_points()
    sdf, wind = run_sdf("triangle")
    check_against_oracle("triangle", sdf, wind, ref=gc.triangle_closed_form(pts, names))
    assert (sdf < 0).all()


@pytest.mark.parametrize("n", [257, 1])
@pytest.mark.parametrize("name", ["tetrahedron", "box255", "box256", "box257", "box513"])
def test_sdf_closed_meshes_at_the_tile_seams(name, n):
    sdf, wind = run_sdf(name, n)
    check_against_oracle(name, sdf, wind)
    if n > 1:
        assert 0.2 < (sdf > 0).mean() < 0.8


@pytest.mark.parametrize("name", ["surface", "surface_shifted"])
def test_sdf_points_on_the_surface(name):
    """Vertices, edge midpoints and face centroids: |sdf| within tolerance of 0 and every output finite; the sign is left open
    (the winding number jumps across the surface)."""
    sdf, wind = run_sdf(name)
    atol_s, _ = gc.sdf_tolerance(name)
    print("GPU SDF %s: max |sdf| %.3e (tolerance %.3e); vertices %.3e, midpoints %.3e, centroids %.3e"
          % (name, np.abs(sdf).max(), atol_s, np.abs(sdf[:64]).max(), np.abs(sdf[64:128]).max(), np.abs(sdf[128:]).max()))
    assert np.isfinite(sdf).all() and np.isfinite(wind).all()
    assert np.abs(sdf).max() <= atol_s


def test_sdf_degenerate_faces_change_nothing():
    """Zero-area faces (i, i, j), (i, j, i) and (a, mid, b) appended to the 256-face box: the result is the clean mesh's (the
    oracle on the clean mesh: on a degenerate face it divides 0 by 0 like the kernel, and its min() keeps the NaN)."""
    sdf, wind = run_sdf("degenerate")
    check_against_oracle("degenerate", sdf, wind)


def test_sdf_open_cube():
    sdf, wind = run_sdf("open_cube")
    check_against_oracle("open_cube", sdf, wind)
    assert ((np.abs(wind) > 0.05) & (np.abs(wind) < 0.95)).mean() > 0.2


def test_sdf_translated_box():
    sdf, wind = run_sdf("box256_shifted")
    check_against_oracle("box256_shifted", sdf, wind)


def test_sdf_of_a_mesh_without_faces_is_pinned():
    """nf = 0: -sqrt(3e38) (the kernel's 'no face yet' squared distance, rooted; outside) and winding 0, with or without vertices."""
    from manus_amd import mano_init as MI
    pts = dev(gc.sdf_case("tetrahedron")["points"])
    for verts in (dev(gc.tetrahedron()[0]), torch.zeros((0, 3), device=DEV)):
        sdf, wind = MI.mesh_sdf(pts, verts, torch.zeros((0, 3), dtype=torch.int64, device=DEV), want_winding=True)
        np.testing.assert_allclose(host(sdf), gc.SDF_EMPTY, rtol=2.0 ** -23, atol=0)         # one rounded root
        assert (host(wind) == 0).all()

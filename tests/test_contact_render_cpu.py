"""CPU: the contact-map fixture (tests/golden/contact_cmap.npz, written by tests/golden/make_contact_golden.py from the
reference's get_colors_from_cmap / calculate_colors_from_sh), the colour tables, the numpy restatements the GPU tests
compare against, and the C ABI of the new entries."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import contact_oracle as co
from oracle import torch_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMAPS = ("magma", "gray", "viridis")
NEW_SYMBOLS = ("mgr_contact_near_workspace_bytes", "mgr_contact_near", "mgr_contact_values", "mgr_contact_colors")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "contact_cmap.npz"))


def test_fixture_luts_equal_matplotlib(fx):
    matplotlib = pytest.importorskip("matplotlib")
    for name in CMAPS:
        ref = matplotlib.colormaps[name](np.arange(256))[:, :3].astype(np.float32)
        np.testing.assert_array_equal(fx["lut_" + name], ref)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(fx["colors_" + name], matplotlib.colormaps[name](fx["values"])[:, :3].astype(np.float32))


def test_lut_gray_without_matplotlib_and_names_need_it(fx, monkeypatch):
    from manus_amd import colormap
    from manus_amd._lib import ManusHipError
    monkeypatch.setattr(colormap, "_CACHE", {})
    monkeypatch.setitem(sys.modules, "matplotlib", None)          # `import matplotlib` now raises ImportError
    t = colormap.lut("gray", "cpu")
    assert t.dtype.is_floating_point and tuple(t.shape) == (256, 3)
    np.testing.assert_array_equal(t.numpy(), fx["lut_gray"])
    with pytest.raises(ManusHipError, match=r"\(256,3\)"):
        colormap.lut("magma", "cpu")
    np.testing.assert_array_equal(colormap.lut(fx["lut_magma"], "cpu").numpy(), fx["lut_magma"])   # a table needs no matplotlib
    with pytest.raises(ManusHipError):
        colormap.lut(np.zeros((255, 3), np.float32), "cpu")


def test_lut_names_resolve_through_matplotlib(fx, monkeypatch):
    pytest.importorskip("matplotlib")
    from manus_amd import colormap
    monkeypatch.setattr(colormap, "_CACHE", {})
    for name in CMAPS:
        np.testing.assert_array_equal(colormap.lut(name, "cpu").numpy(), fx["lut_" + name])
    assert colormap.lut("magma", "cpu") is colormap.lut("magma", "cpu")     # cached per name and device


def test_lookup_restatement_equals_reference_colours(fx):
    """The numpy lookup the GPU tests use (min(int(v * 256), 255), 0 below, 255 from 1.0 up, black for NaN) gives the
    colours the reference's get_colors_from_cmap recorded, on the edge values and 3000 random ones."""
    v = fx["values"]
    assert np.isnan(v).any() and np.isinf(v).any() and (v < 0).any() and (v > 1).any() and (v == 1).any()
    assert len(np.unique(co.lut_index(v))) == 257                 # every entry and the bad colour
    for name in CMAPS:
        np.testing.assert_array_equal(co.lut_colors(v, fx["lut_" + name]), fx["colors_" + name])


@pytest.mark.parametrize("k", [0, 1])
def test_scene_restatements_equal_fixture(fx, k):
    """Near-search contract (brute force + mask) on the fixture scenes against oracle.torch_ref.contact_dist, the value
    formula, and the colour choice of every render type restated from the recorded dist / indices."""
    s = lambda name: fx["s%d_%s" % (k, name)]
    for a, b, pre in ((s("h_posed_xyz"), s("o_xyz"), "h"), (s("o_xyz"), s("h_posed_xyz"), "o")):
        rd, ri = tr.contact_dist(a, b)
        np.testing.assert_array_equal(rd, s(pre + "_dist"))
        np.testing.assert_array_equal(ri, s(pre + "_idx"))
        value, idx, dist = co.near_reference(a, b)
        np.testing.assert_array_equal(value, s(pre + "_value"))     # numpy division == the fixture's float32 torch division
        hit = value > 0
        assert 0.15 < hit.mean() < 0.9
        np.testing.assert_array_equal(idx[hit], ri[hit])
        np.testing.assert_array_equal(dist[hit], rd[hit])
        assert (idx[~hit] == -1).all() and (dist[~hit] == np.float32(1e9)).all()
        d2, i2 = co.nearest_nan_safe(a, b)                           # the NaN-safe loop is the oracle where nothing is NaN
        np.testing.assert_array_equal(d2, rd)
        np.testing.assert_array_equal(i2, ri)
    magma, gray, nocs = fx["lut_magma"], fx["lut_gray"], s("nocs_grid")
    hv, ov = s("h_value"), s("o_value")
    np.testing.assert_array_equal(co.blend(s("rgb_object"), co.lut_colors(ov, magma), 0.3), s("colors_object_only"))
    np.testing.assert_array_equal(co.blend(s("rgb_hand"), co.lut_colors(hv, magma), 0.3), s("colors_hand_only"))
    np.testing.assert_array_equal(co.blend(s("rgb_hand"), co.lut_colors(s("acc_dist"), magma), 0.3), s("colors_accumulated"))
    np.testing.assert_array_equal(co.lut_colors(s("acc_dist"), gray), s("colors_acc_gt_eval"))
    np.testing.assert_array_equal(np.where(hv[:, None] > 0, nocs, 0).astype(np.float32), s("colors_nocs_hand_only"))
    np.testing.assert_array_equal(np.where(ov[:, None] > 0, nocs[np.maximum(s("o_idx"), 0)], 0).astype(np.float32),
                                  s("colors_nocs_object_only"))
    np.testing.assert_array_equal(s("skin_colors"), s("colors_skin_wts"))
    assert (s("acc_dist") > 1).any()                                 # a sum over frames leaves [0,1]: the top entry


def test_nan_points_are_nobodys_neighbour():
    pt1 = np.array([[0, 0, 0], [np.nan, 0, 0], [0.001, 0, 0]], np.float32)
    pt2 = np.array([[np.nan, 0, 0], [0.002, 0, 0], [0, np.nan, 0]], np.float32)
    dist, idx = co.nearest_nan_safe(pt1, pt2)
    np.testing.assert_array_equal(dist, np.array([0.002, 1e9, 0.001], np.float32))
    np.testing.assert_array_equal(idx, [1, 0, 1])
    value, nidx, _ = co.near_reference(pt1, pt2, nearest=co.nearest_nan_safe)
    np.testing.assert_array_equal(value, np.array([0.5, 0.0, 0.75], np.float32))
    np.testing.assert_array_equal(nidx, [1, -1, 1])


def test_new_symbols_declared_bound_and_exported():
    from manus_amd import _lib
    from manus_amd.build import build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mgr_[a-z0-9_]+)\s*\(", hdr))
    build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert n in _lib.SIGNATURES, n
        assert hasattr(L, n), n
    assert len(_lib.SIGNATURES["mgr_contact_near"][1]) == 11 and len(_lib.SIGNATURES["mgr_contact_colors"][1]) == 11


def test_python_surface_exists():
    from manus_amd import contact, modules
    for name in ("get_cmap", "get_cmap_near", "get_colors_from_cmap", "contact_near", "contact_colors"):
        assert callable(getattr(contact, name))
    for name in ("composite_pred", "render_contacts", "contact_render_inputs", "CompositeRenderer"):
        assert callable(getattr(modules, name))
    assert set(modules.RENDER_TYPES) == {"object_only", "hand_only", "nocs_hand_only", "nocs_object_only", "accumulated",
                                         "acc_gt_eval", "skin_wts"}

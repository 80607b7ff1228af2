"""CPU: the input conditions of tests/test_gpu_fused_shapes.py (tests/fused_shapes.py).  Nothing here runs a kernel: these
tests prove on the scalar oracle that every named case is what the GPU tests say it is -- its number of k_inst_fwd ranges, its
tile grid, its articulated / static cut, what every view sees -- that the empty views ARE empty (turned-round cameras, every
opacity below 1/255, everything at or inside the near plane), and they measure how far the fp32 oracle's own projection lies
from the fp64 oracle's at these image sizes: the yardstick of the one bar of assert_north_star that scales with the width."""
import numpy as np
import pytest

import fused_shapes as fs
import regimes as rg


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fs.case_scene(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", fs.NONEMPTY + fs.EMPTY)
def test_case_is_what_it_is_named_for(scenes, name):
    sc = scenes(name)
    c = fs.spec(name)
    facts = [fs.view_facts(sc, v) for v in range(c["views"])]
    fs.assert_case(name, facts, sc, "cpu")
    print("CASE", name, fs.conditions(name), "visible", [f["n_visible"] for f in facts], "pairs", [f["num_rendered"] for f in facts],
          "max tiles", [f["max_tiles_touched"] for f in facts])


def test_conditions_follow_the_block_mapping():
    """The numbers the case table quotes, from the definitions alone."""
    assert fs.conditions("one")["padded"] == 8 and fs.conditions("nine_ranges")["padded"] == 16
    assert [fs.conditions(n)["nrange"] for n in ("one", "subwave_tile", "below_a_tile", "nine_ranges", "mixed_cut", "object_odd")] == [1, 1, 2, 9, 10, 1]
    cut = fs.conditions("mixed_cut")
    assert cut["n_art"] == 2765 and cut["n_art_mod64"] != 0 and cut["n_art"] % fs.RANGE_ROWS != 0
    assert {fs.conditions(n)["w_mod4"] for n in fs.NONEMPTY} == {0, 1, 2, 3}      # both branches of the fill / loss kernels, every remainder
    assert len(fs.NONEMPTY) == 12 and len(fs.EMPTY) == 6


@pytest.mark.parametrize("name", ["empty_first", "empty_middle", "empty_last", "empty_all"])
def test_turned_round_cameras_keep_their_position_and_see_nothing(scenes, name):
    sc, full = scenes(name), scenes("nine_ranges")
    target = fs.scene_target()
    for v in range(3):
        a, b = sc["cameras"][v], full["cameras"][v]
        np.testing.assert_allclose(a["camera_center"], b["camera_center"], atol=1e-12)
        fwd = np.asarray(a["extr"])[2, :3]
        toward = (target - np.asarray(a["camera_center"])) / np.linalg.norm(target - np.asarray(a["camera_center"]))
        if v in fs.spec(name)["away"]:
            np.testing.assert_allclose(fwd, -toward, atol=1e-12)
            _, _, z = rg.raster_oracle_of_view(sc, v)
            assert float(z.max()) < 0.0                      # the whole scene lies behind the camera
        else:
            np.testing.assert_allclose(fwd, toward, atol=1e-12)
            assert np.array_equal(a["full_proj_transform"], b["full_proj_transform"])


def test_appended_away_cameras_are_views_of_their_own(scenes):
    """The scene of the step sequences: views 3, 4, 5 are views 0, 1, 2 turned round, with their poses; 0, 1, 2 are untouched."""
    sc = fs.case_scene("nine_ranges", extra_away=True)
    assert len(sc["cameras"]) == 6 and sc["posed"].shape[0] == 6 and sc["transforms"].shape[0] == 6
    assert [fs.view_facts(sc, v)["n_visible"] for v in (3, 4, 5)] == [0, 0, 0]
    assert [fs.view_facts(sc, v)["n_visible"] for v in range(3)] == [fs.view_facts(scenes("nine_ranges"), v)["n_visible"] for v in range(3)]


def test_faint_rows_of_the_oracle_are_zero(scenes):
    """faint_all: every Gaussian keeps a radius and appears in no list; the oracle's gradient rows are all zero."""
    sc = scenes("faint_all")
    c = fs.spec("faint_all")
    g = np.random.default_rng(7).normal(size=(3, c["H"], c["W"])).astype(np.float32)
    for v in range(c["views"]):
        ro, inp, _ = rg.raster_oracle_of_view(sc, v)
        assert (inp["op"] < np.float32(1.0) / np.float32(255.0)).all() and (ro.radii > 0).any()
        assert np.array_equal(ro.color, np.ones_like(ro.color))
        assert rg.oracle_rows_zero(ro.backward(g), np.ones(c["n"], bool))
        ro.close()


@pytest.mark.parametrize("name", fs.NONEMPTY)
def test_fp32_oracle_projection_against_fp64(scenes, name):
    """The fp32 oracle's own pixel centres and conics against the fp64 oracle's, per case: what assert_north_star's
    proj_pix < 1.1e-6 * width (measured at 1920 px) is to be read against at 7 to 200 px."""
    c = fs.spec(name)
    pix, con = fs.projection_yardstick(scenes(name), c["views"])
    print("YARDSTICK %s W %d: fp32 oracle vs fp64 oracle pix %.3e (bar %.3e) conic %.3e" % (name, c["W"], pix, 1.1e-6 * c["W"], con))
    assert pix < 1e-3 and con < 1e-4       # the fp32 oracle is itself a valid reference at the project's bars

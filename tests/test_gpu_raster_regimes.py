"""GPU: the rasterizer against the oracle on scenes in the regimes training leaves them in (tests/regimes.py): saturated
opacities, the state after reset_opacity, Gaussians below 1/255, exact clones with equal depth keys, 10 : 1 needles, and
a close-up rig with part of the hand inside the near plane.  The scenes lie IN the regimes, not on the thresholds; the
threshold decisions that do occur are handled by the flip accounting of tests/fused_oracle.py, and everything is judged
at the bars the project already uses: assert_north_star on the fused route, bit-exact integer state on the operator
route, the bars of test_fused_equals_modular between the two.

Every test first asserts, on the oracle's side and per view, that its scene IS in its regime (regimes.CONDITIONS): a
scene that drifts out of its regime fails the test instead of passing quietly.  All cases of other kinds, view counts
and seeds than the ones the conditions were measured on (hand, seeds 1 and 2, three views) meet them as they are: no
seed or camera radius had to be changed.  Needles beyond 10 : 1 are left out on purpose: at 30 : 1 the fp32 oracle is
itself 2.4e-4 from the fp64 oracle, so two fp32 chains compared at 1e-4 would say nothing.

The needles are why project_backward (csrc/instance_math.h) evaluates the three sums of d(cov2D) in double: in fp32 the
fused route's `_scaling` gradient was 1.9e-4 from the oracle chain at seed 1 (3.5e-5 at seed 2) with no threshold decision
involved; it is 4e-6 now.  The measured deviations of every case are in DESIGN.md section 3."""
import numpy as np
import pytest

import regimes as rg
from fused_oracle import assert_north_star, run_fused_vs_oracle
from test_gpu_fused import check_fused_equals_modular, check_fused_run_to_run_determinism
from test_gpu_raster import _binning, _check_lists_vs_oracle, _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HAND = list(rg.REGIMES)

# (kind, views, seed, regime): (a) of the issue.  Clones are never drawn across the hand / object boundary of a composite
# scene (a copied row would change kind there and stop being a depth tie): composite scenes are not cloned at all.
FUSED_CASES = ([("hand", 3, seed, name) for seed in (1, 2) for name in HAND]
               + [("composite", 3, 1, name) for name in ("saturated", "post_reset", "faint")]
               + [("object", 2, 1, name) for name in ("saturated", "cloned")]
               + [("hand", 8, 1, "saturated")])


def _report(tag, res):
    """One line per case, the figures DESIGN.md's table of regime deviations holds."""
    print("REGIME", tag, "img_max %.2e sums9 %.2e" % (res["img_max"], res["sums9"]),
          " ".join("%s %.1e" % (k, e) for k, e in res["grads"].items()),
          "ambiguous %d flipped %d stop-flipped %d" % (res["ambiguous"], res["flips"], res["stop_flips"]))


@pytest.mark.parametrize("kind,views,seed,name", FUSED_CASES, ids=lambda x: str(x))
def test_fused_matches_oracle_in_regime(kind, views, seed, name):
    """(a) The fused route against the oracle on identical blend inputs, threshold flips accounted for."""
    S = rg.SHAPE
    res = run_fused_vs_oracle(kind, views, S["n"], S["W"], S["H"], seed, grid_res=S["grid_res"], mutate=rg.mutator(name, seed),
                              **rg.rig(name))
    tag = (kind, views, seed, name)
    assert len(res["regime"]) == views
    rg.assert_in_regime(name, res["regime"], tag)
    if name == "faint":
        assert all(f["oracle_faint_rows_zero"] for f in res["regime"]), tag
    _report(tag, res)
    assert_north_star(res, tag)


@pytest.mark.parametrize("name", HAND)
def test_operator_route_integer_state_in_regime(name):
    """(b) rasterize_views on view 0 of each hand regime, inputs from the torch restatement on the CPU: radii, header pair
    count and tile lists are the oracle's, bit for bit and in the oracle's order (for `cloned`: the index tie-break across
    a third of all adjacent entries), minus pairs proven null.  A Gaussian below 1/255 keeps its radius and its share of
    the pair count and appears in no list; its gradient rows, and those of a Gaussian culled at the near plane, are
    exactly zero."""
    sc = rg.regime_scene(name, "hand", 1)
    S = rg.SHAPE
    cam = sc["cameras"][0]
    ro, inp, z = rg.raster_oracle_of_view(sc, 0)
    rg.assert_in_regime(name, rg.regime_facts(ro, inp["op"], cam, z), name)
    g = np.random.default_rng(11).normal(size=(1, 3, S["H"], S["W"])).astype(np.float32)
    is_faint = inp["op"] < np.float32(1.0) / np.float32(255.0)
    near = z <= np.float32(0.2)
    if name == "faint":
        assert rg.oracle_rows_zero(ro.backward(g[0]), is_faint)
    h = _hip([cam], inp["m"], inp["cov"], inp["col"], inp["op"], grad_img=g)
    assert (h["radii"][0] == ro.radii).all()
    npairs, ranges, pl = _binning(0, 1, S["n"], S["W"], S["H"])
    assert npairs == ro.num_rendered
    n_null = _check_lists_vs_oracle(ro, ranges, pl, S["W"], S["H"])
    listed = pl[: int(ranges[:, 1].max())]
    if name == "faint":
        assert (ro.radii[is_faint] > 0).sum() > S["n"] // 4 and not is_faint[listed].any()
    if name in ("closeup", "saturated_closeup"):
        assert near.sum() >= 300 and not (ro.radii[near] > 0).any()
    dead = is_faint | near
    for k in ("means3D", "cov3D", "colors", "opacity"):
        assert not h[k][dead].any(), (name, k)
    assert not h["means2D"][0][dead].any(), name
    print("REGIME operator", name, "pairs", npairs, "null-culled", n_null, "listed", len(listed))
    ro.close()


def _hand_scene_in_regime(name):
    """The CPU hand scene of a regime at seed 1, every view checked against the regime's conditions on the oracle."""
    sc = rg.regime_scene(name, "hand", 1)
    for v in range(rg.SHAPE["views"]):
        ro, inp, z = rg.raster_oracle_of_view(sc, v)
        rg.assert_in_regime(name, rg.regime_facts(ro, inp["op"], sc["cameras"][v], z), (name, v))
        ro.close()
    return sc


@pytest.mark.parametrize("name", HAND)
def test_fused_equals_modular_in_regime(name):
    """(c) test_gpu_fused.py::test_fused_equals_modular, with its bars, on each hand regime."""
    sc = _hand_scene_in_regime(name)
    from manus_amd.synthetic import camera_table
    check_fused_equals_modular(rg.to_device(sc, DEV), camera_table(sc["cameras"], DEV))


@pytest.mark.parametrize("name", ["saturated_closeup", "cloned"])
def test_fused_run_to_run_determinism_in_regime(name):
    """(c) test_fused_run_to_run_determinism's bitwise check where every covered pixel stops early, and where a third of
    the adjacent list entries tie in depth."""
    sc = _hand_scene_in_regime(name)
    from manus_amd.synthetic import camera_table
    check_fused_run_to_run_determinism(rg.to_device(sc, DEV), camera_table(sc["cameras"], DEV), rg.SHAPE["views"])

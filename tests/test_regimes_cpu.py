"""CPU: the regime scenes of tests/regimes.py are in their regimes.  The mutations do what they say to the leaves, and
`regime_facts` of the scalar oracle meets regimes.CONDITIONS on every view of the hand scene at seeds 1 and 2 -- the
table the GPU tests (tests/test_gpu_raster_regimes.py) rest on, checkable without a GPU."""
import math

import numpy as np
import pytest
import torch

import regimes as rg


def _plain(seed, rig_of="saturated"):
    from manus_amd.synthetic import make_scene
    S = rg.SHAPE
    return make_scene(n_gaussians=S["n"], kind="hand", seed=seed, grid_res=S["grid_res"], n_cameras=S["views"], width=S["W"],
                      height=S["H"], device="cpu", **rg.rig(rig_of))


def test_mutations_do_what_they_say():
    from oracle import torch_ref as tr
    base = _plain(1)["params"]
    n = rg.SHAPE["n"]
    mut = lambda name: rg.regime_scene(name, "hand", 1)["params"]
    p = mut("saturated")
    assert torch.equal(p["_opacity"], base["_opacity"] + 6.0)
    assert all(torch.equal(p[k], base[k]) for k in base if k != "_opacity")
    p = mut("post_reset")
    assert torch.equal(p["_opacity"], tr.reset_opacity(dict(opacity=base["_opacity"]))["opacity"])
    assert float(torch.sigmoid(p["_opacity"]).max()) <= float(np.nextafter(np.float32(0.01), np.float32(1.0)))
    p = mut("faint")
    assert (p["_opacity"][::3] == -6.5).all() and float(torch.sigmoid(p["_opacity"][::3]).max()) < 1.0 / 255.0
    keep = torch.ones(n, dtype=torch.bool)
    keep[::3] = False
    assert torch.equal(p["_opacity"][keep], base["_opacity"][keep])
    p = mut("needles")
    h = 0.5 * math.log(10.0)
    assert torch.equal(p["_scaling"][:, 0], base["_scaling"][:, 0] + h) and torch.equal(p["_scaling"][:, 1:], base["_scaling"][:, 1:] - h)
    # cloned: the last third of EVERY leaf copies rows of the first two thirds, the same source row in every leaf
    p = mut("cloned")
    n_src = n - n // 3
    src = None
    for k in base:
        assert torch.equal(p[k][:n_src], base[k][:n_src]), k
    eq = (p["_xyz"][n_src:, None, :] == base["_xyz"][None, :n_src, :]).all(-1)
    assert (eq.sum(1) == 1).all()
    src = eq.float().argmax(1)
    for k in base:
        assert torch.equal(p[k][n_src:], base[k][src]), k
    # ... within a range only: rows outside it are untouched, sources come from inside it
    q = {k: v.clone() for k, v in base.items()}
    rg.cloned(q, torch.Generator().manual_seed(3), lo=900, hi=2400)
    for k in base:
        assert torch.equal(q[k][:1900], base[k][:1900]) and torch.equal(q[k][2400:], base[k][2400:]), k
    eq = (q["_xyz"][1900:2400, None, :] == base["_xyz"][None, :, :]).all(-1)
    assert (eq.sum(1) == 1).all() and int(eq.float().argmax(1).min()) >= 900 and int(eq.float().argmax(1).max()) < 1900
    assert rg.mutator("closeup", 1) is None and rg.rig("closeup") == dict(cam_radius=0.22, sigma_range=(4e-3, 2e-2))


def test_step0_scene_is_in_no_regime():
    """The conditions separate: the unmutated scene on the default rig meets none of them (so a mutation that silently
    stopped acting would be noticed)."""
    sc = _plain(1)
    ro, inp, z = rg.raster_oracle_of_view(sc, 0)
    f = rg.regime_facts(ro, inp["op"], sc["cameras"][0], z)
    for name in rg.REGIMES:
        with pytest.raises(AssertionError):
            rg.assert_in_regime(name, f)
    assert rg.regime_facts(ro, inp["op"], sc["cameras"][0])["near_culled"] is None     # (no view depth given: no count, no quiet pass)
    ro.close()


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("name", list(rg.REGIMES))
def test_hand_scene_is_in_its_regime(name, seed):
    sc = rg.regime_scene(name, "hand", seed)
    S = rg.SHAPE
    g = np.random.default_rng(seed).normal(size=(3, S["H"], S["W"])).astype(np.float32)
    for v in range(S["views"]):
        ro, inp, z = rg.raster_oracle_of_view(sc, v)
        f = rg.regime_facts(ro, inp["op"], sc["cameras"][v], z)
        rg.assert_in_regime(name, f, (seed, v))
        # the shapes are the smallest at which the regimes still fill tiles to over a thousand entries
        assert f["longest_list"] > 1000 and f["max_n_contrib"] > 512, f
        if name == "faint":      # below 1/255: a radius, a share of num_rendered, and no gradient in the oracle itself
            below = inp["op"] < np.float32(1.0) / np.float32(255.0)
            assert (ro.radii[below] > 0).sum() > S["n"] // 4
            b = ro.backward(g)
            assert rg.oracle_rows_zero(b, below) and np.abs(b["opacity"][~below]).max() > 0
        ro.close()

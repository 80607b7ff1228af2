"""Trained-state regimes for the rasterizer parity tests (helper module, no tests here).

Every oracle comparison of the blend kernels used to run on a scene as it looks at step 0: opacities spread over (0, 1),
distinct positions, mild anisotropy, cameras far from the hand.  Training leaves that state at once; the mutations below
put a `make_scene` scene INTO the regimes training visits (not on their thresholds):

  saturated   opacities saturate: the min(0.99, .) clamp acts in the core of most splats, walks end by T (1 - alpha) < 1e-4
  post_reset  what reset_opacity leaves: everything at 0.01, nothing ever stops, most tile pairs are null
  faint       every third Gaussian below 1/255: positive radius, counted in num_rendered and vis, in no tile list
  cloned      what densify_and_clone leaves: exact duplicates, equal depth keys, order by the index tie-break alone
  needles     10 : 1 anisotropy in 3-D
  closeup     (a camera setting) part of the hand inside the near plane: large rectangles, the 1.3 tanfov clamp

`regime_facts` measures, on the oracle's side alone, whether a view is in its regime; CONDITIONS holds the bounds
(each below the worst of the three views of the hand scene at seeds 1 and 2, measured with the fp32 oracle) and
`assert_in_regime` applies them: a test whose scene is not in its regime fails instead of passing quietly."""
import math

import numpy as np
import torch

SHAPE = dict(n=4000, W=96, H=64, grid_res=24, views=3)
DEFAULT_RIG = dict(cam_radius=0.5, sigma_range=(2e-3, 8e-3))
CLOSEUP_RIG = dict(cam_radius=0.22, sigma_range=(4e-3, 2e-2))


def saturated(params, gen):
    params["_opacity"] += 6.0


def post_reset(params, gen):
    """reset_opacity (oracle.torch_ref.reset_opacity, the reference's gaussian.py:148-151)."""
    o = torch.minimum(torch.sigmoid(params["_opacity"]), torch.full_like(params["_opacity"], 0.01))
    params["_opacity"].copy_(torch.log(o / (1 - o)))


def faint(params, gen):
    params["_opacity"][::3] = -6.5            # sigmoid = 0.0015 < 1/255


def cloned(params, gen, lo=0, hi=None):
    """The last third of rows [lo, hi) of EVERY leaf become copies of rows drawn from the first two thirds of that range
    (densify_and_clone appends exact copies).  (A range: the hand and the object rows of a composite scene are not mixed.)"""
    n = next(iter(params.values())).shape[0]
    hi = n if hi is None else hi
    m = hi - lo
    n_src = m - m // 3
    src = lo + torch.randint(0, n_src, (m // 3,), generator=gen)
    for v in params.values():
        v[lo + n_src:hi] = v[src]


def needles(params, gen):
    params["_scaling"][:, 0] += 0.5 * math.log(10.0)
    params["_scaling"][:, 1:] -= 0.5 * math.log(10.0)


# name -> (mutation or None, camera rig)
REGIMES = {
    "saturated": (saturated, DEFAULT_RIG),
    "post_reset": (post_reset, DEFAULT_RIG),
    "faint": (faint, DEFAULT_RIG),
    "cloned": (cloned, DEFAULT_RIG),
    "needles": (needles, DEFAULT_RIG),
    "closeup": (None, CLOSEUP_RIG),
    "saturated_closeup": (saturated, CLOSEUP_RIG),
}


def mutator(name, seed):
    """The regime's mutation as a function of the params dict alone (what run_fused_vs_oracle's `mutate` takes)."""
    fn = REGIMES[name][0]
    if fn is None:
        return None
    return lambda params: fn(params, torch.Generator().manual_seed(1000 + seed))


def rig(name):
    return dict(REGIMES[name][1])


def regime_scene(name, kind="hand", seed=1, views=SHAPE["views"], n=SHAPE["n"]):
    """The CPU scene of a regime at the small shape (4000 Gaussians, 96 x 64, three cameras)."""
    from manus_amd.synthetic import make_scene
    sc = make_scene(n_gaussians=n, kind=kind, seed=seed, grid_res=SHAPE["grid_res"], n_cameras=views, width=SHAPE["W"],
                    height=SHAPE["H"], device="cpu", **rig(name))
    m = mutator(name, seed)
    if m is not None:
        m(sc["params"])
    return sc


def to_device(sc, device):
    out = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in sc.items() if k != "params"}
    out["params"] = {k: v.to(device) for k, v in sc["params"].items()}
    return out


def view_depth(means3D, cam):
    """View-space z of every Gaussian (fp32, the rule of the near cull: row-major storage of the transposed matrix)."""
    v = np.asarray(cam["world_view_transform"], np.float32).reshape(4, 4)
    m = np.asarray(means3D, np.float32)
    return (m[:, 0] * v[0, 2] + m[:, 1] * v[1, 2] + m[:, 2] * v[2, 2] + v[3, 2]).astype(np.float32)


def raster_oracle_of_view(sc, v, dtype=np.float32):
    """(RasterOracle, rasterizer inputs, view depth) of view v of a scene: the torch restatement of the chain up to
    the rasterizer's inputs on the CPU, then the scalar rasterizer."""
    from oracle import RasterOracle
    from oracle import torch_ref as tr
    c = sc["cameras"][v]
    cc = torch.tensor(np.asarray(c["camera_center"], np.float32))
    with torch.no_grad():
        if sc["kind"] == "hand":
            o = tr.hand_forward(sc["params"], sc["grid"], sc["grid_center"], sc["grid_scale"], sc["posed"][v], sc["rest"], cc)
        elif sc["kind"] == "object":
            o = tr.object_forward(sc["params"], cc)
        else:
            o = tr.composite_forward(sc["params"], sc["n_hand"], sc["grid"], sc["grid_center"], sc["grid_scale"], sc["posed"][v],
                                     sc["rest"], cc)
    inp = dict(m=o["posed_xyz"].numpy(), cov=o["posed_cov"].numpy(), col=o["colors"].numpy(), op=o["opacity"].numpy()[:, 0])
    ro = RasterOracle(c["width"], c["height"], math.tan(c["fovx"] / 2), math.tan(c["fovy"] / 2),
                      np.asarray(c["world_view_transform"], np.float32).reshape(-1),
                      np.asarray(c["full_proj_transform"], np.float32).reshape(-1),
                      inp["m"], inp["cov"], inp["col"], inp["op"], np.ones(3, np.float32), dtype=dtype)
    return ro, inp, view_depth(inp["m"], c)


def regime_facts(oracle, opacity, cam, view_z=None):
    """What one view of a scene looks like to the oracle (numpy only; reads nothing but the oracle's state).
    opacity (N): the opacities the oracle was given.  view_z (N): view-space depth of EVERY Gaussian -- the oracle keeps
    the depth of those it did not cull only, so the two near-plane counts need it; without it they are None (and every
    comparison with them raises)."""
    g = oracle.geom()
    W, H = oracle.W, oracle.H
    vis = oracle.radii > 0
    nvis = max(int(vis.sum()), 1)
    op = np.asarray(opacity, np.float32).reshape(-1)
    ft, nc = oracle.image_state()
    covered = nc > 0
    pl, rg = oracle.binning()
    size = (rg[:, 1] - rg[:, 0]).astype(np.int64)
    tile_of = np.repeat(np.arange(rg.shape[0]), size)        # (the lists lie in tile order)
    if len(pl) > 1:
        d = g["depth"][pl]
        same_tile = tile_of[1:] == tile_of[:-1]
        tie_share = float(((d[1:] == d[:-1]) & same_tile).sum()) / max(int(same_tile.sum()), 1)
    else:
        tie_share = 0.0
    A, B, C = (g["conic_opacity"][vis, k].astype(np.float64) for k in range(3))
    mid, dif = 0.5 * (A + C), np.sqrt(np.maximum(0.25 * (A - C) ** 2 + B * B, 0.0))
    aniso = (mid + dif) / np.maximum(mid - dif, 1e-300)        # ratio of the conic's eigenvalues (= of the 2-D variances)
    # the 1.3 tanfov clamp of the EWA Jacobian acts where the centre's NDC coordinate lies beyond +-1.3
    ndc_x, ndc_y = (2.0 * g["xy"][:, 0] + 1.0) / W - 1.0, (2.0 * g["xy"][:, 1] + 1.0) / H - 1.0
    beyond = vis & ((np.abs(ndc_x) > 1.3) | (np.abs(ndc_y) > 1.3))
    facts = dict(
        n_visible=int(vis.sum()),
        opaque_share=float((op[vis] > 0.99).sum()) / nvis,
        faint_share=float((op[vis] < np.float32(1.0) / np.float32(255.0)).sum()) / nvis,
        max_opacity=float(op[vis].max()) if vis.any() else 0.0,
        near_culled=None if view_z is None else int((np.asarray(view_z) <= np.float32(0.2)).sum()),
        near_visible=None if view_z is None else int((vis & (np.asarray(view_z) < np.float32(0.3))).sum()),
        clamp_visible=int(beyond.sum()),
        covered=float(covered.mean()),
        stopped=float((ft[covered] < 1e-3).mean()) if covered.any() else 0.0,
        min_final_T=float(ft.min()),
        tie_share=tie_share,
        median_anisotropy=float(np.median(aniso)) if vis.any() else 0.0,
        max_tiles_touched=int(g["tiles_touched"].max()) if oracle.N else 0,
        longest_list=int(size.max()) if len(size) else 0,
        max_n_contrib=int(nc.max()),
    )
    return facts


_CLOSEUP = [("near_culled", ">=", 300), ("near_visible", ">=", 2000), ("clamp_visible", ">=", 100), ("covered", ">=", 0.95),
            ("stopped", ">=", 0.60), ("max_tiles_touched", ">=", 20)]
# (fact, relation, bound); the measured range of hand, seeds 1 and 2, all three views, beside each
CONDITIONS = {
    "saturated": [("opaque_share", ">=", 0.75),             # 0.81-0.83
                  ("stopped", ">=", 0.40)],                 # 0.48-0.70
    "post_reset": [("max_opacity", "<=", float(np.nextafter(np.float32(0.01), np.float32(1.0)))),
                   ("stopped", "<=", 0.0),                  # no covered pixel stops ...
                   ("min_final_T", ">=", 0.05)],            # ... 0.17-0.50
    "faint": [("faint_share", ">=", 0.30)],                 # 0.33 (and the oracle's gradient rows of those are zero: the tests)
    "cloned": [("tie_share", ">=", 0.30)],                  # 0.33-0.34
    "needles": [("median_anisotropy", ">=", 12.0)],         # 15-16
    "closeup": _CLOSEUP,                                    # 390-1860, 2116-2891, 138-412, -, 0.65-0.83, -
    "saturated_closeup": [c for c in _CLOSEUP if c[0] != "stopped"] + [("stopped", ">=", 0.65),       # 0.71-0.90
                                                                      ("opaque_share", ">=", 0.75)],
}


def assert_in_regime(name, facts, tag=""):
    """`facts`: one view's regime_facts, or a list of them (every view must be in the regime)."""
    for f in (facts if isinstance(facts, (list, tuple)) else [facts]):
        for key, rel, bound in CONDITIONS[name]:
            ok = f[key] >= bound if rel == ">=" else f[key] <= bound
            assert ok, "%s %s: scene is not in its regime: %s = %r, wanted %s %r; %r" % (name, tag, key, f[key], rel, bound, f)


def oracle_rows_zero(b, rows):
    """Whether the given rows of every per-Gaussian gradient of an oracle backward are exactly zero."""
    return all(not np.asarray(a)[rows].any() for a in b.values())

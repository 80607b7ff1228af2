"""Small, ragged and empty-view shapes for the fused step (helper module, no tests here).

The fused route (mgr_views_forward / mgr_views_backward) met the oracle at two shapes only: 4000 Gaussians at 96 x 64 -- exactly
eight 512-row ranges of k_inst_fwd, whole tiles, W % 4 == 0, even H -- and the BASELINE sizes.  The cases below put a
`make_scene` scene (seed 1, grid_res 24) at the sizes where the fused-only kernels take another path:

  block mapping   k_inst_fwd deals 512-row ranges out to XCDs and pads its grid to 8 * ceil(nrange / 8) * V workgroups: one partial
                  range (N = 1, 63, 511), a partial second one (513), nine ranges padded to sixteen (4097)
  mixed cut       a composite scene whose articulated / static cut lies inside a wave (n_art % 64 != 0)
  ragged tiles    images below one tile, one tile column or row, a last column / row 1 px wide
  scalar branches W % 4 != 0 (background fill, loss scan and list kernels), odd H (an unpaired last row of the loss kernels)
  empty views     cameras that see nothing: facing away, every opacity below 1/255, everything at or inside the near plane

`conditions(name)` states what a case must be, on the oracle's side alone; `assert_case` applies it to the oracle's facts of
every view (regimes.regime_facts): a scene that is not its case fails instead of passing quietly."""
import numpy as np
import torch

import regimes as rg

SEED, GRID_RES = 1, 24
RANGE_ROWS = 512          # rows of one k_inst_fwd workgroup (PRE_THREADS)
NEAR = np.float32(0.2)    # the near cull: view depth <= 0.2

# name -> kind, n, W, H, views, rig, and optionally: away (views whose camera is turned round), faint (every opacity logit
# at -6.5), behind (every camera pushed forward until the whole scene lies at view depth <= 0.2)
CASES = {
    "one":           dict(kind="hand", n=1, W=96, H=64, views=1),         # one live lane, 7 of 8 XCD blocks empty
    "subwave_tile":  dict(kind="hand", n=63, W=16, H=16, views=1),        # N below a wave, exactly one tile
    "below_a_tile":  dict(kind="hand", n=513, W=15, H=9, views=2),        # partial second range; image smaller than a tile; W odd
    "nine_ranges":   dict(kind="hand", n=4097, W=97, H=65, views=3),      # grid padded from 9 to 16 ranges; last tile column and row 1 px
    "mixed_cut":     dict(kind="composite", n=4609, W=50, H=38, views=3), # n_hand = 2765: a cut inside a wave and a range; W % 4 = 2
    "object_odd":    dict(kind="object", n=511, W=33, H=47, views=2),     # static route, odd W and H
    "tall":          dict(kind="hand", n=4000, W=13, H=80, views=3),      # one tile column, 5 rows: all 4000 in one list
    "wide":          dict(kind="hand", n=4000, W=200, H=17, views=3),     # 13 x 2 tiles, second row 1 px; part of the hand off screen
    "speck":         dict(kind="hand", n=2000, W=7, H=5, views=1),        # 35 pixels
    "five":          dict(kind="composite", n=5, W=96, H=64, views=3),    # n_hand = 3
    "nine_views":    dict(kind="hand", n=1500, W=50, H=38, views=9),      # second lane group (accumulating) at a ragged size
    "closeup_ragged": dict(kind="hand", n=1500, W=97, H=65, views=3, rig=rg.CLOSEUP_RIG),   # rectangles of many tiles against the ragged edges
}
_NINE = CASES["nine_ranges"]
EMPTY_CASES = {
    "empty_first":  dict(_NINE, away=(0,)),
    "empty_middle": dict(_NINE, away=(1,)),
    "empty_last":   dict(_NINE, away=(2,)),
    "empty_all":    dict(_NINE, away=(0, 1, 2)),
    "faint_all":    dict(_NINE, faint=True),
    "behind_all":   dict(_NINE, behind=True),
}
NONEMPTY = list(CASES)
EMPTY = list(EMPTY_CASES)
ALL = dict(CASES, **EMPTY_CASES)


def spec(name):
    c = dict(ALL[name])
    c.setdefault("rig", rg.DEFAULT_RIG)
    for k in ("away", "faint", "behind"):
        c.setdefault(k, () if k == "away" else False)
    return c


def scene_target():
    """The point `make_scene`'s cameras look at (the centroid of its first pose)."""
    from manus_amd.synthetic import load_skeleton
    sk = load_skeleton()
    return (0.5 * (sk["pose_heads"][2] + sk["pose_tails"][2])).mean(0)


def _camera(cam, E):
    from manus_amd.cam_utils import get_opengl_camera_attributes
    return get_opengl_camera_attributes(cam["K"], E, cam["width"], cam["height"])


def away_camera(cam, target=None):
    """The camera at `cam`'s position that faces away from the scene: its target mirrored through the camera position."""
    from manus_amd.synthetic import look_at_extrinsics
    pos = np.asarray(cam["camera_center"], np.float64)
    target = scene_target() if target is None else np.asarray(target, np.float64)
    return _camera(cam, look_at_extrinsics(pos, 2.0 * pos - target))


def pushed_camera(cam, shift):
    """`cam` moved by `shift` along its viewing direction, orientation kept."""
    E = np.asarray(cam["extr"], np.float64)[:3, :4]
    R = E[:, :3]
    pos = np.asarray(cam["camera_center"], np.float64) + shift * R[2]
    return _camera(cam, np.concatenate([R, (-R @ pos)[:, None]], 1))


def turn_away(views):
    """A camera hook (run_fused_vs_oracle's `cameras`, `case_scene`): the given views' cameras are turned round in place."""
    def hook(sc):
        for v in views:
            sc["cameras"][v] = away_camera(sc["cameras"][v])
    return hook


def append_away_camera(sc, of_view=0):
    """Append the turned-round camera of view `of_view` as a further view, with that view's pose: -> its view id."""
    sc["cameras"].append(away_camera(sc["cameras"][of_view]))
    for k in ("posed", "transforms", "keypoints"):
        sc[k] = torch.cat([sc[k], sc[k][of_view:of_view + 1]], 0)
    return len(sc["cameras"]) - 1


def push_behind(sc):
    """Every camera pushed forward until the deepest Gaussian of its view lies at view depth 0.19: everything is culled at
    the near plane (z <= 0.2), part of it at a positive depth, the rest behind the camera."""
    for v in range(len(sc["cameras"])):
        ro, _, z = rg.raster_oracle_of_view(sc, v)
        ro.close()
        sc["cameras"][v] = pushed_camera(sc["cameras"][v], float(z.max()) - 0.19)


def faint_all(params):
    params["_opacity"][:] = -6.5              # sigmoid = 0.0015 < 1/255


def mutator(name):
    return faint_all if spec(name)["faint"] else None


def camera_hook(name):
    c = spec(name)
    if c["behind"]:
        return push_behind
    return turn_away(c["away"]) if c["away"] else None


def case_scene(name, extra_away=False):
    """The CPU scene of a case.  extra_away: as many views again (ids views .. 2 views - 1), the turned-round cameras of views
    0 .. views - 1 with their poses."""
    from manus_amd.synthetic import make_scene
    c = spec(name)
    sc = make_scene(n_gaussians=c["n"], kind=c["kind"], seed=SEED, grid_res=GRID_RES, n_cameras=c["views"], width=c["W"], height=c["H"],
                    device="cpu", **c["rig"])
    if c["faint"]:
        faint_all(sc["params"])
    hook = camera_hook(name)
    if hook is not None:
        hook(sc)
    if extra_away:
        for v in range(c["views"]):
            append_away_camera(sc, v)
    return sc


def oracle_args(name):
    """The arguments of fused_oracle.run_fused_vs_oracle for a case."""
    c = spec(name)
    return dict(kind=c["kind"], views=c["views"], n=c["n"], W=c["W"], H=c["H"], seed=SEED, grid_res=GRID_RES, mutate=mutator(name),
                cameras=camera_hook(name), **c["rig"])


def conditions(name):
    """What the case must be, from its definition alone: ranges of k_inst_fwd and its padded grid, tile grid, the cut modulo a
    wave, which views see something, and whether anything is listed at all."""
    c = spec(name)
    n = c["n"]
    n_art = n if c["kind"] == "hand" else 0 if c["kind"] == "object" else int(n * 0.6)
    nrange = (n + RANGE_ROWS - 1) // RANGE_ROWS
    empty = set(range(c["views"])) if (c["behind"]) else set(c["away"])
    return dict(nrange=nrange, padded=8 * ((nrange + 7) // 8), tiles=((c["W"] + 15) // 16, (c["H"] + 15) // 16), n_art=n_art, n_art_mod64=n_art % 64,
                mixed=0 < n_art < n, empty_views=sorted(empty), nothing_listed=bool(c["faint"]), w_mod4=c["W"] % 4, h_odd=c["H"] % 2 == 1,
                closeup=c["rig"] is rg.CLOSEUP_RIG or c["rig"] == rg.CLOSEUP_RIG)


# what the table of the cases promises beyond the generic conditions: name -> {condition: value}
PROMISED = {
    "one": dict(nrange=1, padded=8, tiles=(6, 4)),
    "subwave_tile": dict(nrange=1, tiles=(1, 1)),
    "below_a_tile": dict(nrange=2, tiles=(1, 1), w_mod4=3, h_odd=True),
    "nine_ranges": dict(nrange=9, padded=16, tiles=(7, 5), w_mod4=1, h_odd=True),
    "mixed_cut": dict(nrange=10, n_art=2765, n_art_mod64=13, mixed=True, w_mod4=2),
    "object_odd": dict(nrange=1, n_art=0, w_mod4=1, h_odd=True),
    "tall": dict(tiles=(1, 5), w_mod4=1),
    "wide": dict(tiles=(13, 2), h_odd=True),
    "speck": dict(tiles=(1, 1), w_mod4=3, h_odd=True),
    "five": dict(n_art=3, mixed=True),
    "nine_views": dict(w_mod4=2),
    "closeup_ragged": dict(tiles=(7, 5), closeup=True),
}


def view_facts(sc, v, dtype=np.float32):
    """regimes.regime_facts of view v on the CPU oracle, plus the oracle's pair count and whether the whole scene is at or
    inside the near plane."""
    ro, inp, z = rg.raster_oracle_of_view(sc, v, dtype=dtype)
    f = rg.regime_facts(ro, inp["op"], sc["cameras"][v], z)
    pl, _ = ro.binning()
    f.update(num_rendered=int(ro.num_rendered), listed=int(len(pl)), max_view_depth=float(z.max()), n_positive_depth=int((z > 0).sum()))
    ro.close()
    return f


def projection_yardstick(sc, views):
    """max over the views of |fp32 oracle - fp64 oracle| on the same fp32 inputs: pixel centres (px) and conic (relative to the
    largest entry).  Two independent fp32 chains of this length can each lie that far from the exact value."""
    pix = con = 0.0
    for v in range(views):
        r32, _, _ = rg.raster_oracle_of_view(sc, v, dtype=np.float32)
        r64, _, _ = rg.raster_oracle_of_view(sc, v, dtype=np.float64)
        g32, g64 = r32.geom(), r64.geom()
        both = (r32.radii > 0) & (r64.radii > 0)
        if both.any():
            pix = max(pix, float(np.abs(g32["xy"][both].astype(np.float64) - g64["xy"][both]).max()))
            a, b = g32["conic_opacity"][both, :3].astype(np.float64), g64["conic_opacity"][both, :3].astype(np.float64)
            con = max(con, float(np.abs(a - b).max() / np.abs(b).max()))
        r32.close(), r64.close()
    return pix, con


def assert_case(name, facts, sc=None, tag=""):
    """`facts`: one dict per view (regime_facts, optionally with view_facts' additions).  The scene must be its case."""
    c, cond = spec(name), conditions(name)
    for key, val in PROMISED.get(name, {}).items():
        assert cond[key] == val, "%s %s: %s = %r, the case promises %r" % (name, tag, key, cond[key], val)
    assert len(facts) >= c["views"], (name, tag, len(facts))
    if sc is not None:
        assert sc["params"]["_xyz"].shape[0] == c["n"] and int(sc["n_hand"]) == cond["n_art"], (name, tag)
        assert (sc["width"], sc["height"]) == (c["W"], c["H"]), (name, tag)
    for v, f in enumerate(facts[:c["views"]]):
        if v in cond["empty_views"]:
            assert f["n_visible"] == 0, "%s %s: view %d must see nothing, sees %d" % (name, tag, v, f["n_visible"])
        else:
            assert f["n_visible"] >= 1, "%s %s: view %d sees nothing" % (name, tag, v)
        if cond["nothing_listed"]:
            # radii positive (so the rectangles count in the oracle's num_rendered: it has no null-pair cull), but no pixel of
            # the view has a single contributor
            assert f["n_visible"] >= 1 and f["faint_share"] == 1.0 and f["covered"] == 0.0 and f["max_n_contrib"] == 0, (name, tag, v, f)
        if c["behind"] and "max_view_depth" in f:
            assert f["max_view_depth"] <= float(NEAR) and f["n_positive_depth"] > 0 and f["near_culled"] == c["n"], (name, tag, v, f)
        if name == "wide":
            assert f["n_visible"] < c["n"], (name, tag, v, f)          # part of the hand is off screen
        if cond["closeup"]:
            assert f["max_tiles_touched"] >= 20, (name, tag, v, f)     # of the 35 tiles of 97 x 65
        elif v not in cond["empty_views"]:
            assert f["max_tiles_touched"] <= 6, (name, tag, v, f)

"""GPU: the feature render (mgr_raster_blend_features, rasterizer.blend_features, render_gaussians' extra outputs,
CompositeRenderer(share_binning=True)) -- extra per-Gaussian channels, expected depth and accumulated opacity composited over
the tile lists of the last forward.

Two kinds of check.  Against the forward itself: rendering the forward's colours as features must reproduce its image within
the rounding of the sums, 4 L 2^-24 with L the largest list position of a last contributor (n_contrib of the workspace, an
upper bound of the number of products either side adds per pixel; products of magnitude <= 1) -- a bound without room for a
single differing contributor.  Against oracle.RasterOracle, which composites any three colours with any background: a C-channel
reference is ceil(C/3) oracle runs, alpha is 1 - final_T, depth a run with colours (z, 0, 0) on a zero background; bars are
the image bars of test_gpu_raster.py (max 5e-3, mean 2e-6, "isolated threshold flips only"), per channel, relative to the
channel's largest value."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import RasterOracle

from util import cam_args, cam_table_np, make_camera, random_gaussians

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BG = np.array([0.2, 0.5, 0.9], np.float32)
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# scenes and their references (computed once, never modified)
# ---------------------------------------------------------------------------------------------------------------------
def _giant_scene():
    """One 16x16 tile with more than 16384 pairs (the construction of test_deep_tile_uses_global_sort_path)."""
    W = H = 16
    cam = make_camera(W, H, pos=(0, 0, -2.0), target=(0, 0, 0), focal=30.0)
    n = 20000
    g = np.random.default_rng(3)
    m = (g.normal(size=(n, 3)) * np.array([0.05, 0.05, 0.3])).astype(np.float32)
    m[5] = m[6]  # an exact depth tie
    c = np.repeat(np.array([[1e-4, 0, 0, 1e-4, 0, 1e-4]], np.float32), n, 0)
    col = g.uniform(0, 1, size=(n, 3)).astype(np.float32)
    op = np.full(n, 0.02, np.float32)
    return cam, m, c, col, op


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "giant":
        cam, m, c, col, op = _giant_scene()
    else:
        n, seed, W, H = {"a": (1500, 0, 128, 96), "b": (300, 2, 33, 47)}[name]
        cam = make_camera(W, H)
        m, c, col, op = random_gaussians(n, seed=seed)
    g = np.random.default_rng(100)
    feat = g.uniform(0, 1, size=(m.shape[0], 9)).astype(np.float32)
    bgf = g.uniform(0.1, 0.9, size=(9,)).astype(np.float32)
    for a in (m, c, col, op, feat, bgf):
        a.setflags(write=False)
    return SimpleNamespace(cam=cam, W=cam["width"], H=cam["height"], m=m, c=c, col=col, op=op, feat=feat, bgf=bgf)


def _oracle(cam, m, c, col, op, bg):
    a = cam_args(cam)
    return RasterOracle(a["W"], a["H"], a["tanfovx"], a["tanfovy"], a["view"], a["proj"], m, c, col, op, bg)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(features (channels,H,W), alpha (H,W), depth (H,W), max z of the listed Gaussians) from the oracle; 9 channels, 3 for
    the giant tile."""
    s = scene(name)
    channels = 3 if name == "giant" else 9
    out = []
    for k in range(0, channels, 3):
        o = _oracle(s.cam, s.m, s.c, s.feat[:, k:k + 3], s.op, s.bgf[k:k + 3])
        out.append(np.array(o.color))
    alpha = 1.0 - o.image_state()[0]
    z = o.geom()["depth"].astype(np.float32)
    zc = np.zeros((s.m.shape[0], 3), np.float32)
    zc[:, 0] = np.where(o.radii > 0, z, 0)
    depth = np.array(_oracle(s.cam, s.m, s.c, zc, s.op, np.zeros(3, np.float32)).color[0])
    res = (np.concatenate(out)[:channels], alpha, depth, float(zc.max()))
    for a in res[:3]:
        a.setflags(write=False)
    return res


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def forward(cams, m, c, col, op, bg=BG):
    """An evaluation forward of the views; (V,3,H,W) on the device.  The context's last workspace is this forward's."""
    from manus_amd.rasterizer import rasterize_views
    W, H = cams[0]["width"], cams[0]["height"]
    ct = torch.from_numpy(cam_table_np(cams)).to(DEV)
    with torch.no_grad():
        img, _ = rasterize_views(ct, dev(m), torch.zeros((len(cams), m.shape[0], 3), device=DEV), dev(col), dev(op), dev(c),
                                 dev(bg), W, H)
    return img


def max_list_position():
    """L of the bound: the largest n_contrib (1-based list position of a pixel's last contributor) of the last forward."""
    from manus_amd import rasterizer as rz
    from manus_amd._lib import lib
    ws = rz.context().last_ws
    V, N, W, H = ws.key
    offs = (ctypes.c_size_t * 40)()
    n = lib().mgr_raster_layout(V, N, W, H, ws.cap, offs, 40)
    assert n > 17
    nc = ws.buf[offs[17]:offs[17] + V * H * W * 4].view(torch.int32)
    return int(nc.max())


def tile_pairs(t):
    """Pairs binned into tile t of view 0 by the last forward (tile_start of the workspace)."""
    from manus_amd import rasterizer as rz
    from manus_amd._lib import lib
    ws = rz.context().last_ws
    V, N, W, H = ws.key
    offs = (ctypes.c_size_t * 40)()
    assert lib().mgr_raster_layout(V, N, W, H, ws.cap, offs, 40) > 7
    ts = ws.buf[offs[7] + 4 * t:offs[7] + 4 * t + 8].view(torch.int32)
    return int(ts[1] - ts[0])


def rounding_bound(scale=1.0):
    return 4.0 * max(max_list_position(), 1) * 2.0 ** -24 * max(1.0, scale)


def raw_blend(ws, V, N, C, W, H, feat, stride, bg, with_depth, out, out_alpha, nbytes=None, cap=None):
    from manus_amd._lib import lib, ptr, stream
    return lib().mgr_raster_blend_features(V, N, C, W, H, ptr(feat), stride, ptr(bg), with_depth, ptr(out), ptr(out_alpha),
                                           ptr(ws.buf), ws.nbytes if nbytes is None else nbytes, ws.cap if cap is None else cap,
                                           stream())


def bars(got, ref, scale):
    d = np.abs(np.asarray(got, np.float64) - ref) / scale
    return float(d.max()), float(d.mean())


# ---------------------------------------------------------------------------------------------------------------------
# 1. self-consistency with the forward, 2. against the oracle, 4. the giant tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "giant"])
def test_forward_colours_as_features_reproduce_the_image(name):
    """No allowance for a threshold flip: one (pixel, entry) contribution more or less than the forward's is a term of up to
    0.99 x colour, orders of magnitude above 4 L 2^-24."""
    from manus_amd.rasterizer import blend_features
    s = scene(name)
    img = forward([s.cam], s.m, s.c, s.col, s.op)
    out = blend_features(dev(s.col), bg=BG)
    assert out["depth"] is None and out["alpha"] is None and not out["features"].requires_grad
    L, bound = max_list_position(), rounding_bound()
    err = float((out["features"] - img).abs().max())
    print("%s: L = %d, bound %.3e, max|features - img| = %.3e" % (name, L, bound, err))
    if name == "giant":      # one tile, more than 16384 pairs in its list: the k_tile_split layout (keys2, groups)
        assert tile_pairs(0) > 16384
    assert tuple(out["features"].shape) == (1, 3, s.H, s.W)
    assert err <= bound


@pytest.mark.parametrize("name,C", [("a", 1), ("a", 3), ("a", 5), ("a", 9), ("b", 1), ("b", 3), ("b", 5), ("b", 9), ("giant", 3)])
def test_features_depth_alpha_against_the_oracle(name, C):
    from manus_amd.rasterizer import blend_features
    s = scene(name)
    rf, ra, rd, zmax = reference(name)
    forward([s.cam], s.m, s.c, s.col, s.op)
    out = blend_features(dev(s.feat)[:, :C], bg=dev(s.bgf[:C]), depth=True, alpha=True)   # (a column slice: copied by the wrapper)
    got = out["features"][0].cpu().numpy()
    assert got.shape == (C, s.H, s.W)
    for ch in range(C):
        mx, mean = bars(got[ch], rf[ch], float(np.abs(rf[ch]).max()))
        print("%s C=%d channel %d: max %.3e mean %.3e" % (name, C, ch, mx, mean))
        assert mx < 5e-3 and mean < 2e-6, (ch, mx, mean)
    mx, mean = bars(out["alpha"][0].cpu().numpy(), ra, 1.0)
    print("%s C=%d alpha: max %.3e mean %.3e" % (name, C, mx, mean))
    assert mx < 5e-3 and mean < 2e-6, ("alpha", mx, mean)
    mx, mean = bars(out["depth"][0].cpu().numpy(), rd, zmax)
    print("%s C=%d depth: max %.3e mean %.3e (max z %.3f)" % (name, C, mx, mean, zmax))
    assert mx < 5e-3 and mean < 2e-6, ("depth", mx, mean)
    assert float(out["alpha"].min()) >= 0.0 and float(out["alpha"].max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. views and strides
# ---------------------------------------------------------------------------------------------------------------------
def test_views_and_strides():
    from manus_amd.rasterizer import blend_features
    s = scene("a")
    cams = [s.cam, make_camera(s.W, s.H, pos=(-0.4, 0.3, -1.4))]
    g = torch.Generator().manual_seed(5)
    N = s.m.shape[0]
    per_view = torch.rand((2, N, 5), generator=g).to(DEV)
    shared = per_view[0].contiguous()
    bg = dev(s.bgf[:5])
    single_shared, single_own = [], []
    for v in range(2):
        forward([cams[v]], s.m, s.c, s.col, s.op)
        single_shared.append(blend_features(shared, bg=bg, depth=True, alpha=True))
        single_own.append(blend_features(per_view[v], bg=bg))
    forward(cams, s.m, s.c, s.col, s.op)
    both = blend_features(shared, bg=bg, depth=True, alpha=True)
    own = blend_features(per_view, bg=bg)
    big = torch.full((2, N + 7, 11), NAN, device=DEV)
    big[:, 3:3 + N, 2:7] = per_view
    strided = blend_features(big[:, 3:3 + N, 2:7], bg=bg)
    assert not big[:, 3:3 + N, 2:7].is_contiguous()
    for v in range(2):
        for k in ("features", "depth", "alpha"):
            assert torch.equal(both[k][v], single_shared[v][k][0]), (v, k)
        assert torch.equal(own["features"][v], single_own[v]["features"][0]), v
        assert torch.equal(strided["features"][v], single_own[v]["features"][0]), v
    assert not torch.equal(own["features"][1], both["features"][1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_empty_and_culled_scenes_write_every_element():
    from manus_amd import rasterizer as rz
    W, H = 64, 48
    cam = make_camera(W, H, pos=(0, 0, -2.0), target=(0, 0, 0), focal=80.0)
    bgf = dev([0.25, 0.5, 0.75, 1.5])
    culled = (np.array([[0, 0, -1.9], [0, 0, -3.0], [50.0, 0, 0]], np.float32),
              np.repeat(np.array([[4e-4, 0, 0, 4e-4, 0, 4e-4]], np.float32), 3, 0), np.ones((3, 3), np.float32),
              np.full(3, 0.5, np.float32))
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32), np.zeros((0,), np.float32))
    for m, c, col, op in (empty, culled):
        N = m.shape[0]
        forward([cam], m, c, col, op)
        ws = rz.context().last_ws
        out = torch.full((1, 5, H, W), NAN, device=DEV)
        alpha = torch.full((1, H, W), NAN, device=DEV)
        feat = torch.rand((N, 4), device=DEV) if N else None
        assert raw_blend(ws, 1, N, 4, W, H, feat, 0, bgf, 1, out, alpha) == 0
        for ch in range(4):
            assert (out[0, ch] == bgf[ch]).all(), (N, ch)
        assert (out[0, 4] == 0).all() and (alpha == 0).all(), N


def test_channel_count_edges_and_repeatability():
    from manus_amd.rasterizer import blend_features
    s = scene("b")
    g = torch.Generator().manual_seed(9)
    f32 = torch.rand((s.m.shape[0], 32), generator=g).to(DEV)
    bg32 = torch.rand((32,), generator=g)
    forward([s.cam], s.m, s.c, s.col, s.op)
    only = blend_features(depth=True, alpha=True)                       # C = 0
    assert only["features"] is None and tuple(only["depth"].shape) == (1, s.H, s.W)
    wide = blend_features(f32, bg=bg32, depth=True, alpha=True)        # C = 32: four groups of eight and the depth on its own
    again = blend_features(f32, bg=bg32, depth=True, alpha=True)
    assert tuple(wide["features"].shape) == (1, 32, s.H, s.W)
    for k in ("features", "depth", "alpha"):
        assert torch.isfinite(wide[k]).all() and torch.equal(wide[k], again[k]), k
    assert torch.equal(only["depth"], wide["depth"]) and torch.equal(only["alpha"], wide["alpha"])
    # every channel is what a narrow call gives for it, whatever group it rode in (same walk, same products)
    for lo, hi in ((0, 3), (7, 9), (29, 32)):
        part = blend_features(f32[:, lo:hi], bg=bg32[lo:hi])
        assert torch.equal(part["features"], wide["features"][:, lo:hi]), (lo, hi)
    alone = blend_features(alpha=True)
    assert alone["depth"] is None and torch.equal(alone["alpha"], wide["alpha"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Every refusal is decided on the host from the workspace's header: the NaN-filled outputs stay NaN.  (The refusal after
    a forward with the depth cut needs the fused route: test_fused_route_is_accepted_uncut_and_refused_with_the_depth_cut.)"""
    from manus_amd import rasterizer as rz
    from manus_amd._lib import ManusHipError, lib, ptr, stream
    s = scene("b")
    N, W, H = s.m.shape[0], s.W, s.H
    feat = dev(s.feat[:, :3])
    out = torch.full((1, 3, H, W), NAN, device=DEV)
    alpha = torch.full((1, H, W), NAN, device=DEV)
    untouched = lambda: bool(torch.isnan(out).all() and torch.isnan(alpha).all())
    ctx = rz.context()
    # a fresh context, and a fresh (zero-filled, never used) workspace
    ctx.clear()
    with pytest.raises(ManusHipError):
        rz.blend_features(feat)
    fresh = rz.RasterWorkspace(torch.device(DEV), 1, N, W, H, 8 * N)
    assert raw_blend(fresh, 1, N, 3, W, H, feat, 0, None, 0, out, alpha) == -8 and untouched()
    assert b"no forward" in lib().mgr_last_error()
    # the last forward was made for another image size
    small = make_camera(24, 16)
    forward([small], s.m, s.c, s.col, s.op)
    forward([s.cam], s.m, s.c, s.col, s.op)
    ws = ctx.last_ws
    assert ws.key == (1, N, W, H)
    o2, a2 = torch.full((1, 3, 16, 24), NAN, device=DEV), torch.full((1, 16, 24), NAN, device=DEV)
    assert raw_blend(ws, 1, N, 3, 24, 16, feat, 0, None, 0, o2, a2) == -8
    assert b"another" in lib().mgr_last_error() and bool(torch.isnan(o2).all() and torch.isnan(a2).all())
    assert raw_blend(ws, 1, N, 3, W, H, feat, 0, None, 0, out, alpha, cap=ws.cap + 64, nbytes=1 << 40) == -8 and untouched()
    # C = 33
    wide = torch.zeros((N, 33), device=DEV)
    with pytest.raises(ManusHipError):
        rz.blend_features(wide)
    assert raw_blend(ws, 1, N, 33, W, H, wide, 0, None, 0, out, alpha) == -1 and untouched()
    assert raw_blend(ws, 1, N, 0, W, H, None, 0, None, 0, None, None) == -1                # nothing asked for
    # a forward that stopped before its blend (debug bit 1, value 2), same workspace and arguments
    ct = torch.from_numpy(cam_table_np([s.cam])).to(DEV)
    m, c, col, op, bg = dev(s.m), dev(s.c), dev(s.col), dev(s.op), dev(BG)
    img = torch.empty((1, 3, H, W), device=DEV)
    radii = torch.empty((1, N), dtype=torch.int32, device=DEV)
    args = lambda debug: (1, N, W, H, ptr(ct), ptr(bg), ptr(m), 0, ptr(c), 0, ptr(col), 0, ptr(op), 0, ptr(img), ptr(radii),
                          ptr(ws.buf), ws.nbytes, ws.cap, debug, stream())
    assert lib().mgr_raster_forward(*args(2)) == 0
    assert raw_blend(ws, 1, N, 3, W, H, feat, 0, None, 0, out, alpha) == -8 and untouched()
    assert b"blend" in lib().mgr_last_error()
    with pytest.raises(ManusHipError):
        rz.blend_features(feat)
    # ... and the blend alone (value 4) completes it: the lists are a forward's again
    assert lib().mgr_raster_forward(*args(4)) == 0
    assert raw_blend(ws, 1, N, 3, W, H, dev(s.col), 0, bg, 0, out, alpha) == 0
    assert float((out - img).abs().max()) <= rounding_bound() and not torch.isnan(alpha).any()


def test_fused_route_is_accepted_uncut_and_refused_with_the_depth_cut():
    """mgr_views_forward through HipViewCompute, on the scene of test_gpu_depth_cut.py (opaque Gaussians seen from close: the
    interior tiles saturate and leave hints).  Without the cut the lists of a step's forward are accepted (a backward has run
    on them since): constant features 1 on background 1 composite to sum w + T = 1, on background 0 to the alpha map, both
    within the rounding bound, and the tiles the image shows empty have alpha 0.  With the cut, once a forward has applied
    hints (fewer pairs in the lists than the full binning), the call is refused and writes nothing."""
    from manus_amd import rasterizer as rz
    from manus_amd._lib import lib
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table, make_scene
    V, n, W, H = 2, 40000, 256, 192
    sc = make_scene(n_gaussians=n, kind="hand", seed=3, grid_res=32, n_cameras=V, width=W, height=H, cam_radius=0.45,
                    sigma_range=(2e-3, 5e-3), device=DEV)
    sc["params"]["_opacity"] = sc["params"]["_opacity"] + 2.0
    N = sc["params"]["_xyz"].shape[0]
    targets = torch.rand((V, 3, H, W), generator=torch.Generator().manual_seed(103)).to(DEV)
    ct = camera_table(sc["cameras"], DEV)
    views = list(range(V))
    ctx = rz.context(DEV)
    ctx.clear()
    ctx.cut_retries = 0       # (a new compute object reads a non-zero count as a flagged forward of its own and pauses the cut)
    rz.set_sync_policy(True)
    T = ((W + 15) // 16) * ((H + 15) // 16)

    def listed(compute):      # pairs the binning of the last forward put into the lists
        ws = ctx.last_ws
        off = compute._layout(ws, V, N, W, H)
        return int(ws.buf[off[7] + 4 * V * T:off[7] + 4 * V * T + 4].view(torch.int32).item())

    try:
        ref = HipViewCompute(sc, targets, ct, loss="l1+ssim", depth_cut=False)
        ref(views)
        rz.check_overflow(DEV)
        ref(views)
        ws, full = ctx.last_ws, listed(ref)
        assert ws.key == (V, N, W, H)
        ones = torch.ones((N, 1), device=DEV)
        got = rz.blend_features(ones, bg=[1.0], alpha=True, device=DEV)
        on_black = rz.blend_features(ones, bg=[0.0], device=DEV)["features"]
        bound = rounding_bound()
        assert float((got["features"] - 1.0).abs().max()) <= bound
        assert float((on_black[:, 0] - got["alpha"]).abs().max()) <= bound
        img = ref.last_image
        empty = (img == sc["bg"].reshape(1, 3, 1, 1)).all(1)
        assert bool(empty.any()) and bool((~empty).any())
        assert float(got["alpha"][empty].max()) < 1.0 / 255.0 and float(got["alpha"][~empty].min()) > 0.0
        assert float(got["alpha"].max()) > 0.99
        # the cut: a synchronous step learns the capacity, then fenced steps; hints are applied from the second fenced step on
        cut = HipViewCompute(sc, targets, ct, loss="l1+ssim", depth_cut=True)
        cut(views)
        rz.check_overflow(DEV)
        rz.set_sync_policy(False, DEV)
        for _ in range(3):
            cut(views)
        ws = ctx.last_ws
        assert listed(cut) < full                                       # the last forward's lists ARE cut
        out = torch.full((V, 1, H, W), NAN, device=DEV)
        alpha = torch.full((V, H, W), NAN, device=DEV)
        assert raw_blend(ws, V, N, 1, W, H, ones, 0, None, 0, out, alpha) == -8
        assert b"depth cut" in lib().mgr_last_error()
        assert bool(torch.isnan(out).all() and torch.isnan(alpha).all())
    finally:
        rz.set_sync_policy(True)
        ctx.clear()


def test_backward_in_between_leaves_the_lists_alone():
    from manus_amd.rasterizer import blend_features, rasterize_views
    s = scene("a")
    ct = torch.from_numpy(cam_table_np([s.cam])).to(DEV)
    leaves = [dev(x).requires_grad_(True) for x in (s.m, s.col, s.op, s.c)]
    m2d = torch.zeros((1, s.m.shape[0], 3), device=DEV, requires_grad=True)
    img, _ = rasterize_views(ct, leaves[0], m2d, leaves[1], leaves[2], leaves[3], dev(BG), s.W, s.H)
    before = blend_features(dev(s.feat), bg=dev(s.bgf), depth=True, alpha=True)
    img.sum().backward()
    after = blend_features(dev(s.feat), bg=dev(s.bgf), depth=True, alpha=True)
    for k in before:
        assert torch.equal(before[k], after[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 7. render_gaussians
# ---------------------------------------------------------------------------------------------------------------------
def test_render_gaussians_extra_outputs():
    from manus_amd.render import render_gaussians
    s = scene("a")
    rf, ra, rd, zmax = reference("a")
    c = s.cam
    camera = SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                             world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32),
                             full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32),
                             camera_center=torch.tensor(c["camera_center"], dtype=torch.float32)[None])
    a = (dev(s.m), dev(s.c), dev(s.m), None, dev(s.op), camera, torch.tensor(BG), dev(s.col))
    plain = render_gaussians(*a)
    assert sorted(plain) == ["radii", "render", "viewspace_points", "visibility_filter"]
    full = render_gaussians(*a, extra_features=dev(s.feat[:, :5]), return_depth=True, return_alpha=True, feature_bg=dev(s.bgf[:5]))
    assert sorted(full) == ["alpha", "depth", "features", "radii", "render", "viewspace_points", "visibility_filter"]
    assert torch.equal(plain["render"], full["render"]) and torch.equal(plain["radii"], full["radii"])
    assert tuple(full["features"].shape) == (s.H, s.W, 5) and tuple(full["depth"].shape) == (s.H, s.W)
    assert tuple(full["alpha"].shape) == (s.H, s.W)
    got = full["features"].permute(2, 0, 1).cpu().numpy()
    for ch in range(5):
        mx, mean = bars(got[ch], rf[ch], float(np.abs(rf[ch]).max()))
        assert mx < 5e-3 and mean < 2e-6, (ch, mx, mean)
    for got, ref, scale in ((full["alpha"], ra, 1.0), (full["depth"], rd, zmax)):
        mx, mean = bars(got.cpu().numpy(), ref, scale)
        assert mx < 5e-3 and mean < 2e-6, (mx, mean)
    only = render_gaussians(*a, return_alpha=True)
    assert sorted(only) == ["alpha", "radii", "render", "viewspace_points", "visibility_filter"]
    assert torch.equal(only["alpha"], full["alpha"])


# ---------------------------------------------------------------------------------------------------------------------
# 8. shared binning
# ---------------------------------------------------------------------------------------------------------------------
def test_composite_renderer_shares_the_binning(monkeypatch):
    """'results', 'gt_eval', 'acc_gt_eval' with share_binning on against off, two frames each: the panel that is composited on
    its partner's tile lists within the rounding bound (the colours of these panels lie in [0, 1] or are counted into the
    bound by their largest value), every other panel and the running sum bit for bit."""
    import manus_amd.modules as mod
    from manus_amd.modules import CompositeRenderer
    from manus_amd.structures import Bones
    from manus_amd.synthetic import make_scene
    W, H = 160, 120
    sc = make_scene(n_gaussians=4000, kind="composite", seed=4, grid_res=24, n_cameras=2, width=W, height=H, cam_radius=0.5,
                    sigma_range=(1e-3, 3e-3), device="cpu", n_poses=2)
    n_h = sc["n_hand"]
    P = {k: v.to(DEV) for k, v in sc["params"].items()}

    def model(sl, hand):
        m = SimpleNamespace(_xyz=P["_xyz"][sl].contiguous(), _scaling=P["_scaling"][sl].contiguous(),
                            _rotation=P["_rotation"][sl].contiguous(),
                            get_features=torch.cat([P["_features_dc"][sl], P["_features_rest"][sl]], 1).contiguous(),
                            get_opacity=torch.sigmoid(P["_opacity"][sl]).contiguous())
        if hand:
            m.grid_center, m.grid_scale, m.grid_weights = sc["grid_center"], sc["grid_scale"], sc["grid"]
        return m

    def camera(c):
        return SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                               world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32),
                               full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32),
                               camera_center=torch.tensor(c["camera_center"], dtype=torch.float32)[None])

    batches = [dict(bones_posed=Bones(None, None, None, sc["posed"][f]), bones_rest=Bones(None, None, None, sc["rest"]),
                    camera=camera(sc["cameras"][0]), cano_camera=camera(sc["cameras"][1]), bg_color=torch.tensor([1.0, 0.9, 0.8]))
               for f in range(2)]
    hand, obj = model(slice(0, n_h), True), model(slice(n_h, None), False)
    g = torch.Generator().manual_seed(0)
    skin, accc = torch.rand((n_h, 3), generator=g).to(DEV), torch.rand((n_h,), generator=g).to(DEV)
    # the largest colour any shared panel composites (the SH colours under the contact blend may exceed 1)
    seen = []
    inputs = mod.contact_render_inputs

    def recording(*a, **k):
        r = inputs(*a, **k)
        if k.get("geometry") is not None:
            seen.append(float(r.colors_precomp.abs().max()))
        return r

    monkeypatch.setattr(mod, "contact_render_inputs", recording)
    # kind -> index of the panel that share_binning composites on its partner's lists
    for kind, shared_panel, n_panels in (("results", 3, 4), ("gt_eval", 1, 2), ("acc_gt_eval", 0, 2)):
        off = CompositeRenderer(hand, obj, kind, skin_colors=skin, acc_contacts=accc)
        on = CompositeRenderer(hand, obj, kind, skin_colors=skin, acc_contacts=accc, share_binning=True)
        assert on.share_binning and not off.share_binning
        for batch in batches:
            a = off.render(batch).render.detach()
            del seen[:]
            b = on.render(batch).render.detach()
            bound = rounding_bound(max(seen))      # (the last forward is the shared pair's first render)
            assert tuple(a.shape) == tuple(b.shape) == (H, n_panels * W, 3)
            for p in range(n_panels):
                pa, pb = a[:, p * W:(p + 1) * W], b[:, p * W:(p + 1) * W]
                if p == shared_panel:
                    err = float((pa - pb).abs().max())
                    print("%s panel %d: max diff %.3e, bound %.3e" % (kind, p, err, bound))
                    assert err <= bound, (kind, p, err, bound)
                    assert float((pb - batch["bg_color"].to(DEV)).abs().max()) > 0.1      # (not an empty panel)
                else:
                    assert torch.equal(pa, pb), (kind, p)
        if kind != "acc_gt_eval":
            assert off.n_frames == on.n_frames == 2 and torch.equal(off.acc, on.acc)

"""GPU: the feature render's backward (mgr_raster_blend_features_backward, rasterizer.rasterize_views_features, render_gaussians'
extra outputs under autograd) -- gradients of a loss on feature, depth and alpha maps.

Checks: (1) with the forward's colours as features the gradients must be the colour backward's (both sides sum the same
products: max-rel-err 1e-4, no oracle, no threshold flip can enter); (2) against oracle.RasterOracle, whose backward
composites any three colours: C channels + depth + alpha are ceil(C/3) runs plus one run with colours (z, 1, 0) on a zero
background (the construction tests/test_feature_grad_cpu.py checks against central differences), bars of
test_image_and_gradient_parity (fp32 1e-4, fp64 2e-3); views and strides; every element written, workspace read only,
bit-reproducible; refusals; the autograd surface; a small optimisation on alpha and depth maps.

Measured on one MI355X (max-rel-err, worst gradient tensor of the case): against the colour backward a 7.6e-07, b 4.9e-07, giant
9.6e-07; against the fp32 oracle at most 4.6e-06 and the fp64 oracle at most 1.1e-03 over all cases (the colour backward on the same
scenes against the fp32 oracle: a 2.0e-06, b 1.3e-06); the end-to-end run ends 6.0e-04 from the true offset (start 2e-02), its loss
falls from 5.4e-02 to 1.1e-03."""
import functools

import numpy as np
import pytest
import torch

from oracle import RasterOracle

from test_gpu_feature_render import BG, DEV, NAN, dev, scene, tile_pairs
from util import cam_args, cam_table_np, make_camera, max_rel_err

pytestmark = pytest.mark.gpu

GEO = ("means3D", "cov3D", "opacity", "means2D")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def upstream(name):
    """34 upstream gradient images of a scene: channels 0..31 for the features, 32 the depth, 33 the alpha."""
    s = scene(name)
    g = np.random.default_rng(77).normal(size=(34, s.H, s.W)).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def features32(name):
    s = scene(name)
    g = np.random.default_rng(78)
    f, b = g.uniform(0, 1, size=(s.m.shape[0], 32)).astype(np.float32), g.uniform(0.1, 0.9, size=(32,)).astype(np.float32)
    f.setflags(write=False)
    b.setflags(write=False)
    return f, b


def leaves(s, cams, feat=None):
    L = dict(means3D=dev(s.m).requires_grad_(True), cov3D=dev(s.c).requires_grad_(True), colors=dev(s.col).requires_grad_(True),
             opacity=dev(s.op).requires_grad_(True),
             means2D=torch.zeros((len(cams), s.m.shape[0], 3), device=DEV, requires_grad=True))
    if feat is not None:
        L["features"] = (feat.clone() if torch.is_tensor(feat) else dev(feat)).requires_grad_(True)
    return L


def render(s, cams, L, fbg=None, depth=False, alpha=False, bg=BG):
    from manus_amd.rasterizer import rasterize_views_features
    ct = torch.from_numpy(cam_table_np(cams)).to(DEV)
    return rasterize_views_features(ct, L["means3D"], L["means2D"], L["colors"], L["opacity"], L["cov3D"], dev(bg), s.W, s.H,
                                    features=L.get("features"), feature_bg=fbg, depth=depth, alpha=alpha)


def grads(L, zero=True):
    out = {k: (v.grad.detach().cpu().numpy().copy() if v.grad is not None else None) for k, v in L.items()}
    if zero:
        for v in L.values():
            v.grad = None
    return out


def _oracle(s, col, bg, dtype):
    a = cam_args(s.cam)
    return RasterOracle(a["W"], a["H"], a["tanfovx"], a["tanfovy"], a["view"], a["proj"], s.m, s.c, col, s.op, bg, dtype=dtype)


def pad3(a, axis):
    """The first three entries along `axis`, zero-padded to three."""
    a = np.asarray(a)
    n = a.shape[axis]
    if n == 3:
        return a
    shape = list(a.shape)
    shape[axis] = 3 - n
    return np.concatenate([a, np.zeros(shape, a.dtype)], axis)


@functools.lru_cache(maxsize=None)
def group_backward(name, dtype, i, n):
    """Oracle backward of feature channels 3i .. 3i + n - 1 (n <= 3) under their upstream gradients."""
    s = scene(name)
    f, b = features32(name)
    o = _oracle(s, pad3(f[:, 3 * i:3 * i + n], 1), pad3(b[3 * i:3 * i + n], 0), dtype)
    return o.backward(pad3(upstream(name)[3 * i:3 * i + n], 0))


@functools.lru_cache(maxsize=None)
def depth_alpha_backward(name, dtype, depth, alpha):
    s = scene(name)
    o = _oracle(s, np.zeros((s.m.shape[0], 3), np.float32), np.zeros(3, np.float32), dtype)
    zc = np.zeros((s.m.shape[0], 3), np.float64)
    zc[:, 0] = np.where(o.radii > 0, o.geom()["depth"], 0)
    zc[:, 1] = 1.0
    g = upstream(name)
    z = np.zeros_like(g[0])
    return _oracle(s, zc, np.zeros(3), dtype).backward(np.stack([g[32] if depth else z, g[33] if alpha else z, z]))


def oracle_reference(name, dtype, C, depth, alpha):
    s = scene(name)
    N = s.m.shape[0]
    ref = dict(means3D=np.zeros((N, 3)), cov3D=np.zeros((N, 6)), opacity=np.zeros(N), means2D=np.zeros((N, 3)),
               features=np.zeros((N, C)))
    for i in range((C + 2) // 3):
        n = min(3, C - 3 * i)
        b = group_backward(name, dtype, i, n)
        for k in GEO:
            ref[k] += b[k]
        ref["features"][:, 3 * i:3 * i + n] = b["colors"][:, :n]
    if depth or alpha:
        b = depth_alpha_backward(name, dtype, depth, alpha)
        for k in GEO:
            ref[k] += b[k]
        view = np.asarray(cam_args(s.cam)["view"], np.float64).reshape(4, 4)
        ref["means3D"] += b["colors"][:, :1] * view[:3, 2][None]
    return ref


@functools.lru_cache(maxsize=None)
def colour_backward_error(name):
    """max-rel-err of the COLOUR backward against the fp32 oracle on the scene, under upstream channels 0..2: the yardstick a
    scene must pass before the feature backward is judged on it."""
    s = scene(name)
    L = leaves(s, [s.cam])
    from manus_amd.rasterizer import rasterize_views
    ct = torch.from_numpy(cam_table_np([s.cam])).to(DEV)
    img, _ = rasterize_views(ct, L["means3D"], L["means2D"], L["colors"], L["opacity"], L["cov3D"], dev(BG), s.W, s.H)
    img.backward(dev(upstream(name)[None, :3]))
    got = grads(L)
    ob = _oracle(s, s.col, BG, np.float32).backward(upstream(name)[:3])
    return max(max_rel_err(got[k][0] if k == "means2D" else got[k], ob[k]) for k in GEO + ("colors",))


def maps_loss(extras, name, C, depth, alpha):
    g = dev(upstream(name))
    loss = 0.0
    if C:
        loss = loss + (extras["features"][0] * g[:C]).sum()
    if depth:
        loss = loss + (extras["depth"][0] * g[32]).sum()
    if alpha:
        loss = loss + (extras["alpha"][0] * g[33]).sum()
    return loss


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the colour backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "giant"])
def test_colours_as_features_give_the_colour_backward(name):
    s = scene(name)
    L = leaves(s, [s.cam], feat=s.col)
    color, _, extras = render(s, [s.cam], L, fbg=dev(BG))
    if name == "giant":
        assert tile_pairs(0) > 16384
    g = dev(upstream(name)[None, :3])
    color.backward(g)
    ref = grads(L)
    extras["features"].backward(g)
    got = grads(L)
    assert got["colors"] is None and ref["features"] is None
    worst = 0.0
    for k in GEO:
        e = max_rel_err(got[k], ref[k])
        worst = max(worst, e)
        assert np.abs(ref[k]).max() > 0 and e < 1e-4, (k, e)
    e = max_rel_err(got["features"], ref["colors"])
    print("%s: feature backward vs colour backward, worst max-rel-err %.3e" % (name, max(worst, e)))
    assert e < 1e-4, ("features", e)
    assert (got["means2D"][..., 2] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the oracle
# ---------------------------------------------------------------------------------------------------------------------
CASES = [(0, False, True), (0, True, True), (1, False, False), (1, True, True), (3, False, False), (3, True, False), (8, True, False),
         (8, False, True), (9, False, False), (9, True, True), (32, False, False), (32, True, True)]


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("C,depth,alpha", CASES)
def test_gradients_against_the_oracle(name, C, depth, alpha):
    yard = colour_backward_error(name)
    print("%s: colour backward vs fp32 oracle %.3e" % (name, yard))
    assert yard < 1e-4, "the scene is the wrong one (take another seed): the colour backward misses the bar on it"
    s = scene(name)
    f, b = features32(name)
    L = leaves(s, [s.cam], feat=f[:, :C] if C else None)
    _, _, extras = render(s, [s.cam], L, fbg=dev(b[:C]) if C else None, depth=depth, alpha=alpha)
    maps_loss(extras, name, C, depth, alpha).backward()
    got = grads(L)
    assert got["colors"] is None
    r32, r64 = oracle_reference(name, np.float32, C, depth, alpha), oracle_reference(name, np.float64, C, depth, alpha)
    for k in GEO + (("features",) if C else ()):
        a = got[k][0] if k == "means2D" else got[k]
        e32, e64 = max_rel_err(a, r32[k]), max_rel_err(a, r64[k])
        print("%s C=%d depth=%d alpha=%d %s: fp32 %.3e fp64 %.3e" % (name, C, depth, alpha, k, e32, e64))
        assert np.abs(r64[k]).max() > 0
        assert e32 < 1e-4 and e64 < 2e-3, (k, e32, e64)


# ---------------------------------------------------------------------------------------------------------------------
# 4. views and strides
# ---------------------------------------------------------------------------------------------------------------------
def test_two_views_shared_and_per_view_features():
    s = scene("a")
    cams = [s.cam, make_camera(s.W, s.H, pos=(-0.4, 0.3, -1.4))]
    N = s.m.shape[0]
    per_view = torch.rand((2, N, 5), generator=torch.Generator().manual_seed(5)).to(DEV)
    fbg = dev(scene("a").bgf[:5])
    g = dev(np.random.default_rng(6).normal(size=(2, 7, s.H, s.W)).astype(np.float32))

    def run(cs, feat, gv):
        L = leaves(s, cs, feat=feat)
        _, _, ex = render(s, cs, L, fbg=fbg, depth=True, alpha=True)
        ((ex["features"] * gv[:, :5]).sum() + (ex["depth"] * gv[:, 5]).sum() + (ex["alpha"] * gv[:, 6]).sum()).backward()
        return grads(L)

    for feat_of, feat_both in ((lambda v: per_view[0], per_view[0]), (lambda v: per_view[v], per_view)):
        single = [run([cams[v]], feat_of(v), g[v:v + 1]) for v in range(2)]
        both = run(cams, feat_both, g)
        for k in ("means3D", "cov3D", "opacity"):
            want = single[0][k].astype(np.float64) + single[1][k]
            e = max_rel_err(both[k], want)
            assert e < 1e-6, (k, e)
        for v in range(2):
            assert np.array_equal(both["means2D"][v], single[v]["means2D"][0]), v
        if feat_both.dim() == 2:
            e = max_rel_err(both["features"], single[0]["features"].astype(np.float64) + single[1]["features"])
            assert e < 1e-6, ("features", e)
        else:
            for v in range(2):
                assert np.array_equal(both["features"][v], single[v]["features"]), v


# ---------------------------------------------------------------------------------------------------------------------
# 5. fully written, read only, deterministic (raw ABI)
# ---------------------------------------------------------------------------------------------------------------------
def raw_backward(ws, ct, m, c, feat, C, with_depth, out, out_a, g_out, g_a, W, H, scratch=None, scratch_bytes=None, cap=None,
                 nbytes=None, N=None, V=1):
    from manus_amd._lib import lib, ptr, stream
    N = m.shape[0] if N is None else N
    cap = ws.cap if cap is None else cap
    need = int(lib().mgr_raster_feat_backward_workspace_bytes(V, N, C, W, H, cap))
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    o = dict(means3D=torch.full((V, N, 3), NAN, device=DEV), means2D=torch.full((V, N, 3), NAN, device=DEV),
             opacity=torch.full((V, N), NAN, device=DEV), cov3D=torch.full((V, N, 6), NAN, device=DEV),
             features=torch.full((V, N, C), NAN, device=DEV) if C else None)
    rc = lib().mgr_raster_blend_features_backward(V, N, C, W, H, ptr(ct), ptr(m), 0, ptr(c), 0, ptr(feat), 0, None, int(with_depth),
                                                  ptr(out), ptr(out_a), ptr(g_out), ptr(g_a), ptr(o["means3D"]), ptr(o["means2D"]),
                                                  ptr(o["opacity"]), ptr(o["cov3D"]), ptr(o["features"]), ptr(ws.buf),
                                                  ws.nbytes if nbytes is None else nbytes, cap, ptr(scratch),
                                                  need if scratch_bytes is None else scratch_bytes, 0, stream())
    return rc, o


def test_every_element_written_workspace_read_only_and_repeatable():
    from manus_amd import rasterizer as rz
    from manus_amd.rasterizer import blend_features, rasterize_views
    s = scene("b")
    # three Gaussians no view sees: behind the camera, far off screen, inside the near plane
    extra = np.array([[0.6, -0.4, -3.0], [50.0, 0, 0], [0.3, -0.2, -1.45]], np.float32)
    m = np.concatenate([s.m, extra])
    c = np.concatenate([s.c, s.c[:3]])
    col = np.concatenate([s.col, s.col[:3]])
    op = np.concatenate([s.op, s.op[:3]])
    N, W, H, C = m.shape[0], s.W, s.H, 9
    feat = torch.rand((N, C), generator=torch.Generator().manual_seed(3)).to(DEV)
    ct = torch.from_numpy(cam_table_np([s.cam])).to(DEV)
    tm, tc = dev(m).requires_grad_(True), dev(c)
    img, radii = rasterize_views(ct, tm, torch.zeros((1, N, 3), device=DEV), dev(col), dev(op), tc, dev(BG), W, H)
    ws = rz.context().last_ws
    maps = blend_features(feat, bg=dev(s.bgf), depth=True, alpha=True)
    out = torch.cat([maps["features"], maps["depth"][:, None]], 1).contiguous()
    g = torch.Generator().manual_seed(4)
    g_out, g_a = torch.randn((1, C + 1, H, W), generator=g).to(DEV), torch.randn((1, H, W), generator=g).to(DEV)
    before = ws.buf.clone()
    rc, first = raw_backward(ws, ct, tm.detach(), tc, feat, C, True, out, maps["alpha"], g_out, g_a, W, H)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(ws.buf, before)                                   # the workspace is only read
    culled = radii[0] == 0
    assert int(culled.sum()) >= 3 and int((~culled).sum()) > 100
    for k, v in first.items():
        assert torch.isfinite(v).all(), k
        assert (v[0][culled] == 0).all(), k
        assert float(v.abs().max()) > 0, k
    # a scratch full of stale tags changes nothing: the call clears what it relies on
    need = int(rz.lib().mgr_raster_feat_backward_workspace_bytes(1, N, C, W, H, ws.cap))
    dirty = torch.full((need,), 1, dtype=torch.uint8, device=DEV)
    rc, again = raw_backward(ws, ct, tm.detach(), tc, feat, C, True, out, maps["alpha"], g_out, g_a, W, H, scratch=dirty)
    assert rc == 0
    img.sum().backward()                                                 # a colour backward in between
    rc, third = raw_backward(ws, ct, tm.detach(), tc, feat, C, True, out, maps["alpha"], g_out, g_a, W, H)
    assert rc == 0
    for k in first:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], third[k]), k
    # one gradient at a time: the parts add up to the whole (the expression is linear in g)
    rc, only_a = raw_backward(ws, ct, tm.detach(), tc, feat, C, True, None, maps["alpha"], None, g_a, W, H)
    assert rc == 0 and (only_a["features"] == 0).all()
    rc, only_f = raw_backward(ws, ct, tm.detach(), tc, feat, C, True, out, None, g_out, None, W, H)
    assert rc == 0 and torch.equal(only_f["features"], first["features"])
    for k in ("means3D", "cov3D", "opacity", "means2D"):
        e = max_rel_err((only_a[k] + only_f[k]).cpu().numpy(), first[k].cpu().numpy())
        assert e < 1e-5, (k, e)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from manus_amd import rasterizer as rz
    from manus_amd._lib import ManusHipError, lib, ptr, stream
    s = scene("b")
    N, W, H, C = s.m.shape[0], s.W, s.H, 3
    ct = torch.from_numpy(cam_table_np([s.cam])).to(DEV)
    m, c, col, op, bg, feat = dev(s.m), dev(s.c), dev(s.col), dev(s.op), dev(BG), dev(s.feat[:, :3])
    out, alpha = torch.zeros((1, C, H, W), device=DEV), torch.zeros((1, H, W), device=DEV)
    g_out, g_a = torch.ones((1, C, H, W), device=DEV), torch.ones((1, H, W), device=DEV)
    call = lambda ws, **k: raw_backward(ws, ct, m, c, feat, C, False, out, alpha, g_out, g_a, k.pop("W", W), k.pop("H", H), **k)

    def refused(rc_o, code, text=None):
        rc, o = rc_o
        assert rc == code, rc
        assert all(bool(torch.isnan(v).all()) for v in o.values() if v is not None)      # nothing was launched
        if text:
            assert text in lib().mgr_last_error(), lib().mgr_last_error()

    fresh = rz.RasterWorkspace(torch.device(DEV), 1, N, W, H, 8 * N)
    refused(call(fresh), -8, b"no forward")
    img = torch.empty((1, 3, H, W), device=DEV)
    radii = torch.empty((1, N), dtype=torch.int32, device=DEV)
    fwd = lambda ws, debug: lib().mgr_raster_forward(1, N, W, H, ptr(ct), ptr(bg), ptr(m), 0, ptr(c), 0, ptr(col), 0, ptr(op), 0,
                                                     ptr(img), ptr(radii), ptr(ws.buf), ws.nbytes, ws.cap, debug, stream())
    assert fwd(fresh, 2) == 0                                            # MGR_FWD_NO_BLEND
    refused(call(fresh), -8, b"blend")
    assert fwd(fresh, 0) == 0
    rc, ok = call(fresh)
    assert rc == 0 and all(bool(torch.isfinite(v).all()) for v in ok.values())
    refused(call(fresh, W=24, H=16), -8, b"another")                    # other sizes
    refused(call(fresh, cap=fresh.cap + 64, nbytes=1 << 40), -8, b"another")
    refused(call(fresh, scratch_bytes=1024), -2, b"scratch")            # scratch too small
    rc, _ = raw_backward(fresh, ct, m, c, feat, C, False, out, alpha, None, None, W, H)
    assert rc == -1                                                      # both gradients NULL
    word = fresh.buf[4:8].view(torch.int32)                              # MgrHeader::overflow
    word.fill_(1)
    refused(call(fresh), -8, b"overflow")
    word.fill_(0)
    assert call(fresh)[0] == 0
    # under autograd: a newer forward on the leased workspace before .backward()
    L = leaves(s, [s.cam])
    _, _, extras = render(s, [s.cam], L, alpha=True)
    ws = rz.context().last_ws
    assert ws.busy
    assert fwd(ws, 0) == 0
    with pytest.raises(ManusHipError):
        extras["alpha"].sum().backward()


# ---------------------------------------------------------------------------------------------------------------------
# 7. autograd surface
# ---------------------------------------------------------------------------------------------------------------------
def test_colour_and_alpha_losses_add_and_share_one_lease():
    from manus_amd import rasterizer as rz
    s = scene("a")
    L = leaves(s, [s.cam])
    color, _, extras = render(s, [s.cam], L, alpha=True)
    (color.sum() + extras["alpha"].sum()).backward()
    both = grads(L)
    del color, extras
    color, _, extras = render(s, [s.cam], L, alpha=True)
    ws = rz.context().last_ws
    color.sum().backward()
    assert ws.busy                                                       # the alpha node still needs the lists
    only_c = grads(L)
    extras["alpha"].sum().backward()
    only_a = grads(L)
    del color, extras
    assert not ws.busy
    for k in both:
        want = only_c[k].astype(np.float64) + (only_a[k] if only_a[k] is not None else 0.0)
        assert max_rel_err(both[k], want) < 1e-6, k
    # the colour inputs need no gradient, the features do: the workspace stays leased for the feature node
    feat = dev(s.feat[:, :4]).requires_grad_(True)
    ct = torch.from_numpy(cam_table_np([s.cam])).to(DEV)
    _, _, ex = rz.rasterize_views_features(ct, dev(s.m), torch.zeros((1, s.m.shape[0], 3), device=DEV), dev(s.col), dev(s.op), dev(s.c),
                                           dev(BG), s.W, s.H, features=feat)
    held = rz.context().last_ws
    assert held.busy
    ex["features"].sum().backward()
    assert feat.grad is not None and float(feat.grad.abs().max()) > 0
    del ex
    assert not held.busy


def test_render_gaussians_alpha_carries_gradient_only_when_recording():
    from types import SimpleNamespace
    from manus_amd.render import render_gaussians
    s = scene("a")
    c = s.cam
    camera = SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                             world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32),
                             full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32),
                             camera_center=torch.tensor(c["camera_center"], dtype=torch.float32)[None])
    plain = render_gaussians(dev(s.m), dev(s.c), dev(s.m), None, dev(s.op), camera, torch.tensor(BG), dev(s.col), return_alpha=True,
                             return_depth=True)
    assert plain["alpha"].grad_fn is None and plain["depth"].grad_fn is None and not plain["alpha"].requires_grad
    m, op = dev(s.m).requires_grad_(True), dev(s.op).requires_grad_(True)
    rec = render_gaussians(m, dev(s.c), dev(s.m), None, op, camera, torch.tensor(BG), dev(s.col), return_alpha=True, return_depth=True)
    assert sorted(rec) == sorted(plain)
    assert rec["alpha"].grad_fn is not None and rec["depth"].grad_fn is not None
    for k in ("render", "radii", "alpha", "depth", "visibility_filter"):
        assert torch.equal(rec[k].detach(), plain[k]), k
    (rec["alpha"].sum() + rec["depth"].sum()).backward()
    assert float(m.grad.abs().max()) > 0 and float(op.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_alpha_and_depth_loss_recovers_a_shift():
    from manus_amd.rasterizer import blend_features, rasterize_views, rasterize_views_features
    s = scene("a")
    N = s.m.shape[0]
    ct = torch.from_numpy(cam_table_np([s.cam])).to(DEV)
    m2d = torch.zeros((1, N, 3), device=DEV)
    col, op, c, bg = dev(s.col), dev(s.op), dev(s.c), dev(BG)
    with torch.no_grad():
        rasterize_views(ct, dev(s.m), m2d, col, op, c, bg, s.W, s.H)
        target = blend_features(depth=True, alpha=True)
    shifted = dev(s.m) + torch.tensor([0.02, 0.0, 0.0], device=DEV)
    truth = torch.tensor([-0.02, 0.0, 0.0], device=DEV)
    offset = torch.zeros(3, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([offset], lr=1e-3)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        _, _, ex = rasterize_views_features(ct, shifted + offset, m2d, col, op, c, bg, s.W, s.H, depth=True, alpha=True)
        loss = (ex["alpha"] - target["alpha"]).abs().mean() + (ex["depth"] - target["depth"]).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    err = float((offset.detach() - truth).norm())
    print("offset error %.3e (start 2e-02), loss %.4e -> %.4e" % (err, losses[0], losses[-1]))
    assert err < 0.02 and losses[-1] < losses[0]

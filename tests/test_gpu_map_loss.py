"""GPU: mask and depth-map supervision on the fused step -- mgr_map_loss against its fp64 restatement (tests/map_loss_ref.py),
mgr_views_maps_backward against the operator route under autograd (ops.skin_weights -> ops.lbs_cov ->
rasterize_views_features -> .backward), its accumulate / hygiene / refusal contracts, and HipViewCompute with the map terms on,
fused against fused=False.

Bars: tensor-wide max_rel_err (tests/util.py) below 1e-4, the project's fused-against-modular bar; every row is compared.
Measured on MI355X (gfx950), 56x40, 2000 Gaussians: mgr_map_loss sums at most 3.1e-8 relative (bar 1e-6); mgr_views_maps_backward
against the operator route at most 6.0e-6 (composite, B = 32, a Gaussian over the whole image, _rotation), typically 1e-7 .. 4e-7;
the colour gradient's own fused-against-operator error on the same scenes at most 8.9e-7; HipViewCompute fused against fused=False
with the terms on at most 8.6e-7."""
import functools

import numpy as np
import pytest
import torch

from map_loss_ref import map_loss_grads_fp32, map_loss_ref, term_sums_fp64
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-4
W, H = 56, 40                      # a ragged edge: 3.5 x 2.5 tiles
LEAVES = ("_xyz", "_scaling", "_rotation", "_opacity")


# ---------------------------------------------------------------------------------------------------------------------
# 1. mgr_map_loss
# ---------------------------------------------------------------------------------------------------------------------
def _maps(V, Hh, Ww, seed):
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand((V, Hh, Ww), generator=g)
    mask = (torch.rand((V, Hh, Ww), generator=g) * 3 - 1).clamp(0, 1)                     # zeros, ones, fractions
    eq = torch.rand((V, Hh, Ww), generator=g) < 0.1
    mask = torch.where(eq, alpha, mask)                                                    # pixels equal to alpha
    depth = torch.rand((V, Hh, Ww), generator=g) * 3
    dtgt = torch.where(torch.rand((V, Hh, Ww), generator=g) < 0.1, depth, torch.rand((V, Hh, Ww), generator=g) * 3)
    return [t.to(DEV) for t in (alpha, mask, depth, dtgt)]


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("hw", [(17, 23), (48, 64)])
@pytest.mark.parametrize("with_depth", [False, True])
def test_map_loss_against_the_fp64_restatement(V, hw, with_depth):
    from manus_amd import ops
    alpha, mask, depth, dtgt = _maps(V, hw[0], hw[1], 10 * V + hw[0])
    w_mask, w_depth, k = 0.7, 0.3, 1.7
    d, t = (depth, dtgt) if with_depth else (None, None)
    sums, g_a, g_d = ops.map_loss_grad(alpha, mask, w_mask, d, t, w_depth, k)
    sums2, g_a2, g_d2 = ops.map_loss_grad(alpha, mask, w_mask, d, t, w_depth, k)
    ra, rd = map_loss_grads_fp32(alpha, mask, d, t, w_mask, w_depth, k)
    assert torch.equal(g_a, ra)
    assert bool((g_a[alpha == mask] == 0).all()) and bool((alpha == mask).any())
    if with_depth:
        assert torch.equal(g_d, rd) and bool((g_d[depth == dtgt] == 0).all())
    else:
        assert g_d is None
    lm, ld = term_sums_fp64(alpha, mask, d, t)
    tot = float(np.float32(w_mask)) * float(lm) + (float(np.float32(w_depth)) * float(ld) if with_depth else 0.0)
    got = sums.double().cpu()
    print("map loss V=%d %s depth=%d: rel err mask %.2e depth %.2e total %.2e" % (
        V, hw, with_depth, abs(float(got[0]) - float(lm)) / float(lm), abs(float(got[1]) - float(ld)) / max(float(ld), 1e-30),
        abs(float(got[2]) - tot) / tot))
    assert abs(float(got[0]) - float(lm)) <= 1e-6 * float(lm)
    assert abs(float(got[1]) - float(ld)) <= 1e-6 * float(ld)
    assert abs(float(got[2]) - tot) <= 1e-6 * tot
    ref = map_loss_ref(alpha, mask, d, t, w_mask, w_depth, k)                               # the fp64 statement itself
    assert abs(float(got[2]) - float(ref["total"])) <= 1e-6 * float(ref["total"])
    assert torch.equal(sums, sums2) and torch.equal(g_a, g_a2) and (g_d is None or torch.equal(g_d, g_d2))


def test_map_loss_non_finite_input_and_autograd():
    from manus_amd import losses, ops
    alpha, mask, depth, dtgt = _maps(2, 17, 23, 5)
    bad = alpha.clone()
    bad[1, 3, 4] = float("nan")
    sums, _, _ = ops.map_loss_grad(bad, mask, 1.0, depth, dtgt, 1.0)
    assert bool(torch.isnan(sums[0])) and bool(torch.isnan(sums[2])) and bool(torch.isfinite(sums[1]))
    inf = depth.clone()
    inf[0, 0, 0] = float("inf")
    m1 = mask.clone()
    m1[0, 0, 0] = 1.0
    sums, _, _ = ops.map_loss_grad(alpha, m1, 1.0, inf, dtgt, 1.0)
    assert bool(torch.isnan(sums[1])) and bool(torch.isnan(sums[2])) and bool(torch.isfinite(sums[0]))
    # losses.map_loss: the same kernel under autograd
    a, d = alpha.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    loss, s3 = losses.map_loss(a, mask, 0.7, d, dtgt, 0.3)
    (loss * 2.0).backward()
    ra, rd = map_loss_grads_fp32(alpha, mask, depth, dtgt, 0.7, 0.3, 1.0)
    assert torch.equal(a.grad, ra * 2.0) and torch.equal(d.grad, rd * 2.0)
    assert float(loss.detach()) == float(s3[2]) and not s3.requires_grad


# ---------------------------------------------------------------------------------------------------------------------
# scenes (made once, never modified) and the two routes
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(kind, B, V, giant=False, n=2000):
    """make_scene at 56x40; B != 21: the 21 transforms re-targeted to B (grid' = grid @ M, M non-negative without a zero row;
    transforms'[v,b] = transforms[v, b % 21]).  giant: Gaussian 0 covers the whole image."""
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=n, kind=kind, seed=6, grid_res=24, n_cameras=V, width=W, height=H, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device="cpu")
    if kind != "object" and B != 21:
        g = torch.Generator().manual_seed(400 + B)
        M = torch.rand((21, B), generator=g) ** 2
        M[torch.rand((21, B), generator=g) < 0.4] = 0.0
        M[torch.arange(21), torch.arange(21) % B] += 0.5
        sc["grid"] = (sc["grid"].double() @ M.double()).float()
        sc["transforms"] = sc["transforms"][:, torch.arange(B) % 21].contiguous()
    if giant:
        p = sc["params"]
        p["_xyz"][0] = p["_xyz"].mean(0)
        p["_scaling"][0] = float(np.log(0.25))
        p["_opacity"][0] = 0.0
    ct = camera_table(sc["cameras"], DEV)
    out = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in sc.items() if k != "params"}
    out["params"] = {k: v.to(DEV) for k, v in sc["params"].items()}
    return out, ct


def upstream(V, seed=0):
    g = torch.Generator().manual_seed(900 + seed)
    return (torch.randn((V, H, W), generator=g).to(DEV), torch.randn((V, H, W), generator=g).to(DEV))


def rand_targets(V, seed=1):
    return torch.rand((V, 3, H, W), generator=torch.Generator().manual_seed(seed)).to(DEV)


def operator_route(sc, ct, V, g_alpha, g_depth, g_img=None):
    """dL/d(leaves) of sum(alpha g_alpha) + sum(depth g_depth) (+ sum(image g_img)) through the modular operators."""
    from manus_amd.engine import HipViewCompute
    mod = HipViewCompute(sc, rand_targets(V), ct, fused=False)
    img, _, _, ex = mod.forward_views(list(range(V)), maps=(True, True))
    roots, gs = [], []
    for r, g in ((ex["alpha"], g_alpha), (ex["depth"], g_depth), (img, g_img)):
        if g is not None:
            roots.append(r)
            gs.append(g)
    torch.autograd.backward(roots, gs)
    return {k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in mod.params.items()}


class Fused:
    """A fused step on a scene, then raw calls of mgr_views_maps_backward on the workspace it left."""

    def __init__(self, sc, ct, V, **kw):
        from manus_amd import rasterizer as rz
        from manus_amd.engine import HipViewCompute
        self.V, self.ids = V, list(range(V))
        self.hc = HipViewCompute(sc, rand_targets(V), ct, fused=True, persistent_grads=False, **kw)
        self.out = self.hc(self.ids, 1.0)
        self.ws = rz.context(DEV).last_ws
        self.maps = rz.blend_features(depth=True, alpha=True, device=DEV)
        p = {k: v.detach() for k, v in self.hc.params.items()}
        self.p, self.N, self.na = p, p["_xyz"].shape[0], self.hc.n_art
        self.w, self.B = self.hc._skin_weights(p["_xyz"], self.na)
        self.sel = self.hc._select(self.ids)

    def scratch_bytes(self):
        from manus_amd._lib import lib
        return int(lib().mgr_views_maps_backward_workspace_bytes(self.V, self.N, W, H, self.ws.cap))

    def outputs(self, fill=None):
        mk = (lambda s: torch.full(s, fill, device=DEV)) if fill is not None else (lambda s: torch.empty(s, device=DEV))
        o = {"_xyz": mk((self.N, 3)), "_scaling": mk((self.N, 3)), "_rotation": mk((self.N, 4)), "_opacity": mk((self.N, 1))}
        o["_skin_w"] = mk((self.na, self.B)) if self.na else None
        return o

    def call(self, g_alpha, g_depth, accumulate=0, o=None, scratch=None, scratch_bytes=None, ws_buf=None, V=None, Wd=None, cap=None):
        from manus_amd._lib import lib, ptr, stream
        o = o if o is not None else self.outputs()
        nb = self.scratch_bytes()
        scratch = scratch if scratch is not None else torch.empty(nb, dtype=torch.uint8, device=DEV)
        p, ws = self.p, self.ws
        buf = ws.buf if ws_buf is None else ws_buf
        rc = lib().mgr_views_maps_backward(
            self.V if V is None else V, self.N, self.B, self.na, W if Wd is None else Wd, H, ptr(self.sel["cams"]), ptr(p["_xyz"]),
            ptr(p["_scaling"]), ptr(p["_rotation"]), ptr(p["_opacity"].reshape(-1)), ptr(self.w), ptr(self.sel["T"]),
            ptr(self.maps["alpha"]) if g_alpha is not None else None, ptr(self.maps["depth"].contiguous()) if g_depth is not None else None,
            ptr(g_alpha), ptr(g_depth), accumulate, ptr(o["_xyz"]), ptr(o["_scaling"]), ptr(o["_rotation"]), ptr(o["_opacity"]),
            ptr(o["_skin_w"]), ptr(buf), buf.numel(), ws.cap if cap is None else cap, ptr(scratch),
            nb if scratch_bytes is None else scratch_bytes, 1, stream())
        return rc, o

    def with_skin(self, o):
        """The leaf gradients with the skin weights' path folded into d_xyz, as the step does (full-row mgr_skin_weights_bwd)."""
        from manus_amd._lib import check, lib, ptr, stream
        g = {k: o[k].clone() for k in LEAVES}
        if self.na:
            s, sg = self.hc.s, self.hc.grid
            check(lib().mgr_skin_weights_bwd(self.na, ptr(self.p["_xyz"]), ptr(sg.data), sg.D, sg.H, sg.W, sg.B, sg.stride, ptr(s["grid_center"]),
                                             ptr(s["grid_scale"]), ptr(o["_skin_w"]), ptr(g["_xyz"]), 1, stream()), "mgr_skin_weights_bwd")
        return g


def compare(tag, got, ref, names=LEAVES):
    worst = 0.0
    for k in names:
        a, b = got[k].double().cpu().numpy(), ref[k].double().cpu().numpy().reshape(got[k].shape)
        assert float(np.abs(b).max()) > 0.0, (tag, k, "the reference gradient is all zero")
        e = max_rel_err(a, b)
        print("%s %-10s max_rel_err %.3e" % (tag, k, e))
        worst = max(worst, e)
    return worst


CASES = [("hand", 21, 1, "both", False), ("hand", 21, 2, "both", False), ("hand", 21, 3, "both", True), ("hand", 21, 8, "both", False),
         ("hand", 21, 9, "both", False), ("hand", 1, 3, "alpha", False), ("hand", 32, 8, "depth", False), ("hand", 21, 3, "alpha", False),
         ("hand", 21, 3, "depth", False), ("composite", 21, 3, "both", False), ("composite", 21, 9, "alpha", False),
         ("composite", 32, 2, "depth", True), ("object", 21, 2, "both", False), ("object", 21, 8, "depth", False),
         ("object", 21, 1, "alpha", True)]


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the operator route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,V,case,giant", CASES)
def test_maps_backward_against_the_operator_route(kind, B, V, case, giant):
    sc, ct = scene(kind, B, V, giant)
    ga, gd = upstream(V)
    ga, gd = (ga if case != "depth" else None), (gd if case != "alpha" else None)
    ref = operator_route(sc, ct, V, ga, gd)
    fz = Fused(sc, ct, V)
    if giant:
        assert float(fz.maps["alpha"].min()) > 0.0          # Gaussian 0 reaches every pixel
    rc, o = fz.call(ga, gd)
    assert rc == 0
    got = fz.with_skin(o)
    tag = "%s B=%d V=%d %s%s" % (kind, B, V, case, " giant" if giant else "")
    worst = compare(tag, got, ref)
    # the colour gradient's own fused-against-operator error on the same scene (existing code), for the record
    g_img = torch.randn((V, 3, H, W), generator=torch.Generator().manual_seed(3)).to(DEV)
    ref_c = operator_route(sc, ct, V, None, None, g_img=g_img)
    out_c = fz.hc._step_direct(fz.ids, 1.0, g_img=g_img)
    compare(tag + " [colour]", out_c["grads"], ref_c)          # (printed only: the bar on it is test_gpu_fused.py's)
    assert worst < BAR, (tag, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. accumulate and hygiene
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,V", [("composite", 3), ("hand", 9)])
def test_accumulate_scratch_repeatability_and_read_only_workspace(kind, V):
    sc, ct = scene(kind, 21, V)
    ga, gd = upstream(V, 1)
    fz = Fused(sc, ct, V)
    before = fz.ws.buf.clone()
    nb = fz.scratch_bytes()
    rc, base = fz.call(ga, gd, scratch=torch.zeros(nb, dtype=torch.uint8, device=DEV))
    assert rc == 0
    rc, ones_scr = fz.call(ga, gd, scratch=torch.full((nb,), 0x3F, dtype=torch.uint8, device=DEV))      # (bytes of 0.747..: tags non-zero)
    rc2, again = fz.call(ga, gd)
    assert rc == 0 and rc2 == 0
    names = [k for k in base if base[k] is not None]
    for k in names:
        assert torch.equal(base[k], ones_scr[k]) and torch.equal(base[k], again[k]), k
        assert bool(torch.isfinite(base[k]).all()), k
    assert torch.equal(fz.ws.buf, before)
    # accumulate = 1 into ones: contributing rows are 1 + grad to rounding, every other row is still exactly 1
    rc, acc = fz.call(ga, gd, accumulate=1, o=fz.outputs(fill=1.0))
    assert rc == 0
    contrib = torch.zeros(fz.N, dtype=torch.bool, device=DEV)
    for k in LEAVES:
        contrib |= base[k].reshape(fz.N, -1).abs().amax(1) > 0
    assert bool(contrib.any()) and bool((~contrib).any())
    for k in names:
        n = base[k].shape[0]
        c = contrib[:n]
        assert bool((acc[k][~c] == 1.0).all()), k
        err = (acc[k][c].double() - (1.0 + base[k][c].double())).abs().max()
        assert float(err) <= 2.0 ** -22 * max(1.0, float(base[k].abs().max())), (k, float(err))
        assert bool((base[k][~c] == 0).all()), k                # accumulate = 0 wrote zeros there


def test_colour_backward_is_undisturbed_by_the_map_backward():
    V = 3
    sc, ct = scene("hand", 21, V)
    ga, gd = upstream(V, 2)
    from manus_amd.engine import HipViewCompute
    hc = HipViewCompute(sc, rand_targets(V), ct, fused=True, persistent_grads=False)
    ref = {k: v.clone() for k, v in hc(list(range(V)), 1.0)["grads"].items()}
    fz = Fused(sc, ct, V)                                       # step (colour backward), then the map backward ...
    assert fz.call(ga, gd)[0] == 0
    for k, v in fz.out["grads"].items():
        assert torch.equal(v, ref[k]), k
    after = fz.hc(fz.ids, 1.0)["grads"]                         # ... and a step behind it
    for k, v in after.items():
        assert torch.equal(v, ref[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    from manus_amd._lib import MGR_EINVAL, MGR_ENOMEM, MGR_ESTATE, lib
    V = 2
    sc, ct = scene("hand", 21, V)
    ga, gd = upstream(V, 3)
    fz = Fused(sc, ct, V)

    def refused(rc_o, code, text=None):
        rc, o = rc_o
        assert rc == code, (rc, code, lib().mgr_last_error())
        if text:
            assert text in lib().mgr_last_error(), lib().mgr_last_error()
        for k, v in o.items():
            assert v is None or bool(torch.isnan(v).all()), k

    nan = lambda: fz.outputs(fill=float("nan"))
    refused(fz.call(None, None, o=nan()), MGR_EINVAL, b"both NULL")
    refused(fz.call(ga, gd, o=nan(), scratch_bytes=fz.scratch_bytes() - 1), MGR_ENOMEM, b"scratch")
    refused(fz.call(ga, gd, o=nan(), ws_buf=torch.zeros_like(fz.ws.buf)), MGR_ESTATE, b"no forward")
    refused(fz.call(ga, gd, o=nan(), cap=fz.ws.cap - 64), MGR_ESTATE, b"another V, N, W, H")
    rc, o = fz.call(ga, gd, o=nan())                             # the same arguments, unrefused
    assert rc == 0 and all(v is None or bool(torch.isfinite(v).all()) for v in o.values())


def test_depth_cut_forward_is_refused():
    """The scene of test_gpu_feature_render.py::test_fused_route_is_accepted_uncut_and_refused_with_the_depth_cut."""
    from manus_amd import rasterizer as rz
    from manus_amd._lib import MGR_ESTATE, lib, ptr, stream
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table, make_scene
    V, n, Wc, Hc = 2, 40000, 256, 192
    sc = make_scene(n_gaussians=n, kind="hand", seed=3, grid_res=32, n_cameras=V, width=Wc, height=Hc, cam_radius=0.45,
                    sigma_range=(2e-3, 5e-3), device=DEV)
    sc["params"]["_opacity"] = sc["params"]["_opacity"] + 2.0
    N = sc["params"]["_xyz"].shape[0]
    targets = torch.rand((V, 3, Hc, Wc), generator=torch.Generator().manual_seed(103)).to(DEV)
    ct = camera_table(sc["cameras"], DEV)
    views = list(range(V))
    ctx = rz.context(DEV)
    ctx.clear()
    ctx.cut_retries = 0
    try:
        cut = HipViewCompute(sc, targets, ct, loss="l1+ssim", depth_cut=True)
        rz.set_sync_policy(True)
        cut(views)
        rz.check_overflow(DEV)
        rz.set_sync_policy(False, DEV)
        for _ in range(3):
            cut(views)
        ws = ctx.last_ws
        p = {k: v.detach() for k, v in cut.params.items()}
        w, B = cut._skin_weights(p["_xyz"], N)
        sel = cut._select(views)
        maps = torch.zeros((V, Hc, Wc), device=DEV)
        g = torch.ones((V, Hc, Wc), device=DEV)
        o = [torch.full(s, float("nan"), device=DEV) for s in ((N, 3), (N, 3), (N, 4), (N, 1), (N, B))]
        nb = int(lib().mgr_views_maps_backward_workspace_bytes(V, N, Wc, Hc, ws.cap))
        scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
        rc = lib().mgr_views_maps_backward(V, N, B, N, Wc, Hc, ptr(sel["cams"]), ptr(p["_xyz"]), ptr(p["_scaling"]), ptr(p["_rotation"]),
                                           ptr(p["_opacity"].reshape(-1)), ptr(w), ptr(sel["T"]), ptr(maps), None, ptr(g), None, 0,
                                           *[ptr(t) for t in o], ptr(ws.buf), ws.nbytes, ws.cap, ptr(scratch), nb, 0, stream())
        assert rc == MGR_ESTATE and b"depth cut" in lib().mgr_last_error()
        assert all(bool(torch.isnan(t).all()) for t in o)
    finally:
        rz.set_sync_policy(True)
        ctx.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 7. HipViewCompute
# ---------------------------------------------------------------------------------------------------------------------
def map_targets(sc, ct, V, shift=0.01):
    """Mask and depth targets: the alpha / depth maps of the model shifted along x (a target the model does not meet)."""
    from manus_amd import rasterizer as rz
    from manus_amd.engine import HipViewCompute
    moved = dict(sc, params={k: (v + torch.tensor([shift, 0.0, 0.0], device=DEV) if k == "_xyz" else v) for k, v in sc["params"].items()})
    hc = HipViewCompute(moved, rand_targets(V), ct, fused=True)
    with torch.no_grad():
        hc.forward_views_fused(list(range(V)))
        m = rz.blend_features(depth=True, alpha=True, device=DEV)
    return m["alpha"].clone(), m["depth"].clone()


def clone_out(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


@pytest.mark.parametrize("kind,V,depth", [("hand", 1, False), ("hand", 3, True), ("hand", 8, False), ("composite", 3, False),
                                           ("composite", 8, True), ("composite", 1, True)])
def test_compute_fused_against_modular_with_map_terms(kind, V, depth):
    from manus_amd.engine import HipViewCompute
    sc, ct = scene(kind, 21, V)
    mask, dt = map_targets(sc, ct, V)
    kw = dict(mask_targets=mask, w_mask=0.5, depth_targets=dt if depth else None, w_depth=0.25 if depth else 0.0)
    ids = list(range(V))
    tg = rand_targets(V)
    om = HipViewCompute(sc, tg, ct, fused=False, **kw)(ids, 1.0 / V)
    fus = HipViewCompute(sc, tg, ct, fused=True, **kw)
    of = fus(ids, 1.0 / V)
    assert fus._pg_ws is None and fus.last_active is None
    tag = "compute %s V=%d depth=%d" % (kind, V, depth)
    for k in ("loss", "loss_mask", "loss_depth"):
        a, b = float(of[k]), float(om[k])
        print("%s %-10s fused %.6e modular %.6e" % (tag, k, a, b))
        assert abs(a - b) <= BAR * max(abs(b), 1e-30) + (0.0 if b != 0.0 else 0.0), (k, a, b)
    assert float(om["loss_mask"]) > 0.0 and (float(om["loss_depth"]) > 0.0) == depth
    worst = compare(tag, of["grads"], om["grads"], names=list(om["grads"]))
    assert worst < BAR, (tag, worst)
    assert torch.equal(of["vis"], om["vis"])


def test_kept_buffers_are_refilled_with_a_map_term_on():
    from manus_amd.engine import HipViewCompute
    V = 3
    sc, ct = scene("hand", 21, V)
    mask, dt = map_targets(sc, ct, V)
    kw = dict(mask_targets=mask, w_mask=0.5, depth_targets=dt, w_depth=0.25)
    ids, tg = list(range(V)), rand_targets(V)
    a = HipViewCompute(sc, tg, ct, fused=True, persistent_grads=True, **kw)
    b = HipViewCompute(sc, tg, ct, fused=True, persistent_grads=False, **kw)
    gen = torch.Generator(device=DEV).manual_seed(7)
    for step in range(3):
        with torch.no_grad():   # the model moves between the steps (as in test_gpu_fused.py): positions jitter, a tenth of the
            noise = 0.004 * torch.randn(a.params["_xyz"].shape, device=DEV, generator=gen)      # Gaussians turn transparent / opaque
            flip = torch.rand(a.params["_opacity"].shape, device=DEV, generator=gen) < 0.1
            for hc in (a, b):
                hc.params["_xyz"].add_(noise)
                hc.params["_opacity"][flip] = -hc.params["_opacity"][flip]
                hc.mark_params_changed()
        oa, ob = clone_out(a(ids, 1.0 / V)), clone_out(b(ids, 1.0 / V))
        for k in oa["grads"]:
            ga, gb = oa["grads"][k], ob["grads"][k]
            print("kept step %d %-14s non-finite %d / %d, max|diff| %.3e" % (step, k, int((~torch.isfinite(ga)).sum()), int((~torch.isfinite(gb)).sum()),
                                                                           float(torch.nan_to_num(ga - gb).abs().max())))
            assert bool(torch.isfinite(ga).all()), (step, k)
            assert torch.equal(ga, gb), (step, k)
        assert torch.equal(oa["grad2d"], ob["grad2d"]) and torch.equal(oa["loss_mask"], ob["loss_mask"]) and torch.equal(oa["loss_depth"], ob["loss_depth"])
        assert abs(float(oa["loss"]) - float(ob["loss"])) < 1e-6   # (the colour term's loss scalar is summed with float atomics)


def test_rows_outside_the_colour_backwards_active_list():
    """loss = "l1" on the object's own render: the colour gradient is zero and its active list empty; everything comes from the
    mask term, including the d_xyz part through the skin-weight backward (full rows, not the list)."""
    from manus_amd.engine import HipViewCompute
    V = 2
    sc, ct = scene("hand", 21, V)
    ids = list(range(V))
    own = HipViewCompute(sc, rand_targets(V), ct, fused=True)
    with torch.no_grad():
        img = own.forward_views_fused(ids)[0].clone()
    mask, _ = map_targets(sc, ct, V, shift=0.008)
    kw = dict(loss="l1", mask_targets=mask, w_mask=1.0)
    plain = HipViewCompute(sc, img, ct, fused=True, loss="l1")(ids, 1.0 / V)
    assert all(float(g.abs().max()) == 0.0 for g in plain["grads"].values())                # the colour term alone: nothing
    of = HipViewCompute(sc, img, ct, fused=True, **kw)(ids, 1.0 / V)
    # (the modular route's own render: its image differs from the fused one by rounding, and the L1 gradient is a sign)
    mod = HipViewCompute(sc, img, ct, fused=False, **kw)
    with torch.no_grad():
        mod.targets = mod.forward_views(ids)[0].detach().clone()
    om = mod(ids, 1.0 / V)
    assert float(om["grads"]["_features_dc"].abs().max()) == 0.0                             # the colour term is silent there too
    for k in LEAVES:
        assert float(of["grads"][k].abs().max()) > 0.0, k
    worst = compare("mask term alone", of["grads"], om["grads"], names=LEAVES)
    assert worst < BAR, worst
    assert float(of["grads"]["_features_dc"].abs().max()) == 0.0
    # the d_xyz part through the skin-weight backward is there: without it (a raw map backward, no skin step) d_xyz differs
    fz = Fused(sc, ct, V)
    ga = torch.sign(fz.maps["alpha"] - mask)
    rc, o = fz.call(ga.contiguous(), None)
    assert rc == 0
    d_no, d_with = o["_xyz"], fz.with_skin(o)["_xyz"]
    assert float((d_with - d_no).abs().max()) > 1e-3 * float(d_with.abs().max())


def test_off_means_off():
    from manus_amd.engine import HipViewCompute
    V = 3
    sc, ct = scene("hand", 21, V)
    mask, dt = map_targets(sc, ct, V)
    ids, tg = list(range(V)), rand_targets(V)
    outs = []
    for kw in (dict(), dict(mask_targets=mask, w_mask=0.0, depth_targets=dt, w_depth=0.0), dict(mask_targets=None, w_mask=1.0, w_depth=1.0)):
        hc = HipViewCompute(sc, tg, ct, fused=True, **kw)
        hc(ids, 1.0 / V)
        outs.append(clone_out(hc(ids, 1.0 / V)))
        assert hc._pg_ws is not None and hc.last_active is not None       # the selective fills and the list stay in use
        assert "loss_mask" not in outs[-1]
    for o in outs[1:]:
        for k in outs[0]["grads"]:
            assert torch.equal(o["grads"][k], outs[0]["grads"][k]), k
        for k in ("grad2d", "vis", "radii"):
            assert torch.equal(o[k], outs[0][k]), k
        assert abs(float(o["loss"]) - float(outs[0]["loss"])) < 1e-6   # (the colour term's loss scalar is summed with float atomics)


# ---------------------------------------------------------------------------------------------------------------------
# 8. recovery, end to end
# ---------------------------------------------------------------------------------------------------------------------
def _scene_a():
    """Scene a of test_gpu_feature_grad.py's recovery case (1500 random Gaussians, 128x96, one camera) as a static "object" of
    canonical parameters: the posed covariances factored into rotation and scale (eigen-decomposition), the colours as SH band 0."""
    from test_gpu_feature_render import BG, scene as fr_scene
    from util import cam_table_np
    s = fr_scene("a")
    c = s.c.astype(np.float64)
    S = np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], -1), np.stack([c[:, 1], c[:, 3], c[:, 4]], -1), np.stack([c[:, 2], c[:, 4], c[:, 5]], -1)], -2)
    ev, R = np.linalg.eigh(S)
    R[:, :, 2] *= np.sign(np.linalg.det(R))[:, None]             # proper rotations
    q = np.zeros((R.shape[0], 4))
    for i, m in enumerate(R):                                    # (w, x, y, z), the largest component first for stability
        t = np.trace(m)
        cand = np.array([t, m[0, 0] - m[1, 1] - m[2, 2], m[1, 1] - m[0, 0] - m[2, 2], m[2, 2] - m[0, 0] - m[1, 1]])
        j = int(np.argmax(cand))
        r = np.sqrt(max(1.0 + cand[j], 1e-30)) * 2.0
        if j == 0:
            q[i] = [0.25 * r, (m[2, 1] - m[1, 2]) / r, (m[0, 2] - m[2, 0]) / r, (m[1, 0] - m[0, 1]) / r]
        elif j == 1:
            q[i] = [(m[2, 1] - m[1, 2]) / r, 0.25 * r, (m[0, 1] + m[1, 0]) / r, (m[0, 2] + m[2, 0]) / r]
        elif j == 2:
            q[i] = [(m[0, 2] - m[2, 0]) / r, (m[0, 1] + m[1, 0]) / r, 0.25 * r, (m[1, 2] + m[2, 1]) / r]
        else:
            q[i] = [(m[1, 0] - m[0, 1]) / r, (m[0, 2] + m[2, 0]) / r, (m[1, 2] + m[2, 1]) / r, 0.25 * r]
    N = s.m.shape[0]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    op = np.clip(s.op.astype(np.float64), 1e-6, 1 - 1e-6)
    params = {"_xyz": f32(s.m), "_scaling": f32(0.5 * np.log(np.maximum(ev, 1e-20))), "_rotation": f32(q),
              "_opacity": f32(np.log(op / (1 - op))).reshape(N, 1), "_features_dc": f32((s.col - 0.5) / 0.28209479177387814).reshape(N, 1, 3),
              "_features_rest": torch.zeros((N, 15, 3), device=DEV)}
    sc = dict(kind="object", params=params, N=N, n_hand=0, bg=f32(BG), width=s.W, height=s.H, grid=None)
    return sc, torch.from_numpy(cam_table_np([s.cam])).to(DEV)


def test_mask_term_recovers_a_shift_on_the_fused_step():
    """Scene a shifted by 0.02 along x; mask targets = the alpha map of the true position; the image term held at zero gradient
    (loss "l1" on the step's own render).  60 Adam steps at 1e-3 on _xyz: the mask loss falls, the offset has the right sign,
    and the fused route's final loss is at most 10 % above the same loop on fused=False."""
    from manus_amd import rasterizer as rz
    from manus_amd.engine import HipViewCompute
    sc, ct = _scene_a()
    true = HipViewCompute(sc, torch.zeros((1, 3, sc["height"], sc["width"]), device=DEV), ct, fused=True)
    with torch.no_grad():
        true.forward_views_fused([0])
        mask = rz.blend_features(alpha=True, device=DEV)["alpha"].clone()
    x0 = sc["params"]["_xyz"].clone()
    shifted = dict(sc, params=dict(sc["params"], _xyz=x0 + torch.tensor([0.02, 0.0, 0.0], device=DEV)))
    final, offs = {}, {}
    for fused in (True, False):
        hc = HipViewCompute(shifted, torch.zeros((1, 3, sc["height"], sc["width"]), device=DEV), ct, fused=fused, loss="l1",
                            mask_targets=mask, w_mask=1.0)
        xyz = hc.params["_xyz"]
        opt = torch.optim.Adam([xyz], lr=1e-3)
        hist = []
        for _ in range(60):
            with torch.no_grad():      # the image term's target is the step's own render: zero colour gradient
                hc.targets = (hc.forward_views_fused([0])[0] if fused else hc.forward_views([0])[0]).detach().clone()
            out = hc([0], 1.0)
            hist.append(float(out["loss_mask"]))
            opt.zero_grad()
            xyz.grad = out["grads"]["_xyz"].clone()
            opt.step()
            hc.mark_params_changed()
        final[fused], offs[fused] = hist, float((xyz.detach() - x0)[:, 0].mean())
        print("recovery fused=%d: mask loss %.5e -> %.5e, mean x offset %.4e (start 2e-02)" % (fused, hist[0], hist[-1], offs[fused]))
    assert final[True][-1] < final[True][0]
    assert offs[True] < 0.02                                      # moved back towards the true position
    assert final[True][-1] <= 1.10 * final[False][-1], (final[True][-1], final[False][-1])

"""GPU: map terms with pose and skin-grid gradients on the fused step -- mgr_views_maps_backward_pose against the operator route
under autograd (ops.skin_weights -> ops.lbs_cov with the transforms a leaf -> rasterize_views_features -> a loss on alpha and
depth), its leaf outputs against mgr_views_maps_backward (bit for bit), accumulate / determinism / refusal contracts, the one-view
identity that isolates the reduction, and HipViewCompute with a map term and pose_grad / skin_grid_grad on, fused against
fused=False (the modular route is autograd through the operators end to end: the checker's independent chain).

Bars: d_transforms per view max_rel_err (tests/util.py) < 5e-3, the bar test_gpu_pose_grad.py holds two independent fp32 chains
to; leaf gradients the file-level BAR = 1e-4 of test_gpu_map_loss.py; d_skin_grid the fused-against-modular bar of
test_gpu_skin_grid_grad.py (max_rel_err < 5e-3, fewer than 3 % of the rows off by more than 2e-5 of the largest entry).
Scenes, upstream gradients and the raw-call harness are those of test_gpu_map_loss.py (56x40, 2000 Gaussians)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_map_loss import BAR, DEV, H, LEAVES, W, Fused, clone_out, compare, map_targets, rand_targets, scene, upstream
from util import max_rel_err

pytestmark = pytest.mark.gpu
POSE_BAR = 5e-3


def pose_call(fz, g_alpha, g_depth, accumulate=0, acc_pose=0, o=None, d_T=None, pose_ws=None, pose_bytes=None, scratch_bytes=None,
              ws_buf=None, null_skin=False):
    """One mgr_views_maps_backward_pose on the workspace of a `Fused` -> (rc, leaf outputs, d_transforms (V,B,4,4))."""
    from manus_amd._lib import lib, ptr, stream
    o = o if o is not None else fz.outputs()
    d_T = d_T if d_T is not None else torch.empty((fz.V, fz.B, 4, 4), device=DEV)
    nb = fz.scratch_bytes()
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    need = int(lib().mgr_views_maps_pose_workspace_bytes(fz.V, fz.N, fz.B))
    pose_ws = pose_ws if pose_ws is not None else torch.empty(need, dtype=torch.uint8, device=DEV)
    p, ws = fz.p, fz.ws
    buf = ws.buf if ws_buf is None else ws_buf
    rc = lib().mgr_views_maps_backward_pose(
        fz.V, fz.N, fz.B, fz.na, W, H, ptr(fz.sel["cams"]), ptr(p["_xyz"]), ptr(p["_scaling"]), ptr(p["_rotation"]),
        ptr(p["_opacity"].reshape(-1)), None if null_skin else ptr(fz.w), ptr(fz.sel["T"]),
        ptr(fz.maps["alpha"]) if g_alpha is not None else None, ptr(fz.maps["depth"].contiguous()) if g_depth is not None else None,
        ptr(g_alpha), ptr(g_depth), accumulate, ptr(o["_xyz"]), ptr(o["_scaling"]), ptr(o["_rotation"]), ptr(o["_opacity"]),
        ptr(o["_skin_w"]), ptr(buf), buf.numel(), ws.cap, ptr(scratch), nb if scratch_bytes is None else scratch_bytes, 1,
        acc_pose, ptr(d_T), ptr(pose_ws), need if pose_bytes is None else pose_bytes, stream())
    return rc, o, d_T


@functools.lru_cache(maxsize=None)
def operator_pose(kind, B, V, giant, n, case):
    """dL/dT (V,B,4,4) of sum(alpha g_alpha) + sum(depth g_depth) through the modular operators, the transforms a leaf."""
    from manus_amd.engine import HipViewCompute
    sc, ct = scene(kind, B, V, giant, n)
    ga, gd = upstream(V)
    mod = HipViewCompute(sc, rand_targets(V), ct, fused=False)
    T = mod._select(list(range(V)))["T"].detach().clone().requires_grad_(True)
    _, _, _, ex = mod.forward_views(list(range(V)), T=T, maps=(True, True))
    roots = [(ex["alpha"], ga)] if case != "depth" else []
    roots += [(ex["depth"], gd)] if case != "alpha" else []
    torch.autograd.backward([r for r, _ in roots], [g for _, g in roots])
    return T.grad.detach().clone()


#        kind         B   V  case     giant  n
CASES = [("hand", 21, 1, "both", False, 2000), ("hand", 21, 2, "both", False, 2000), ("hand", 21, 3, "both", True, 2000),
         ("hand", 21, 8, "both", False, 2000), ("hand", 21, 9, "both", False, 2000), ("hand", 21, 11, "alpha", False, 2000),
         ("hand", 1, 3, "alpha", False, 2000), ("hand", 32, 8, "depth", False, 2000), ("hand", 21, 3, "depth", False, 2000),
         ("composite", 21, 3, "both", False, 2000), ("composite", 32, 2, "depth", True, 2000), ("composite", 21, 9, "alpha", False, 2000),
         # the small cases of test_gpu_pose_grad.py::FUSED_CASES: a partial chunk, one Gaussian, a composite below one chunk
         ("hand", 21, 8, "both", False, 37), ("hand", 21, 2, "both", False, 1), ("composite", 21, 4, "both", False, 263)]


def _upstream_of(V, case):
    ga, gd = upstream(V)
    return (ga if case != "depth" else None), (gd if case != "alpha" else None)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the entry against the operator route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,V,case,giant,n", CASES)
def test_entry_against_the_operator_route(kind, B, V, case, giant, n):
    """Measured on MI355X (gfx950): at most 4.6e-7 per view over these cases (hand, B = 21, V = 8, both maps); DESIGN.md section 2 row f8."""
    sc, ct = scene(kind, B, V, giant, n)
    ga, gd = _upstream_of(V, case)
    ref = operator_pose(kind, B, V, giant, n, case)
    fz = Fused(sc, ct, V)
    rc, o, d_T = pose_call(fz, ga, gd, d_T=torch.full((V, fz.B, 4, 4), float("nan"), device=DEV))
    assert rc == 0
    assert d_T.shape == ref.shape
    assert bool(torch.isfinite(d_T).all()) and float(d_T[..., 3, :].abs().max()) == 0.0
    assert all(v is None or bool(torch.isfinite(v).all()) for v in o.values())
    worst = 0.0
    for v in range(V):
        a, b = d_T[v].cpu().numpy(), ref[v].cpu().numpy()
        e = max_rel_err(a, b)
        worst = max(worst, e)
        print("entry %s B=%d V=%d %s%s n=%d view %d max_rel_err %.3e max|dT| %.3e" % (kind, B, V, case, " giant" if giant else "", n, v, e,
                                                                                       float(np.abs(b).max())))
    print("FIGURE entry vs operator %s B=%d V=%d %s n=%d worst view %.3e" % (kind, B, V, case, n, worst))
    # every scene here has its Gaussians on the hand in front of every camera: an all-zero pair would pass the bar vacuously
    assert float(ref.abs().max()) > 0.0 and float(d_T.abs().max()) > 0.0
    assert worst < POSE_BAR, worst


# ---------------------------------------------------------------------------------------------------------------------
# 2. the leaf outputs are those of mgr_views_maps_backward; 3. accumulate and determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,V,case,giant,n", [c for c in CASES if (c[2], c[5]) in ((1, 2000), (3, 2000), (9, 2000), (11, 2000), (2, 2000), (8, 37),
                                                                                        (2, 1), (4, 263))])
def test_leaf_outputs_accumulate_and_determinism(kind, B, V, case, giant, n):
    sc, ct = scene(kind, B, V, giant, n)
    ga, gd = _upstream_of(V, case)
    fz = Fused(sc, ct, V)
    before = fz.ws.buf.clone()
    names = [k for k, v in fz.outputs().items() if v is not None]
    gen = torch.Generator(device=DEV).manual_seed(11)
    start = {k: torch.randn(v.shape, device=DEV, generator=gen) for k, v in fz.outputs().items() if v is not None}
    for accumulate in (0, 1):
        mk = lambda: {k: (start[k].clone() if k in start else None) for k in fz.outputs()}
        rc0, plain = fz.call(ga, gd, accumulate=accumulate, o=mk())
        rc1, o, _ = pose_call(fz, ga, gd, accumulate=accumulate, o=mk())
        assert rc0 == 0 and rc1 == 0
        for k in names:
            assert torch.equal(o[k], plain[k]), (accumulate, k)
    assert torch.equal(fz.ws.buf, before)                            # the workspace is only read
    # accumulate_pose: the fold adds last, so the sum is the fp32 sum of the two operands -- bit for bit
    rc, _, base = pose_call(fz, ga, gd)
    rc2, _, again = pose_call(fz, ga, gd, pose_ws=torch.full((int(1 << 24),), 0x3F, dtype=torch.uint8, device=DEV))
    assert rc == 0 and rc2 == 0 and torch.equal(base, again)         # two runs, whatever the pose workspace held: the same bits
    buf = torch.randn((V, fz.B, 4, 4), device=DEV, generator=gen)
    rc, _, acc = pose_call(fz, ga, gd, acc_pose=1, d_T=buf.clone())
    assert rc == 0
    assert torch.equal(acc, buf + base)
    assert torch.equal(acc[..., 3, :], buf[..., 3, :])
    assert torch.equal(fz.ws.buf, before)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the reduction, isolated from the blend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3000, 37])
def test_one_view_identity_between_pose_and_skin_weight_gradients(n):
    """V = 1: sum_b <d_transforms[0][b][:3,:], T_b[:3,:]> == sum_n sum_b w_nb d_skin_w[n][b]: both contract the same dtf with the
    same w and T.  Both sides from one call, summed in fp64 on the host, to 1e-5 relative."""
    sc, ct = scene("hand", 21, 1, False, n)
    ga, gd = upstream(1)
    fz = Fused(sc, ct, 1)
    rc, o, d_T = pose_call(fz, ga, gd)
    assert rc == 0
    w, d_w = fz.w.double().cpu(), o["_skin_w"].double().cpu()
    T = fz.sel["T"][0].double().cpu().reshape(fz.B, 4, 4)
    lhs = float((d_T[0].double().cpu()[:, :3, :] * T[:, :3, :]).sum())
    rhs = float((w * d_w).sum())
    scale = float((w * d_w).abs().sum())
    print("identity n=%d: lhs %.9e rhs %.9e |terms| %.3e" % (n, lhs, rhs, scale))
    assert scale > 0.0
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    from manus_amd._lib import MGR_EINVAL, MGR_ENOMEM, MGR_ESTATE, lib
    V = 2
    sc, ct = scene("hand", 21, V)
    ga, gd = upstream(V, 3)
    fz = Fused(sc, ct, V)
    need = int(lib().mgr_views_maps_pose_workspace_bytes(V, fz.N, fz.B))

    def refused(code, text, **kw):
        o = fz.outputs(fill=float("nan"))
        rc, o, d_T = pose_call(fz, ga, gd, o=o, d_T=torch.full((V, fz.B, 4, 4), float("nan"), device=DEV), **kw)
        err = lib().mgr_last_error()
        assert rc == code, (rc, code, err)
        assert b"mgr_views_maps_backward_pose" in err and text in err, err
        torch.cuda.synchronize()
        assert bool(torch.isnan(d_T).all())
        for k, v in o.items():
            assert v is None or bool(torch.isnan(v).all()), k

    refused(MGR_ESTATE, b"no forward", ws_buf=torch.zeros_like(fz.ws.buf))
    refused(MGR_ENOMEM, b"scratch", scratch_bytes=fz.scratch_bytes() - 1)
    refused(MGR_ENOMEM, b"pose workspace", pose_bytes=need - 1)
    refused(MGR_EINVAL, b"skin_w", null_skin=True)
    rc, o, d_T = pose_call(fz, ga, gd, o=fz.outputs(fill=float("nan")))            # the same arguments, unrefused
    assert rc == 0 and bool(torch.isfinite(d_T).all()) and all(v is None or bool(torch.isfinite(v).all()) for v in o.values())


def test_depth_cut_forward_is_refused():
    """The scene of test_gpu_map_loss.py::test_depth_cut_forward_is_refused."""
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
        o = [torch.full(s, float("nan"), device=DEV) for s in ((N, 3), (N, 3), (N, 4), (N, 1), (N, B), (V, B, 16))]
        nb = int(lib().mgr_views_maps_backward_workspace_bytes(V, N, Wc, Hc, ws.cap))
        scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
        npose = int(lib().mgr_views_maps_pose_workspace_bytes(V, N, B))
        pose_ws = torch.empty(npose, dtype=torch.uint8, device=DEV)
        rc = lib().mgr_views_maps_backward_pose(V, N, B, N, Wc, Hc, ptr(sel["cams"]), ptr(p["_xyz"]), ptr(p["_scaling"]), ptr(p["_rotation"]),
                                                ptr(p["_opacity"].reshape(-1)), ptr(w), ptr(sel["T"]), ptr(maps), None, ptr(g), None, 0,
                                                *[ptr(t) for t in o[:5]], ptr(ws.buf), ws.nbytes, ws.cap, ptr(scratch), nb, 0, 0, ptr(o[5]),
                                                ptr(pose_ws), npose, stream())
        assert rc == MGR_ESTATE and b"depth cut" in lib().mgr_last_error() and b"mgr_views_maps_backward_pose" in lib().mgr_last_error()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in o)
    finally:
        rz.set_sync_policy(True)
        ctx.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 6. HipViewCompute: map term + pose_grad
# ---------------------------------------------------------------------------------------------------------------------
def _entry_on_step_state(hc, V):
    """mgr_views_maps_backward_pose (accumulate_pose = 0, leaf outputs thrown away) on the state the fused step `hc` just left:
    its workspace, its maps and their gradients."""
    from manus_amd import rasterizer as rz
    from manus_amd._lib import check, lib, ptr, stream
    ws = rz.context(DEV).last_ws
    (mb,) = hc._map_bufs.values()
    p = {k: v.detach() for k, v in hc.params.items()}
    N, na = p["_xyz"].shape[0], hc.n_art
    w, B = hc._skin_weights(p["_xyz"], na)
    sel = hc._select(list(range(V)))
    o = [torch.empty(s, device=DEV) for s in ((N, 3), (N, 3), (N, 4), (N, 1), (na, B))]
    d_T = torch.empty((V, B, 4, 4), device=DEV)
    pose_ws = torch.empty(int(lib().mgr_views_maps_pose_workspace_bytes(V, N, B)), dtype=torch.uint8, device=DEV)
    scratch = torch.empty_like(mb["scratch"])
    check(lib().mgr_views_maps_backward_pose(V, N, B, na, W, H, ptr(sel["cams"]), ptr(p["_xyz"]), ptr(p["_scaling"]), ptr(p["_rotation"]),
                                             ptr(p["_opacity"].reshape(-1)), ptr(w), ptr(sel["T"]), ptr(mb["alpha"]), ptr(mb["depth"]),
                                             ptr(mb["g_alpha"]), ptr(mb["g_depth"]), 0, *[ptr(t) for t in o], ptr(ws.buf), ws.nbytes, ws.cap,
                                             ptr(scratch), scratch.numel(), 0, 0, ptr(d_T), ptr(pose_ws), pose_ws.numel(), stream()),
          "mgr_views_maps_backward_pose")
    return d_T


@pytest.mark.parametrize("kind,V,depth", [("hand", 1, False), ("hand", 3, True), ("hand", 8, False), ("hand", 11, True), ("composite", 3, True)])
def test_compute_fused_against_modular_with_map_term_and_pose_grad(kind, V, depth):
    """Fails on the parent commit: `_map_terms` raises ValueError."""
    from manus_amd.engine import HipViewCompute
    sc, ct = scene(kind, 21, V)
    mask, dt = map_targets(sc, ct, V)
    kw = dict(mask_targets=mask, w_mask=0.5, depth_targets=dt if depth else None, w_depth=0.25 if depth else 0.0)
    ids, tg = list(range(V)), rand_targets(V)
    on = HipViewCompute(sc, tg, ct, fused=True, pose_grad=True, **kw)
    of = clone_out(on(ids, 1.0 / V))
    entry = _entry_on_step_state(on, V)                              # (before any other forward replaces the workspace's lists)
    om = HipViewCompute(sc, tg, ct, fused=False, pose_grad=True, **kw)(ids, 1.0 / V)
    off = clone_out(HipViewCompute(sc, tg, ct, fused=True, **kw)(ids, 1.0 / V))
    colour = clone_out(HipViewCompute(sc, tg, ct, fused=True, pose_grad=True, **dict(kw, w_mask=0.0, w_depth=0.0))(ids, 1.0 / V))
    tag = "compute+pose %s V=%d depth=%d" % (kind, V, depth)
    a, b = of["d_transforms"], om["d_transforms"]
    assert a.shape == b.shape and bool(torch.isfinite(a).all()) and float(a[..., 3, :].abs().max()) == 0.0
    for v in range(V):
        e = max_rel_err(a[v].cpu().numpy(), b[v].cpu().numpy())
        print("%s view %d d_transforms max_rel_err %.3e max|dT| %.3e" % (tag, v, e, float(b[v].abs().max())))
        assert float(b[v].abs().max()) > 0.0
        assert e < POSE_BAR, (v, e)
    worst = compare(tag, of["grads"], om["grads"], names=list(om["grads"]))
    assert worst < BAR, (tag, worst)
    # pose_grad leaves everything else bit for bit
    assert "d_transforms" not in off
    for k in of["grads"]:
        assert torch.equal(of["grads"][k], off["grads"][k]), k
    for k in ("grad2d", "vis", "radii", "loss_mask", "loss_depth"):
        assert torch.equal(of[k], off[k]), k
    # the map term is in d_transforms, and it is the entry's own output on the step's state
    diff = a.double() - colour["d_transforms"].double()
    assert float(diff.abs().max()) > 0.0
    err = float((diff - entry.double()).abs().max())
    print("%s (with - without the map term) against the entry: %.3e of max %.3e" % (tag, err, float(entry.abs().max())))
    assert err <= 1e-5 * float(entry.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 7. HipViewCompute: map term + skin_grid_grad (+ pose_grad)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,pose", [(3, False), (8, True), (9, False)])
def test_compute_fused_against_modular_with_map_term_and_skin_grid_grad(V, pose):
    from manus_amd import ops
    from manus_amd.engine import HipViewCompute
    sc, ct = scene("hand", 21, V)
    mask, dt = map_targets(sc, ct, V)
    kw = dict(mask_targets=mask, w_mask=0.5, depth_targets=dt, w_depth=0.25, skin_grid_grad=True, pose_grad=pose)
    ids, tg = list(range(V)), rand_targets(V)
    fus = HipViewCompute(sc, tg, ct, fused=True, **kw)
    of = fus(ids, 1.0 / V)
    d = of["d_skin_grid"]
    Bn = d.shape[3]
    vox, rows = d.rows()
    assert bool((vox[1:] > vox[:-1]).all()) and bool((rows[:, Bn:] == 0).all())
    dense_f = d.to_dense().clone().reshape(-1, Bn)
    d_w = fus.last_skin_w_grad.clone()
    mod = HipViewCompute(sc, tg, ct, fused=False, **kw)
    om = mod(ids, 1.0 / V)
    dense_m = om["d_skin_grid"].to_dense().reshape(-1, Bn)
    a, b = dense_f.cpu().numpy().astype(np.float64), dense_m.cpu().numpy().astype(np.float64)
    e = max_rel_err(a, b)
    off_rows = np.abs(a - b).max(1) > 2e-5 * np.abs(b).max()
    print("FIGURE map term: fused vs modular d_skin_grid V=%d pose=%d max_rel_err %.3e, rows off %d of %d" % (V, pose, e, off_rows.sum(), len(off_rows)))
    assert e < 5e-3, e
    assert off_rows.mean() < 0.03, off_rows.sum()
    # the voxel list: that of the rows of the summed d_w that are not all zero (beyond 8 views: of all rows)
    live = torch.nonzero((d_w != 0).any(1)).reshape(-1).to(torch.int32)
    xyz = fus.params["_xyz"].detach()[:fus.n_art]
    want = ops.skin_grid_grad(xyz, fus.grid, sc["grid_center"], sc["grid_scale"], d_w, index=live if V <= 8 else None)
    assert torch.equal(vox, want.rows()[0])
    every = ops.skin_grid_grad(xyz, fus.grid, sc["grid_center"], sc["grid_scale"], d_w).rows()[0]
    print("voxels listed %d, under all rows %d, rows of d_w not all zero %d of %d" % (vox.numel(), every.numel(), live.numel(), d_w.shape[0]))
    if V <= 8:
        assert live.numel() < d_w.shape[0] and vox.numel() < every.numel()      # some voxel lies under all-zero rows only: not listed
        assert torch.equal(vox, om["d_skin_grid"].rows()[0])                     # the two routes step the same voxels
    # the map term is in the skin-weight gradient
    no_map = HipViewCompute(sc, tg, ct, fused=True, **dict(kw, w_mask=0.0, w_depth=0.0))
    no_map(ids, 1.0 / V)
    assert float((no_map.last_skin_w_grad - d_w).abs().max()) > 0.0
    worst = compare("compute+grid V=%d" % V, of["grads"], om["grads"], names=list(om["grads"]))
    assert worst < BAR, worst
    if pose:
        for v in range(V):
            assert max_rel_err(of["d_transforms"][v].cpu().numpy(), om["d_transforms"][v].cpu().numpy()) < POSE_BAR, v


@pytest.mark.parametrize("n,B", [(1, 1), (255, 21), (1300, 32), (2049, 21)])
def test_row_list_of_a_skin_weight_gradient(n, B):
    """mgr_skin_rows_mask + mgr_exchange_index: the ascending rows with an entry != 0 (a NaN counts), exact; the sizes cross the
    mask kernel's 256 and the index kernel's 1024 block."""
    from manus_amd._lib import lib, ptr, stream
    L = lib()
    g = torch.Generator().manual_seed(70 + n)
    d_w = torch.randn((n, B), generator=g)
    d_w[torch.rand(n, generator=g) < 0.5] = 0.0
    d_w[torch.rand((n, B), generator=g) < 0.3] = 0.0
    if n > 1:
        d_w[n - 1] = 0.0
        d_w[n - 1, B - 1] = float("nan")
        d_w[n // 2] = 0.0
        d_w[n // 2, 0] = -0.0                            # a row of signed zeros is a zero row
    expect = (d_w != 0).any(1).nonzero().reshape(-1).to(torch.int32)
    d_w = d_w.to(DEV)
    mask = torch.full((n + 8,), 7, dtype=torch.uint8, device=DEV)
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(L.mgr_exchange_index_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    assert L.mgr_skin_rows_mask(n, B, ptr(d_w), ptr(mask), stream()) == 0
    assert L.mgr_exchange_index(n, ptr(mask), ptr(idx), ptr(count), ptr(ws), ws.numel(), stream()) == 0
    assert int(count) == expect.numel()
    assert torch.equal(idx[:expect.numel()].cpu(), expect)
    assert bool((idx[expect.numel():] == -1).all()) and bool((mask[n:] == 7).all()) and int(mask[:n].max()) <= 1


def test_flags_still_need_articulated_gaussians():
    from manus_amd.engine import HipViewCompute
    sc, ct = scene("object", 21, 2)
    mask = torch.zeros((2, H, W), device=DEV)
    hc = HipViewCompute(sc, rand_targets(2), ct, mask_targets=mask, w_mask=1.0)
    for name in ("pose_grad", "skin_grid_grad"):
        setattr(hc, name, True)
        with pytest.raises(ValueError, match=name):
            hc([0, 1], 0.5)
        setattr(hc, name, False)
    hand, ct = scene("hand", 21, 2)
    with pytest.raises(ValueError, match="depth_cut"):
        HipViewCompute(hand, rand_targets(2), ct, mask_targets=mask, w_mask=1.0, pose_grad=True, depth_cut=True)


# ---------------------------------------------------------------------------------------------------------------------
# 8. pose recovery with the silhouette
# ---------------------------------------------------------------------------------------------------------------------
def test_pose_recovery_with_the_silhouette():
    """The setup of test_gpu_pose_grad.py::test_pose_recovery_end_to_end (hand, n = 3000, 3 views at 96x64, three bones rotated by
    0.05 rad, PoseCorrection under Adam at 1e-3 for 50 steps, Gaussians frozen) with mask_targets = the alpha maps of the true
    pose and w_mask = 1.  Asserted: loss, loss_mask and the mean geodesic angle end below their initial values.  The final angle
    is printed beside that of the same loop with w_mask = 0 (LAB.md); which is smaller is not asserted."""
    from manus_amd import rasterizer as rz
    from manus_amd.engine import HipViewCompute
    from manus_amd.pose import PoseCorrection, _exp_so3, pose_backward
    from manus_amd.transforms import bone_transforms
    from test_gpu_pose_grad import _geodesic, _scene
    views, ids = 3, [0, 1, 2]
    sc, ct = _scene("hand", 3000, views)
    rest = sc["rest"]
    nb = rest.shape[0]
    true_T = sc["transforms"].clone()
    bones = [3, 7, 12]
    axes = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], device=DEV)
    delta = torch.eye(4, device=DEV).repeat(nb, 1, 1)
    delta[bones, :3, :3] = _exp_so3(0.05 * axes)
    posed_bad = [sc["posed"][v] @ delta for v in ids]
    final = {}
    for w_mask in (1.0, 0.0):
        with torch.no_grad():
            sc["transforms"][ids] = true_T[ids]
        hc = HipViewCompute(sc, torch.zeros((views, 3, 64, 96), device=DEV), ct, fused=True, pose_grad=True, loss="l1+ssim")
        with torch.no_grad():
            hc.targets = hc.forward_views_fused(ids)[0].clone()
            hc.mask_targets = rz.blend_features(alpha=True, device=DEV)["alpha"].clone()
        hc.w_mask = w_mask
        corr = PoseCorrection(views, nb, device=DEV)
        opt = torch.optim.Adam(corr.parameters(), lr=1e-3)

        def angle():
            with torch.no_grad():
                return float(torch.stack([_geodesic(corr(posed_bad[v], v)[bones, :3, :3], sc["posed"][v][bones, :3, :3]) for v in ids]).mean())

        losses, lm, a0 = [], [], angle()
        for step in range(50):
            opt.zero_grad()
            corrected = [corr(posed_bad[v], v) for v in ids]
            with torch.no_grad():
                sc["transforms"][ids] = torch.stack([bone_transforms(c, rest) for c in corrected])
            out = hc(ids, 1.0 / views)
            losses.append(float(out["loss"]))
            lm.append(float(out["loss_mask"]) if "loss_mask" in out else 0.0)
            for v in ids:
                corrected[v].backward(pose_backward(out["d_transforms"][v], corrected[v], rest))
            opt.step()
        final[w_mask] = (losses[0], losses[-1], lm[0], lm[-1], a0, angle())
        print("FIGURE silhouette pose recovery w_mask=%g: loss %.6f -> %.6f, loss_mask %.6f -> %.6f, mean geodesic angle %.4f -> %.4f rad"
              % ((w_mask,) + final[w_mask]))
    with torch.no_grad():
        sc["transforms"][ids] = true_T[ids]
    l0, l1, m0, m1, a0, a1 = final[1.0]
    assert l1 < l0 and m1 < m0 and a1 < a0

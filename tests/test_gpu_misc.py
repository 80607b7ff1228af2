"""GPU: simple-knn replacement, drop-in package surface, reference-signature render call,
L1 loss kernel, and the multi-view engine step against the oracle."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import RasterOracle, knn3_mean_dist2
from oracle import torch_ref as tr

from util import cam_args, make_camera, max_rel_err, psnr, random_gaussians

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n,kind", [(1, "normal"), (3, "normal"), (2000, "normal"), (3000, "hand"), (500, "dup"), (800, "line")])
def test_distcuda2_equals_brute_force(n, kind):
    from simple_knn._C import distCUDA2
    g = np.random.default_rng(n)
    if kind == "normal":
        pts = g.normal(size=(n, 3)).astype(np.float32)
    elif kind == "hand":
        from manus_amd.synthetic import make_scene
        pts = make_scene(n_gaussians=n, kind="hand", seed=0, grid_res=8, n_cameras=1, width=32, height=32)["params"]["_xyz"].numpy()
    elif kind == "dup":
        pts = np.repeat(g.normal(size=(n // 5, 3)), 5, 0).astype(np.float32)  # coincident points -> distance 0
    else:
        pts = np.zeros((n, 3), np.float32); pts[:, 0] = g.uniform(0, 1, n)  # degenerate extent in y, z
    got = distCUDA2(torch.tensor(pts, device=DEV)).cpu().numpy()
    ref = knn3_mean_dist2(pts)
    if n < 4:
        assert np.isinf(got).all() and np.isinf(ref).all()
    else:
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-12)


def test_distcuda2_full_size_property():
    """300k points: equals brute force on a random subset (the oracle is O(N^2))."""
    from simple_knn._C import distCUDA2
    from manus_amd.synthetic import make_scene
    pts = make_scene(n_gaussians=300000, kind="hand", seed=0, grid_res=8, n_cameras=1, width=32, height=32)["params"]["_xyz"]
    got = distCUDA2(pts.to(DEV)).cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all()
    p = pts.numpy().astype(np.float32)
    for i in np.random.default_rng(0).integers(0, p.shape[0], 50):
        d = ((p - p[i]) ** 2).sum(1)
        d[i] = np.inf
        ref = np.sort(d)[:3].mean()
        assert abs(got[i] - ref) <= 2e-5 * ref + 1e-12


def test_dropin_packages_and_argument_errors():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    cam = make_camera(64, 48)
    a = cam_args(cam)
    st = GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=a["tanfovx"], tanfovy=a["tanfovy"],
                                       bg=torch.ones(3, device=DEV), scale_modifier=1,
                                       viewmatrix=torch.tensor(a["view"], device=DEV).reshape(1, 4, 4),
                                       projmatrix=torch.tensor(a["proj"], device=DEV).reshape(1, 4, 4), sh_degree=3,
                                       campos=torch.tensor(cam["camera_center"], device=DEV).reshape(1, 3),
                                       prefiltered=False, debug=False)
    assert len(st) == 12
    r = GaussianRasterizer(raster_settings=st)
    m, c, col, op = [torch.tensor(x, device=DEV) for x in random_gaussians(100, seed=0)]
    m2 = torch.zeros_like(m)
    with pytest.raises(Exception):
        r(means3D=m, means2D=m2, opacities=op[:, None], shs=None, colors_precomp=None, cov3D_precomp=c)
    with pytest.raises(Exception):
        r(means3D=m, means2D=m2, opacities=op[:, None], colors_precomp=col, scales=None, rotations=None, cov3D_precomp=None)
    with pytest.raises(Exception):
        r(means3D=m, means2D=m2, opacities=op[:, None], colors_precomp=col, scales=torch.ones_like(m),
          rotations=torch.ones((100, 4), device=DEV), cov3D_precomp=c)
    img, radii = r(means3D=m, means2D=m2, opacities=op[:, None], shs=None, colors_precomp=col, scales=None,
                   rotations=None, cov3D_precomp=c)
    assert img.shape == (3, 48, 64) and radii.shape == (100,) and radii.dtype == torch.int32
    assert r.markVisible(m).dtype == torch.bool
    with pytest.raises(Exception):  # no CPU fallback
        r(means3D=m.cpu(), means2D=m2.cpu(), opacities=op[:, None].cpu(), colors_precomp=col.cpu(), cov3D_precomp=c.cpu())


def test_transposed_view_matrices_and_the_camera_cache():
    """The reference keeps `world_view_transform` as a transposed VIEW (non-contiguous): the operator packs it on the device
    (same image as from a contiguous copy), reuses the packed table while the camera tensors are the same unmodified objects,
    and builds a new one after an in-place change of a camera tensor."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from manus_amd import _lib
    cam = make_camera(64, 48)
    a = cam_args(cam)
    m, c, col, op = [torch.tensor(x, device=DEV) for x in random_gaussians(400, seed=3)]
    view_c = torch.tensor(a["view"], device=DEV).reshape(1, 4, 4).contiguous()
    view_t = view_c[0].t().contiguous().t()[None]             # same values, column-major strides
    assert not view_t.is_contiguous() and torch.equal(view_t, view_c)
    proj = torch.tensor(a["proj"], device=DEV).reshape(1, 4, 4)
    pos = torch.tensor(cam["camera_center"], device=DEV).reshape(1, 3)

    def render(view):
        st = GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=a["tanfovx"], tanfovy=a["tanfovy"], bg=torch.ones(3, device=DEV),
                                           scale_modifier=1, viewmatrix=view, projmatrix=proj, sh_degree=3, campos=pos, prefiltered=False, debug=False)
        return GaussianRasterizer(raster_settings=st)(means3D=m, means2D=torch.zeros_like(m), opacities=op[:, None], colors_precomp=col, cov3D_precomp=c)[0]

    want = render(view_c)
    n0 = len(_lib._PACKED)
    got = render(view_t)
    assert torch.equal(got, want)
    n1 = len(_lib._PACKED)
    assert n1 == n0 + 1
    assert torch.equal(render(view_t), want) and len(_lib._PACKED) == n1        # the table of these tensor objects is reused
    moved = view_c.clone()
    moved[0, 3, 0] += 0.05                                                      # (row-vector convention: the translation row)
    want_moved = render(moved)
    assert not torch.equal(want_moved, want)
    view_t[0, 3, 0] += 0.05                                                     # in place: same object, new version
    assert torch.equal(render(view_t), want_moved)


def test_auto_fenced_operator_route_never_returns_a_truncated_image():
    """Operator route after RasterContext.AUTO_FENCE_AFTER clean forwards of one (V, N, W, H): the blocking read of the pair
    count gives way to a fence the next forward resolves.  A forward that nothing after it would check -- an evaluation render
    under no_grad, or the first forward of a camera the context has not read back -- must not return an image cut short by the
    capacity learnt on another camera; two cameras used in turn still reach the fenced mode; and an overflow of a fenced
    forward (same camera, Gaussians grown in place) is reported by poll()."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from manus_amd import rasterizer as rz
    from manus_amd._lib import ManusHipError
    W, H, n = 320, 240, 20000
    ctx = rz.context(DEV)
    m, cov, col, op = [torch.tensor(x, device=DEV) for x in random_gaussians(n, seed=11)]
    leaves = [t.requires_grad_(True) for t in (m, cov, col)]
    op = op[:, None].clone().requires_grad_(True)
    leaves.append(op)
    m2 = torch.zeros_like(m, requires_grad=True)
    w_img = torch.rand((3, H, W), generator=torch.Generator().manual_seed(4)).to(DEV)

    def settings(focal=None, pos=(0.3, -0.2, -1.5)):
        cam = make_camera(W, H, pos=pos, focal=focal)        # fresh camera tensor objects on every call
        a = cam_args(cam)
        return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=a["tanfovx"], tanfovy=a["tanfovy"],
                                             bg=torch.ones(3, device=DEV), scale_modifier=1,
                                             viewmatrix=torch.tensor(a["view"], device=DEV).reshape(1, 4, 4),
                                             projmatrix=torch.tensor(a["proj"], device=DEV).reshape(1, 4, 4), sh_degree=3,
                                             campos=torch.tensor(cam["camera_center"], device=DEV).reshape(1, 3),
                                             prefiltered=False, debug=False)

    def render(st):
        return GaussianRasterizer(raster_settings=st)(means3D=m, means2D=m2, opacities=op, colors_precomp=col, cov3D_precomp=cov)

    def step(st):
        for t in leaves + [m2]:
            t.grad = None
        img, radii = render(st)
        (img * w_img).sum().backward()
        return img.detach().clone(), radii.clone(), [t.grad.clone() for t in leaves + [m2]]

    def pairs(st):
        ctx.clear()
        with torch.no_grad():
            render(st)
        return ctx.check_overflow()

    st_a, st_b = settings(focal=0.6 * W), settings(focal=3.0 * W)    # B: the same view zoomed in
    n_a, n_b = pairs(st_a), pairs(st_b)
    # B outgrows the capacity learnt on A (at least the default capacity of the key)
    assert n_b > max(1.25 * n_a + 4096, rz.default_pair_capacity(1, n)), (n_a, n_b)
    ctx.clear()
    with torch.no_grad():
        want_img, want_radii = [t.clone() for t in render(st_b)]
    ctx.clear()
    want_step = step(st_b)
    assert torch.equal(want_step[0], want_img)

    def warm_on_a():
        ctx.clear()
        ctx.auto_fenced = 0
        for _ in range(rz.RasterContext.AUTO_FENCE_AFTER + 1):
            step(st_a)
        assert ctx.auto_fenced > 0

    try:
        # (a) an evaluation render of B
        warm_on_a()
        with torch.no_grad():
            img, radii = render(st_b)
        assert torch.equal(img, want_img) and torch.equal(radii, want_radii)
        rz.poll(DEV)
        # (b) a training forward of B through camera tensors the context has not seen
        warm_on_a()
        got = step(settings(focal=3.0 * W))                    # (new tensors: a new packed camera table)
        assert torch.equal(got[0], want_img) and torch.equal(got[1], want_radii)
        for g, w in zip(got[2], want_step[2]):
            assert torch.equal(g, w)
        rz.poll(DEV)
        # (c) two cameras in turn (bench.py --route dropin cycles over its cameras) still switch to the fences
        st_c = settings(focal=0.6 * W, pos=(0.32, -0.18, -1.5))
        ctx.clear()
        ctx.auto_fenced = 0
        for k in range(12):
            step(st_a if k % 2 == 0 else st_c)
        assert ctx.auto_fenced > 0
        rz.poll(DEV)
        # (d) a camera seen before, but the Gaussians grow in place beyond the capacity: reported by the poll after the forward
        warm_on_a()
        fenced_before = ctx.auto_fenced
        with torch.no_grad():
            cov.mul_(9.0)
        try:
            render(st_a)
            assert ctx.auto_fenced == fenced_before + 1
            with pytest.raises(ManusHipError):
                rz.poll(DEV)
        finally:
            with torch.no_grad():
                cov.div_(9.0)
    finally:
        ctx.clear()


def test_render_gaussians_reference_signature(golden_dir):
    """The reference call sequence (hand module forward -> render_gaussians) end to end vs the oracles."""
    from types import SimpleNamespace
    from manus_amd.modules import hand_forward
    from manus_amd.render import render_gaussians
    from manus_amd.structures import Bones
    from manus_amd.synthetic import make_scene
    sc = make_scene(n_gaussians=3000, kind="hand", seed=5, grid_res=24, n_cameras=1, width=96, height=64,
                    cam_radius=0.5, sigma_range=(2e-3, 8e-3), device="cpu")
    P = {k: v.clone().to(DEV).requires_grad_(True) for k, v in sc["params"].items()}
    model = SimpleNamespace(_xyz=P["_xyz"], _scaling=P["_scaling"], _rotation=P["_rotation"],
                            get_features=torch.cat([P["_features_dc"], P["_features_rest"]], 1),
                            get_opacity=torch.sigmoid(P["_opacity"]), grid_center=sc["grid_center"],
                            grid_scale=sc["grid_scale"], grid_weights=sc["grid"])
    batch = dict(bones_posed=Bones(None, None, None, sc["posed"][0]), bones_rest=Bones(None, None, None, sc["rest"]))
    pred = hand_forward(model, batch)
    assert pred.tf.shape == (3000, 4, 4)
    c = sc["cameras"][0]
    camera = SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                             world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32)[None],
                             full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32)[None],
                             camera_center=torch.tensor(c["camera_center"], dtype=torch.float32)[None])
    out = render_gaussians(pred.posed_xyz, pred.posed_cov, pred.cano_xyz, pred.cano_features, pred.cano_opacity,
                           camera, torch.ones(3), sh_degree=3, tf=pred.tf, device=torch.device(DEV))
    assert out["render"].shape == (64, 96, 3) and out["visibility_filter"].dtype == torch.bool
    g = torch.randn((64, 96, 3), generator=torch.Generator().manual_seed(0)).to(DEV)
    (out["render"] * g).sum().backward()
    assert out["viewspace_points"].grad is not None and out["viewspace_points"].grad.shape == (3000, 3)
    # oracle: torch chain -> C rasterizer -> torch backward
    Pc = {k: v.clone().requires_grad_(True) for k, v in sc["params"].items()}
    o = tr.hand_forward(Pc, sc["grid"], sc["grid_center"], sc["grid_scale"], sc["posed"][0], sc["rest"],
                        torch.tensor(c["camera_center"], dtype=torch.float32))
    a = cam_args(c)
    ro = RasterOracle(a["W"], a["H"], a["tanfovx"], a["tanfovy"], a["view"], a["proj"], o["posed_xyz"].detach().numpy(),
                      o["posed_cov"].detach().numpy(), o["colors"].detach().numpy(), o["opacity"].detach().numpy()[:, 0],
                      np.ones(3, np.float32))
    img_o = np.transpose(ro.color, (1, 2, 0))
    assert np.abs(out["render"].detach().cpu().numpy() - img_o).max() < 5e-3
    tgt = np.clip(img_o + 0.05, 0, 1)
    assert abs(psnr(out["render"].detach().cpu().numpy(), tgt) - psnr(img_o, tgt)) < 0.01
    b = ro.backward(np.transpose(g.cpu().numpy(), (2, 0, 1)))
    (o["posed_xyz"] * torch.tensor(b["means3D"])).sum().backward(retain_graph=True)
    (o["posed_cov"] * torch.tensor(b["cov3D"])).sum().backward(retain_graph=True)
    (o["colors"] * torch.tensor(b["colors"])).sum().backward(retain_graph=True)
    (o["opacity"][:, 0] * torch.tensor(b["opacity"])).sum().backward()
    # End to end the two chains feed the rasterizer inputs that differ by fp32 roundoff
    # (1e-7), which can move a single (pixel, Gaussian) pair across the alpha < 1/255
    # decision; stage by stage on identical inputs every kernel agrees to < 1e-5 (see
    # test_gpu_raster / test_gpu_lbs_sh).  A flipped pair rescales the transmittance of
    # every Gaussian behind it at that pixel, so a handful of rows move by ~1e-3 of the
    # largest gradient while all other rows agree to roundoff.  Hence: a max-norm bound that
    # admits such flips, and a bound on how many rows may be affected at all.
    for k in P:
        a_, b_ = P[k].grad.cpu().numpy().astype(np.float64), Pc[k].grad.numpy().astype(np.float64)
        assert max_rel_err(a_, b_) < 5e-3, (k, max_rel_err(a_, b_))
        rows = np.abs(a_ - b_).reshape(a_.shape[0], -1).max(1) > 2e-5 * np.abs(b_).max()
        assert rows.mean() < 0.03, (k, rows.sum())
    vis = ro.radii > 0
    assert (out["visibility_filter"].cpu().numpy() == vis).all()
    assert max_rel_err(out["viewspace_points"].grad.cpu().numpy(), b["means2D"]) < 5e-3  # flips, as above


def test_l1_loss_kernel():
    from manus_amd.ops import l1_loss_grad
    a = torch.rand((2, 3, 37, 53), device=DEV)
    b = torch.rand((2, 3, 37, 53), device=DEV)
    a[0, 0, 0, :5] = b[0, 0, 0, :5]
    s, g = l1_loss_grad(a, b)
    assert abs(float(s) - float((a - b).abs().sum())) < 1e-2
    assert torch.equal(g, torch.sign(a - b) / a.numel())


@pytest.mark.parametrize("loss", ["l1", "l1+ssim"])
def test_engine_step_matches_sequential_reference_steps(loss):
    """V views in one batched step == the mean of V single-view reference-style steps."""
    from manus_amd.engine import HipViewCompute, ViewShardedStep
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=4000, kind="hand", seed=2, grid_res=24, n_cameras=4, width=96, height=64,
                    cam_radius=0.5, sigma_range=(2e-3, 8e-3), device=DEV)
    ct = camera_table(sc["cameras"], DEV)
    tg = torch.rand((4, 3, 64, 96), device=DEV)
    hc = HipViewCompute(sc, tg, ct, loss=loss)
    shapes = {k: v.shape for k, v in hc.params.items()}
    from util import keep
    full = keep(ViewShardedStep(sc["N"], shapes, hc, 4).step())     # (hc keeps its output buffers: the steps below reuse them)
    if loss == "l1+ssim":  # loss value = mean over views of 0.8 L1 + 0.2 (1 - ssim) of the oracle restatement
        with torch.no_grad():
            img = torch.cat([hc.forward_views([v])[0] for v in range(4)]).cpu()
        ref = np.mean([float(tr.rgb_ssim_loss(img[v].permute(1, 2, 0), tg[v].cpu().permute(1, 2, 0))) for v in range(4)])
        assert abs(float(full["loss"]) - ref) < 2e-5
    acc = None
    for v in range(4):
        o = hc([v], 1.0)
        if acc is None:
            acc = {k: g.clone() for k, g in o["grads"].items()}
            g2, vis, rad, loss = o["grad2d"].clone(), o["vis"].clone(), o["radii"].clone(), o["loss"].clone()
        else:
            for k in acc:
                acc[k] += o["grads"][k]
            g2 += o["grad2d"]; vis += o["vis"]; rad = torch.maximum(rad, o["radii"]); loss += o["loss"]
    for k in acc:
        assert max_rel_err(full["grads"][k].cpu().numpy(), (acc[k] / 4).cpu().numpy()) < 1e-5, k
    assert max_rel_err(full["grad2d"].cpu().numpy(), g2.cpu().numpy()) < 1e-5
    assert torch.equal(full["vis"], vis) and torch.equal(full["radii"], rad.to(torch.int32))
    assert abs(float(full["loss"]) - float(loss) / 4) < 1e-5


def test_packed_step_writes_gradients_in_place():
    """The multi-GPU step's flat all-reduce buffer: from the second step on the backward kernels write most leaves
    straight into it (grad arena).  Same numbers as the unpacked single-GPU step, and no packing copy for those
    leaves (their gradients alias the buffer)."""
    from manus_amd.engine import GRAD_LAYOUT, HipViewCompute, ViewShardedStep
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=3000, kind="hand", seed=3, grid_res=24, n_cameras=2, width=96, height=64,
                    cam_radius=0.5, sigma_range=(2e-3, 8e-3), device=DEV)
    ct = camera_table(sc["cameras"], DEV)
    tg = torch.rand((2, 3, 64, 96), device=DEV)
    hc = HipViewCompute(sc, tg, ct, loss="l1+ssim")
    shapes = {k: v.shape for k, v in hc.params.items()}
    plain = ViewShardedStep(sc["N"], shapes, hc, 2).step()
    ref = {k: v.clone() for k, v in plain["grads"].items()}
    ref_g2, ref_vis, ref_loss = plain["grad2d"].clone(), plain["vis"].clone(), float(plain["loss"])
    hc.grad_arena = None
    st = ViewShardedStep(sc["N"], shapes, hc, 2)
    st.always_pack = True
    st.step()                      # allocates the flat buffer
    out = st.step()                # arena in use
    flat = st._flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for name, _ in GRAD_LAYOUT:
        assert torch.equal(out["grads"][name], ref[name]), name
        assert lo <= out["grads"][name].data_ptr() < hi
    assert torch.equal(out["grad2d"], ref_g2) and torch.equal(out["vis"], ref_vis)
    assert abs(float(out["loss"]) - ref_loss) < 1e-7
    # every leaf gradient (xyz included: the skin-weight path is accumulated into it by the kernel) and both
    # statistics alias the buffer: the step makes no packing copy at all
    assert lo <= out["grad2d"].data_ptr() < hi and lo <= out["vis"].data_ptr() < hi
    assert float(out["overflow"]) == 0.0
    raw = hc(st.local_views, 0.5)  # what the kernels themselves return: views of the flat buffer
    assert all(lo <= raw["grads"][n].data_ptr() < hi for n, _ in GRAD_LAYOUT)


def test_forward_from_another_host_thread_and_after_device_churn():
    """include/manus_hip.h "Conventions": the library's own state is host-side and per device / per (thread, device).
    A forward issued from a second host thread (fresh thread-local side stream; the per-tile sort route is the one that
    uses it) after set_device churn gives the bit-identical image of the main thread's default route."""
    import os
    import threading
    from manus_amd.rasterizer import rasterize_views
    from util import cam_table_np, make_camera, random_gaussians
    cam = make_camera(160, 96)
    m, c, col, op = random_gaussians(3000, seed=5)
    ct = torch.from_numpy(cam_table_np([cam])).to(DEV)
    args = [torch.tensor(x, device=DEV) for x in (m, col, op, c)]
    bg = torch.ones(3, device=DEV)

    def render():
        m2d = torch.zeros((1, 3000, 3), device=DEV)
        with torch.no_grad():
            img, radii = rasterize_views(ct, args[0], m2d, args[1], args[2], args[3], bg, 160, 96)
        torch.cuda.synchronize()
        return img.cpu(), radii.cpu()

    ref = render()
    out = {}

    def worker():
        for _ in range(3):
            torch.cuda.set_device(0)
        os.environ["MGR_BINNING"] = "sorted"
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=DEV)):
                out["sorted"] = render()
        finally:
            os.environ.pop("MGR_BINNING", None)
        out["ordered"] = render()

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    for k in ("sorted", "ordered"):
        assert torch.equal(out[k][0], ref[0]) and torch.equal(out[k][1], ref[1]), k


def test_glue_kernels_equal_the_torch_expressions():
    """mgr_pack_camera / mgr_bone_transforms (one launch each on the reference-shaped route) against the torch expressions
    they replace: the camera row exactly, posed @ inv(rest) (hand_dynamic.py:93-102) to fp32 roundoff; tensors that carry a
    gradient, or live on the host, still take the torch route."""
    from manus_amd import _lib
    from manus_amd.synthetic import make_scene
    from manus_amd.transforms import bone_transforms
    sc = make_scene(n_gaussians=100, kind="hand", seed=3, grid_res=16, n_cameras=3, width=96, height=64, device="cpu")
    cams = sc["cameras"]
    g = lambda c, k: torch.tensor(c[k], dtype=torch.float32)
    tfx = [math.tan(c["fovx"] / 2) for c in cams]
    tfy = [math.tan(c["fovy"] / 2) for c in cams]
    host = _lib.pack_cameras(tfx, tfy, [g(c, "world_view_transform")[None] for c in cams], [g(c, "full_proj_transform")[None] for c in cams],
                             [g(c, "camera_center")[None] for c in cams], DEV)       # host tensors: cat + copies
    dev = _lib.pack_cameras(tfx, tfy, [g(c, "world_view_transform")[None].to(DEV) for c in cams],
                            [g(c, "full_proj_transform")[None].to(DEV) for c in cams], [g(c, "camera_center")[None].to(DEV) for c in cams], DEV)
    assert dev.shape == (3, _lib.MGR_CAM_FLOATS) and torch.equal(host, dev)
    one = _lib.pack_cameras(tfx[1], tfy[1], g(cams[1], "world_view_transform").to(DEV), g(cams[1], "full_proj_transform").to(DEV),
                            g(cams[1], "camera_center").to(DEV), torch.device("cuda"))
    assert torch.equal(one[0], host[1])
    posed, rest = sc["posed"][0].float(), sc["rest"].float()
    for bgd in (True, False):
        want = bone_transforms(posed, rest, background=bgd)                       # host tensors: torch.linalg.inv + einsum
        got = bone_transforms(posed.to(DEV), rest.to(DEV), background=bgd)
        assert got.shape == want.shape and got.is_cuda
        assert float((got.cpu() - want).abs().max()) < 2e-6 * float(want.abs().max())
    pg = posed.to(DEV).requires_grad_(True)
    t = bone_transforms(pg, rest.to(DEV))
    t.sum().backward()
    assert pg.grad is not None and torch.isfinite(pg.grad).all()


@pytest.mark.parametrize("extra", [[], ["--dropin-fenced"], ["--kind", "object"]])
def test_bench_dropin_route_runs(extra):
    """`bench.py --route dropin` (the zero-change operator route: modules.hand_forward / object_forward + render_gaussians +
    losses under autograd, one view per step) at a tiny size: one JSON line, labelled as not the headline, finite gradients."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--route", "dropin", "--gaussians", "4000", "--views", "2", "--width", "160",
           "--height", "96", "--steps", "2", "--warmup", "1", "--full"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["headline"] is False and d["value"] > 0 and d["config"]["route"] == "dropin" and d["config"]["finite_grads"] is True
    # (without the flag the context itself stops reading the pair count back after RasterContext.AUTO_FENCE_AFTER clean forwards:
    #  with --full -- five timed loops and the breakdown loop -- this run has more than that many)
    assert d["config"]["host_syncs_per_step"] == 0 and d["config"]["host_issue_ms_per_step"] > 0
    assert (d["config"]["width"], d["config"]["height"]) == (160, 96)

"""GPU: the pose gradient dL/d(bone transforms) -- the modular kernel (mgr_lbs_pose_bwd behind ops.lbs_cov), the fused route
(mgr_views_backward_pose behind HipViewCompute(pose_grad=True)) and the pose module on top of them.

Reference of (a) and (b): oracle/torch_ref.py in float64 on the CPU, the transforms a leaf.  A reduced quantity is judged
against the magnitude it was summed from: A[p,b,k] = sum_n |w_nb * G_nk| (G = the fp64 oracle's dL/d(blended transform)),
e(x) = max |x - ref64| / max(A, 1e-3 max A).  Tolerance: this project's rule (test_gpu_articulation_edges.check_rows),
e(kernel) <= 8 * max(e32, 2^-23), where e32 is the larger e() of the same oracle in float32 with the Gaussians in natural and
in reversed order (the kernel is free to sum in another order).  The inputs are those of `lbs_inputs` of that file, restated."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr

from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
FACTOR = 8.0
F32, F64 = torch.float32, torch.float64


def rounded(x):
    return x.to(F32).to(F64)


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def lbs_inputs(B, P, N, seed=0):
    """General affine transforms, skin rows with exact zeros, quaternion norms over four decades, random r_xyz / r_cov / r_tf."""
    g = torch.Generator().manual_seed(9000 + 101 * B + 11 * P + N + seed)
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)
    ru = lambda *s: torch.rand(s, generator=g, dtype=F64)
    q = rn(N, 4)
    q = q / q.norm(dim=1, keepdim=True) * 10.0 ** (ru(N, 1) * 4.0 - 2.0)
    T = torch.eye(4, dtype=F64).repeat(P, B, 1, 1)
    T[:, :, :3, :] += 0.2 * rn(P, B, 3, 4)
    w = ru(N, B) ** 2
    w[ru(N, B) < 0.3] = 0.0
    w[torch.arange(N), torch.randint(0, B, (N,), generator=g)] += 0.1
    return dict(B=B, P=P, N=N, xyz=rounded(0.2 * rn(N, 3)), log_scale=rounded(ru(N, 3) * 7.0 - 9.0), rot=rounded(q),
                r_xyz=rounded(rn(P, N, 3)), r_cov=rounded(rn(P, N, 6)), r_tf=rounded(rn(P, N, 3, 4)),
                T=rounded(T), w=rounded(w / w.sum(1, keepdim=True)))


def pose_oracle(inp, dtype, tf_loss, flip=False, colour=None):
    """dL/dT (P,B,4,4) of tr.lbs_forward looped over the poses with T a leaf, and A (P,B,12) (module docstring).  flip: the
    Gaussians in reversed order.  colour = (features, cams (P,3), r_col (P,N,3)): the loss is the random linear one on the
    colours of tr.sh_colors alone (test b); also returns the smallest |pre-clamp colour| and camera distance."""
    f = (lambda x, d=0: x.flip(d)) if flip else (lambda x, d=0: x)
    xyz, ls, rot, w = (f(inp[k]).to(dtype) for k in ("xyz", "log_scale", "rot", "w"))
    T = inp["T"].to(dtype).clone().requires_grad_(True)
    loss, tfs, margin, dist = 0, [], math.inf, math.inf
    for p in range(inp["P"]):
        px, pc, tf = tr.lbs_forward(xyz, ls, rot, w, T[p])
        tf.retain_grad()
        tfs.append(tf)
        if colour is None:
            loss = loss + (px * f(inp["r_xyz"][p]).to(dtype)).sum() + (pc * f(inp["r_cov"][p]).to(dtype)).sum()
            if tf_loss:
                loss = loss + (tf[:, :3, :] * f(inp["r_tf"][p]).to(dtype)).sum()
        else:
            feats, cams, r_col = colour
            col = tr.sh_colors(px, f(feats).to(dtype), xyz, cams[p].to(dtype), 3, tf)
            loss = loss + (col * f(r_col[p]).to(dtype)).sum()
            with torch.no_grad():
                cam_h = torch.nn.functional.pad(cams[p].to(dtype).reshape(1, 3).expand(xyz.shape[0], 3), (0, 1), value=1.0)
                d = xyz - torch.einsum("nij,nj->ni", torch.linalg.inv(tf), cam_h)[:, :3]
                dist = min(dist, float(d.norm(dim=1).min()))
                shs = f(feats).to(dtype).transpose(1, 2).reshape(-1, 3, 16)
                pre = tr.eval_sh(3, shs, d / d.norm(dim=1, keepdim=True)) + 0.5
                margin = min(margin, float(pre.abs().min()))
    loss.backward()
    A = torch.stack([w.abs().T @ t.grad[:, :3, :].reshape(-1, 12).abs() for t in tfs])
    return T.grad.detach(), A.detach(), margin, dist


def err_of(x, ref64, A):
    x = x.detach().cpu().double().reshape(ref64.shape)[..., :3, :].reshape(A.shape)
    den = torch.maximum(A, 1e-3 * A.max())
    return float(((x - ref64[..., :3, :].reshape(A.shape)).abs() / den).max())


def check_pose(tag, got, inp, tf_loss, colour=None):
    ref64, A, margin, dist = pose_oracle(inp, F64, tf_loss, colour=colour)
    e32 = max(err_of(pose_oracle(inp, F32, tf_loss, flip=fl, colour=colour)[0], ref64, A) for fl in (False, True))
    ek = err_of(got, ref64, A)
    print("RATIO %-40s e_kernel %.3e  e32 %.3e  ratio %.2f" % (tag, ek, e32, ek / max(e32, EPS32)))
    assert ek <= FACTOR * max(e32, EPS32), (tag, ek, e32)
    if colour is None:      # (through tr.sh_colors the oracle's inv(tf) also reads the constant row, which the kernels do not carry)
        assert float(ref64[..., 3, :].abs().max()) == 0.0
    return margin, dist


# =================================================================================================================
# (a) the modular kernel against fp64
# =================================================================================================================
#             B   P    N    tf44  dL_dtf  T as (B,4,4)
POSE_CASES = [(1, 1, 1, False, False, True), (1, 3, 777, True, True, False), (3, 1, 63, False, True, False),
              (3, 3, 257, True, False, False), (21, 1, 64, True, True, True), (21, 3, 65, False, False, False),
              (21, 1, 777, False, True, False), (25, 3, 255, True, True, False), (25, 1, 257, False, False, True),
              (32, 1, 255, False, True, False), (32, 3, 1, True, False, False), (32, 3, 777, False, True, False),
              # more chunks of 256 than workgroups (1024): a workgroup takes several chunks before it writes its partial
              (3, 1, 1024 * 256 + 257, False, True, True)]


@pytest.mark.parametrize("B,P,N,tf44,tf_loss,squeeze", POSE_CASES)
def test_lbs_cov_pose_gradient_vs_fp64(B, P, N, tf44, tf_loss, squeeze):
    """ops.lbs_cov with transforms.requires_grad_(True): T.grad against tr.lbs_forward in fp64.  N: partial wave, partial
    workgroup, one / two / four partials for the fold; B: below 8, no multiple of 8, the MANUS count, above 24, MGR_MAX_BONES.
    Row 3 of every 4x4 exactly zero; the gradient has the shape `transforms` had.  Fails without the feature: T.grad is None."""
    from manus_amd import ops
    inp = lbs_inputs(B, P, N)
    T = _dev(inp["T"][0] if squeeze else inp["T"]).requires_grad_(True)
    leaves = [_dev(inp[k]).requires_grad_(True) for k in ("xyz", "log_scale", "rot", "w")]
    px, pc, tf = ops.lbs_cov(*leaves, T, tf44=tf44)
    loss = (px * _dev(inp["r_xyz"])).sum() + (pc * _dev(inp["r_cov"])).sum()
    if tf_loss:
        t3 = tf[:, :, :3, :] if tf44 else tf.reshape(P, N, 3, 4)
        loss = loss + (t3 * _dev(inp["r_tf"])).sum()
    loss.backward()
    assert T.grad is not None and T.grad.shape == T.shape
    g = T.grad.cpu()
    assert float(g[..., 3, :].abs().max()) == 0.0
    check_pose("pose B=%d P=%d N=%d tf44=%d tf=%d" % (B, P, N, tf44, tf_loss), g, inp, tf_loss)
    assert all(x.grad is not None and torch.isfinite(x.grad).all() for x in leaves)


def test_lbs_cov_without_pose_gradient_launches_as_before():
    """transforms that does not require a gradient: no gradient for it, the leaf gradients are bit for bit those of a call in
    which it does."""
    from manus_amd import ops
    inp = lbs_inputs(21, 3, 257)
    out = []
    for need in (False, True):
        T = _dev(inp["T"]).requires_grad_(need)
        leaves = [_dev(inp[k]).requires_grad_(True) for k in ("xyz", "log_scale", "rot", "w")]
        px, pc, tf = ops.lbs_cov(*leaves, T)
        ((px * _dev(inp["r_xyz"])).sum() + (pc * _dev(inp["r_cov"])).sum()).backward()
        assert (T.grad is not None) == need
        out.append([x.grad.clone() for x in leaves])
    assert all(torch.equal(a, b) for a, b in zip(*out))


# =================================================================================================================
# (b) the SH view-direction path reaches the pose
# =================================================================================================================
def test_sh_colour_path_reaches_the_pose():
    """ops.lbs_cov(tf44=False) -> ops.sh_colors(features, xyz, tf, cams) -> a random linear loss on the colours only: T.grad
    against tr.lbs_forward + tr.sh_colors in fp64, rule of (a).  Camera distances >= 0.3 and no pre-clamp colour within 1e-3
    of the clamp (both checked in the fp64 oracle): a fifth of the Gaussians is dark in every view, the rest is lit."""
    from manus_amd import ops
    V, N, B = 3, 257, 21
    inp = lbs_inputs(B, V, N, seed=5)
    g = torch.Generator().manual_seed(77)
    feats = 0.02 * torch.randn((N, 16, 3), generator=g, dtype=F64)
    feats[:, 0, :] = torch.where(torch.rand((N, 1), generator=g, dtype=F64) < 0.2, -3.0, 1.0) + 0.3 * torch.rand((N, 3), generator=g, dtype=F64)
    feats = rounded(feats)
    d = torch.randn((V, 3), generator=g, dtype=F64)
    cams3 = rounded(d / d.norm(dim=1, keepdim=True) * torch.tensor([[1.5], [2.5], [4.0]], dtype=F64))
    r_col = rounded(torch.randn((V, N, 3), generator=g, dtype=F64))
    colour = (feats, cams3, r_col)
    T = _dev(inp["T"]).requires_grad_(True)
    px, pc, tf = ops.lbs_cov(_dev(inp["xyz"]), _dev(inp["log_scale"]), _dev(inp["rot"]), _dev(inp["w"]), T, tf44=False)
    cams = torch.zeros((V, 40), dtype=F32, device=DEV)
    cams[:, 34:37] = _dev(cams3)
    col = ops.sh_colors(_dev(feats), _dev(inp["xyz"]), tf, cams)
    (col * _dev(r_col)).sum().backward()
    assert T.grad is not None and T.grad.shape == (V, B, 4, 4)
    assert float(T.grad[..., 3, :].abs().max()) == 0.0
    margin, dist = check_pose("pose through sh_colors", T.grad.cpu(), inp, False, colour=colour)
    print("smallest |pre-clamp colour| %.3e, smallest camera distance %.3f" % (margin, dist))
    assert margin > 1e-3 and dist >= 0.3
    assert float(T.grad.abs().max()) > 0.0


# =================================================================================================================
# (c) .. (f): the fused route
# =================================================================================================================
def _scene(kind, n, views):
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=n, kind=kind, seed=6, grid_res=24, n_cameras=views, width=96, height=64,
                    cam_radius=0.5, sigma_range=(2e-3, 8e-3), device=DEV)
    return sc, camera_table(sc["cameras"], DEV)


def _clone(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else v.clone()) for k, v in o.items()}


def _targets(views):
    return torch.rand((views, 3, 64, 96), device=DEV, generator=torch.Generator(device=DEV).manual_seed(views))


FUSED_CASES = [("hand", 1, 3000), ("hand", 3, 3000), ("hand", 8, 3000), ("hand", 11, 3000), ("composite", 7, 6000),
               ("hand", 8, 37), ("hand", 2, 1), ("composite", 4, 263)]


@pytest.mark.parametrize("kind,views,n", FUSED_CASES)
def test_fused_pose_gradient_equals_modular(kind, views, n):
    """HipViewCompute(pose_grad=True): d_transforms of the fused step (mgr_views_backward_pose) against the modular route
    (autograd through ops.lbs_cov / ops.sh_colors / the rasterizer with the transforms a leaf), per view to the bar the leaf
    gradients of test_gpu_fused.py are held to (5e-3: threshold decisions of two independent fp32 chains).  The object rows of
    a composite have no transform: the modular route gives them none.  With pose_grad the gradients and statistics are bit for
    bit those of a step without it."""
    from manus_amd.engine import HipViewCompute
    sc, ct = _scene(kind, n, views)
    tg, ids = _targets(views), list(range(views))
    B = sc["transforms"].shape[1]
    of = _clone(HipViewCompute(sc, tg, ct, fused=True, pose_grad=True)(ids, 1.0 / views))
    om = HipViewCompute(sc, tg, ct, fused=False, pose_grad=True)(ids, 1.0 / views)
    plain = HipViewCompute(sc, tg, ct, fused=True)(ids, 1.0 / views)
    assert "d_transforms" not in plain
    a, b = of["d_transforms"], om["d_transforms"]
    assert a.shape == b.shape == (views, B, 4, 4)
    assert float(a[..., 3, :].abs().max()) == 0.0 and torch.isfinite(a).all()
    assert float(b.abs().max()) > 0.0
    for v in range(views):
        e = max_rel_err(a[v].cpu().numpy(), b[v].cpu().numpy())
        print("view %d  max_rel_err %.3e  max|dT| %.3e" % (v, e, float(b[v].abs().max())))
        assert e < 5e-3, (v, e)
    for k in plain["grads"]:
        assert torch.equal(plain["grads"][k], of["grads"][k]), k
    assert set(plain) | {"d_transforms"} == set(of)
    for k in ("grad2d", "vis", "radii", "overflow"):
        assert torch.equal(plain[k], of[k]), k
    # (the loss scalar is summed with float atomics in either setting: test_fused_run_to_run_determinism holds it to 1e-6)
    assert abs(float(plain["loss"]) - float(of["loss"])) < 1e-6


@pytest.mark.parametrize("kind,views,n", [c for c in FUSED_CASES if c[1] in (8, 4, 2, 1)])
def test_fused_pose_gradient_run_lists_and_determinism(kind, views, n):
    """Run lists on twice: the same bits.  Off (one lane per view): within 1e-5 max|.| of on, the bound the existing run-list
    test holds the leaf gradients to (the same per-lane values, summed in another order)."""
    from manus_amd._lib import lib
    from manus_amd.engine import HipViewCompute
    sc, ct = _scene(kind, n, views)
    tg, ids = _targets(views), list(range(views))
    hc = HipViewCompute(sc, tg, ct, fused=True, pose_grad=True)
    prev = lib().mgr_views_backward_run_lists(1)
    try:
        on1 = hc(ids, 1.0 / views)["d_transforms"].clone()
        on2 = hc(ids, 1.0 / views)["d_transforms"].clone()
        assert lib().mgr_views_backward_run_lists(0) == 1
        off = hc(ids, 1.0 / views)["d_transforms"].clone()
    finally:
        lib().mgr_views_backward_run_lists(prev)
    assert torch.equal(on1, on2)
    d, m = float((on1.double() - off.double()).abs().max()), float(off.abs().max())
    print("on/off max diff %.3e of max %.3e" % (d, m))
    assert d <= 1e-5 * max(m, 1e-30)


@pytest.mark.parametrize("n", [3000, 37])
def test_one_view_identity_between_pose_and_skin_weight_gradients(n):
    """V = 1, fused: sum_b <d_transforms[0][b][:3,:], T_b[:3,:]> == sum_n sum_b w_nb * d_skin_w[n][b] -- both contract the same
    dtf with the same w and T, so this isolates the new reduction from the blend.  Both sides from one call (d_skin_w is the
    kept buffer the step's backward wrote), accumulated in fp64 on the host, to 1e-5 relative."""
    from manus_amd import ops
    from manus_amd.engine import HipViewCompute
    sc, ct = _scene("hand", n, 1)
    hc = HipViewCompute(sc, _targets(1), ct, fused=True, pose_grad=True)
    out = hc([0], 1.0)
    d_w = hc._kept.tensors["_skin_w"].double().cpu()
    with torch.no_grad():
        w = ops.skin_weights(hc.params["_xyz"].detach(), hc.grid, sc["grid_center"], sc["grid_scale"]).double().cpu()
    T = sc["transforms"][0].double().cpu()
    lhs = float((out["d_transforms"][0].double().cpu()[:, :3, :] * T[:, :3, :]).sum())
    rhs = float((w * d_w).sum())
    scale = float((w * d_w).abs().sum())
    print("identity: lhs %.9e rhs %.9e  |terms| %.3e" % (lhs, rhs, scale))
    assert scale > 0.0
    assert abs(lhs - rhs) <= 1e-5 * max(abs(rhs), abs(lhs))


def _geodesic(Ra, Rb):
    c = ((Ra.transpose(-1, -2) @ Rb).diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0) * 0.5
    return torch.acos(c.clamp(-1.0, 1.0))


def test_pose_recovery_end_to_end():
    """Hand scene, n = 3000, 3 views, 96x64; targets = the fused forward at the true pose.  The posed transforms of three
    non-root bones are right-multiplied by rotations of 0.05 rad about fixed axes (in every view's frame); a zero-initialised
    PoseCorrection on the perturbed poses is optimised with torch.optim.Adam (lr 1e-3, 50 steps), each step through the fused step and pose_backward,
    the Gaussians frozen.  Asserted: the loss ends below the initial loss, the mean geodesic angle of the three bones below
    its initial value.  Measured on an MI355X: loss 0.000647 -> 0.000494, angle 0.0500 -> 0.0335 rad (LAB.md)."""
    from manus_amd.engine import HipViewCompute
    from manus_amd.pose import PoseCorrection, _exp_so3, pose_backward
    from manus_amd.transforms import bone_transforms
    views, ids = 3, [0, 1, 2]
    sc, ct = _scene("hand", 3000, views)
    rest = sc["rest"]                                               # (the scene has one pose = one frame per view)
    nb = rest.shape[0]
    hc = HipViewCompute(sc, torch.zeros((views, 3, 64, 96), device=DEV), ct, fused=True, pose_grad=True, loss="l1+ssim")
    with torch.no_grad():
        T_true = torch.stack([bone_transforms(sc["posed"][v], rest) for v in ids]).contiguous()
        assert torch.allclose(T_true, sc["transforms"][ids], atol=1e-5)
        hc.targets = hc.forward_views_fused(ids)[0].clone()
    bones = [3, 7, 12]
    axes = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], device=DEV)
    delta = torch.eye(4, device=DEV).repeat(nb, 1, 1)
    delta[bones, :3, :3] = _exp_so3(0.05 * axes)
    posed_bad = [sc["posed"][v] @ delta for v in ids]
    corr = PoseCorrection(views, nb, device=DEV)
    opt = torch.optim.Adam(corr.parameters(), lr=1e-3)

    def angle():
        with torch.no_grad():
            return float(torch.stack([_geodesic(corr(posed_bad[v], v)[bones, :3, :3], sc["posed"][v][bones, :3, :3]) for v in ids]).mean())

    losses, a0 = [], angle()
    for step in range(50):
        opt.zero_grad()
        corrected = [corr(posed_bad[v], v) for v in ids]
        with torch.no_grad():
            sc["transforms"][ids] = torch.stack([bone_transforms(c, rest) for c in corrected])
        out = hc(ids, 1.0 / views)
        losses.append(float(out["loss"]))
        for v in ids:
            corrected[v].backward(pose_backward(out["d_transforms"][v], corrected[v], rest))
        opt.step()
    a1 = angle()
    print("pose recovery: loss %.6f -> %.6f, mean geodesic angle %.4f -> %.4f rad" % (losses[0], losses[-1], a0, a1))
    assert losses[-1] < losses[0]
    assert a1 < a0


# =================================================================================================================
# errors
# =================================================================================================================
def test_pose_grad_on_an_object_scene_raises():
    from manus_amd.engine import HipViewCompute
    sc, ct = _scene("object", 500, 1)
    with pytest.raises(ValueError):
        HipViewCompute(sc, _targets(1), ct, pose_grad=True)


def test_lbs_pose_bwd_reports_bad_arguments():
    """skin_w = NULL (a static object has no transforms) and a workspace that is too small: non-zero, with a message."""
    from manus_amd._lib import lib, ptr, stream
    L = lib()
    inp = lbs_inputs(21, 1, 257)
    x, ls, q, w, T = (_dev(inp[k]) for k in ("xyz", "log_scale", "rot", "w", "T"))
    gx, gc = _dev(inp["r_xyz"]), _dev(inp["r_cov"])
    out = torch.full((1, 21, 4, 4), 7.0, device=DEV)
    nbytes = int(L.mgr_lbs_pose_workspace_bytes(1, 257, 21))
    assert nbytes == 2 * 21 * 12 * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = L.mgr_lbs_pose_bwd(1, 257, 21, ptr(x), ptr(ls), ptr(q), None, ptr(T), ptr(gx), ptr(gc), None, 12, ptr(out), ptr(ws), nbytes, stream())
    assert rc != 0 and b"skin_w" in L.mgr_last_error()
    rc = L.mgr_lbs_pose_bwd(1, 257, 21, ptr(x), ptr(ls), ptr(q), ptr(w), ptr(T), ptr(gx), ptr(gc), None, 12, ptr(out), ptr(ws), nbytes - 1, stream())
    assert rc != 0 and b"workspace" in L.mgr_last_error()
    rc = L.mgr_lbs_pose_bwd(1, 257, 33, ptr(x), ptr(ls), ptr(q), ptr(w), ptr(T), ptr(gx), ptr(gc), None, 12, ptr(out), ptr(ws), nbytes, stream())
    assert rc != 0
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0          # nothing was launched
    assert L.mgr_lbs_pose_bwd(1, 257, 21, ptr(x), ptr(ls), ptr(q), ptr(w), ptr(T), ptr(gx), ptr(gc), None, 12, ptr(out), ptr(ws), nbytes, stream()) == 0
    torch.cuda.synchronize()
    assert float(out[..., 3, :].abs().max()) == 0.0 and float(out.abs().max()) > 0.0

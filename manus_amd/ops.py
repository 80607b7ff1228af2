"""Autograd operators over the articulation kernels of libmanus_hip.so.

Each op mirrors one block of MANUS Python code (reference tree brown-ivl/manus):

    skin_weights   skinning_weights_from_voxel_grid      src/utils/gaussian_utils.py:167-196
    skin_grid_grad the grid's gradient of the same line   src/utils/gaussian_utils.py:173 (autograd there)
    lbs_cov        TrainingModule.forward LBS block      src/modules/hand_dynamic.py:106-127
                   + GaussianModel.get_covariance        src/models/gaussian.py:49-53,84-93
    sh_colors      calculate_colors_from_sh / eval_sh    src/utils/gaussian_utils.py:431-449
    project_points project_points                        src/utils/transforms.py:304-311
    distCUDA2      simple_knn._C.distCUDA2               src/models/gaussian.py:110
    eval_views, eval_triptych   validation_step's metrics / image   src/modules/base.py:112-154
    image_loss2d_grad           L1 + ssim() as it computes on CHW images   src/utils/loss_utils.py:22-97
    exposure_apply              per-camera affine colour correction of the render (no reference counterpart)

All of them require GPU tensors; there is no CPU or PyTorch fallback.
"""
import ctypes

import torch

from ._lib import MGR_IL2D_DENSE, MGR_MAX_BONES, ManusHipError, check, f32c, lib, ptr, stream


class SkinGrid:
    """Skin-weight voxel grid prepared for the kernels: the reference's channel-last (D,H,W,B)
    tensor, uploaded once and zero-padded to 24 channels (96 B per voxel) so that every trilinear
    corner is six aligned float4 loads.

    `version` counts the writes to `data`, and what is derived from the grid (the engine's kept skin weights) is keyed on it."""

    def __init__(self, grid_weights, device=None):
        g = torch.as_tensor(grid_weights, dtype=torch.float32)
        if device is not None:
            g = g.to(device)
        self.D, self.H, self.W, self.B = g.shape
        if self.B > MGR_MAX_BONES:
            raise ManusHipError("skin grid: at most %d transforms" % MGR_MAX_BONES)
        if self.B <= 24:
            self.stride = 24
            p = torch.zeros((self.D, self.H, self.W, 24), dtype=torch.float32, device=g.device)
            p[..., : self.B] = g
            self.data = p.contiguous()
        else:
            self.stride = self.B
            self.data = g.contiguous()
        self._bumps, self._v0 = 0, self.data._version

    @property
    def version(self):
        """Writes to `data` so far: torch's in-place operations on it (counted by the tensor itself) plus the `bump()`s of those
        who wrote it through its device pointer."""
        return self._bumps + self.data._version - self._v0

    def bump(self):
        """`data` was written by a kernel through its pointer (torch does not see such a write)."""
        self._bumps += 1

    def dense(self):
        """The (D,H,W,B) tensor in the reference's layout (a copy without the pad channels): what `checkpoint` stores as
        `grid_weights`."""
        return self.data[..., : self.B].clone(memory_format=torch.contiguous_format)


class SkinGridGrad:
    """Sparse dL/d(grid) of `mgr_skin_grid_bwd`: `voxel` (capacity,) int32 linear indices (z*H + y)*W + x, ascending over the
    first `count[0]` entries; `grad` (capacity, stride) one row per listed voxel, channels >= B zero; `count` (1,) int32 on the
    same device; `shape` = (D,H,W,B).  Entries beyond the count are undefined."""

    def __init__(self, voxel, grad, count, shape):
        self.voxel, self.grad, self.count, self.shape = voxel, grad, count, tuple(int(x) for x in shape)

    def rows(self):
        """(voxel (n,), grad (n, stride)) trimmed to the count (synchronises with the host)."""
        n = int(self.count.reshape(-1)[0])
        return self.voxel[:n], self.grad[:n]

    def to_dense(self):
        """(D,H,W,B): zeros plus the rows."""
        D, H, W, B = self.shape
        v, g = self.rows()
        out = torch.zeros((D * H * W, B), dtype=self.grad.dtype, device=self.grad.device)
        out[v.long()] = g[:, :B]
        return out.reshape(D, H, W, B)


def _skin_grid_grad(N, xyz, sg, center, scale, g_w, index, index_count, max_count, kept=None):
    """`mgr_skin_grid_bwd` on raw list pointers (index None: all N rows).  kept: a dict in which the outputs and the workspace are
    kept from call to call (the engine's: at the bench size they are 230 MB + 100 MB) -- the result then lives until the next call."""
    dev = xyz.device
    nvox = sg.D * sg.H * sg.W
    cap = max(1, min(8 * max_count, nvox))
    nbytes = int(lib().mgr_skin_grid_bwd_workspace_bytes(sg.D, sg.H, sg.W, max_count))
    key = (cap, sg.stride, nbytes, str(dev))
    if kept is not None and kept.get("key") == key:
        voxel, grad, count, ws = kept["bufs"]
    else:
        voxel = torch.empty(cap, dtype=torch.int32, device=dev)
        grad = torch.empty((cap, sg.stride), dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        if kept is not None:
            kept["key"], kept["bufs"] = key, (voxel, grad, count, ws)
    check(lib().mgr_skin_grid_bwd(N, ptr(xyz), ptr(sg.data), sg.D, sg.H, sg.W, sg.B, sg.stride, ptr(center), ptr(scale), ptr(g_w),
                                  index, index_count, max_count, ptr(voxel), ptr(grad), ptr(count), cap, ptr(ws), nbytes, stream()),
          "mgr_skin_grid_bwd")
    return SkinGridGrad(voxel, grad, count, (sg.D, sg.H, sg.W, sg.B))


def skin_grid_grad(xyz, sg, center, scale, g_w, index=None, index_count=None):
    """Sparse dL/d(grid) of `skin_weights(xyz, sg, center, scale)` for dL/dw = g_w (N,B) -> `SkinGridGrad`.  index (int32
    Gaussian indices, entries >= N skipped) + index_count ((1,) int32 on the device, default: the whole list): only those
    Gaussians are processed; the result does not depend on the order of the list.  A Gaussian whose raw sum is zero or not
    finite contributes nothing (include/manus_hip.h).  No reference counterpart (autograd through F.grid_sample there)."""
    if not isinstance(sg, SkinGrid):
        raise ManusHipError("skin_grid_grad takes a SkinGrid")
    xyz, g_w = f32c(xyz), f32c(g_w)
    center, scale = f32c(center).reshape(-1), f32c(scale).reshape(-1)
    N = xyz.shape[0]
    if tuple(g_w.shape) != (N, sg.B):
        raise ManusHipError("skin_grid_grad: g_w must be (N,B) = (%d,%d)" % (N, sg.B))
    if index is None:
        return _skin_grid_grad(N, xyz, sg, center, scale, g_w, None, None, N)
    if index.dtype != torch.int32 or (index_count is not None and index_count.dtype != torch.int32):
        raise ManusHipError("skin_grid_grad: index and index_count must be int32")
    index = index.contiguous()
    if index_count is None:
        index_count = torch.full((1,), index.numel(), dtype=torch.int32, device=index.device)
    return _skin_grid_grad(N, xyz, sg, center, scale, g_w, ptr(index), ptr(index_count), index.numel())


class _SkinWeights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, sg, center, scale, grid_leaf=None):
        # grid_leaf: the caller's (D,H,W,B) tensor when it requires grad (sg was prepared from it), for autograd's bookkeeping
        xyz = f32c(xyz)
        center, scale = f32c(center).reshape(-1), f32c(scale).reshape(-1)
        N = xyz.shape[0]
        w = torch.empty((N, sg.B), dtype=torch.float32, device=xyz.device)
        check(lib().mgr_skin_weights_fwd(N, ptr(xyz), ptr(sg.data), sg.D, sg.H, sg.W, sg.B, sg.stride, ptr(center),
                                         ptr(scale), ptr(w), stream()), "mgr_skin_weights_fwd")
        ctx.save_for_backward(xyz, center, scale)
        ctx.sg = sg
        return w

    @staticmethod
    def backward(ctx, g_w):
        xyz, center, scale = ctx.saved_tensors
        sg = ctx.sg
        N = xyz.shape[0]
        g_w = f32c(g_w)
        g_xyz = torch.empty((N, 3), dtype=torch.float32, device=xyz.device)
        check(lib().mgr_skin_weights_bwd(N, ptr(xyz), ptr(sg.data), sg.D, sg.H, sg.W, sg.B, sg.stride, ptr(center),
                                         ptr(scale), ptr(g_w), ptr(g_xyz), 0, stream()), "mgr_skin_weights_bwd")
        g_grid = None
        if len(ctx.needs_input_grad) > 4 and ctx.needs_input_grad[4]:
            g_grid = _skin_grid_grad(N, xyz, sg, center, scale, g_w, None, None, N).to_dense()
        return (g_xyz, None, None, None, g_grid)[:len(ctx.needs_input_grad)]


def skin_weights(xyz, grid_weights, grid_center, grid_scale):
    """xyz (N,3); grid_weights: a `SkinGrid` (prepared once) or the reference's (D,H,W,B)
    channel-last tensor (prepared on the fly) -> (N,B), rows sum to 1.  A tensor that requires grad receives the dense
    dL/d(grid) (`mgr_skin_grid_bwd`; training on a `SkinGrid` uses the sparse `skin_grid_grad` instead)."""
    leaf = None
    if not isinstance(grid_weights, SkinGrid):
        if not xyz.is_cuda:
            raise ManusHipError("manus_amd ops need GPU tensors; there is no CPU fallback")
        if torch.is_tensor(grid_weights) and grid_weights.requires_grad and torch.is_grad_enabled():
            leaf = grid_weights
        grid_weights = SkinGrid(grid_weights.detach() if torch.is_tensor(grid_weights) else grid_weights, xyz.device)
    if leaf is None:
        return _SkinWeights.apply(xyz, grid_weights, grid_center, grid_scale)
    return _SkinWeights.apply(xyz, grid_weights, grid_center, grid_scale, leaf)


class _LbsCov(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, log_scale, rot, skin_w, transforms, tf44=False):
        xyz, log_scale, rot = f32c(xyz), f32c(log_scale), f32c(rot)
        N = xyz.shape[0]
        if skin_w is not None:
            skin_w = f32c(skin_w)
            t_shape = transforms.shape
            transforms = f32c(transforms)
            if transforms.dim() == 3:
                transforms = transforms[None]
            P, B = transforms.shape[0], transforms.shape[1]
            if skin_w.shape[1] != B:
                raise ManusHipError("lbs_cov: skin weights have %d columns, %d transforms given"
                                    % (skin_w.shape[1], B))  # hand_dynamic.py:104
        else:
            P, B, t_shape = 1, 0, None
        dev = xyz.device
        pxyz = torch.empty((P, N, 3), dtype=torch.float32, device=dev)
        pcov = torch.empty((P, N, 6), dtype=torch.float32, device=dev)
        rows = 16 if tf44 else 12     # (4x4 rows: the reference's (N,4,4) layout written by the kernel, no cat of the constant row)
        tf = torch.empty((P, N, 4, 4) if tf44 else (P, N, 12), dtype=torch.float32, device=dev)
        check(lib().mgr_lbs_cov_fwd_rows(P, N, B, ptr(xyz), ptr(log_scale), ptr(rot), ptr(skin_w), ptr(transforms),
                                         ptr(pxyz), ptr(pcov), ptr(tf), rows, stream()), "mgr_lbs_cov_fwd")
        ctx.save_for_backward(xyz, log_scale, rot, skin_w, transforms)
        ctx.meta = (P, N, B, rows)
        ctx.t_shape = t_shape
        return pxyz, pcov, tf

    @staticmethod
    def backward(ctx, g_xyz, g_cov, g_tf):
        xyz, log_scale, rot, skin_w, transforms = ctx.saved_tensors
        P, N, B, rows = ctx.meta
        dev = xyz.device
        g_xyz = f32c(g_xyz) if g_xyz is not None else torch.zeros((P, N, 3), dtype=torch.float32, device=dev)
        g_cov = f32c(g_cov) if g_cov is not None else torch.zeros((P, N, 6), dtype=torch.float32, device=dev)
        g_tf = f32c(g_tf) if g_tf is not None else None
        d_xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
        d_ls = torch.empty((N, 3), dtype=torch.float32, device=dev)
        d_rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
        d_w = torch.empty((N, B), dtype=torch.float32, device=dev) if skin_w is not None else None
        check(lib().mgr_lbs_cov_bwd_rows(P, N, B, ptr(xyz), ptr(log_scale), ptr(rot), ptr(skin_w), ptr(transforms),
                                         ptr(g_xyz), ptr(g_cov), ptr(g_tf), rows, ptr(d_xyz), ptr(d_ls), ptr(d_rot),
                                         ptr(d_w), stream()), "mgr_lbs_cov_bwd")
        d_t = None
        if ctx.needs_input_grad[4] and skin_w is not None:      # the pose gradient (no reference counterpart): two more launches
            d_t = torch.empty((P, B, 4, 4), dtype=torch.float32, device=dev)
            nbytes = int(lib().mgr_lbs_pose_workspace_bytes(P, N, B))
            ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
            check(lib().mgr_lbs_pose_bwd(P, N, B, ptr(xyz), ptr(log_scale), ptr(rot), ptr(skin_w), ptr(transforms), ptr(g_xyz),
                                         ptr(g_cov), ptr(g_tf), rows, ptr(d_t), ptr(ws), nbytes, stream()), "mgr_lbs_pose_bwd")
            d_t = d_t.reshape(ctx.t_shape)
        return d_xyz, d_ls, d_rot, d_w, d_t, None


def lbs_cov(xyz, log_scale, rot, skin_w, transforms, tf44=False):
    """Skin means and covariances for P poses.

    xyz (N,3), log_scale (N,3) (`_scaling`), rot (N,4) raw (`_rotation`),
    skin_w (N,B) or None (static object: identity transform),
    transforms (P,B,4,4) / (B,4,4) = posed @ inv(rest) (+ identity background); differentiable (`mgr_lbs_pose_bwd`:
    the gradient has the shape of `transforms`, its rows 3 are zero).
    Returns posed_xyz (P,N,3), posed_cov (P,N,6), tf (P,N,12) (rows 0..2 of the
    blended 4x4) -- or, with tf44, (P,N,4,4): the reference's layout, constant last row included, written by the kernel."""
    return _LbsCov.apply(xyz, log_scale, rot, skin_w, transforms, bool(tf44))


class _ShColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sh, xyz, tf, cams):
        sh, xyz = f32c(sh), f32c(xyz)
        N = sh.shape[0]
        V = cams.shape[0]
        if sh.shape[1:] != (16, 3):
            raise ManusHipError("sh_colors: features must be (N,16,3) (sh_degree 3)")
        s_xyz = xyz.stride(0) if xyz.dim() == 3 else 0
        s_tf, rows, tf_per_view = 0, 12, False
        if tf is not None:
            tf = f32c(tf)
            if tf.dim() >= 3 and tuple(tf.shape[-2:]) == (4, 4):      # (N,4,4) / (V,N,4,4): the reference's layout, read in place
                rows, tf_per_view = 16, tf.dim() == 4
            else:                                                     # (N,12) / (V,N,12)
                tf_per_view = tf.dim() == 3
            s_tf = tf.stride(0) if tf_per_view else 0
        col = torch.empty((V, N, 3), dtype=torch.float32, device=sh.device)
        check(lib().mgr_sh_color_fwd_rows(V, N, ptr(sh), ptr(xyz), s_xyz, ptr(tf), s_tf, rows, ptr(cams), ptr(col),
                                          stream()), "mgr_sh_color_fwd")
        ctx.save_for_backward(sh, xyz, tf, cams)
        ctx.meta = (V, N, s_xyz, s_tf, rows, tf_per_view)
        return col

    @staticmethod
    def backward(ctx, g_col):
        sh, xyz, tf, cams = ctx.saved_tensors
        V, N, s_xyz, s_tf, rows, tf_per_view = ctx.meta
        dev = sh.device
        g_col = f32c(g_col)
        d_sh = torch.empty((N, 16, 3), dtype=torch.float32, device=dev)
        d_xyz = torch.empty((V, N, 3), dtype=torch.float32, device=dev)
        d_tf = torch.empty((V, N, 4, 4) if rows == 16 else (V, N, 12), dtype=torch.float32, device=dev) if tf is not None else None
        check(lib().mgr_sh_color_bwd_rows(V, N, ptr(sh), ptr(xyz), s_xyz, ptr(tf), s_tf, rows, ptr(cams), ptr(g_col),
                                          ptr(d_sh), ptr(d_xyz), ptr(d_tf), stream()), "mgr_sh_color_bwd")
        g_xyz = d_xyz if xyz.dim() == 3 else (d_xyz.sum(0) if V > 1 else d_xyz[0])
        g_tf = None
        if tf is not None:
            g_tf = d_tf if tf_per_view else (d_tf.sum(0) if V > 1 else d_tf[0])
        return d_sh, g_xyz, g_tf, None


def sh_colors(features, xyz, tf, cams):
    """Degree-3 SH colour for V views: features (N,16,3); xyz (N,3) or (V,N,3)
    (canonical means when tf is given, posed means otherwise); tf (N,12)/(V,N,12)
    or None; cams (V,40).  Returns (V,N,3) = max(sh2rgb + 0.5, 0)."""
    return _ShColors.apply(features, xyz, tf, cams)


def project_points(points, K, extrin):
    """points (B,N,3) or (N,3); K (3,3); extrin (3,4) -> (...,N,2)."""
    p = f32c(points)
    shape = p.shape
    flat = p.reshape(-1, 3)
    K, E = f32c(K).reshape(-1)[:9].contiguous(), f32c(extrin).reshape(-1)[:12].contiguous()
    uv = torch.empty((flat.shape[0], 2), dtype=torch.float32, device=p.device)
    check(lib().mgr_project_points(flat.shape[0], ptr(flat), ptr(K), ptr(E), ptr(uv), stream()),
          "mgr_project_points")
    return uv.reshape(shape[:-1] + (2,))


def distCUDA2(points):
    """Mean squared distance to the 3 nearest other points, (N,3) -> (N,)."""
    p = f32c(points)
    N = p.shape[0]
    out = torch.empty((N,), dtype=torch.float32, device=p.device)
    nbytes = int(lib().mgr_knn3_workspace_bytes(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    check(lib().mgr_knn3_mean_dist2(N, ptr(p), ptr(out), ptr(ws), nbytes, stream()), "mgr_knn3_mean_dist2")
    return out


def l1_loss_grad(pred, target, scale=None):
    """sum|pred-target| (device scalar) and d(mean|pred-target|)/dpred * weight.
    `scale` defaults to 1/numel (the reference's torch.mean of the L1 map)."""
    pred, target = f32c(pred), f32c(target)
    n = pred.numel()
    if scale is None:
        scale = 1.0 / n
    g = torch.empty_like(pred)
    s = torch.zeros(1, dtype=torch.float32, device=pred.device)
    check(lib().mgr_l1_loss_grad(n, ptr(pred), ptr(target), float(scale), ptr(g), ptr(s), stream()),
          "mgr_l1_loss_grad")
    return s, g


def map_loss_grad(alpha, mask, w_mask=1.0, depth=None, depth_target=None, w_depth=0.0, grad_scale=1.0):
    """Silhouette and depth terms on (V,H,W) maps of the feature render (mgr_map_loss), value and gradient in one pass:
    L_mask = mean|alpha - mask|, L_depth = mean(mask |depth - depth_target|) (off without `depth`).  Returns (sums, dL_dalpha,
    dL_ddepth or None): sums = [L_mask, L_depth, w_mask L_mask + w_depth L_depth] (device tensor of 3 floats, without
    grad_scale); the gradients are those of grad_scale * sums[2]."""
    alpha, mask = f32c(alpha), f32c(mask)
    if alpha.dim() != 3 or mask.shape != alpha.shape:
        raise ManusHipError("map_loss: alpha and mask must be (V,H,W) maps of one shape (got %s, %s)" % (tuple(alpha.shape), tuple(mask.shape)))
    if (depth is None) != (depth_target is None):
        raise ManusHipError("map_loss: the depth term takes depth and depth_target together")
    V, H, W = alpha.shape
    g_d = None
    if depth is not None:
        depth, depth_target = f32c(depth), f32c(depth_target)
        if depth.shape != alpha.shape or depth_target.shape != alpha.shape:
            raise ManusHipError("map_loss: depth and depth_target must have the shape of alpha")
        g_d = torch.empty_like(depth)
    g_a = torch.empty_like(alpha)
    sums = torch.empty(3, dtype=torch.float32, device=alpha.device)
    nbytes = int(lib().mgr_map_loss_workspace_bytes(V, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=alpha.device)
    check(lib().mgr_map_loss(V, H, W, ptr(alpha), ptr(mask), ptr(depth), ptr(depth_target), float(w_mask), float(w_depth),
                             float(grad_scale), ptr(g_a), ptr(g_d), ptr(sums), ptr(ws), nbytes, stream()), "mgr_map_loss")
    return sums, g_a, g_d


def exposure_block():
    """Pixels per workgroup of the exposure kernels (`mgr_exposure_block`)."""
    return int(lib().mgr_exposure_block())


def _exposure_args(img, E, cam_of_view, what):
    """(V, H, W, C, cam_of_view as a device int32 vector) of an exposure call; ManusHipError for anything else."""
    for t in (img, E):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ManusHipError("%s needs GPU tensors; there is no CPU fallback" % what)
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32:
        raise ManusHipError("%s: the image must be (V,3,H,W) fp32 (got %s %s)" % (what, tuple(img.shape), img.dtype))
    if E.dim() != 3 or tuple(E.shape[1:]) != (3, 4) or E.dtype != torch.float32 or E.device != img.device:
        raise ManusHipError("%s: the table must be (C,3,4) fp32 on the image's device (got %s %s)" % (what, tuple(E.shape), E.dtype))
    V = img.shape[0]
    if not torch.is_tensor(cam_of_view):
        cam_of_view = torch.tensor([int(c) for c in cam_of_view], dtype=torch.int32, device=img.device)
    if cam_of_view.dtype != torch.int32 or tuple(cam_of_view.shape) != (V,) or cam_of_view.device != img.device:
        raise ManusHipError("%s: cam_of_view must be %d int32 entries on the image's device" % (what, V))
    return V, img.shape[2], img.shape[3], E.shape[0], cam_of_view.contiguous()


def exposure_forward(img, E, cam_of_view):
    """out'[k] = A[r] img[k] + b[r] per pixel, r = cam_of_view[k], A = E[:,:,:3], b = E[:,:,3] (`mgr_exposure_apply`); a row
    outside [0,C) copies the view.  No autograd: `exposure_apply` is the differentiable form."""
    V, H, W, C, cov = _exposure_args(img, E, cam_of_view, "exposure_apply")
    img, E = img.contiguous(), E.contiguous()
    out = torch.empty_like(img)
    check(lib().mgr_exposure_apply(V, H, W, C, ptr(cov), ptr(E), ptr(img), ptr(out), stream()), "mgr_exposure_apply")
    return out


def exposure_backward(img, E, cam_of_view, g, inplace=False, workspace=None):
    """The raw backward (`mgr_exposure_backward`): (dL/dimg, dE) from g = dL/dout' (V,3,H,W).  dE is (V,3,4) BY POSITION: the
    rows of views that share a camera are summed by whoever consumes them (`mgr_exposure_adam`, `exposure_apply`'s backward).
    inplace: dL/dimg overwrites g (same bits).  Deterministic: two calls give equal bits."""
    V, H, W, C, cov = _exposure_args(img, E, cam_of_view, "exposure_backward")
    if not torch.is_tensor(g) or g.shape != img.shape or g.dtype != torch.float32 or g.device != img.device:
        raise ManusHipError("exposure_backward: the gradient must have the image's shape, dtype and device")
    img, E = img.contiguous(), E.contiguous()
    if inplace and not g.is_contiguous():
        raise ManusHipError("exposure_backward: an in-place gradient must be contiguous")
    g = g.contiguous()
    g_out = g if inplace else torch.empty_like(g)
    dE = torch.empty((V, 3, 4), dtype=torch.float32, device=img.device)
    nbytes = int(lib().mgr_exposure_workspace_bytes(V, H, W))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    check(lib().mgr_exposure_backward(V, H, W, C, ptr(cov), ptr(E), ptr(img), ptr(g), ptr(g_out), ptr(dE), ptr(workspace),
                                      workspace.numel(), stream()), "mgr_exposure_backward")
    return g_out, dE


class _ExposureApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, E, cov):
        ctx.save_for_backward(img, E, cov)
        return exposure_forward(img, E, cov)

    @staticmethod
    def backward(ctx, g):
        img, E, cov = ctx.saved_tensors
        g_img, dE = exposure_backward(img, E, cov, g.contiguous())
        # the dense table gradient: the per-view rows added in ascending position (index_add_ over sorted positions is not
        # ordered, a loop over the views is)
        d_tab = torch.zeros_like(E)
        rows = cov.tolist()
        for k, r in enumerate(rows):
            if 0 <= r < E.shape[0]:
                d_tab[r] += dE[k]
        return g_img, d_tab, None


def exposure_apply(img, E, cam_of_view):
    """Per-camera affine colour correction under autograd: out' as `exposure_forward`, gradients to `img` and to the table `E`
    (dense (C,3,4), the per-view rows of `exposure_backward` summed per camera in ascending position)."""
    V, H, W, C, cov = _exposure_args(img, E, cam_of_view, "exposure_apply")
    return _ExposureApply.apply(img, E, cov)


def image_loss_grad(pred, target, w_l1=0.8, w_ssim=0.2, grad_scale=1.0, loss_offset=0.0, bg=None, tile_start_ptr=None):
    """Fused L1 + SSIM image loss of the training step (loss_utils.py:22-97 as called at
    base.py:323-365), forward and backward, on (V,3,H,W) images.

    Returns (sums, grad): sums[0] = sum|pred-target|, sums[1] = sum of the SSIM map, sums[2] =
    grad_scale * (w_l1 * sums[0] - w_ssim * sums[1]) + loss_offset (device tensor of 3 floats); grad = grad_scale * d/dpred [w_l1 * sum|pred-target| - w_ssim * sum ssim_map].
    The SSIM statistic is the reference's: ssim() called on HWC images, i.e. the 11x11 window
    slides over the (W,3) plane of every row.

    bg (3 floats on the device) + tile_start_ptr (device address of the tile-list offsets of the forward that rendered
    `pred`): `mgr_image_loss_tiles` -- spans under empty tiles are settled from the target alone and their gradient is
    left unwritten (nothing reads it); the sums are the same."""
    pred, target = f32c(pred), f32c(target)
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if pred.shape != target.shape or pred.shape[1] != 3:
        raise ManusHipError("image_loss_grad: pred and target must both be (V,3,H,W)")
    V, _, H, W = pred.shape
    g = torch.empty_like(pred)
    sums = torch.empty(3, dtype=torch.float32, device=pred.device)
    nbytes = int(lib().mgr_image_loss_workspace_bytes(V, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    if tile_start_ptr is not None and bg is not None:
        check(lib().mgr_image_loss_tiles(V, H, W, ptr(pred), ptr(target), ptr(f32c(bg)), ctypes.c_void_p(int(tile_start_ptr)),
                                         float(w_l1), float(w_ssim), float(grad_scale), float(loss_offset), ptr(g), ptr(sums),
                                         ptr(ws), nbytes, stream()), "mgr_image_loss_tiles")
        return sums, g
    check(lib().mgr_image_loss(V, H, W, ptr(pred), ptr(target), float(w_l1), float(w_ssim), float(grad_scale),
                               float(loss_offset), ptr(g), ptr(sums), ptr(ws), nbytes, stream()), "mgr_image_loss")
    return sums, g


def image_loss2d_block():
    """(block_w, block_h) of `mgr_image_loss2d`: the pixel blocks it settles or lists."""
    word = int(lib().mgr_image_loss2d_block())
    return word >> 16, word & 0xFFFF


def image_loss2d_grad(pred, target, w_l1=0.8, w_ssim=0.2, grad_scale=1.0, loss_offset=0.0, mask=None, need_grad=True, dense=False):
    """Fused L1 + SPATIAL SSIM image loss (`mgr_image_loss2d`), forward and backward, on (V,3,H,W) images: the standard
    SSIM -- an 11x11 Gaussian window (sigma 1.5) over H x W of every colour channel separately, zero padding 5 -- where
    `image_loss_grad` is the reference's statistic on HWC images.  mask (V,H,W), possibly fractional: both images are
    multiplied by it at load.

    Returns (sums, view_sums, grad or None): sums[0] = sum|x - y|, sums[1] = sum of the SSIM map, sums[2] = grad_scale *
    (w_l1 * sums[0] - w_ssim * sums[1]) + loss_offset (device tensor of 3 floats); view_sums (V,2): the two sums of every view;
    grad = d sums[2] / d pred (need_grad=False: None, the same sums).  Blocks of `image_loss2d_block()` pixels whose 10 px
    surroundings hold no difference are settled without the heavy kernel (sum S += their values, gradient 0); dense=True runs
    every block.  Deterministic: two calls give the same bits.  GPU tensors only."""
    for t in (pred, target, mask):
        if t is not None and not t.is_cuda:
            raise ManusHipError("image_loss2d_grad needs GPU tensors (got %s); there is no CPU fallback" % t.device)
    pred, target = f32c(pred), f32c(target)
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if pred.dim() != 4 or pred.shape != target.shape or pred.shape[1] != 3:
        raise ManusHipError("image_loss2d_grad: pred and target must both be (V,3,H,W)")
    V, _, H, W = pred.shape
    if mask is not None:
        mask = f32c(mask)
        if mask.dim() == 2:
            mask = mask[None]
        if tuple(mask.shape) != (V, H, W):
            raise ManusHipError("image_loss2d_grad: mask must be (V,H,W)")
    dev = pred.device
    g = torch.empty_like(pred) if need_grad else None
    sums = torch.empty(3, dtype=torch.float32, device=dev)
    view_sums = torch.empty((V, 2), dtype=torch.float32, device=dev)
    nbytes = int(lib().mgr_image_loss2d_workspace_bytes(V, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().mgr_image_loss2d(V, H, W, ptr(pred), ptr(target), ptr(mask), float(w_l1), float(w_ssim), float(grad_scale),
                                 float(loss_offset), ptr(g), ptr(sums), ptr(view_sums), MGR_IL2D_DENSE if dense else 0, ptr(ws), nbytes,
                                 stream()), "mgr_image_loss2d")
    return sums, view_sums, g


def isotropic_reg_grad(log_scale, condition_number=0.4, weight=1.0, grad_out=None):
    """weight * mean((min s / (max s + 1e-8) - condition_number)^2), s = exp(log_scale), and its gradient
    w.r.t. log_scale (base.py:349-356).  grad_out: optional (N,3) tensor to ADD the gradient to.
    Returns (loss (1,), gradient tensor)."""
    ls = f32c(log_scale)
    N = ls.shape[0]
    acc = grad_out is not None
    g = grad_out if acc else torch.empty_like(ls)
    if acc and (g.dtype != torch.float32 or not g.is_contiguous() or g.shape != ls.shape):
        raise ManusHipError("isotropic_reg_grad: grad_out must be a contiguous fp32 (N,3) tensor")
    loss = torch.empty(1, dtype=torch.float32, device=ls.device)
    nbytes = int(lib().mgr_isotropic_reg_workspace_bytes(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ls.device)
    check(lib().mgr_isotropic_reg(N, ptr(ls), float(condition_number), float(weight), ptr(g), 1 if acc else 0, ptr(loss),
                                  ptr(ws), nbytes, stream()), "mgr_isotropic_reg")
    return loss, g


def _eval_images(name, pred, target):
    for t in (pred, target):
        if not t.is_cuda:
            raise ManusHipError("%s needs GPU tensors (got %s); there is no CPU fallback" % (name, t.device))
    pred, target = f32c(pred), f32c(target)
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if pred.dim() != 4 or pred.shape != target.shape or pred.shape[1] != 3:
        raise ManusHipError("%s: pred and target must both be (V,3,H,W)" % name)
    return pred, target


def eval_views(pred, target, mask=None, flags=False):
    """Validation metrics of V views in one launch chain (`mgr_eval_views`; base.py:138-147, loss_utils.py:100-108),
    forward only.  pred, target (V,3,H,W); mask (V,H,W), possibly fractional, None = ones.

    Returns (sq_sum, ssim_sum, gt_max), each (V,) fp32 on the device: sq_sum[v] = sum (pred*mask - target*mask)^2 over the
    3*H*W elements (psnr = -10 log10(sq_sum / (3*H*W))), ssim_sum[v] = sum of the reference's HWC SSIM map of the two
    masked images (ssim = ssim_sum / (3*H*W)), gt_max[v] = max of the unmasked target (for `eval_triptych`).  A view whose
    inputs hold a NaN or Inf reports NaN for both sums, the other views are not affected; flags=True appends the (V,)
    int32 flags of those views.  Deterministic: two calls give the same bits."""
    pred, target = _eval_images("eval_views", pred, target)
    V, _, H, W = pred.shape
    if mask is not None:
        if not mask.is_cuda:
            raise ManusHipError("eval_views needs GPU tensors (got %s); there is no CPU fallback" % mask.device)
        mask = f32c(mask)
        if mask.dim() == 2:
            mask = mask[None]
        if tuple(mask.shape) != (V, H, W):
            raise ManusHipError("eval_views: mask must be (V,H,W)")
    dev = pred.device
    out = torch.empty((3, V), dtype=torch.float32, device=dev)
    fl = torch.empty(V, dtype=torch.int32, device=dev)
    nbytes = int(lib().mgr_eval_workspace_bytes(V, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().mgr_eval_views(V, H, W, ptr(pred), ptr(target), ptr(mask), out[0].data_ptr(), out[1].data_ptr(),
                               out[2].data_ptr(), fl.data_ptr(), ptr(ws), nbytes, stream()), "mgr_eval_views")
    return (out[0], out[1], out[2], fl) if flags else (out[0], out[1], out[2])


_DIFF_TABLES = {}     # device -> the 256x256 difference table (validation.diff_table) on that device


def eval_triptych(pred, target, gt_max):
    """render | ground truth | difference of V views as (V,3H,W,3) uint8 (`mgr_eval_triptych`; base.py:116-128): the
    three HWC panels stacked along the rows.  gt_max (V,): the third output of `eval_views` (dump_image scales the
    ground truth by 255 when its maximum is <= 1).  A NaN pixel is written as 0 -- this package's definition, numpy
    leaves that cast undefined."""
    pred, target = _eval_images("eval_triptych", pred, target)
    if not gt_max.is_cuda:
        raise ManusHipError("eval_triptych needs GPU tensors (got %s); there is no CPU fallback" % gt_max.device)
    V, _, H, W = pred.shape
    gt_max = f32c(gt_max).reshape(-1)
    if gt_max.numel() != V:
        raise ManusHipError("eval_triptych: gt_max must hold one value per view")
    dev = pred.device
    tab = _DIFF_TABLES.get(dev)
    if tab is None:
        from .validation import diff_table
        tab = _DIFF_TABLES[dev] = torch.from_numpy(diff_table()).to(dev).contiguous()
    out = torch.empty((V, 3 * H, W, 3), dtype=torch.uint8, device=dev)
    check(lib().mgr_eval_triptych(V, H, W, ptr(pred), ptr(target), ptr(gt_max), ptr(tab), ptr(out), stream()),
          "mgr_eval_triptych")
    return out

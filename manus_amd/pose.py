"""Pose refinement on top of the pose gradient (`HipViewCompute(pose_grad=True)`, `ops.lbs_cov` with a differentiable
`transforms`): a per-frame, per-bone correction of the posed bone matrices and the chain rule from dL/d(bone transforms) back
to them.  Plain host torch on B small matrices.

No reference counterpart: the reference's config/model/pose_optimizer.yaml names `src.models.pose_optimizer`, which was
never released.  `Trainer` does not schedule pose refinement; a caller drives it (tests/test_gpu_pose_grad.py)."""
import torch


def _exp_so3(r):
    """Rodrigues: (...,3) rotation vectors -> (...,3,3).  The exact identity at r = 0, differentiable there (series below
    |r|^2 = 1e-6, where they are exact to fp32 rounding)."""
    t2 = (r * r).sum(-1)
    small = t2 < 1e-6
    t2s = torch.where(small, torch.ones_like(t2), t2)
    th = torch.sqrt(t2s)
    a = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(th)) / t2s)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(r.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=r.dtype, device=r.device)
    return eye + a[..., None, None] * K + b[..., None, None] * (K @ K)


class PoseCorrection(torch.nn.Module):
    """rotvec (F,B,3) and trans (F,B,3), zero-initialised: frame f, bone b is corrected in the bone's local frame,
    posed_b @ [[exp(rotvec_b), trans_b], [0, 0, 0, 1]] -- the identity (bit for bit) at zero."""

    def __init__(self, n_frames, n_bones, dtype=torch.float32, device=None):
        super().__init__()
        self.rotvec = torch.nn.Parameter(torch.zeros((n_frames, n_bones, 3), dtype=dtype, device=device))
        self.trans = torch.nn.Parameter(torch.zeros((n_frames, n_bones, 3), dtype=dtype, device=device))

    def forward(self, posed, frame):
        """posed (B,4,4) of frame `frame` -> corrected (B,4,4)."""
        rv, tr = self.rotvec[frame], self.trans[frame]
        top = torch.cat([_exp_so3(rv), tr[..., None]], -1)                             # (B,3,4)
        last = torch.zeros((rv.shape[0], 1, 4), dtype=rv.dtype, device=rv.device)
        last[..., 3] = 1.0
        return posed @ torch.cat([top, last], -2).to(posed.dtype)


def pose_backward(d_transforms, posed, rest, background=True):
    """dL/dposed from dL/dT of T_b = posed_b @ inv(rest_b) (`transforms.bone_transforms`): d_posed_b = dT_b @ inv(rest_b)^T.
    d_transforms (...,B[+1],4,4) -- with `background` the last row is the identity transform's and is dropped; posed
    (...,B,4,4) gives the shape and dtype of the result, rest is (B,4,4).  A caller of the fused step, which has no autograd
    graph, finishes the chain with `corrected.backward(pose_backward(out["d_transforms"][k], corrected, rest))`."""
    dT = d_transforms[..., :-1, :, :] if background else d_transforms
    if dT.shape[-3:] != posed.shape[-3:]:
        raise ValueError("pose_backward: %s transforms for %s posed matrices" % (tuple(dT.shape), tuple(posed.shape)))
    inv_t = torch.linalg.inv(rest.to(device=dT.device, dtype=posed.dtype)).transpose(-1, -2)
    return dT.to(posed.dtype) @ inv_t

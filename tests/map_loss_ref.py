"""fp64 restatement of the map loss (mgr_map_loss, losses.map_loss), in torch, for the tests.

    L_mask  = mean over V H W of |alpha - mask|
    L_depth = mean over V H W of mask |depth - depth_target|
    total   = w_mask L_mask + w_depth L_depth            gradients: those of grad_scale * total, 0 at the kinks
"""
import numpy as np
import torch


def map_loss_ref(alpha, mask, depth=None, depth_target=None, w_mask=1.0, w_depth=0.0, grad_scale=1.0):
    """-> dict(L_mask, L_depth, total, g_alpha, g_depth) in fp64 (g_depth None without the depth term)."""
    a, m = alpha.double(), mask.double()
    n = a.numel()
    d = a - m
    out = dict(L_mask=d.abs().sum() / n, L_depth=torch.zeros((), dtype=torch.float64), g_depth=None)
    out["g_alpha"] = (grad_scale * w_mask / n) * torch.sign(d)
    if depth is not None:
        dd = depth.double() - depth_target.double()
        out["L_depth"] = (m * dd.abs()).sum() / n
        out["g_depth"] = (grad_scale * w_depth / n) * m * torch.sign(dd)
    else:
        w_depth = 0.0
    out["total"] = w_mask * out["L_mask"] + w_depth * out["L_depth"]
    return out


def map_loss_grads_fp32(alpha, mask, depth=None, depth_target=None, w_mask=1.0, w_depth=0.0, grad_scale=1.0):
    """The kernel's gradient formula in fp32, operation for operation: the factor grad_scale * w / n is formed in fp64 from the
    fp32 arguments and rounded to fp32 once; an element is that factor (times its mask) times the sign of its difference."""
    n = alpha.numel()
    f32 = lambda x: float(np.float32(x))
    ca = np.float32(f32(grad_scale) * f32(w_mask) / n)
    g_a = torch.sign(alpha - mask) * float(ca)
    g_d = None
    if depth is not None:
        cd = np.float32(f32(grad_scale) * f32(w_depth) / n)
        g_d = (mask * float(cd)) * torch.sign(depth - depth_target)
    return g_a, g_d


def term_sums_fp64(alpha, mask, depth=None, depth_target=None):
    """fp64 means of the FP32 terms |alpha - mask| and mask |depth - depth_target| (what an exact accumulation returns)."""
    n = alpha.numel()
    lm = (alpha - mask).abs().double().sum() / n
    ld = (mask * (depth - depth_target).abs()).double().sum() / n if depth is not None else torch.zeros((), dtype=torch.float64)
    return lm, ld

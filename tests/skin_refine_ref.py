"""The skin-grid refinement step (`mgr_skin_grid_refine`, `optim.SkinGridRefiner`) restated in torch on the CPU, in fp64 and
fp32: the prior's gradient on the listed rows, `torch.optim.SparseAdam`, the clamp on the stepped rows, the projection of those
rows onto sum 1 under the min_sum rule, and the prior's value on the grid before the step.  Shared by
tests/test_skin_refine_cpu.py and tests/test_gpu_skin_refine.py; no GPU, no manus_amd import.

The recovery loop is that of tests/test_gpu_skin_grid_grad.py (`recovery_reference`: 150 steps, lr 0.01, clamp at 0) with the
projection and the prior added."""
import torch

from oracle import torch_ref as tr

import test_gpu_skin_grid_grad as G

F32, F64 = torch.float32, torch.float64


def prior_value(x, x0, weight):
    """weight * sum d^2 with d = x - x0 formed in the tensors' own precision and squared and added in fp64."""
    d = (x - x0).double()
    return float(weight) * float((d * d).sum())


def prior_grad(x, x0, weight):
    """d/dx of `prior_value`: w2 * d with w2 = 2 * weight rounded once to the tensors' precision."""
    return torch.tensor(2.0 * float(weight), dtype=x.dtype) * (x - x0)


def project_rows(x, min_sum):
    """Rows whose sum exceeds min_sum (false for a NaN sum) divided by it; every other row as it is.  No NaN is created."""
    S = x.sum(1, keepdim=True)
    return torch.where(S > min_sum, x / torch.where(S > min_sum, S, torch.ones_like(S)), x)


def refine_chain(grid, sets, grads, dtype, lr=0.01, betas=(0.9, 0.999), eps=1e-8, clamp_min=0.0, prior_weight=0.0, project=True,
                 min_sum=1e-12, grid0=None):
    """`grid` (V,B); per step a list of rows `sets[k]` (strictly ascending) and their loss gradient `grads[k]`.
    -> (grid, exp_avg, exp_avg_sq, [prior value per step]) in `dtype`."""
    p = grid.to(dtype).clone().requires_grad_(True)
    p0 = (grid if grid0 is None else grid0).to(dtype).clone()
    opt = torch.optim.SparseAdam([p], lr=lr, betas=betas, eps=eps)
    values = []
    for v, g in zip(sets, grads):
        g = g.to(dtype)
        with torch.no_grad():
            if prior_weight != 0:
                values.append(prior_value(p[v], p0[v], prior_weight))
                g = g + prior_grad(p[v], p0[v], prior_weight)
            else:
                values.append(0.0)
        p.grad = torch.sparse_coo_tensor(v[None], g, p.shape)
        opt.step()
        with torch.no_grad():      # clamp and projection follow the step on the rows it stepped, nowhere else
            x = p[v]
            if clamp_min is not None:
                x = x.clamp(min=clamp_min)
            if project:
                x = project_rows(x, min_sum)
            p[v] = x
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], values


_REC = {}


def recovery_reference(prior_weight=0.0, project=True):
    """The recovery loop of tests/test_gpu_skin_grid_grad.py in fp64 with the refinement's extras: rho = final / initial loss,
    dist = ||grid - start||, the range of the touched rows' sums, the number of touched rows."""
    key = (float(prior_weight), bool(project))
    if key in _REC:
        return _REC[key]
    inp = G.recovery_inputs()
    xyz, c, s, T = inp["xyz"], inp["center"], inp["scale"], inp["T"]
    target = G._posed_means(xyz, tr.skin_weights_from_grid(xyz, c, s, inp["true"]), T)
    start = inp["start"].reshape(-1, 21)
    p = start.clone().requires_grad_(True)
    opt = torch.optim.SparseAdam([p], lr=G.REC_LR)
    losses, touched = [], torch.zeros(p.shape[0], dtype=torch.bool)
    for _ in range(G.REC_STEPS + 1):
        p.grad = None
        loss = ((G._posed_means(xyz, tr.skin_weights_from_grid(xyz, c, s, p.reshape(8, 8, 8, 21)), T) - target) ** 2).sum()
        losses.append(float(loss.detach()))
        if len(losses) == G.REC_STEPS + 1:
            break
        loss.backward()
        rows = torch.nonzero(p.grad.abs().sum(1) > 0).reshape(-1)
        touched[rows] = True
        g = p.grad[rows]
        if prior_weight != 0:
            g = g + prior_grad(p.detach()[rows], start[rows], prior_weight)
        p.grad = torch.sparse_coo_tensor(rows[None], g, p.shape)
        opt.step()
        with torch.no_grad():
            x = p[rows].clamp(min=0.0)
            p[rows] = project_rows(x, 1e-12) if project else x
    sums = p.detach()[touched].sum(1)
    _REC[key] = dict(inp=inp, target=target, rho_ref=losses[-1] / losses[0], loss0=losses[0], dist=float((p.detach() - start).norm()),
                     sum_min=float(sums.min()), sum_max=float(sums.max()), touched=int(touched.sum()))
    return _REC[key]

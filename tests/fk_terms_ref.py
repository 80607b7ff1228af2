"""The checker of the terms on the kinematic refiner's angles (mgr_fk_backward_terms, csrc/fk.hip; manus_amd.pose.KinematicPoseRefiner
with w_dev_* / w_smooth_* / w_kp): the deviation, smoothness and 3-D keypoint terms as host torch on top of `fk_chain_ref.fk` in a
given dtype on the CPU under autograd, with the count-once rule of the values on a list of rows and the skip rule c > 0 of the
keypoints; the committed inputs of the tests, derived from `fk_chain_ref.chain_inputs`; and the Adam loop of the descent and
recovery tests.

    E_dev    = sum_f sum_{mask != 0} w_dev(r)    (theta_f - theta_ref_f)^2
    E_smooth = sum_{edges (f, next f)} sum_{mask != 0} w_smooth(r) (theta_f - theta_next)^2
    E_kp     = w_kp sum_f sum_k c[f,k] |(M_bone[k](theta_f) [o_k; 1])[:3] - y[f,k]|^2

Tolerance of the GPU tests that use it: `check_rows`, e_kernel <= 8 * max(e32, 2^-23) per (frame, row) against this restatement in
fp64, e32 the error of the same restatement in fp32 (test_fk_terms_cpu.py keeps e32 <= 1e-4 on every case)."""
import numpy as np
import torch

import fk_chain_ref as R
from fk_chain_ref import F32, F64, rounded

FRAME_KEYS = [("a", 0), ("a", 1), ("a", 2), ("a", 3), ("b", 0), ("b", 1)]       # F = 6 in two takes of 4 + 2
WEIGHTS = dict(w_dev_rot=0.5, w_smooth_rot=0.25, w_dev_trans=2.0, w_smooth_trans=1.0, w_kp=10.0)
NAMES = tuple(WEIGHTS)
ZERO = dict.fromkeys(NAMES, 0.0)
COMBOS = {"all": dict(WEIGHTS), "dev": dict(ZERO, w_dev_rot=0.5, w_dev_trans=2.0), "smooth": dict(ZERO, w_smooth_rot=0.25, w_smooth_trans=1.0),
          "kp": dict(ZERO, w_kp=10.0)}
# LISTED (2: listed and unviewed), one interior row of take a, a first, a last, two adjacent
LISTS = {"listed": list(R.LISTED), "interior": [2], "first": [0], "last": [3], "adjacent": [1, 2]}
FINGERTIPS = (4, 8, 12, 16, 20)                  # the tails of bones 3, 7, 11, 15, 19 in the dataset's keypoint convention


def neighbours(frame_keys=FRAME_KEYS):
    from manus_amd.pose import neighbour_table
    return neighbour_table(frame_keys)


def keypoint_bones(case, J):
    """one: K = 1; chain4: two keypoints on bone 1 and none on bone 2; hand / fan: the dataset's convention [0, 0, 1, .., J-1];
    chain_max: K = 64, two per bone."""
    if case == "one":
        return [0]
    if case == "chain4":
        return [0, 1, 1, 3]
    if case == "chain_max":
        return [k // 2 for k in range(64)]
    return [0] + list(range(J))


def terms_inputs(case, seed=0):
    """`chain_inputs(case)` plus the terms' tables, fp32-representable fp64: theta_ref = theta + 0.3 uniform(+-1); keypoint bones
    (`keypoint_bones`), offsets 0.05 N(0,1), weights c uniform in [0.5, 1.5] (the hand's fingertips 2), targets = the FK keypoints
    at theta + 0.2 uniform(+-1) plus 0.01 N(0,1).  Where K > 1, keypoint 1 of frame 1 is a missing detection: c = 0 and a NaN
    target, which every term must skip."""
    inp = R.chain_inputs(case, seed)
    J, F = inp["J"], inp["F"]
    g = torch.Generator().manual_seed(8800 + 31 * R.CASES.index(case) + seed)
    uni = lambda *s: 2 * torch.rand(s, generator=g, dtype=F64) - 1
    bones = keypoint_bones(case, J)
    K = len(bones)
    theta_ref = rounded(inp["theta"] + 0.3 * uni(F, J + 2, 3))
    offsets = rounded(0.05 * torch.randn((K, 3), generator=g, dtype=F64))
    c = 1.0 + 0.5 * uni(F, K)
    if case == "hand":
        c[:, list(FINGERTIPS)] = 2.0
    other = rounded(inp["theta"] + 0.2 * uni(F, J + 2, 3))
    y = keypoints_of(R.fk(other, inp["rest"], inp["parents"], inp["base"]), bones, offsets) + 0.01 * torch.randn((F, K, 3), generator=g, dtype=F64)
    if K > 1:
        c[1, 1] = 0.0
        y[1, 1] = float("nan")
    inp.update(K=K, kp_bone=bones, kp_offset=offsets, kp_target=rounded(y), kp_weight=rounded(c), theta_ref=theta_ref,
               neighbours=neighbours(), frame_keys=list(FRAME_KEYS))
    return inp


def keypoints_of(M, bones, offsets):
    """p (F,K,3) = (M[:, bone[k]] [o_k; 1])[:3] in the dtype of M."""
    o = offsets.to(M.dtype)
    hom = torch.cat([o, torch.ones((o.shape[0], 1), dtype=M.dtype)], 1)
    return (M[:, list(bones)] @ hom[None, :, :, None])[:, :, :3, 0]


def terms(inp, th, M, w, listed=None):
    """(E_dev, E_smooth, E_kp) in the dtype of th, differentiable: the part that touches the rows `listed` (None: all), each term
    once -- the deviation and keypoint terms of the listed rows, every edge with at least one listed end.  A keypoint counts
    only where c > 0 (zero, negative and NaN weights skip it, whatever its target holds)."""
    dt = th.dtype
    F, J = th.shape[0], inp["J"]
    rows = set(range(F) if listed is None else listed)
    on = (inp["mask"] != 0).to(dt)
    wd = torch.full((J + 2, 1), float(w["w_dev_rot"]), dtype=dt)
    ws = torch.full((J + 2, 1), float(w["w_smooth_rot"]), dtype=dt)
    wd[-1], ws[-1] = float(w["w_dev_trans"]), float(w["w_smooth_trans"])
    zero = th.sum() * 0.0
    e_dev, e_smooth, e_kp = zero, zero, zero
    ref = inp["theta_ref"].to(dt)
    for f in sorted(rows):
        if 0 <= f < F:
            e_dev = e_dev + (wd * on * (th[f] - ref[f]) ** 2).sum()
    for f, (_, nxt) in enumerate(inp["neighbours"].tolist()):
        if nxt >= 0 and (f in rows or nxt in rows):
            e_smooth = e_smooth + (ws * on * (th[f] - th[nxt]) ** 2).sum()
    if float(w["w_kp"]) != 0.0:
        c, y = inp["kp_weight"].to(dt), inp["kp_target"].to(dt)
        live = c > 0
        p = keypoints_of(M, inp["kp_bone"], inp["kp_offset"])
        r = torch.where(live[..., None], p - torch.where(live[..., None], y, torch.zeros_like(y)), torch.zeros_like(p))
        per = (torch.where(live, c, torch.zeros_like(c)) * (r * r).sum(-1)).sum(-1)
        for f in sorted(rows):
            if 0 <= f < F:
                e_kp = e_kp + float(w["w_kp"]) * per[f]
    return e_dev, e_smooth, e_kp


def host_terms(inp, dtype, w, listed=None, chain=True, frames=None, theta=None, dT=None):
    """-> values (4,) = E_dev, E_smooth, E_kp and their sum on the rows `listed` (None: all), and d_theta (F,J+2,3) of
    sum(T * dT) over the views with a frame (chain=True) plus those terms, times the mask -- on a listed row the true gradient
    of the full E, since every term that touches the row is counted."""
    frames = inp.get("frames") if frames is None else frames
    th = (inp["theta"] if theta is None else theta).to(dtype).clone().requires_grad_(True)
    rest = inp["rest"].to(dtype)
    M = R.fk(th, rest, inp["parents"], inp["base"])
    parts = terms(inp, th, M, w, listed)
    loss = parts[0] + parts[1] + parts[2]
    if chain:
        dT = (inp["dT"] if dT is None else dT).to(dtype)
        inv = torch.linalg.inv(rest)
        shown = [(k, f) for k, f in enumerate(frames) if 0 <= f < th.shape[0]]
        if shown:
            T = torch.stack([M[f] for _, f in shown]) @ inv
            loss = loss + (T * dT[[k for k, _ in shown], :inp["J"]]).sum()
    grad, = torch.autograd.grad(loss, th)
    values = torch.stack([p.detach() for p in parts] + [(parts[0] + parts[1] + parts[2]).detach()])
    return values, grad * inp["mask"].to(dtype)


def adam_loop(inp, dtype, w, steps, listed, lr_rot, lr_trans, theta0=None, lo=None, hi=None):
    """`steps` steps of the terms alone on the rows `listed`: the gradient of `host_terms(chain=False)` in `dtype`, then
    `fk_chain_ref.adam_step`.  -> the final theta, and per step the values (4,) on the listed rows at the angles BEFORE the step."""
    th = (inp["theta"] if theta0 is None else theta0).to(dtype).clone()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    inf = torch.full_like(inp["mask"], float("inf"))
    lo, hi = (-inf if lo is None else lo), (inf if hi is None else hi)
    history = []
    for step in range(1, steps + 1):
        values, grad = host_terms(inp, dtype, w, listed, chain=False, theta=th)
        history.append(values.double())
        th, m, v = R.adam_step(th, m, v, grad[listed], listed, inp["mask"], lo, hi, lr_rot, lr_trans, step)
    return th, torch.stack(history)


# ------------------------------------------------------------------------------------------------------------------------------
# the recovery fixture: the golden hand in the dataset's keypoint convention
# ------------------------------------------------------------------------------------------------------------------------------
RECOVERY = dict(frames=3, steps=100, lr_rot=0.02, lr_trans=0.002, w=dict(ZERO, w_kp=10.0))


def recovery_inputs():
    """The golden hand (world rest matrices, heads and tails of tests/golden/fk_novel_pose.npz), `dof_mask` with both global rows
    free, theta0 = 0 on 3 frames, base = identity; theta_true = mask * 0.4 uniform(+-1), its translation row scaled by a further
    0.05; targets = the FK keypoints at theta_true in fp64 (K = 21 = the first head + all tails, `pose.keypoint_offsets`),
    fingertips weighted twice."""
    from manus_amd.pose import dof_mask, keypoint_offsets
    d = np.load(R.GOLDEN)
    parents = [int(p) for p in d["parents"]]
    rest = torch.tensor(d["world_rest_matrixs"], dtype=F64)
    J, F = len(parents), RECOVERY["frames"]
    bones, offsets = keypoint_offsets(rest, d["world_rest_heads"], d["world_rest_tails"])
    mask = dof_mask(["bone_%d" % i for i in range(J)], True, True).to(F64)
    g = torch.Generator().manual_seed(2323)
    true = mask * 0.4 * (2 * torch.rand((F, J + 2, 3), generator=g, dtype=F64) - 1)
    true[:, -1] *= 0.05
    true = rounded(true)
    base = torch.eye(4, dtype=F64).repeat(F, 1, 1)
    y = keypoints_of(R.fk(true, rest, parents, base), bones.tolist(), offsets.to(F64))
    c = torch.ones((F, J + 1), dtype=F64)
    c[:, list(FINGERTIPS)] = 2.0
    return dict(case="recovery", J=J, F=F, K=J + 1, parents=parents, rest=rest, base=base, theta=torch.zeros((F, J + 2, 3), dtype=F64),
                theta_true=true, theta_ref=torch.zeros((F, J + 2, 3), dtype=F64), mask=mask, kp_bone=bones.tolist(), kp_offset=offsets.to(F64),
                kp_target=rounded(y), kp_weight=c, frame_keys=[("take", f) for f in range(F)],
                neighbours=neighbours([("take", f) for f in range(F)]))

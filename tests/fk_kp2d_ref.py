"""The checker of the multi-view 2-D keypoint term on the kinematic refiner's angles (mgr_fk_backward_terms2d, csrc/fk.hip;
manus_amd.pose.KinematicPoseRefiner with w_kp2d): the term as host torch on top of `fk_terms_ref.terms` / `fk_chain_ref.fk` in a
given dtype on the CPU under autograd; the committed inputs of the tests -- the trees of `fk_chain_ref.CASES` and the lists of
`fk_terms_ref.LISTS` unchanged, plus small camera rigs around the posed skeleton --; the Adam loop; and the recovery fixture.

    q = P_c [p_k(theta_f); 1],  u = q[:2] / q[2],  d = |u - t[f,c,k]|
    rho(d) = d^2 where delta == 0 or d <= delta, 2 delta d - delta^2 otherwise
    E_kp2d = w_kp2d sum_f sum_c sum_k s[f,c,k] rho(d)           over s > 0 and q[2] > z_min

Tolerance of the GPU tests that use it: `check_rows`, e_kernel <= 8 * max(e32, 2^-23) per (frame, row) against this restatement in
fp64, e32 the error of the same restatement in fp32.  The one discontinuous decision of the term is the depth skip; the fixture
keeps every detection's fp64 depth outside (z_min / 4, 4 z_min) -- a detection that falls inside gets weight 0 -- so fp32 and
fp64 decide alike (test_fk_kp2d_cpu.py asserts it)."""
import math

import torch

import fk_chain_ref as R
import fk_terms_ref as T
from fk_chain_ref import F64, rounded

# row of the table: (tree, K, C)
ROWS = {"one": ("one", 1, 1), "chain4": ("chain4", 2, 2), "hand": ("hand", 21, 5), "chain_max": ("chain_max", 64, 3),
        "fan65": ("fan", 3, 65), "fan9": ("fan", 7, 9)}
Z_MIN = 0.01
DELTA = 4.0                                      # pixels
W2D = 0.002                                      # pixels^2 to the scale of the other terms
ZERO = dict(T.ZERO, w_kp2d=0.0)
# weight combinations: the 2-D term alone, with the 3-D term, with all priors, and all five; `chain` = with d_transforms
COMBOS = {"2d": dict(ZERO, w_kp2d=W2D), "2d3d": dict(ZERO, w_kp2d=W2D, w_kp=10.0),
          "2dpriors": dict(T.WEIGHTS, w_kp=0.0, w_kp2d=W2D), "all": dict(T.WEIGHTS, w_kp2d=W2D)}
FOCAL, CENTRE = 500.0, (320.0, 240.0)


def keypoint_bones(row, J):
    """one: K = 1; chain4: both keypoints on bone 1, bones 0, 2, 3 with none; hand: the dataset's [0, 0, 1, .., 19]; chain_max: K = 64,
    two per bone; fan65: bones 0, 2, 5; fan9: [0, 0, 1, .., 5]."""
    return {"one": [0], "chain4": [1, 1], "chain_max": [k // 2 for k in range(64)], "fan65": [0, 2, 5]}.get(row, [0] + list(range(J)))


def look_at(centre, axis):
    """E (3,4) world to camera, fp64: the camera at `centre` looking along the unit vector `axis` (its +z)."""
    z = axis / axis.norm()
    up = torch.tensor([0.0, 0.0, 1.0], dtype=F64) if abs(float(z[2])) < 0.9 else torch.tensor([1.0, 0.0, 0.0], dtype=F64)
    x = torch.linalg.cross(up, z)
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    Rm = torch.stack([x, y, z])
    return torch.cat([Rm, -(Rm @ centre)[:, None]], 1)


def sphere(n, g):
    """n unit vectors spread over the sphere (a Fibonacci lattice, turned by a random rotation)."""
    i = torch.arange(n, dtype=F64) + 0.5
    phi, z = math.pi * (1 + 5 ** 0.5) * i, 1 - 2 * i / n
    r = (1 - z * z).sqrt()
    v = torch.stack([r * phi.cos(), r * phi.sin(), z], 1)
    return v @ R.rigid(g, scale=0.0)[:3, :3].T


def project(P, p):
    """q (F,C,K,3) = P_c [p; 1] in the dtype of p."""
    P = P.to(p.dtype)
    return torch.einsum("cij,fkj->fcki", P[:, :, :3], p) + P[:, None, :, 3]


NEAR, BEHIND = (1, 0, 0), (3, 0, -1)            # (f, c, k) of the detections planted in front of camera 0; k = -1: the last
NEAREST = 0.5                                    # no active detection is nearer to its camera than this


def kp2d_inputs(row, seed=0):
    """`fk_terms_ref.terms_inputs(tree)` with the keypoints of `keypoint_bones(row)` (offsets, 3-D targets and weights made as there)
    plus C cameras, fp32-representable fp64.  The cameras stand on a sphere of radius 4 R + 1 around the centroid of the posed
    keypoints of all frames (R: their largest distance from it) and look at it.  The bases of frames 1 and 3 are then moved along
    camera 0's axis, so that keypoint 0 of frame 1 lies z_min / 8 in front of camera 0 (skipped by depth) and the last keypoint
    of frame 3 `NEAREST` behind it; the other cameras see those frames from the side.  Intrinsics: focal 500, centre (320, 240).
    Weights s uniform in [0.5, 1.5]; every detection whose fp64 depth lies inside (z_min / 4, NEAREST) gets weight 0: the active
    ones are well in front (>= 4 z_min by far), where fp32 projects them accurately.  Targets: the fp64 projection at theta plus a vector of length
    delta U(0.2, 0.8) (even detections) or delta U(3, 10) (odd ones: several delta large).  Planted besides: (2, C-1, 0) weight 0
    with a NaN target; (5, C-1, K-1) a NaN weight (the one-keypoint one-camera row: in frame 4)."""
    tree, K, C = ROWS[row]
    inp = T.terms_inputs(tree, seed)
    J, F = inp["J"], inp["F"]
    g = torch.Generator().manual_seed(5100 + 53 * list(ROWS).index(row) + seed)
    uni = lambda *s: 2 * torch.rand(s, generator=g, dtype=F64) - 1
    bones = keypoint_bones(row, J)
    assert len(bones) == K
    offsets = rounded(0.05 * torch.randn((K, 3), generator=g, dtype=F64))
    c3 = 1.0 + 0.5 * uni(F, K)
    other = rounded(inp["theta"] + 0.2 * uni(F, J + 2, 3))
    keypoints = lambda theta, base: T.keypoints_of(R.fk(theta, inp["rest"], inp["parents"], base), bones, offsets)      # (F,K,3)
    p = keypoints(inp["theta"], inp["base"])
    centroid = p.reshape(-1, 3).mean(0)
    radius = float((p.reshape(-1, 3) - centroid).norm(dim=1).max())
    dist = 4.0 * radius + 1.0
    Kin = torch.tensor([[FOCAL, 0.0, CENTRE[0]], [0.0, FOCAL, CENTRE[1]], [0.0, 0.0, 1.0]], dtype=F64)
    dirs = sphere(C, g)
    proj = rounded(Kin @ torch.stack([look_at(centroid + dist * d, -d) for d in dirs]))      # (C,3,4)
    # the two planted frames are moved along camera 0's axis by their base
    axis, c0 = -dirs[0], centroid + dist * dirs[0]
    base = inp["base"].clone()
    base[NEAR[0], :3, 3] -= axis * (float((p[NEAR[0], NEAR[2]] - c0) @ axis) - Z_MIN / 8.0)
    base[BEHIND[0], :3, 3] -= axis * (float((p[BEHIND[0], BEHIND[2]] - c0) @ axis) + NEAREST)
    base = rounded(base)
    p = keypoints(inp["theta"], base)
    y3 = keypoints(other, base) + 0.01 * torch.randn((F, K, 3), generator=g, dtype=F64)
    q = project(proj, p)
    s = 1.0 + 0.5 * uni(F, C, K)
    qz = q[..., 2]
    s[(qz > Z_MIN / 4.0) & (qz < NEAREST)] = 0.0
    uv = q[..., :2] / qz[..., None]
    uv = torch.where(torch.isfinite(uv), uv, torch.zeros_like(uv)).clamp(-1e6, 1e6)
    ang = math.pi * uni(F, C, K)
    odd = (torch.arange(F * C * K).reshape(F, C, K) % 2 == 1)
    mag = DELTA * torch.where(odd, 6.5 + 3.5 * uni(F, C, K), 0.5 + 0.3 * uni(F, C, K))
    t = uv + mag[..., None] * torch.stack([ang.cos(), ang.sin()], -1)
    s[2, C - 1, 0] = 0.0
    t[2, C - 1, 0] = float("nan")
    s[4 if C * K == 1 else 5, C - 1, K - 1] = float("nan")
    inp.update(row=row, K=K, C=C, base=base, kp_bone=bones, kp_offset=offsets, kp_target=rounded(y3), kp_weight=rounded(c3), kp2d_proj=proj,
               kp2d_target=rounded(t), kp2d_weight=rounded(s), kp2d_delta=DELTA, kp2d_zmin=Z_MIN)
    return inp


def term2d(inp, M, delta, zmin, proj=None, target=None, weight=None):
    """-> per (F,) = sum_c sum_k s rho(d) of every frame, dist (F,C,K) (NaN where skipped) and live (F,C,K), in the dtype of M,
    differentiable.  A detection counts only where s > 0 and q[2] > z_min; what a skipped one holds never enters a product."""
    dt = M.dtype
    p = T.keypoints_of(M, inp["kp_bone"], inp["kp_offset"])
    q = project(inp["kp2d_proj"] if proj is None else proj, p)
    s = (inp["kp2d_weight"] if weight is None else weight).to(dt)
    t = (inp["kp2d_target"] if target is None else target).to(dt)
    live = (s > 0) & (q[..., 2] > zmin)
    qz = torch.where(live, q[..., 2], torch.ones_like(s))
    u = q[..., :2] / qz[..., None]
    r = torch.where(live[..., None], u - torch.where(live[..., None], t, torch.zeros_like(t)), torch.zeros_like(u))
    d2 = (r * r).sum(-1)
    pos = d2 > 0
    d = torch.where(pos, torch.where(pos, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
    if float(delta) == 0.0:
        rho = d2
    else:
        rho = torch.where(d <= delta, d2, 2.0 * float(delta) * d - float(delta) ** 2)
    per = (torch.where(live, s, torch.zeros_like(s)) * rho).sum((1, 2))
    return per, torch.where(live, d, torch.full_like(d, float("nan"))), live


def host_terms2d(inp, dtype, w, delta=None, listed=None, chain=True, theta=None, zmin=None, **tables):
    """-> values (5,) = E_dev, E_smooth, E_kp, the sum of all four, E_kp2d on the rows `listed` (None: all); d_theta (F,J+2,3) of
    sum(T * dT) over the views with a frame (chain=True) plus the four terms, times the mask; dist (F,C,K)."""
    delta = inp["kp2d_delta"] if delta is None else delta
    zmin = inp["kp2d_zmin"] if zmin is None else zmin
    th = (inp["theta"] if theta is None else theta).to(dtype).clone().requires_grad_(True)
    rest = inp["rest"].to(dtype)
    F = th.shape[0]
    M = R.fk(th, rest, inp["parents"], inp["base"])
    parts = list(T.terms(inp, th, M, w, listed))
    per, dist, _ = term2d(inp, M, delta, zmin, **tables)
    e2d = th.sum() * 0.0
    if float(w["w_kp2d"]) != 0.0:
        for f in sorted(set(range(F) if listed is None else listed)):
            if 0 <= f < F:
                e2d = e2d + float(w["w_kp2d"]) * per[f]
    total = ((parts[0] + parts[1]) + parts[2]) + e2d
    loss = total
    if chain:
        dT = inp["dT"].to(dtype)
        inv = torch.linalg.inv(rest)
        shown = [(k, f) for k, f in enumerate(inp["frames"]) if 0 <= f < F]
        T_ = torch.stack([M[f] for _, f in shown]) @ inv
        loss = loss + (T_ * dT[[k for k, _ in shown], :inp["J"]]).sum()
    grad, = torch.autograd.grad(loss, th)
    values = torch.stack([parts[0].detach(), parts[1].detach(), parts[2].detach(), total.detach(), e2d.detach()])
    return values, grad * inp["mask"].to(dtype), dist.detach()


def host_values(inp, theta, w, delta, zmin=None):
    """The full E of all rows at theta, a scalar in the dtype of theta."""
    M = R.fk(theta, inp["rest"].to(theta.dtype), inp["parents"], inp["base"])
    per = term2d(inp, M, delta, inp["kp2d_zmin"] if zmin is None else zmin)[0]
    return sum(T.terms(inp, theta, M, w)) + float(w["w_kp2d"]) * per.sum()


def adam_loop(inp, dtype, w, delta, steps, listed, lr_rot, lr_trans, theta0=None):
    """`steps` steps of the terms alone on the rows `listed`, as `fk_terms_ref.adam_loop`.  -> the final theta and per step the
    values (5,) at the angles BEFORE the step."""
    th = (inp["theta"] if theta0 is None else theta0).to(dtype).clone()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    inf = torch.full_like(inp["mask"], float("inf"))
    history = []
    for step in range(1, steps + 1):
        values, grad, _ = host_terms2d(inp, dtype, w, delta, listed, chain=False, theta=th)
        history.append(values.double())
        th, m, v = R.adam_step(th, m, v, grad[listed], listed, inp["mask"], -inf, inf, lr_rot, lr_trans, step)
    return th, torch.stack(history)


# ------------------------------------------------------------------------------------------------------------------------------
# the recovery fixture: the golden hand, one bent joint, four cameras, one of them wrong about the bent finger
# ------------------------------------------------------------------------------------------------------------------------------
RECOVERY = dict(steps=150, lr_rot=0.05, lr_trans=0.002, delta=5.0, w=dict(ZERO, w_kp2d=0.01), bone=6, bend=(-0.5, -0.8, -1.1),
                finger=(6, 7, 8), camera=1, shift=(40.0, -30.0))


def recovery_inputs():
    """`fk_terms_ref.recovery_inputs()`'s hand (3 frames, theta0 = 0, K = 21) with the global rows fixed (`dof_mask`: 23 free angles);
    theta_true = 0 but angle 2 of bone 6, bent by -0.5 / -0.8 / -1.1 rad in the three frames.  Four cameras on a sphere around the
    keypoints at theta_true; detections = `pose.project_keypoints` of the fp64 truth through them, weight 1; camera 1's
    detections of keypoints 6, 7, 8 (the tails of bones 5, 6, 7: the bent finger) are displaced by (40, -30) pixels."""
    from manus_amd.pose import dof_mask, project_keypoints, projection_matrices
    cfg = RECOVERY
    fx = T.recovery_inputs()
    J, F, K = fx["J"], fx["F"], fx["K"]
    mask = dof_mask(["bone_%d" % i for i in range(J)], False, False).to(F64)
    true = torch.zeros((F, J + 2, 3), dtype=F64)
    for f, b in enumerate(cfg["bend"]):
        true[f, 1 + cfg["bone"], 2] = b
    assert float(mask[1 + cfg["bone"], 2]) == 1.0
    true = rounded(true)
    p = T.keypoints_of(R.fk(true, fx["rest"], fx["parents"], fx["base"]), fx["kp_bone"], fx["kp_offset"])
    centroid = p.reshape(-1, 3).mean(0)
    radius = float((p.reshape(-1, 3) - centroid).norm(dim=1).max())
    g = torch.Generator().manual_seed(2424)
    Kin = torch.tensor([[FOCAL, 0.0, CENTRE[0]], [0.0, FOCAL, CENTRE[1]], [0.0, 0.0, 1.0]], dtype=F64)
    ext = torch.stack([look_at(centroid + (4.0 * radius) * d, -d) for d in sphere(4, g)])
    proj = projection_matrices(Kin.repeat(4, 1, 1), ext).double()
    t = project_keypoints(proj, p)                                                           # (F,4,K,2)
    t[:, cfg["camera"], list(cfg["finger"])] += torch.tensor(cfg["shift"], dtype=F64)
    fx.update(C=4, mask=mask, theta_true=true, kp2d_proj=proj, kp2d_target=rounded(t), kp2d_weight=torch.ones((F, 4, K), dtype=F64),
              kp2d_delta=cfg["delta"], kp2d_zmin=Z_MIN, kp_target=rounded(p))
    return fx

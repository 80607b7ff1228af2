"""The checker of the device pose chain (csrc/pose.hip, manus_amd.pose.PoseRefiner): the existing host chain --
`PoseCorrection` + `torch.linalg.inv` + autograd -- in a given dtype on the CPU, the committed inputs of the tests, and a numpy
restatement of the analytic Rodrigues vector-Jacobian product the backward kernel evaluates.

Tolerance of the tests that use it: the project's `check_rows`, e_kernel <= 8 * max(e32, 2^-23) in `row_rel_err` against this
chain in fp64, where e32 is the error of this same chain run in fp32."""
import numpy as np
import torch

from util import row_rel_err

F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -23
FACTOR = 8.0
SMALL = 1e-6                                   # |r|^2 below which pose._exp_so3 takes its series
FRAMES = [0, 1, 1, 3, 0, 1, 3, 3, 0]           # frame of position k (the first V are used); F = 4, frame 2 is never viewed
N_FRAMES = 4
BONES = (1, 20, 32)
VIEWS = (1, 3, 9)


def bound_of(e32):
    return FACTOR * max(e32, EPS32)


def check_rows(tag, got, ref64, ref32):
    """e_kernel <= 8 * max(e32, 2^-23), both in `row_rel_err` against fp64 over the rows of the first axis; prints the figures
    before it asserts."""
    got, ref64, ref32 = (x.detach().cpu().double() for x in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    e32, ek = row_rel_err(ref32, ref64), row_rel_err(got, ref64)
    ratio = ek / max(e32, EPS32)
    print("RATIO %-40s e_kernel %.3e  e32 %.3e  ratio %.2f" % (tag, ek, e32, ratio))
    assert ek <= bound_of(e32), "%s: e_kernel %.3e  e32 %.3e  ratio %.2f > %g" % (tag, ek, e32, ratio, FACTOR)
    return ek, e32


def rounded(x):
    return x.to(F32).to(F64)


def chain_inputs(B, V, seed=0, n_all=None):
    """fp32-representable fp64 inputs: posed (n_all,B,4,4) and rest (B,4,4) rigid plus a little shear, corrections
    rotvec ~ 0.2 N(0,1) / trans ~ 0.01 N(0,1) (F,B,3) with single rows at exactly 0 and at |r| = 9.4e-4 / 1.05e-3 (either side
    of the series threshold |r|^2 = 1e-6), a random dL/dT (V,B+1,4,4), the view rows of the V positions (a permutation of a
    table two rows larger) and their frames.

    The row just above the threshold is where the fp32 host chain is least accurate: 1 - cos(1.05e-3) keeps three bits in
    fp32, b = (1 - cos th) / th^2 is off by 2.7 %, and d_rotvec of that row by 6e-6 .. 4e-5 of itself depending on how much
    of dC is symmetric (every other row: below 8e-7).  The committed base seed is one at which that row stays below 1e-5 at all
    nine shapes (test_pose_chain_cpu.py asserts it), which keeps the bound 8 * e32 of the GPU tests tight."""
    from manus_amd.pose import _exp_so3
    g = torch.Generator().manual_seed(7826 + 131 * B + 17 * V + seed)
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)
    n_all = V + 2 if n_all is None else n_all

    def rigid(*lead):
        m = torch.eye(4, dtype=F64).repeat(*lead, 1, 1)
        m[..., :3, :3] = _exp_so3(0.8 * rn(*lead, 3)) + 0.02 * rn(*lead, 3, 3)
        m[..., :3, 3] = 0.1 * rn(*lead, 3)
        return m
    rotvec, trans = 0.2 * rn(N_FRAMES, B, 3), 0.01 * rn(N_FRAMES, B, 3)
    unit = rn(3)
    unit = unit / unit.norm()
    rotvec[0, 0] = 0.0                                       # exactly zero (frame 0 is viewed at every V)
    if B > 2:
        rotvec[0, 1] = 9.4e-4 * unit                         # |r|^2 = 8.8e-7: the series
        rotvec[0, 2] = 1.05e-3 * unit                        # |r|^2 = 1.1e-6: the closed form
    rows = torch.randperm(n_all, generator=g)[:V].tolist()
    return dict(B=B, V=V, F=N_FRAMES, n_all=n_all, posed=rounded(rigid(n_all, B)), rest=rounded(rigid(B)), rotvec=rounded(rotvec),
                trans=rounded(trans), dT=rounded(rn(V, B + 1, 4, 4)), rows=rows, frames=FRAMES[:V])


def host_chain(inp, dtype, frames=None):
    """The existing host chain in `dtype` on the CPU: T (V,B+1,4,4) by position (PoseCorrection.forward, then posed @ inv(rest),
    then the identity row), and d_rotvec / d_trans (F,B,3) of sum(T * dT) by autograd.  frames: other frame rows (-1: none)."""
    from manus_amd.pose import PoseCorrection
    B, frames = inp["B"], (inp["frames"] if frames is None else frames)
    corr = PoseCorrection(inp["F"], B, dtype=dtype)
    with torch.no_grad():
        corr.rotvec.copy_(inp["rotvec"].to(dtype))
        corr.trans.copy_(inp["trans"].to(dtype))
    inv = torch.linalg.inv(inp["rest"].to(dtype))
    eye = torch.eye(4, dtype=dtype)[None]
    Ts = []
    for k, (v, f) in enumerate(zip(inp["rows"], frames)):
        p = inp["posed"][v].to(dtype)
        c = corr(p, f) if f >= 0 else p
        Ts.append(torch.cat([c @ inv, eye], 0))
    T = torch.stack(Ts)
    loss = (T * inp["dT"].to(dtype)).sum()
    if loss.requires_grad:
        loss.backward()
    zero = torch.zeros_like(corr.rotvec)
    return T.detach(), (corr.rotvec.grad if corr.rotvec.grad is not None else zero), (corr.trans.grad if corr.trans.grad is not None else zero)


def rodrigues_vjp(r, G):
    """numpy, float64: dL/dr (3,) of R = exp(r) (pose._exp_so3, the series branch differentiated as a series) for G = dL/dR (3,3)
    -- the closed form the backward kernel evaluates."""
    r, G = np.asarray(r, np.float64), np.asarray(G, np.float64)
    x, y, z = r
    t = float(r @ r)
    if t < SMALL:
        a, b = 1.0 - t / 6.0 + t * t / 120.0, 0.5 - t / 24.0
        da, db = -1.0 / 6.0 + t / 60.0, -1.0 / 24.0
    else:
        th = np.sqrt(t)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / t
        da, db = (np.cos(th) - a) / (2.0 * t), (0.5 * a - b) / t
    axial = np.array([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])        # <G, dK/dr_i>
    sym = (G + G.T) @ r                                                                  # d(r^T G r)/dr
    gk, gk2 = float(axial @ r), float(r @ G @ r) - t * np.trace(G)                       # <G,K>, <G,K^2>, K^2 = r r^T - t I
    return a * axial + b * (sym - 2.0 * r * np.trace(G)) + 2.0 * (da * gk + db * gk2) * r

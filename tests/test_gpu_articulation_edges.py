"""GPU: the articulation kernels (skin weights, LBS of means / covariances, SH colour) and the fused step where their code
branches: every bone count that picks another kernel or another tail (1 <= B <= 32), cells on the grid border with some
corners padded, ragged N (1, 255, 257, 777), pose / view counts and strides, badly scaled leaves, the colour clamp.

Reference: oracle/torch_ref.py evaluated in float64 on the CPU.  Inputs are drawn in fp64 and rounded to fp32 once, so the
kernels and the oracle see the same numbers.  Norm: `util.row_rel_err` (every row judged at its own scale).  Tolerance:
measured, not fixed -- the same oracle evaluated in float32 on the CPU gives e32 = row_rel_err(fp32 oracle, fp64 oracle), and
a kernel must satisfy  row_rel_err(kernel, fp64 oracle) <= 8 * max(e32, 2^-23)  (three bits for another summation order, FMA
contraction and the division by `scale`; the floor is one fp32 epsilon).  The thresholds of section 4 that are not of this
form are those of tests/test_gpu_fused.py, taken verbatim and named where they are used.

The generators, both oracle evaluations and the cap checks need no GPU: `python tests/test_gpu_articulation_edges.py`
prints the reference-only report (shares of rows left out, clamped share, kink band, e32 per tensor)."""
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import torch_ref as tr  # noqa: E402

from util import max_rel_err, row_rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
FACTOR = 8.0          # three bits over the fp32 oracle's own error
F32, F64 = torch.float32, torch.float64


def rounded(x):
    """fp64 tensor whose values are exactly representable in fp32 (drawn in fp64, rounded once)."""
    return x.to(F32).to(F64)


def bound_of(e32):
    return FACTOR * max(e32, EPS32)


def check_rows(tag, got, ref64, ref32, rows=None):
    """The one tolerance of this file: e_kernel <= 8 * max(e32, 2^-23), both in `row_rel_err` against the fp64 oracle, over
    the rows `rows` (boolean mask or None = all).  Prints the figures before it asserts."""
    got, ref64, ref32 = (x.detach().cpu().double() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, np.float64)) for x in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    if rows is not None:
        rows = torch.as_tensor(rows).reshape(-1)
        got, ref64, ref32 = got[rows], ref64[rows], ref32[rows]
    e32, ek = row_rel_err(ref32, ref64), row_rel_err(got, ref64)
    ratio = ek / max(e32, EPS32)
    print("RATIO %-44s e_kernel %.3e  e32 %.3e  ratio %.2f" % (tag, ek, e32, ratio))
    assert ek <= bound_of(e32), "%s: e_kernel %.3e  e32 %.3e  ratio %.2f > %g" % (tag, ek, e32, ratio, FACTOR)
    return ek, e32


def ulp_equal(got, a, b, n_ulp=2):
    """got == a + b to n_ulp units of the last place (fp32) of the larger term, element for element."""
    got, a, b = (x.detach().cpu().numpy().astype(np.float32) for x in (got, a, b))
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - (a.astype(np.float64) + b.astype(np.float64))) <= n_ulp * ulp


# =================================================================================================================
# 1. skin weights at the borders, over the bone counts
# =================================================================================================================
SKIN_DIMS = (5, 6, 7)                 # (D,H,W)
SKIN_BONES = (1, 3, 8, 20, 21, 24, 25, 32)
SKIN_N = 777
S_FLOOR = 1e-2                        # rows whose raw sum is below S_FLOOR * max S are ill-conditioned in any precision
NODE_BAND = 1e-4                      # (index units) the fp32 and the fp64 cell index may differ this close to a node plane
LEFT_OUT_CAP = 0.10


def skin_inputs(B, seed=0):
    """Grid rand**3 with 30 % exact zeros; N = 777 points uniform in u in [-1.15, 1.15]^3 (about a third of the rows have
    padded corners); a random dL/dw; forward-only points: the eight corners u = (+-1,+-1,+-1) and six points exactly on
    nodes (border and interior)."""
    g = torch.Generator().manual_seed(7000 + 37 * B + seed)
    D, H, W = SKIN_DIMS
    grid = torch.rand((D, H, W, B), generator=g, dtype=F64) ** 3
    grid[torch.rand((D, H, W, B), generator=g, dtype=F64) < 0.3] = 0.0
    center, scale = rounded(torch.tensor([0.01, -0.02, 0.03], dtype=F64)), rounded(torch.tensor([0.5, 0.4, 0.3], dtype=F64))
    u = torch.rand((SKIN_N, 3), generator=g, dtype=F64) * 2.3 - 1.15
    corners = torch.tensor([[sx, sy, sz] for sz in (-1.0, 1.0) for sy in (-1.0, 1.0) for sx in (-1.0, 1.0)], dtype=F64)
    nodes = torch.tensor([[0, 0, 0], [3, 2, 1], [6, 5, 4], [2, 0, 3], [6, 3, 0], [4, 5, 2]], dtype=F64)   # (x,y,z) node indices
    u_nodes = nodes / torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=F64) * 2.0 - 1.0
    return dict(B=B, grid=rounded(grid), center=center, scale=scale, xyz=rounded(u * scale + center),
                xyz_fwd=rounded(torch.cat([corners, u_nodes]) * scale + center),
                g_w=rounded(torch.randn((SKIN_N, B), generator=g, dtype=F64)),
                start=rounded(torch.randn((SKIN_N, 3), generator=g, dtype=F64)))


def skin_raw_sum(inp, xyz):
    """fp64 raw (un-normalised) sum S of the sampled channels, and the distance of the sample position from the nearest
    node plane in index units (smallest over the three axes)."""
    D, H, W = SKIN_DIMS
    grid = inp["grid"]
    u = ((xyz - inp["center"]) / inp["scale"]).reshape(1, -1, 1, 1, 3)
    raw = torch.nn.functional.grid_sample(grid.permute(3, 0, 1, 2).unsqueeze(0), u, mode="bilinear", padding_mode="zeros",
                                          align_corners=True).reshape(grid.shape[3], -1).T
    idx = (u.reshape(-1, 3) + 1.0) * 0.5 * torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=F64)
    return raw.sum(1), (idx - idx.round()).abs().min(1).values


def skin_oracle(inp, dtype, xyz=None, grad=True):
    """(weights, dL/dxyz) of tr.skin_weights_from_grid in `dtype` on the CPU (dL/dw = inp["g_w"])."""
    x = (inp["xyz"] if xyz is None else xyz).to(dtype).clone().requires_grad_(grad)
    w = tr.skin_weights_from_grid(x, inp["center"].to(dtype), inp["scale"].to(dtype), inp["grid"].to(dtype))
    if not grad:
        return w.detach(), None
    w.backward(inp["g_w"].to(dtype))
    return w.detach(), x.grad.detach()


def skin_reference(B):
    """Everything of section 1 that needs no GPU, computed once per B: both oracles, the NaN rows, the rows left out of the
    gradient comparison and their share."""
    if B in _SKIN_REF:
        return _SKIN_REF[B]
    inp = skin_inputs(B)
    w64, g64 = skin_oracle(inp, F64)
    w32, g32 = skin_oracle(inp, F32)
    S, node_dist = skin_raw_sum(inp, inp["xyz"])
    nan_rows = torch.isnan(w64).any(1)
    fin = ~nan_rows
    small = fin & (S < S_FLOOR * S.max())
    near = fin & (node_dist < NODE_BAND)
    grad_rows = fin & ~small & ~near
    if B == 1:
        # one channel: w = raw / raw = 1 wherever it is finite, so dL/dxyz is identically zero and what any precision returns
        # is rounding noise.  The reference is the exact zero (the fp64 oracle agrees to its own rounding); `row_rel_err` then
        # measures absolute errors, and the kernel's noise is held against the fp32 oracle's by the same factor.
        assert float(g64[grad_rows].abs().max()) < 1e-9
        g64 = torch.zeros_like(g64)
    wf64, _ = skin_oracle(inp, F64, inp["xyz_fwd"], grad=False)
    wf32, _ = skin_oracle(inp, F32, inp["xyz_fwd"], grad=False)
    Sf, _ = skin_raw_sum(inp, inp["xyz_fwd"])
    # a point exactly on a node whose channels are all zero (or whose own value is dwarfed by its neighbours') has no
    # continuous value: w = 0/0 with a direction-dependent limit.  The same conditioning floor as for the gradient rows.
    fwd_rows = Sf >= S_FLOOR * S.max()
    ref = dict(inp=inp, w64=w64, w32=w32, g64=g64, g32=g32, nan_rows=nan_rows, fin=fin, grad_rows=grad_rows,
               share_small=float(small.sum()) / float(fin.sum()), share_near=float(near.sum()) / float(fin.sum()),
               padded_rows=float(((inp["xyz"] - inp["center"]).abs() / inp["scale"] > 1.0).any(1).double().mean()),
               wf64=wf64, wf32=wf32, fwd_rows=fwd_rows)
    _SKIN_REF[B] = ref
    return ref


_SKIN_REF = {}


def assert_skin_caps(ref):
    assert ref["share_small"] <= LEFT_OUT_CAP and ref["share_near"] <= LEFT_OUT_CAP, (ref["share_small"], ref["share_near"])
    n_nan = int(ref["nan_rows"].sum())                            # rows whose every in-bounds corner is zero: 0/0
    assert n_nan < 0.05 * SKIN_N and (n_nan > 0 or ref["inp"]["B"] > 1)
    assert 0.2 < ref["padded_rows"] < 0.5                         # about a third of the rows sample across the border
    assert int(ref["fwd_rows"].sum()) >= 7                        # (of 14 forward-only points)


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def _skin_generic(inp, xyz, g_w=None, start=None, index=None, count=None, max_count=0):
    """The generic kernels through the C ABI with grid_stride = B (the reference's unpadded layout): forward, or backward
    with accumulate = (start is not None), or the indexed backward.  The grid starts 4 bytes into its buffer: rows of B = 24
    floats on a 16-byte aligned base are the padded layout and would take the fast path."""
    from manus_amd._lib import check, lib, ptr, stream
    B = inp["B"]
    buf = torch.empty(inp["grid"].numel() + 1, dtype=F32, device=DEV)
    grid = buf[1:].view(inp["grid"].shape)
    grid.copy_(inp["grid"])
    assert grid.data_ptr() % 16 == 4 and grid.is_contiguous()
    return _skin_raw(lib, check, ptr, stream, grid, B, B, inp, xyz, g_w, start, index, count, max_count)


def _skin_padded(inp, xyz, g_w=None, start=None, index=None, count=None, max_count=0):
    """The same calls on the grid `ops.SkinGrid` prepares (24-channel rows for B <= 24, the unpadded grid above)."""
    from manus_amd import ops
    from manus_amd._lib import check, lib, ptr, stream
    sg = ops.SkinGrid(_dev(inp["grid"]), DEV)
    return _skin_raw(lib, check, ptr, stream, sg.data, inp["B"], sg.stride, inp, xyz, g_w, start, index, count, max_count)


def _skin_raw(lib, check, ptr, stream, grid, B, stride, inp, xyz, g_w, start, index, count, max_count):
    D, H, W = SKIN_DIMS
    N = xyz.shape[0]
    c, s = _dev(inp["center"]), _dev(inp["scale"])
    if g_w is None:
        w = torch.empty((N, B), dtype=F32, device=DEV)
        check(lib().mgr_skin_weights_fwd(N, ptr(xyz), ptr(grid), D, H, W, B, stride, ptr(c), ptr(s), ptr(w), stream()), "skin fwd")
        return w
    out = torch.full((N, 3), float("nan"), dtype=F32, device=DEV) if start is None else start.clone()
    if index is not None:
        check(lib().mgr_skin_weights_bwd_indexed(N, ptr(xyz), ptr(grid), D, H, W, B, stride, ptr(c), ptr(s), ptr(g_w), ptr(out),
                                                 ptr(index), ptr(count), max_count, stream()), "skin bwd indexed")
    else:
        check(lib().mgr_skin_weights_bwd(N, ptr(xyz), ptr(grid), D, H, W, B, stride, ptr(c), ptr(s), ptr(g_w), ptr(out),
                                         0 if start is None else 1, stream()), "skin bwd")
    return out


@pytest.mark.parametrize("B", SKIN_BONES)
def test_skin_weights_at_the_borders_vs_fp64_grid_sample(B):
    """ops.skin_weights forward and backward (k_skin_fwd24x8 / k_skin_bwd24 for B <= 24, k_skin_fwd / k_skin_bwd above)
    against fp64 grid_sample: same NaN rows, weights and dL/dxyz per row; the corners and on-node points forward only."""
    from manus_amd import ops
    ref = skin_reference(B)
    assert_skin_caps(ref)
    inp = ref["inp"]
    xyz = _dev(inp["xyz"]).requires_grad_(True)
    w = ops.skin_weights(xyz, _dev(inp["grid"]), _dev(inp["center"]), _dev(inp["scale"]))
    assert w.shape == (SKIN_N, B)
    w.backward(_dev(inp["g_w"]))
    wk, gk = w.detach().cpu(), xyz.grad.cpu()
    assert torch.equal(torch.isnan(wk).any(1), ref["nan_rows"]) and torch.equal(torch.isnan(wk).all(1), ref["nan_rows"])
    check_rows("skin B=%d weights" % B, wk, ref["w64"], ref["w32"], ref["fin"])
    check_rows("skin B=%d dL/dxyz" % B, gk, ref["g64"], ref["g32"], ref["grad_rows"])
    with torch.no_grad():
        wf = ops.skin_weights(_dev(inp["xyz_fwd"]), _dev(inp["grid"]), _dev(inp["center"]), _dev(inp["scale"])).cpu()
    check_rows("skin B=%d corner/node weights" % B, wf, ref["wf64"], ref["wf32"], ref["fwd_rows"])


@pytest.mark.parametrize("B", [3, 21, 24])
def test_skin_generic_kernels_at_small_bone_counts(B):
    """grid_stride = B (and, for B = 24, a base that is not 16-byte aligned) reaches k_skin_fwd / k_skin_bwd at B <= 24:
    against the oracle and against the padded route, to the same bound."""
    ref = skin_reference(B)
    inp = ref["inp"]
    xyz, g_w = _dev(inp["xyz"]), _dev(inp["g_w"])
    wg, wp = _skin_generic(inp, xyz).cpu(), _skin_padded(inp, xyz).cpu()
    gg, gp = _skin_generic(inp, xyz, g_w).cpu(), _skin_padded(inp, xyz, g_w).cpu()
    assert torch.equal(torch.isnan(wg).any(1), ref["nan_rows"])
    _, e32w = check_rows("skin generic B=%d weights" % B, wg, ref["w64"], ref["w32"], ref["fin"])
    _, e32g = check_rows("skin generic B=%d dL/dxyz" % B, gg, ref["g64"], ref["g32"], ref["grad_rows"])
    ew, eg = row_rel_err(wg[ref["fin"]], wp[ref["fin"]]), row_rel_err(gg[ref["grad_rows"]], gp[ref["grad_rows"]])
    print("RATIO skin generic-vs-padded B=%d weights %.3e (e32 %.3e)  dL/dxyz %.3e (e32 %.3e)" % (B, ew, e32w, eg, e32g))
    assert ew <= bound_of(e32w) and eg <= bound_of(e32g), (ew, e32w, eg, e32g)


@pytest.mark.parametrize("B,route", [(3, "padded"), (21, "padded"), (24, "padded"), (21, "generic"), (25, "padded"), (32, "padded")])
def test_skin_backward_accumulates_onto_a_given_gradient(B, route):
    """accumulate = 1: the result is the given dL_dxyz plus the accumulate = 0 result, row for row, to 2 ulp of the larger
    term (k_skin_bwd24 for the padded route at B <= 24, k_skin_bwd otherwise)."""
    ref = skin_reference(B)
    inp = ref["inp"]
    call = _skin_padded if route == "padded" else _skin_generic
    xyz, g_w, start = _dev(inp["xyz"]), _dev(inp["g_w"]), _dev(inp["start"])
    fresh = call(inp, xyz, g_w)
    acc = call(inp, xyz, g_w, start=start)
    fin = ref["fin"]
    assert torch.isfinite(fresh.cpu()[fin]).all()
    check_rows("skin acc B=%d %s fresh dL/dxyz" % (B, route), fresh.cpu(), ref["g64"], ref["g32"], ref["grad_rows"])
    ok = ulp_equal(acc, start, fresh)[fin.numpy()]
    assert ok.all(), int((~ok).sum())


@pytest.mark.parametrize("B", [3, 21, 25])
def test_skin_backward_indexed_touches_only_the_listed_rows(B):
    """mgr_skin_weights_bwd_indexed: a device list of 300 distinct indices (40 of them >= N: static rows of a composite),
    device count 300, max_count 512.  Listed rows = start + fresh, every other row bit-identical to the start.  (The slots
    behind the count hold valid, unlisted indices: a kernel that ignored the count would write them.)"""
    ref = skin_reference(B)
    inp = ref["inp"]
    N = SKIN_N
    g = torch.Generator().manual_seed(B)
    perm = torch.randperm(N, generator=g)
    listed, unlisted = perm[:260], perm[260:]
    entries = torch.cat([listed, N + torch.randperm(200, generator=g)[:40]])
    entries = entries[torch.randperm(300, generator=g)]
    index = torch.cat([entries, unlisted[:212]]).to(torch.int32).to(DEV)
    assert index.numel() == 512 and len(set(index.cpu().tolist())) == 512
    count = torch.tensor([300], dtype=torch.int32, device=DEV)
    xyz, g_w, start = _dev(inp["xyz"]), _dev(inp["g_w"]), _dev(inp["start"])
    fresh = _skin_padded(inp, xyz, g_w)
    got = _skin_padded(inp, xyz, g_w, start=start, index=index, count=count, max_count=512)
    is_listed = torch.zeros(N, dtype=torch.bool)
    is_listed[listed] = True
    assert torch.equal(got.cpu()[~is_listed], start.cpu()[~is_listed])
    rows = (is_listed & ref["fin"]).numpy()
    ok = ulp_equal(got, start, fresh)[rows]
    assert rows.sum() > 200 and ok.all(), int((~ok).sum())
    assert int((got.cpu() != start.cpu()).any(1).sum()) > 200


# =================================================================================================================
# 2. LBS over B, P, ragged N, badly scaled leaves
# =================================================================================================================
#            B   P   N   tf44   loss term on tf
LBS_CASES = [(1, 1, 1, False, False), (1, 5, 777, True, True), (8, 2, 255, False, True), (8, 1, 257, True, False),
             (21, 5, 257, False, False), (21, 2, 777, True, True), (24, 1, 255, True, True), (24, 5, 1, False, True),
             (25, 2, 257, False, True), (25, 1, 777, True, False), (32, 5, 255, True, True), (32, 1, 1, False, False),
             (32, 2, 777, False, True),
             # static path (skin_w = None): B = 0
             (0, 1, 1, False, False), (0, 1, 255, True, True), (0, 1, 257, False, True), (0, 1, 777, True, False)]
LBS_LEAVES = ("xyz", "log_scale", "rot", "w")


def lbs_inputs(B, P, N, seed=0):
    g = torch.Generator().manual_seed(9000 + 101 * B + 11 * P + N + seed)
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)
    ru = lambda *s: torch.rand(s, generator=g, dtype=F64)
    q = rn(N, 4)
    q = q / q.norm(dim=1, keepdim=True) * 10.0 ** (ru(N, 1) * 4.0 - 2.0)       # norms log-uniform over [1e-2, 1e2]
    inp = dict(B=B, P=P, N=N, xyz=rounded(0.2 * rn(N, 3)), log_scale=rounded(ru(N, 3) * 7.0 - 9.0), rot=rounded(q),
               r_xyz=rounded(rn(P, N, 3)), r_cov=rounded(rn(P, N, 6)), r_tf=rounded(rn(P, N, 3, 4)))
    if B:
        T = torch.eye(4, dtype=F64).repeat(P, B, 1, 1)
        T[:, :, :3, :] += 0.2 * rn(P, B, 3, 4)                                    # general affine, last row (0,0,0,1)
        w = ru(N, B) ** 2
        w[ru(N, B) < 0.3] = 0.0
        w[torch.arange(N), torch.randint(0, B, (N,), generator=g)] += 0.1         # no all-zero row
        inp.update(T=rounded(T), w=rounded(w / w.sum(1, keepdim=True)))
    return inp


def lbs_oracle(inp, dtype, tf_loss):
    """Outputs (P,N,.) and leaf gradients of tr.lbs_forward looped over the poses (static path: tr.covariance_3x3 alone)."""
    B, P = inp["B"], inp["P"]
    leaf = {k: inp[k].to(dtype).clone().requires_grad_(True) for k in LBS_LEAVES if k in inp}
    px, pc, tf, loss = [], [], [], 0
    for p in range(P):
        if B:
            x, c, t = tr.lbs_forward(leaf["xyz"], leaf["log_scale"], leaf["rot"], leaf["w"], inp["T"][p].to(dtype))
            tf.append(t[:, :3, :])
            if tf_loss:
                loss = loss + (t[:, :3, :] * inp["r_tf"][p].to(dtype)).sum()
        else:
            x, c = leaf["xyz"], tr.pack_sym6(tr.covariance_3x3(leaf["log_scale"], leaf["rot"]))
        px.append(x)
        pc.append(c)
        loss = loss + (x * inp["r_xyz"][p].to(dtype)).sum() + (c * inp["r_cov"][p].to(dtype) * 1e3).sum()
    loss.backward()
    out = dict(posed_xyz=torch.stack(px).detach(), posed_cov=torch.stack(pc).detach())
    if B:
        out["tf"] = torch.stack(tf).detach()
    out.update({"d_" + k: v.grad.detach() for k, v in leaf.items()})
    return out


def lbs_kernel(inp, tf44, tf_loss):
    from manus_amd import ops
    B, P, N = inp["B"], inp["P"], inp["N"]
    leaf = {k: _dev(inp[k]).requires_grad_(True) for k in LBS_LEAVES if k in inp}
    pxyz, pcov, tf = ops.lbs_cov(leaf["xyz"], leaf["log_scale"], leaf["rot"], leaf.get("w"), _dev(inp["T"]) if B else None, tf44=tf44)
    assert pxyz.shape == (P, N, 3) and pcov.shape == (P, N, 6) and tf.shape == ((P, N, 4, 4) if tf44 else (P, N, 12))
    rows = tf[:, :, :3, :] if tf44 else tf.reshape(P, N, 3, 4)
    loss = (pxyz * _dev(inp["r_xyz"])).sum() + (pcov * _dev(inp["r_cov"]) * 1e3).sum()
    if tf_loss:
        loss = loss + (rows * _dev(inp["r_tf"])).sum()
    loss.backward()
    out = dict(posed_xyz=pxyz.detach().cpu(), posed_cov=pcov.detach().cpu(), tf=rows.detach().cpu(), tf_raw=tf.detach().cpu())
    out.update({"d_" + k: v.grad.cpu() for k, v in leaf.items()})
    return out


def per_row(x, lead):
    """(lead, N, ...) -> (lead * N, ...): a row of `row_rel_err` is one Gaussian of one pose / view."""
    return x.reshape((-1,) + tuple(x.shape[2:])) if lead else x


@pytest.mark.parametrize("B,P,N,tf44,tf_loss", LBS_CASES)
def test_lbs_over_bones_poses_ragged_sizes_vs_fp64(B, P, N, tf44, tf_loss):
    """ops.lbs_cov (k_lbs_fwd / k_lbs_bwd) against tr.lbs_forward in fp64: general affine transforms, skin rows with exact
    zeros, quaternion norms over four decades (dL/drot rows then differ by 1e4), log-scales in [-9,-2]; dL_dtf given and
    NULL; (N,12) and (N,4,4) transform rows; the static path (B = 0 here: skin_w = None)."""
    inp = lbs_inputs(B, P, N)
    o64, o32 = lbs_oracle(inp, F64, tf_loss), lbs_oracle(inp, F32, tf_loss)
    k = lbs_kernel(inp, tf44, tf_loss)
    tag = "lbs B=%d P=%d N=%d %s%s " % (B, P, N, "4x4" if tf44 else "12", " +tf" if tf_loss else "")
    names = ["posed_xyz", "posed_cov"] + (["tf"] if B else [])
    for n in names:
        check_rows(tag + n, per_row(k[n], True), per_row(o64[n], True), per_row(o32[n], True))
    for n in ["d_xyz", "d_log_scale", "d_rot"] + (["d_w"] if B else []):
        check_rows(tag + n, k[n], o64[n], o32[n])
    if tf44:   # the constant last row is written by the kernel
        assert torch.equal(k["tf_raw"][:, :, 3, :], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(P, N, 4))
    if not B:  # identity transform: the means pass through, bit for bit
        assert torch.equal(k["posed_xyz"], inp["xyz"].to(F32).expand(P, N, 3))


# =================================================================================================================
# 3. SH colour over views and strides, and the clamp
# =================================================================================================================
SH_VIEWS, SH_NS, SH_TF = (1, 3, 9), (1, 257, 777), ("none", "N12", "VN12", "VN44")
SH_CASES = [(V, SH_NS[(iv + ix + it) % 3], per_view_xyz, tfk)
            for iv, V in enumerate(SH_VIEWS) for ix, per_view_xyz in enumerate((False, True)) for it, tfk in enumerate(SH_TF)]
KINK = 1e-4
SAFE = 1e-3            # rgb + 0.5 < -SAFE in fp64: clamped in fp32 too (colour magnitudes are O(1): 1e-3 is 1e4 fp32 ulps)


def sh_inputs(V, N, per_view_xyz, tfk, seed=0):
    g = torch.Generator().manual_seed(5000 + 97 * V + N + 7 * SH_TF.index(tfk) + int(per_view_xyz) + seed)
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)
    ru = lambda *s: torch.rand(s, generator=g, dtype=F64)
    sh = torch.cat([1.5 * rn(N, 1, 3) - 0.6, 0.2 * rn(N, 15, 3)], 1)
    dark = torch.arange(N) % 16 == 5                                 # Gaussians clamped in all channels of all views
    sh[dark, 0, :] = -10.0
    xyz = 0.1 * rn(*((V, N, 3) if per_view_xyz else (N, 3)))
    d = rn(V, 3)
    cam = d / d.norm(dim=1, keepdim=True) * 10.0 ** torch.linspace(-2.0, 2.0, V, dtype=F64)[:, None] if V > 1 else \
        d / d.norm(dim=1, keepdim=True) * 1e-2
    inp = dict(V=V, N=N, tfk=tfk, per_view_xyz=per_view_xyz, sh=rounded(sh), xyz=rounded(xyz), cam=rounded(cam),
               r_col=rounded(rn(V, N, 3)), dark=dark)
    if tfk != "none":
        shape = (N,) if tfk == "N12" else (V, N)
        A = torch.eye(3, dtype=F64).expand(shape + (3, 3)) + 0.3 * rn(*shape, 3, 3)
        det = torch.linalg.det(A)
        A = torch.where((det.abs() < 0.2)[..., None, None], torch.eye(3, dtype=F64).expand_as(A), A)   # invertible, well away from singular
        flip = ru(*shape) < 0.5
        A[..., 0, :] = torch.where(flip[..., None], -A[..., 0, :], A[..., 0, :])                       # determinants of both signs
        inp["tf"] = rounded(torch.cat([A, 0.1 * rn(*shape, 3, 1)], -1))                                 # (.., 3, 4)
    return inp


def sh_oracle(inp, dtype):
    """colours (V,N,3) pre- and post-clamp, dL/dsh, dL/dxyz, dL/dtf (3x4 rows; the constant last row is no leaf) of
    tr.sh_colors looped over the views."""
    V, N = inp["V"], inp["N"]
    sh = inp["sh"].to(dtype).clone().requires_grad_(True)
    xyz = inp["xyz"].to(dtype).clone().requires_grad_(True)
    tf = inp["tf"].to(dtype).clone().requires_grad_(True) if "tf" in inp else None
    last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=dtype).expand(N, 1, 4)
    cols, loss = [], 0
    for v in range(V):
        xv = xyz[v] if inp["per_view_xyz"] else xyz
        t44 = None
        if tf is not None:
            t44 = torch.cat([tf[v] if tf.dim() == 4 else tf, last], 1)
        c = tr.sh_colors(xv, sh, xv, inp["cam"][v].to(dtype), 3, t44)
        cols.append(c)
        loss = loss + (c * inp["r_col"][v].to(dtype)).sum()
    loss.backward()
    out = dict(colors=torch.stack(cols).detach(), d_sh=sh.grad.detach(), d_xyz=xyz.grad.detach())
    if tf is not None:
        out["d_tf"] = tf.grad.detach()
    return out


def sh_preclamp(inp):
    """fp64 rgb + 0.5 before the clamp, (V,N,3)."""
    pre = []
    last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=F64).expand(inp["N"], 1, 4)
    for v in range(inp["V"]):
        xv = inp["xyz"][v] if inp["per_view_xyz"] else inp["xyz"]
        if "tf" in inp:
            t = inp["tf"][v] if inp["tf"].dim() == 4 else inp["tf"]
            cam_h = torch.nn.functional.pad(inp["cam"][v].reshape(1, 3).expand(inp["N"], 3), (0, 1), value=1.0)
            d = xv - torch.einsum("nij,nj->ni", torch.linalg.inv(torch.cat([t, last], 1)), cam_h)[:, :3]
        else:
            d = xv - inp["cam"][v]
        d = d / d.norm(dim=1, keepdim=True)
        pre.append(tr.eval_sh(3, inp["sh"].transpose(1, 2), d) + 0.5)
    return torch.stack(pre)


def sh_reference(V, N, per_view_xyz, tfk):
    inp = sh_inputs(V, N, per_view_xyz, tfk)
    o64, o32 = sh_oracle(inp, F64), sh_oracle(inp, F32)
    pre = sh_preclamp(inp)
    assert torch.equal(pre.clamp_min(0.0), o64["colors"]) or float((pre.clamp_min(0.0) - o64["colors"]).abs().max()) < 1e-12
    kink = pre.abs() < KINK                         # (V,N,3) channels on the kink: left out
    kv = kink.any(2)                                # (V,N)
    return dict(inp=inp, o64=o64, o32=o32, pre=pre, clamped_share=float((pre < 0).double().mean()),
                kink=kink, kink_share=float(kink.double().mean()), rows_vn=~kv, rows_n=~kv.any(0),
                all_dark=(pre < -SAFE).all(2).all(0))


def assert_sh_caps(ref):
    if ref["inp"]["N"] > 1:    # (one Gaussian has three channels per view: its share is whatever the draw gave)
        assert 0.10 <= ref["clamped_share"] <= 0.50, ref["clamped_share"]
        assert int(ref["all_dark"].sum()) >= ref["inp"]["N"] // 16
    assert ref["kink_share"] <= 0.01, ref["kink_share"]


def sh_kernel(inp, tf44_layout=None, expand_shared=False):
    """ops.sh_colors forward + backward.  expand_shared: the shared xyz / tf passed as per-view copies (their gradients then
    come back per view)."""
    from manus_amd import ops
    V, N, tfk = inp["V"], inp["N"], inp["tfk"]
    cams = torch.zeros((V, 40), dtype=F32, device=DEV)
    cams[:, 34:37] = _dev(inp["cam"])
    sh = _dev(inp["sh"]).requires_grad_(True)
    x = inp["xyz"]
    if expand_shared and x.dim() == 2:
        x = x.expand(V, N, 3)
    xyz = _dev(x).requires_grad_(True)
    tf = None
    if tfk != "none":
        t = inp["tf"]
        if expand_shared and t.dim() == 3:
            t = t.expand(V, N, 3, 4)
        if tfk == "VN44":
            t = torch.cat([t, torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=F64).expand(V, N, 1, 4)], 2)     # (V,N,4,4)
        else:
            t = t.reshape(t.shape[:-2] + (12,))
        tf = _dev(t).requires_grad_(True)
    col = ops.sh_colors(sh, xyz, tf, cams)
    assert col.shape == (V, N, 3)
    (col * _dev(inp["r_col"])).sum().backward()
    out = dict(colors=col.detach().cpu(), d_sh=sh.grad.cpu(), d_xyz=xyz.grad.cpu())
    if tf is not None:
        gt = tf.grad.cpu()
        if tfk == "VN44":
            out["d_tf_last"] = gt[:, :, 3, :]
            gt = gt[:, :, :3, :]
        out["d_tf"] = gt.reshape(gt.shape[:-1] + (3, 4)) if tfk != "VN44" else gt
    return out


@pytest.mark.parametrize("V,N,per_view_xyz,tfk", SH_CASES)
def test_sh_colour_over_views_strides_and_the_clamp_vs_fp64(V, N, per_view_xyz, tfk):
    """ops.sh_colors (k_sh_fwd / k_sh_bwd) against tr.sh_colors in fp64: shared and per-view xyz, tf absent / (N,12) /
    (V,N,12) / (V,N,4,4), camera distances 1e-2 .. 1e2, transforms with determinants of both signs; 10-50 % of the colour
    channels clamped; exact zeros behind the clamp and in the last row of a 4x4 dL/dtf."""
    ref = sh_reference(V, N, per_view_xyz, tfk)
    assert_sh_caps(ref)
    inp, o64, o32 = ref["inp"], ref["o64"], ref["o32"]
    k = sh_kernel(inp)
    tag = "sh V=%d N=%d xyz=%s tf=%s " % (V, N, "VN3" if per_view_xyz else "N3", tfk)
    keep = (~ref["kink"]).double()                  # channels on the kink are left out of the colour comparison
    check_rows(tag + "colors", per_row(k["colors"].double() * keep, True), per_row(o64["colors"] * keep, True),
               per_row(o32["colors"].double() * keep, True))
    check_rows(tag + "d_sh", k["d_sh"], o64["d_sh"], o32["d_sh"], ref["rows_n"])
    check_rows(tag + "d_xyz", per_row(k["d_xyz"], per_view_xyz), per_row(o64["d_xyz"], per_view_xyz), per_row(o32["d_xyz"], per_view_xyz),
               ref["rows_vn"] if per_view_xyz else ref["rows_n"])
    if tfk != "none":
        pv = tfk != "N12"
        assert k["d_tf"].shape == o64["d_tf"].shape
        check_rows(tag + "d_tf", per_row(k["d_tf"], pv), per_row(o64["d_tf"], pv), per_row(o32["d_tf"], pv), ref["rows_vn"] if pv else ref["rows_n"])
    if tfk == "VN44":
        assert float(k["d_tf_last"].abs().max()) == 0.0
    dark = ref["all_dark"]          # every channel of every view clamped, safely: no gradient at all, exactly
    if dark.any():
        assert float(k["colors"][:, dark].abs().max()) == 0.0
        assert float(k["d_sh"][dark].abs().max()) == 0.0
        assert float((k["d_xyz"][:, dark] if per_view_xyz else k["d_xyz"][dark]).abs().max()) == 0.0
        if tfk != "none":
            assert float((k["d_tf"][dark] if tfk == "N12" else k["d_tf"][:, dark]).abs().max()) == 0.0
    # the shared-layout gradients are the per-view ones summed
    if not per_view_xyz or tfk == "N12":
        e = sh_kernel(inp, expand_shared=True)
        assert torch.equal(e["colors"], k["colors"])
        for name, shared in (("d_xyz", not per_view_xyz), ("d_tf", tfk == "N12")):
            if shared:
                rows = ref["rows_n"]
                err = row_rel_err(k[name][rows], e[name].double().sum(0)[rows])
                e32 = row_rel_err(o32[name][rows], o64[name][rows])
                assert err <= bound_of(e32), (name, err, e32)


# =================================================================================================================
# 4. the fused step at other bone counts
# =================================================================================================================
_SCENES = {}


def retargeted_scene(B2, views, kind="hand", n=3000, device=DEV):
    """make_scene(kind) with its 21 transforms re-targeted to B2: grid' = grid @ M with a fixed seeded non-negative (21,B2)
    matrix without a zero row (a voxel has weight exactly where it had weight), transforms'[v,b] = transforms[v, b % 21]
    composed with a small seeded rigid perturbation.  The size of tests/test_gpu_fused.py: 96 x 64, grid_res 24."""
    key = (B2, views, kind, n, str(device))
    if key in _SCENES:
        return _SCENES[key]
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=n, kind=kind, seed=6, grid_res=24, n_cameras=views, width=96, height=64, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device="cpu")
    g = torch.Generator().manual_seed(400 + B2)
    M = torch.rand((21, B2), generator=g) ** 2
    M[torch.rand((21, B2), generator=g) < 0.4] = 0.0
    M[torch.arange(21), torch.arange(21) % B2] += 0.5
    assert bool((M >= 0).all()) and bool((M.sum(1) > 0).all())
    grid2 = (sc["grid"].double() @ M.double()).float()
    assert torch.equal(grid2.sum(-1) > 0, sc["grid"].sum(-1) > 0)
    ax = torch.randn((B2, 3), generator=g)
    ang = 0.02 * torch.randn((B2,), generator=g)
    ax = ax / ax.norm(dim=1, keepdim=True)
    Kx = torch.zeros((B2, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    R = torch.eye(3)[None] + torch.sin(ang)[:, None, None] * Kx + (1 - torch.cos(ang))[:, None, None] * (Kx @ Kx)    # Rodrigues
    E = torch.eye(4).repeat(B2, 1, 1)
    E[:, :3, :3] = R
    E[:, :3, 3] = 1e-3 * torch.randn((B2, 3), generator=g)
    T2 = (sc["transforms"][:, torch.arange(B2) % 21] @ E[None]).contiguous()
    out = dict(sc, grid=grid2, transforms=T2)
    dev = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in out.items() if k != "params"}
    dev["params"] = {k: v.to(device) for k, v in out["params"].items()}
    _SCENES[key] = (dev, camera_table(sc["cameras"], device), out)
    return _SCENES[key]


def _targets(views, seed):
    return torch.rand((views, 3, 64, 96), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


FUSED_CASES = [("hand", B2, v) for B2 in (8, 24, 25, 32) for v in (3, 8)] + [("composite", 25, 3)]


@pytest.mark.parametrize("kind,B2,views", FUSED_CASES)
def test_fused_equals_modular_at_other_bone_counts(kind, B2, views):
    """HipViewCompute(fused=True) against fused=False on a scene re-targeted to B' transforms, under the assertions -- and
    the thresholds, verbatim -- of tests/test_gpu_fused.py::test_fused_equals_modular (k_inst_bwd_runs for B' <= 24,
    k_inst_bwd<., MGR_MAX_BONES, ..> above; 3 views = lane groups of 4, 8 views = lane groups of 8)."""
    from manus_amd.engine import HipViewCompute
    sc, ct, _ = retargeted_scene(B2, views, kind)
    tg = _targets(views, 11)
    ids = list(range(views))
    mod = HipViewCompute(sc, tg, ct, fused=False)
    fus = HipViewCompute(sc, tg, ct, fused=True)
    with torch.no_grad():
        im_m, rad_m, _ = mod.forward_views(ids)
        im_f, rad_f = fus.forward_views_fused(ids)
    assert torch.equal(rad_m, rad_f)
    d = (im_m - im_f).abs()
    assert float(d.max()) < 5e-3 and float(d.mean()) < 2e-6
    om, of = mod(ids, 1.0 / views), fus(ids, 1.0 / views)
    assert abs(float(om["loss"]) - float(of["loss"])) < 1e-6
    for k in om["grads"]:
        a, b = of["grads"][k].cpu().numpy().astype(np.float64), om["grads"][k].cpu().numpy().astype(np.float64)
        assert a.shape == b.shape, k
        assert max_rel_err(a, b) < 5e-3, (k, max_rel_err(a, b))
        rows = np.abs(a - b).reshape(a.shape[0], -1).max(1) > 2e-5 * np.abs(b).max()
        assert rows.mean() < 0.03, (k, rows.sum())
    assert torch.equal(of["vis"], om["vis"])
    assert torch.equal(of["radii"].to(torch.int32), om["radii"].to(torch.int32))
    assert max_rel_err(of["grad2d"].cpu().numpy(), om["grad2d"].cpu().numpy()) < 5e-3


@pytest.mark.parametrize("kind,B2,views", FUSED_CASES)
def test_run_lists_at_other_bone_counts(kind, B2, views):
    """B' <= 24: run lists on against off under the assertions -- and thresholds, verbatim -- of
    tests/test_gpu_fused.py::test_run_lists_equal_one_lane_per_view.  B' > 24: the run lists are off either way (up to 24
    transforms), so the two settings are bit-identical."""
    from manus_amd._lib import lib
    from manus_amd.engine import HipViewCompute
    from util import keep
    sc, ct, _ = retargeted_scene(B2, views, kind)
    tg = _targets(views, views)
    ids = list(range(views))
    hc = HipViewCompute(sc, tg, ct, fused=True)
    prev = lib().mgr_views_backward_run_lists(1)
    try:
        on1 = keep(hc(ids, 1.0 / views))
        on2 = keep(hc(ids, 1.0 / views))
        assert lib().mgr_views_backward_run_lists(0) == 1
        off = keep(hc(ids, 1.0 / views))
    finally:
        lib().mgr_views_backward_run_lists(prev)
    assert float(on1["grads"]["_xyz"].abs().sum()) > 0
    if B2 > 24:
        for k in on1["grads"]:
            assert torch.equal(on1["grads"][k], off["grads"][k]), k
        assert torch.equal(on1["grad2d"], off["grad2d"]) and torch.equal(on1["vis"], off["vis"]) and torch.equal(on1["radii"], off["radii"])
        return
    for k in on1["grads"]:
        assert torch.equal(on1["grads"][k], on2["grads"][k]), k
        a, b = on1["grads"][k].double(), off["grads"][k].double()
        assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-30), (k, float((a - b).abs().max()), float(b.abs().max()))
        assert torch.equal(a.reshape(a.shape[0], -1).abs().sum(1) == 0, b.reshape(b.shape[0], -1).abs().sum(1) == 0), k
    assert torch.equal(on1["vis"], off["vis"]) and torch.equal(on1["radii"], off["radii"])
    assert float((on1["grad2d"].double() - off["grad2d"].double()).abs().max()) <= 1e-5 * float(off["grad2d"].abs().max())
    assert abs(float(on1["loss"]) - float(off["loss"])) < 1e-6


def retargeted_oracle(scene_cpu, dtype, view=0):
    """tr.hand_forward on the re-targeted scene: its transforms enter as `posed` with identity rest matrices; the
    background transform hand_forward appends meets an extra all-zero grid channel (weight exactly 0)."""
    B2 = scene_cpu["transforms"].shape[1]
    grid = torch.cat([scene_cpu["grid"], torch.zeros_like(scene_cpu["grid"][..., :1])], -1).to(dtype)
    par = {k: v.to(dtype) for k, v in scene_cpu["params"].items()}
    cc = torch.tensor(np.asarray(scene_cpu["cameras"][view]["camera_center"], np.float32)).to(dtype)
    o = tr.hand_forward(par, grid, scene_cpu["grid_center"].to(dtype), scene_cpu["grid_scale"].to(dtype),
                        scene_cpu["transforms"][view].to(dtype), torch.eye(4, dtype=dtype).repeat(B2, 1, 1), cc)
    return {k: o[k] for k in ("posed_xyz", "posed_cov", "colors")}


@pytest.mark.parametrize("B2", [8, 24, 25, 32])
def test_retargeted_scene_vs_fp64_oracle(B2):
    """Ties the inputs of the two tests above to the reference, not only to each other: skin weights from the re-targeted
    grid -> LBS -> SH colour through the operators, against tr.hand_forward in fp64."""
    from manus_amd import ops
    sc, ct, cpu = retargeted_scene(B2, 3)
    o64, o32 = retargeted_oracle(cpu, F64), retargeted_oracle(cpu, F32)
    p = sc["params"]
    with torch.no_grad():
        w = ops.skin_weights(p["_xyz"], sc["grid"], sc["grid_center"], sc["grid_scale"])
        pxyz, pcov, tf = ops.lbs_cov(p["_xyz"], p["_scaling"], p["_rotation"], w, sc["transforms"][:1])
        col = ops.sh_colors(torch.cat([p["_features_dc"], p["_features_rest"]], 1), p["_xyz"], tf, ct[:1])
    assert w.shape[1] == B2 and bool(torch.isfinite(w).all())
    check_rows("retarget B'=%d posed_xyz" % B2, pxyz[0], o64["posed_xyz"], o32["posed_xyz"])
    check_rows("retarget B'=%d posed_cov" % B2, pcov[0], o64["posed_cov"], o32["posed_cov"])
    band = (o64["colors"] > 0) & (o64["colors"] < KINK)   # channels on the kink of the clamp: left out, at most 1 %
    assert float(band.double().mean()) <= 0.01
    keep_ch = (~band).double()
    check_rows("retarget B'=%d colors" % B2, col[0].cpu().double() * keep_ch, o64["colors"] * keep_ch, o32["colors"].double() * keep_ch)


# =================================================================================================================
# reference-only report (no GPU): caps and e32 per tensor
# =================================================================================================================
def cpu_report():
    print("section 1: skin weights, N = %d, grid %s" % (SKIN_N, SKIN_DIMS))
    for B in SKIN_BONES:
        r = skin_reference(B)
        assert_skin_caps(r)
        print("  B=%2d  NaN rows %2d  padded-corner rows %.1f %%  left out: small S %.1f %% (%d), near node %.1f %%  fwd-only kept %d/14"
              "  e32 weights %.2e  dL/dxyz %.2e  fwd-only %.2e"
              % (B, int(r["nan_rows"].sum()), 100 * r["padded_rows"], 100 * r["share_small"], round(r["share_small"] * float(r["fin"].sum())),
                 100 * r["share_near"], int(r["fwd_rows"].sum()), row_rel_err(r["w32"][r["fin"]], r["w64"][r["fin"]]),
                 row_rel_err(r["g32"][r["grad_rows"]], r["g64"][r["grad_rows"]]),
                 row_rel_err(r["wf32"][r["fwd_rows"]], r["wf64"][r["fwd_rows"]])))
    print("section 2: LBS")
    for B, P, N, tf44, tf_loss in LBS_CASES:
        inp = lbs_inputs(B, P, N)
        o64, o32 = lbs_oracle(inp, F64, tf_loss), lbs_oracle(inp, F32, tf_loss)
        print("  B=%2d P=%d N=%3d tf_loss=%d  e32: %s" % (B, P, N, tf_loss, "  ".join(
            "%s %.1e" % (k, row_rel_err(per_row(o32[k], not k.startswith("d_")), per_row(o64[k], not k.startswith("d_")))) for k in o64)))
    print("section 3: SH colour")
    for V, N, pv, tfk in SH_CASES:
        r = sh_reference(V, N, pv, tfk)
        assert_sh_caps(r)
        tail = lambda k, x: x.reshape((-1,) + tuple(x.shape[-2:] if k in ("d_tf", "d_sh") else x.shape[-1:]))
        print("  V=%d N=%3d xyz=%s tf=%-4s  clamped %.1f %%  kink band %.3f %%  all-dark Gaussians %d  e32: %s"
              % (V, N, "VN3" if pv else "N3 ", tfk, 100 * r["clamped_share"], 100 * r["kink_share"], int(r["all_dark"].sum()),
                 "  ".join("%s %.1e" % (k, row_rel_err(tail(k, r["o32"][k]), tail(k, r["o64"][k]))) for k in r["o64"])))
    print("section 4: re-targeted scene (forward chain)")
    for B2 in (8, 24, 25, 32):
        _, _, cpu = retargeted_scene(B2, 3, device="cpu")
        o64, o32 = retargeted_oracle(cpu, F64), retargeted_oracle(cpu, F32)
        band = ((o64["colors"] < KINK) & (o64["colors"] > 0)).double().mean()
        assert float(band) <= 0.01
        print("  B'=%2d  kink band %.3f %%  e32: %s" % (B2, 100 * float(band), "  ".join("%s %.1e" % (k, row_rel_err(o32[k], o64[k])) for k in o64)))


if __name__ == "__main__":
    cpu_report()

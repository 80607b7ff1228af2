"""GPU: the skin-weight grid gradient (`mgr_skin_grid_bwd`: sparse dL/d(grid)), its Python surface (`ops.skin_grid_grad`,
autograd through `ops.skin_weights`, `HipViewCompute(skin_grid_grad=True)`) and the row Adam (`mgr_skin_grid_adam`,
`optim.SkinGridAdam`).

Reference: oracle/torch_ref.skin_weights_from_grid with a grid that requires grad, evaluated in float64 on the CPU.  Norm and
tolerance are those of tests/test_gpu_articulation_edges.py, copied from there: `util.row_rel_err` -- here over VOXEL rows, the
(D*H*W, B) view of the gradient -- against the fp64 oracle, and  e_kernel <= 8 * max(e32, 2^-23)  with e32 the same oracle
evaluated in float32 on the CPU (measured, not fixed; every ratio is printed before it is asserted).  Inputs follow that file's
recipe (grid (5,6,7), N = 777 points uniform in u in [-1.15, 1.15]^3, drawn in fp64 and rounded once), with strictly positive
grid values so that no raw sum S is tiny.  Gaussians left out of a comparison (small S, within 1e-4 index units of a node
plane, where the fp32 and the fp64 cell may differ) are left out through the `index` list, never by masking rows; their share
is capped at 10 % (checked in tests/test_skin_grid_grad_cpu.py and by `python tests/test_gpu_skin_grid_grad.py`, which needs no
GPU).  The fused-vs-operator bar of section 8 is that of tests/test_gpu_fused.py, taken verbatim and named there."""
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
FACTOR = 8.0          # three bits over the fp32 oracle's own error (tests/test_gpu_articulation_edges.py)
F32, F64 = torch.float32, torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SKIN_DIMS = (5, 6, 7)                 # (D,H,W)
SKIN_BONES = (1, 3, 8, 20, 21, 24, 25, 32)
SKIN_N = 777
S_FLOOR = 1e-2                        # rows whose raw sum is below S_FLOOR * max S are ill-conditioned in any precision
NODE_BAND = 1e-4                      # (index units) the fp32 and the fp64 cell index may differ this close to a node plane
LEFT_OUT_CAP = 0.10


def rounded(x):
    """fp64 tensor whose values are exactly representable in fp32 (drawn in fp64, rounded once)."""
    return x.to(F32).to(F64)


def bound_of(e32):
    return FACTOR * max(e32, EPS32)


def check_rows(tag, got, ref64, ref32):
    """The one tolerance of this file (tests/test_gpu_articulation_edges.py: check_rows): e_kernel <= 8 * max(e32, 2^-23), both
    in `row_rel_err` against the fp64 oracle, over the rows of the first axis.  Prints the figures before it asserts."""
    got, ref64, ref32 = (x.detach().cpu().double() for x in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    e32, ek = row_rel_err(ref32, ref64), row_rel_err(got, ref64)
    ratio = ek / max(e32, EPS32)
    print("RATIO %-52s e_kernel %.3e  e32 %.3e  ratio %.2f" % (tag, ek, e32, ratio))
    assert ek <= bound_of(e32), "%s: e_kernel %.3e  e32 %.3e  ratio %.2f > %g" % (tag, ek, e32, ratio, FACTOR)
    return ek, e32


def vox_rows(g):
    """(D,H,W,B) -> (D*H*W, B): one row per voxel."""
    return g.reshape(-1, g.shape[-1])


# =================================================================================================================
# inputs and the CPU oracle (no GPU)
# =================================================================================================================
def grid_inputs(B, dims=SKIN_DIMS, n=SKIN_N, seed=0, half=1.15, unit_box=False):
    """Grid 0.05 + rand**3 (strictly positive); n points uniform in u in [-half, half]^3; a random dL/dw."""
    g = torch.Generator().manual_seed(9100 + 37 * B + seed)
    D, H, W = dims
    grid = 0.05 + torch.rand((D, H, W, B), generator=g, dtype=F64) ** 3
    if unit_box:
        center, scale = torch.zeros(3, dtype=F64), torch.ones(3, dtype=F64)
    else:
        center, scale = rounded(torch.tensor([0.01, -0.02, 0.03], dtype=F64)), rounded(torch.tensor([0.5, 0.4, 0.3], dtype=F64))
    u = torch.rand((n, 3), generator=g, dtype=F64) * (2.0 * half) - half
    return dict(B=B, dims=dims, grid=rounded(grid), center=center, scale=scale, xyz=rounded(u * scale + center),
                g_w=rounded(torch.randn((n, B), generator=g, dtype=F64)))


def raw_sum(inp):
    """fp64 raw sum S of the sampled channels; the distance of every sample from the nearest node plane in index units; the
    fp64 index-space position (N,3) in (x,y,z) order."""
    D, H, W = inp["dims"]
    grid = inp["grid"]
    u = ((inp["xyz"] - inp["center"]) / inp["scale"]).reshape(1, -1, 1, 1, 3)
    raw = torch.nn.functional.grid_sample(grid.permute(3, 0, 1, 2).unsqueeze(0), u, mode="bilinear", padding_mode="zeros",
                                          align_corners=True).reshape(grid.shape[3], -1).T
    idx = (u.reshape(-1, 3) + 1.0) * 0.5 * torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=F64)
    return raw.sum(1), (idx - idx.round()).abs().min(1).values, idx


def kept_rows(inp):
    """(indices of the Gaussians that take part in a comparison, share left out for a small S, share left out near a node)."""
    S, node_dist, _ = raw_sum(inp)
    small = S < S_FLOOR * S.max()
    near = node_dist < NODE_BAND
    keep = torch.nonzero(~small & ~near).reshape(-1)
    n = float(S.numel())
    return keep, float(small.sum()) / n, float(near.sum()) / n


def grid_oracle(inp, dtype, rows=None):
    """dL/d(grid) (D,H,W,B) of tr.skin_weights_from_grid in `dtype` on the CPU for the Gaussians `rows` (None: all)."""
    grid = inp["grid"].to(dtype).clone().requires_grad_(True)
    xyz, g_w = (inp["xyz"], inp["g_w"]) if rows is None else (inp["xyz"][rows], inp["g_w"][rows])
    if xyz.shape[0] == 0:
        return torch.zeros_like(grid)
    w = tr.skin_weights_from_grid(xyz.to(dtype), inp["center"].to(dtype), inp["scale"].to(dtype), grid)
    w.backward(g_w.to(dtype))
    return grid.grad.detach()


def closed_form(inp, rows=None, skip=True):
    """The definition of include/manus_hip.h restated as a loop, in fp64: (dense gradient, set of listed voxels)."""
    D, H, W = inp["dims"]
    B = inp["B"]
    grid = inp["grid"].numpy()
    G = np.zeros((D * H * W, B))
    listed = set()
    _, _, idx = raw_sum(inp)
    idx = idx.numpy()
    a_all = inp["g_w"].numpy()
    for n in (range(idx.shape[0]) if rows is None else [int(r) for r in rows]):
        base = np.floor(idx[n]).astype(int)
        f = idx[n] - base
        cs = []
        for k in range(8):
            x, y, z = base[0] + (k & 1), base[1] + ((k >> 1) & 1), base[2] + (k >> 2)
            t = (f[0] if k & 1 else 1 - f[0]) * (f[1] if k & 2 else 1 - f[1]) * (f[2] if k & 4 else 1 - f[2])
            if 0 <= x < W and 0 <= y < H and 0 <= z < D:
                cs.append(((z * H + y) * W + x, t))
        s = sum(t * grid.reshape(-1, B)[v] for v, t in cs) if cs else np.zeros(B)
        S = s.sum()
        if skip and (S == 0 or not np.isfinite(S)):
            continue
        with np.errstate(all="ignore"):
            w = s / S
            r = (a_all[n] - (a_all[n] * w).sum()) / S
        for v, t in cs:
            G[v] += t * r
            listed.add(v)
    return torch.from_numpy(G.reshape(D, H, W, B)), listed


_REF = {}


def parity_reference(B):
    """Both oracles over the kept Gaussians of `grid_inputs(B)`, once per B."""
    if B not in _REF:
        inp = grid_inputs(B)
        keep, share_small, share_near = kept_rows(inp)
        g64, g32 = grid_oracle(inp, F64, keep), grid_oracle(inp, F32, keep)
        if B == 1:
            # one channel: w = 1 wherever it is finite, so r and the whole gradient are identically zero and what any precision
            # returns is rounding noise.  The reference is the exact zero; `row_rel_err` then measures absolute errors, and the
            # kernel's noise is held against the fp32 oracle's by the same factor (tests/test_gpu_articulation_edges.py does
            # the same for dL/dxyz).
            assert float(g64.abs().max()) < 1e-9
            g64 = torch.zeros_like(g64)
        _REF[B] = dict(inp=inp, keep=keep, share_small=share_small, share_near=share_near, g64=g64, g32=g32)
    return _REF[B]


def assert_caps(ref):
    assert ref["share_small"] + ref["share_near"] <= LEFT_OUT_CAP, (ref["share_small"], ref["share_near"])


def border_inputs(B=21):
    """Unit box (u = xyz): 20 points outside each of the six faces with some corners padded, 150 inside, and points exactly on
    nodes -- ix = W-1, iy = H-1 and iz = D-1 among them (u = +-1 and the node coordinates of D = 5 are exact in fp32)."""
    inp = grid_inputs(B, n=150, seed=3, half=0.9, unit_box=True)
    g = torch.Generator().manual_seed(411)
    D, H, W = inp["dims"]
    parts = [inp["xyz"]]
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = torch.rand((20, 3), generator=g, dtype=F64) * 1.8 - 0.9
            p[:, axis] = sign * (1.02 + 0.12 * torch.rand(20, generator=g, dtype=F64))
            parts.append(p)
    nodes = torch.tensor([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [1.0, 0.2, 0.0], [0.2, 1.0, -0.5], [0.3, -0.3, 1.0], [1.0, 1.0, 0.5],
                          [0.1, 0.7, 0.0], [-1.0, 0.4, 0.5]], dtype=F64)
    parts.append(nodes)
    inp["xyz"] = rounded(torch.cat(parts))
    inp["g_w"] = rounded(torch.randn((inp["xyz"].shape[0], B), generator=g, dtype=F64))
    inp["n_nodes"] = nodes.shape[0]
    return inp


def skip_inputs(B=21):
    """`grid_inputs` plus a cell of all-zero voxels holding three Gaussians and three Gaussians fully outside the grid: the six
    degenerate rows are the LAST six."""
    inp = grid_inputs(B, n=300, seed=5)
    D, H, W = inp["dims"]
    inp["grid"][1:3, 2:4, 2:4, :] = 0.0                       # the cell x, y in [2,3], z in [1,2]
    inside = raw_sum(inp)[0] > 0                              # (points the generator put into that cell are dropped: the six are the only degenerate ones)
    inp["xyz"], inp["g_w"] = inp["xyz"][inside], inp["g_w"][inside]
    idx_in = torch.tensor([[2.3, 2.6, 1.5], [2.5, 2.5, 1.2], [2.8, 2.1, 1.7]], dtype=F64)
    u_in = idx_in / torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=F64) * 2.0 - 1.0
    u_out = torch.tensor([[1.6, 0.0, 0.1], [0.2, -1.9, 0.3], [-0.4, 0.5, 1.8]], dtype=F64)
    g = torch.Generator().manual_seed(77)
    inp["xyz"] = rounded(torch.cat([inp["xyz"], torch.cat([u_in, u_out]) * inp["scale"] + inp["center"]]))
    inp["g_w"] = rounded(torch.cat([inp["g_w"], torch.randn((6, B), generator=g, dtype=F64)]))
    return inp


# -- section 10: recovery of a blended grid --------------------------------------------------------------------------
REC_STEPS, REC_LR, REC_N = 150, 0.01, 2000


def recovery_inputs():
    """(8,8,8,21) grid: softmax of -distance / 0.02 to the 20 bone mid-points of tests/golden/fk_novel_pose.npz, the 21st
    (background, identity transform) channel at a constant logit of -8; 2000 Gaussians inside the grid; the 4 poses of the
    fixture; the starting grid = every row blended 30 % towards uniform."""
    d = np.load(os.path.join(GOLDEN, "fk_novel_pose.npz"))
    heads, tails = torch.tensor(d["world_rest_heads"], dtype=F64), torch.tensor(d["world_rest_tails"], dtype=F64)
    mid = 0.5 * (heads + tails)
    pts = torch.cat([heads, tails])
    lo, hi = pts.min(0).values, pts.max(0).values
    center, scale = rounded(0.5 * (lo + hi)), rounded(0.6 * (hi - lo) + 0.01)
    R = 8
    ax = torch.linspace(-1.0, 1.0, R, dtype=F64)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    pos = torch.stack([xx, yy, zz], -1) * scale + center                       # (D,H,W,3)
    dist = (pos[..., None, :] - mid).norm(dim=-1)                              # (D,H,W,20)
    logits = torch.cat([-dist / 0.02, torch.full(dist.shape[:-1] + (1,), -8.0, dtype=F64)], -1)
    true = rounded(torch.softmax(logits, -1))
    start = rounded(0.7 * true + 0.3 / 21.0)
    g = torch.Generator().manual_seed(2024)
    xyz = rounded((torch.rand((REC_N, 3), generator=g, dtype=F64) * 1.8 - 0.9) * scale + center)
    T = torch.stack([tr.bone_transforms(torch.tensor(d["world_pose_matrixs"][p], dtype=F64), torch.tensor(d["world_rest_matrixs"], dtype=F64))
                     for p in range(4)])
    return dict(true=true, start=start, center=center, scale=scale, xyz=xyz, T=rounded(T))


def _posed_means(xyz, w, T):
    """(P,N,3) linear-blend-skinned means (oracle/torch_ref.lbs_forward's mean path for P poses)."""
    tf = torch.einsum("nb,pbij->pnij", w, T)
    return torch.einsum("pnij,nj->pni", tf[..., :3, :3], xyz) + tf[..., :3, 3]


_REC = {}


def recovery_reference():
    """The checker of section 10: the same loop on the CPU in fp64 (torch_ref + torch.optim.SparseAdam, clamped at 0 like
    `SkinGridAdam`).  Returns the inputs and rho_ref = final / initial loss."""
    if "r" in _REC:
        return _REC["r"]
    inp = recovery_inputs()
    xyz, c, s, T = inp["xyz"], inp["center"], inp["scale"], inp["T"]
    target = _posed_means(xyz, tr.skin_weights_from_grid(xyz, c, s, inp["true"]), T)
    p = inp["start"].reshape(-1, 21).clone().requires_grad_(True)
    opt = torch.optim.SparseAdam([p], lr=REC_LR)
    losses = []
    for _ in range(REC_STEPS + 1):
        p.grad = None
        loss = ((_posed_means(xyz, tr.skin_weights_from_grid(xyz, c, s, p.reshape(8, 8, 8, 21)), T) - target) ** 2).sum()
        losses.append(float(loss.detach()))
        if len(losses) == REC_STEPS + 1:
            break
        loss.backward()
        rows = torch.nonzero(p.grad.abs().sum(1) > 0).reshape(-1)
        p.grad = torch.sparse_coo_tensor(rows[None], p.grad[rows], p.shape)
        opt.step()
        with torch.no_grad():
            p.clamp_(min=0.0)
    _REC["r"] = dict(inp=inp, target=target, rho_ref=losses[-1] / losses[0], loss0=losses[0])
    return _REC["r"]


# =================================================================================================================
# GPU helpers
# =================================================================================================================
def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def _grid_on_device(inp, layout):
    """(grid tensor, grid_stride): `padded` = what ops.SkinGrid prepares (24-float rows for B <= 24, aligned); `generic` =
    grid_stride = B on a base 4 bytes off 16-byte alignment."""
    from manus_amd import ops
    if layout == "padded":
        sg = ops.SkinGrid(_dev(inp["grid"]), DEV)
        return sg.data, sg.stride
    buf = torch.empty(inp["grid"].numel() + 1, dtype=F32, device=DEV)
    grid = buf[1:].view(inp["grid"].shape)
    grid.copy_(inp["grid"])
    assert grid.data_ptr() % 16 == 4 and grid.is_contiguous()
    return grid, inp["B"]


SENT_V, SENT_G, SENT_C = -7, 123.0, 0x5A5A5A5A


def raw_call(inp, grid, stride, xyz=None, g_w=None, index=None, count=None, max_count=None, B=None, capacity=None, ws_bytes=None):
    """mgr_skin_grid_bwd through the C ABI on sentinel-filled outputs: (code, voxel, grad, count, capacity)."""
    from manus_amd._lib import lib, ptr, stream
    D, H, W = inp["dims"]
    B = inp["B"] if B is None else B
    xyz = _dev(inp["xyz"]) if xyz is None else xyz
    g_w = _dev(inp["g_w"]) if g_w is None else g_w
    N = xyz.shape[0]
    mc = (N if index is None else index.numel()) if max_count is None else max_count
    need = max(1, min(8 * max(mc, 0), D * H * W))
    cap = need if capacity is None else capacity
    voxel = torch.full((max(cap, need),), SENT_V, dtype=torch.int32, device=DEV)
    grad = torch.full((max(cap, need), max(stride, 1)), SENT_G, dtype=F32, device=DEV)
    cnt = torch.full((1,), SENT_C, dtype=torch.int32, device=DEV)
    nbytes = int(lib().mgr_skin_grid_bwd_workspace_bytes(D, H, W, max(mc, 0)))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    c, s = _dev(inp["center"]), _dev(inp["scale"])
    code = lib().mgr_skin_grid_bwd(N, ptr(xyz), ptr(grid), D, H, W, B, stride, ptr(c), ptr(s), ptr(g_w),
                                   ptr(index) if index is not None else None, ptr(count) if count is not None else None, mc,
                                   ptr(voxel), ptr(grad), ptr(cnt), cap, ptr(ws), nbytes if ws_bytes is None else ws_bytes, stream())
    torch.cuda.synchronize()
    return code, voxel, grad, cnt, need


def dense_of(inp, voxel, grad, cnt):
    from manus_amd import ops
    D, H, W = inp["dims"]
    return ops.SkinGridGrad(voxel, grad, cnt, (D, H, W, inp["B"])).to_dense()


def assert_list(inp, voxel, grad, cnt, n_processed, expect=None):
    """The list itself: ascending, unique, in bounds, count <= min(8 n, D*H*W), pad channels exactly zero, entries beyond the
    count untouched; expect: the exact set of listed voxels."""
    D, H, W = inp["dims"]
    n = int(cnt[0])
    assert 0 <= n <= min(8 * n_processed, D * H * W), n
    v = voxel[:n].cpu().numpy().astype(np.int64)
    assert np.all(np.diff(v) > 0) and (n == 0 or (v[0] >= 0 and v[-1] < D * H * W))
    assert bool((grad[:n, inp["B"]:] == 0).all())
    assert bool((voxel[n:] == SENT_V).all()) and bool((grad[n:] == SENT_G).all())
    if expect is not None:
        assert set(v.tolist()) == set(expect)
    return v


def int_index(rows, pad_to=None, fill=0):
    idx = torch.as_tensor(rows, dtype=torch.int64).to(torch.int32)
    if pad_to is not None and pad_to > idx.numel():
        idx = torch.cat([idx, torch.full((pad_to - idx.numel(),), fill, dtype=torch.int32)])
    return idx.to(DEV).contiguous()


def count_of(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


# =================================================================================================================
# 1. parity over the bone counts, both layouts
# =================================================================================================================
@pytest.mark.parametrize("layout", ["padded", "generic"])
@pytest.mark.parametrize("B", SKIN_BONES)
def test_parity_over_bone_counts(B, layout):
    ref = parity_reference(B)
    assert_caps(ref)
    inp, keep = ref["inp"], ref["keep"]
    grid, stride = _grid_on_device(inp, layout)
    _, listed = closed_form(inp, keep)
    # the kept Gaussians through the index list
    code, voxel, grad, cnt, _ = raw_call(inp, grid, stride, index=int_index(keep), count=count_of(keep.numel()))
    assert code == 0
    assert_list(inp, voxel, grad, cnt, keep.numel(), expect=listed)
    check_rows("grid grad B=%d %s indexed" % (B, layout), vox_rows(dense_of(inp, voxel, grad, cnt)), vox_rows(ref["g64"]), vox_rows(ref["g32"]))
    # the dense call on the same Gaussians
    code, voxel2, grad2, cnt2, _ = raw_call(inp, grid, stride, xyz=_dev(inp["xyz"][keep]), g_w=_dev(inp["g_w"][keep]))
    assert code == 0
    assert_list(inp, voxel2, grad2, cnt2, keep.numel(), expect=listed)
    check_rows("grid grad B=%d %s dense" % (B, layout), vox_rows(dense_of(inp, voxel2, grad2, cnt2)), vox_rows(ref["g64"]), vox_rows(ref["g32"]))


def test_ops_skin_grid_grad_surface():
    """`ops.skin_grid_grad` (index and dense) is the same call: rows(), to_dense(), shape."""
    from manus_amd import ops
    ref = parity_reference(21)
    inp, keep = ref["inp"], ref["keep"]
    sg = ops.SkinGrid(_dev(inp["grid"]), DEV)
    c, s = _dev(inp["center"]), _dev(inp["scale"])
    a = ops.skin_grid_grad(_dev(inp["xyz"]), sg, c, s, _dev(inp["g_w"]), index=int_index(keep))
    b = ops.skin_grid_grad(_dev(inp["xyz"][keep]), sg, c, s, _dev(inp["g_w"][keep]))
    assert a.shape == (5, 6, 7, 21) and a.to_dense().shape == (5, 6, 7, 21)
    (va, ga), (vb, gb) = a.rows(), b.rows()
    assert torch.equal(va, vb) and torch.equal(ga, gb) and ga.shape[1] == 24
    check_rows("ops.skin_grid_grad B=21", vox_rows(a.to_dense()), vox_rows(ref["g64"]), vox_rows(ref["g32"]))


# =================================================================================================================
# 2. ragged sizes and long segments
# =================================================================================================================
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("B,layout", [(21, "padded"), (25, "generic")])
def test_ragged_sizes(N, B, layout):
    inp = grid_inputs(B, n=N, seed=11 + N)
    keep, _, _ = kept_rows(inp)
    assert keep.numel() >= max(1, int(0.9 * N))
    g64, g32 = grid_oracle(inp, F64, keep), grid_oracle(inp, F32, keep)
    grid, stride = _grid_on_device(inp, layout)
    code, voxel, grad, cnt, _ = raw_call(inp, grid, stride, index=int_index(keep), count=count_of(keep.numel()))
    assert code == 0
    assert_list(inp, voxel, grad, cnt, keep.numel(), expect=closed_form(inp, keep)[1])
    check_rows("ragged N=%d B=%d %s" % (N, B, layout), vox_rows(dense_of(inp, voxel, grad, cnt)), vox_rows(g64), vox_rows(g32))


def long_segment_inputs():
    """2000 Gaussians inside the one cell of a 2x2x2 grid (u in [-0.99, 0.99]^3): eight voxels, 2000 contributors each."""
    return grid_inputs(21, dims=(2, 2, 2), n=2000, seed=21, half=0.99)


def test_long_segments_in_one_cell():
    inp = long_segment_inputs()
    keep, small, near = kept_rows(inp)
    assert small + near <= LEFT_OUT_CAP
    g64, g32 = grid_oracle(inp, F64, keep), grid_oracle(inp, F32, keep)
    grid, stride = _grid_on_device(inp, "padded")
    perm = keep[torch.randperm(keep.numel(), generator=torch.Generator().manual_seed(1))]
    outs = []
    for rows in (keep, perm):
        code, voxel, grad, cnt, _ = raw_call(inp, grid, stride, index=int_index(rows), count=count_of(rows.numel()))
        assert code == 0
        assert_list(inp, voxel, grad, cnt, rows.numel(), expect=range(8))
        outs.append((voxel, grad))
    check_rows("2000 in one cell", vox_rows(dense_of(inp, outs[0][0], outs[0][1], count_of(8))), vox_rows(g64), vox_rows(g32))
    assert torch.equal(outs[0][1], outs[1][1])      # the order of the list does not reach the sums


# =================================================================================================================
# 3. borders
# =================================================================================================================
@pytest.mark.parametrize("layout", ["padded", "generic"])
def test_borders_and_nodes(layout):
    inp = border_inputs()
    n_all = inp["xyz"].shape[0]
    keep, _, _ = kept_rows(inp)
    # the points ON nodes are the subject here: they stay in whatever their distance from a node plane (on a node the cells on
    # both sides give the same value: an fp32 cell index one lower moves weight ~1e-7 between neighbours)
    keep = torch.unique(torch.cat([keep, torch.arange(n_all - inp["n_nodes"], n_all)]))
    assert keep.numel() >= 0.9 * n_all
    g64, g32 = grid_oracle(inp, F64, keep), grid_oracle(inp, F32, keep)
    grid, stride = _grid_on_device(inp, layout)
    code, voxel, grad, cnt, _ = raw_call(inp, grid, stride, index=int_index(keep), count=count_of(keep.numel()))
    assert code == 0
    assert_list(inp, voxel, grad, cnt, keep.numel())       # (in bounds: no listed voxel is outside)
    # the exact list of the Gaussians off the node planes is a subset of what is listed
    off = keep[keep < n_all - inp["n_nodes"]]
    assert closed_form(inp, off)[1] <= set(voxel[:int(cnt[0])].cpu().tolist())
    check_rows("borders %s" % layout, vox_rows(dense_of(inp, voxel, grad, cnt)), vox_rows(g64), vox_rows(g32))


# =================================================================================================================
# 4. the skip rule
# =================================================================================================================
@pytest.mark.parametrize("layout", ["padded", "generic"])
def test_degenerate_gaussians_contribute_nothing(layout):
    inp = skip_inputs()
    n_all = inp["xyz"].shape[0]
    keep, _, _ = kept_rows(dict(inp, xyz=inp["xyz"][:-6], g_w=inp["g_w"][:-6]))
    assert keep.numel() >= 0.9 * (n_all - 6)
    g64, g32 = grid_oracle(inp, F64, keep), grid_oracle(inp, F32, keep)           # the oracle WITHOUT the six
    rows = torch.cat([keep, torch.arange(n_all - 6, n_all)])
    grid, stride = _grid_on_device(inp, layout)
    code, voxel, grad, cnt, _ = raw_call(inp, grid, stride, index=int_index(rows), count=count_of(rows.numel()))
    assert code == 0
    assert_list(inp, voxel, grad, cnt, rows.numel(), expect=closed_form(inp, keep)[1])
    got = dense_of(inp, voxel, grad, cnt)
    assert bool(torch.isfinite(got).all())
    check_rows("skip rule %s" % layout, vox_rows(got), vox_rows(g64), vox_rows(g32))
    # the forward still reports them: NaN weights
    from manus_amd import ops
    w = ops.skin_weights(_dev(inp["xyz"][-6:]), _dev(inp["grid"]), _dev(inp["center"]), _dev(inp["scale"]))
    assert bool(torch.isnan(w).all())


# =================================================================================================================
# 5. indexed calls: order, entries past N, count < max_count; run to run
# =================================================================================================================
@pytest.mark.parametrize("B,layout", [(21, "padded"), (25, "generic")])
def test_indexed_is_bitwise_independent_of_the_list_order(B, layout):
    ref = parity_reference(B)
    inp, keep = ref["inp"], ref["keep"]
    N = inp["xyz"].shape[0]
    g = torch.Generator().manual_seed(5)
    sub = keep[torch.randperm(keep.numel(), generator=g)[:300]]
    grid, stride = _grid_on_device(inp, layout)
    outs = []
    for k in range(2):
        order = sub[torch.randperm(300, generator=g)]
        past = torch.tensor([N, N + 5, 2 ** 31 - 1, N + 1000], dtype=torch.int64)
        lst = torch.cat([order[:100], past[:2], order[100:], past[2:]]) if k == 0 else torch.cat([past[2:], order, past[:2]])
        # behind the count: valid Gaussians that would change the result if they were read
        idx = torch.cat([lst, keep[:50]]).to(torch.int32).to(DEV).contiguous()
        code, voxel, grad, cnt, _ = raw_call(inp, grid, stride, index=idx, count=count_of(lst.numel()))
        assert code == 0
        n = int(cnt[0])
        outs.append((voxel[:n].clone(), grad[:n].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ordered = torch.sort(sub).values
    for _ in range(2):      # the dense call on the same subset, twice
        code, voxel, grad, cnt, _ = raw_call(inp, grid, stride, xyz=_dev(inp["xyz"][ordered]), g_w=_dev(inp["g_w"][ordered]))
        assert code == 0
        n = int(cnt[0])
        assert torch.equal(voxel[:n], outs[0][0]) and torch.equal(grad[:n], outs[0][1])


# =================================================================================================================
# 6. refusals
# =================================================================================================================
def test_refusals_launch_nothing():
    from manus_amd._lib import MGR_MAX_BONES, lib
    inp = grid_inputs(21, n=64)
    padded, _ = _grid_on_device(inp, "padded")
    off4, _ = _grid_on_device(dict(inp, grid=torch.zeros((5, 6, 7, 24), dtype=F64)), "generic")     # 24-float rows, 4 bytes off alignment
    idx = int_index(range(64))
    wide = _dev(torch.zeros((64, MGR_MAX_BONES + 1), dtype=F64))
    cases = [
        ("B > MGR_MAX_BONES", dict(grid=padded, stride=MGR_MAX_BONES + 1, B=MGR_MAX_BONES + 1, g_w=wide)),
        ("grid_stride neither B nor 24", dict(grid=padded, stride=22)),
        ("padded layout off alignment", dict(grid=off4, stride=24)),
        ("capacity too small", dict(grid=padded, stride=24, capacity=min(8 * 64, 5 * 6 * 7) - 1)),
        ("workspace too small", dict(grid=padded, stride=24, ws_bytes=int(lib().mgr_skin_grid_bwd_workspace_bytes(5, 6, 7, 64)) - 1)),
        ("max_count < 0", dict(grid=padded, stride=24, index=idx, count=count_of(64), max_count=-1)),
    ]
    for tag, kw in cases:
        code, voxel, grad, cnt, _ = raw_call(inp, kw.pop("grid"), kw.pop("stride"), **kw)
        assert code != 0, tag
        assert lib().mgr_last_error().decode().startswith("mgr_skin_grid_bwd"), tag
        assert bool((voxel == SENT_V).all()) and bool((grad == SENT_G).all()) and int(cnt[0]) == SENT_C, tag
    code, voxel, grad, cnt, _ = raw_call(inp, padded, 24)      # and the same call without a fault is accepted
    assert code == 0 and 0 < int(cnt[0]) <= 210


# =================================================================================================================
# 7. autograd through ops.skin_weights
# =================================================================================================================
@pytest.mark.parametrize("B", [21, 25])
def test_autograd_grid_leaf(B):
    from manus_amd import ops
    ref = parity_reference(B)
    inp, keep = ref["inp"], ref["keep"]
    c, s = _dev(inp["center"]), _dev(inp["scale"])
    g_w = _dev(inp["g_w"][keep])
    grid = _dev(inp["grid"]).requires_grad_(True)
    x1 = _dev(inp["xyz"][keep]).requires_grad_(True)
    ops.skin_weights(x1, grid, c, s).backward(g_w)
    assert grid.grad is not None and grid.grad.shape == grid.shape
    check_rows("autograd grid.grad B=%d" % B, vox_rows(grid.grad), vox_rows(ref["g64"]), vox_rows(ref["g32"]))
    x2 = _dev(inp["xyz"][keep]).requires_grad_(True)
    ops.skin_weights(x2, ops.SkinGrid(_dev(inp["grid"]), DEV), c, s).backward(g_w)
    assert torch.equal(x1.grad, x2.grad)
    # a tensor that does not require grad: as before
    x3 = _dev(inp["xyz"][keep]).requires_grad_(True)
    plain = _dev(inp["grid"])
    ops.skin_weights(x3, plain, c, s).backward(g_w)
    assert plain.grad is None and torch.equal(x3.grad, x2.grad)


# =================================================================================================================
# 8. HipViewCompute(skin_grid_grad=True)
# =================================================================================================================
def _hand_scene(n=3000, views=3):
    """The smallest hand scene of tests/test_gpu_fused.py (its `_scene`, n = 3000)."""
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=n, kind="hand", seed=6, grid_res=24, n_cameras=views, width=96, height=64,
                    cam_radius=0.5, sigma_range=(2e-3, 8e-3), device=DEV)
    return sc, camera_table(sc["cameras"], DEV)


def _same(a, b):
    for k in a:
        if isinstance(a[k], dict):
            for n in a[k]:
                assert torch.equal(a[k][n], b[k][n]), (k, n)
        elif torch.is_tensor(a[k]) and k != "loss":
            assert torch.equal(a[k], b[k]), k
    assert abs(float(a["loss"]) - float(b["loss"])) < 1e-6      # (the loss scalar is summed with float atomics: test_gpu_fused.py)


@pytest.mark.parametrize("views", [3, 11])
def test_compute_flag_both_routes(views):
    from manus_amd.engine import HipViewCompute
    from util import keep as keep_out
    sc, ct = _hand_scene(views=views)
    tg = torch.rand((views, 3, 64, 96), device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    ids = list(range(views))
    outs = {}
    for fused in (False, True):
        off = keep_out(HipViewCompute(sc, tg, ct, fused=fused)(ids, 1.0 / views))
        assert "d_skin_grid" not in off
        hc = HipViewCompute(sc, tg, ct, fused=fused, skin_grid_grad=True)
        on = hc(ids, 1.0 / views)
        d = on["d_skin_grid"]
        dense = d.to_dense().clone()
        v, g = d.rows()
        assert bool((v[1:] > v[:-1]).all()) and bool((g[:, d.shape[3]:] == 0).all())
        _same(off, {k: x for k, x in on.items() if k != "d_skin_grid"})      # every other output is bitwise what it is with it off
        outs[fused] = (dense, hc)
    a, b = vox_rows(outs[True][0]).cpu().numpy().astype(np.float64), vox_rows(outs[False][0]).cpu().numpy().astype(np.float64)
    # the bar tests/test_gpu_fused.py applies to the leaf gradients between the two routes, verbatim: max_rel_err < 5e-3, and
    # fewer than 3 % of the rows off by more than 2e-5 of the largest entry
    print("FIGURE fused vs operator d_skin_grid V=%d max_rel_err %.3e" % (views, max_rel_err(a, b)))
    assert max_rel_err(a, b) < 5e-3, max_rel_err(a, b)
    rows = np.abs(a - b).max(1) > 2e-5 * np.abs(b).max()
    assert rows.mean() < 0.03, rows.sum()
    # both routes against the fp64 oracle chain behind the skin-weight gradient each of them formed
    for fused in (False, True):
        hc = outs[fused][1]
        na = hc.n_art
        d_w = hc.last_skin_w_grad.detach().double().cpu()
        inp = dict(B=d_w.shape[1], dims=tuple(sc["grid"].shape[:3]), grid=sc["grid"].double().cpu(), center=sc["grid_center"].double().cpu().reshape(-1),
                   scale=sc["grid_scale"].double().cpu().reshape(-1), xyz=hc.params["_xyz"].detach()[:na].double().cpu(), g_w=d_w)
        live = torch.nonzero(d_w.abs().sum(1) > 0).reshape(-1)
        # (no Gaussian is left out here: unlike dL/dxyz, the grid gradient is continuous across the node planes)
        check_rows("compute fused=%s V=%d vs oracle" % (fused, views), vox_rows(outs[fused][0]), vox_rows(grid_oracle(inp, F64, live)),
                   vox_rows(grid_oracle(inp, F32, live)))


def test_compute_flag_needs_a_hand_scene():
    from manus_amd.engine import HipViewCompute, ViewShardedStep
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=500, kind="object", seed=6, grid_res=24, n_cameras=1, width=96, height=64, cam_radius=0.5, device=DEV)
    with pytest.raises(ValueError):
        HipViewCompute(sc, torch.zeros((1, 3, 64, 96), device=DEV), camera_table(sc["cameras"], DEV), skin_grid_grad=True)
    sc, ct = _hand_scene(n=500, views=1)
    hc = HipViewCompute(sc, torch.zeros((1, 3, 64, 96), device=DEV), ct, skin_grid_grad=True)
    with pytest.raises(ValueError):
        ViewShardedStep(500, {}, hc, 1, rank=0, world_size=2)


def test_step_after_adam_samples_the_updated_grid():
    """The kept forward-only skin weights are keyed on the grid's version: a forward after `SkinGridAdam.step` differs from the
    one before and equals that of a fresh compute on the updated grid."""
    from manus_amd.engine import HipViewCompute
    from manus_amd.optim import SkinGridAdam
    sc, ct = _hand_scene(views=2)
    tg = torch.rand((2, 3, 64, 96), device=DEV)
    hc = HipViewCompute(sc, tg, ct, fused=True, skin_grid_grad=True)
    with torch.no_grad():
        before = hc.forward_views_fused([0, 1])[0].clone()
        assert torch.equal(before, hc.forward_views_fused([0, 1])[0])
    opt = SkinGridAdam(hc.grid, lr=0.05)
    v0 = hc.grid.version
    opt.step(hc([0, 1], 0.5)["d_skin_grid"])
    assert hc.grid.version == v0 + 1 and opt.steps == 1
    with torch.no_grad():
        after = hc.forward_views_fused([0, 1])[0].clone()
    assert not torch.equal(before, after)
    fresh = HipViewCompute(dict(sc, grid=hc.grid.dense()), tg, ct, fused=True)
    with torch.no_grad():
        assert torch.equal(after, fresh.forward_views_fused([0, 1])[0])


# =================================================================================================================
# 9. the row Adam against torch.optim.SparseAdam
# =================================================================================================================
def adam_inputs(B):
    """Three sparse gradients on a (5,6,7,B) grid whose touched sets differ and overlap; rows 200.. are never touched."""
    g = torch.Generator().manual_seed(300 + B)
    grid = rounded(0.05 + torch.rand((210, B), generator=g, dtype=F64))
    sets = [torch.arange(0, 120), torch.arange(60, 200, 2), torch.cat([torch.arange(0, 30), torch.arange(100, 180)])]
    grads = [rounded(torch.randn((v.numel(), B), generator=g, dtype=F64) * 10.0 ** float(k - 1)) for k, v in enumerate(sets)]
    return grid, sets, grads


def adam_checker(grid, sets, grads, dtype, clamp_min):
    p = grid.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.SparseAdam([p], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
    for v, g in zip(sets, grads):
        p.grad = torch.sparse_coo_tensor(v[None], g.to(dtype), p.shape)
        opt.step()
        if clamp_min is not None:
            with torch.no_grad():      # the kernel's clamp follows the step on the rows it stepped, nowhere else
                p[v] = p[v].clamp(min=clamp_min)
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("clamp_min", [None, 0.3])
@pytest.mark.parametrize("B", [21, 25])
def test_row_adam_equals_sparse_adam(B, clamp_min):
    from manus_amd import ops
    from manus_amd.optim import SkinGridAdam
    grid, sets, grads = adam_inputs(B)
    sg = ops.SkinGrid(_dev(grid.reshape(5, 6, 7, B)), DEV)
    start = sg.data.clone()
    opt = SkinGridAdam(sg, lr=0.01, betas=(0.9, 0.999), eps=1e-8, clamp_min=clamp_min)
    for v, g in zip(sets, grads):
        cap = v.numel() + 7          # rows behind the count are not read
        voxel = torch.full((cap,), 205, dtype=torch.int32, device=DEV)
        voxel[:v.numel()] = v.to(torch.int32).to(DEV)
        rows = torch.full((cap, sg.stride), 1e3, dtype=F32, device=DEV)
        rows[:v.numel()] = 0.0
        rows[:v.numel(), :B] = _dev(g)
        opt.step(ops.SkinGridGrad(voxel, rows, count_of(v.numel()), (5, 6, 7, B)))
    assert sg.version == 3 and opt.steps == 3
    r64, r32 = adam_checker(grid, sets, grads, F64, clamp_min), adam_checker(grid, sets, grads, F32, clamp_min)
    data = sg.data.reshape(210, sg.stride)
    for name, got, k in (("grid", data, 0), ("exp_avg", opt.exp_avg.reshape(210, -1), 1), ("exp_avg_sq", opt.exp_avg_sq.reshape(210, -1), 2)):
        check_rows("adam %s B=%d clamp=%s" % (name, B, clamp_min), got[:, :B], r64[k], r32[k])
        assert bool((got[:, B:] == 0).all())                                    # the pad channels stay zero
    assert torch.equal(data[200:], start.reshape(210, -1)[200:])                # untouched rows: bitwise unchanged
    assert bool((opt.exp_avg.reshape(210, -1)[200:] == 0).all())


# =================================================================================================================
# 10. recovery, end to end
# =================================================================================================================
def test_recovery_of_a_blended_grid():
    """150 `SkinGridAdam` steps on the squared error of the posed means recover a grid that was blended 30 % towards uniform:
    the GPU loop's loss ratio is at most twice the fp64 CPU loop's (fp32 moments over 150 steps)."""
    from manus_amd import ops
    from manus_amd.optim import SkinGridAdam
    ref = recovery_reference()
    assert ref["rho_ref"] < 0.1, ref["rho_ref"]
    inp = ref["inp"]
    xyz, c, s, T = _dev(inp["xyz"]), _dev(inp["center"]), _dev(inp["scale"]), _dev(inp["T"])
    ls, rot = torch.full((REC_N, 3), -5.0, device=DEV), torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV).repeat(REC_N, 1)
    target = _dev(ref["target"])
    sg = ops.SkinGrid(_dev(inp["start"]), DEV)
    opt = SkinGridAdam(sg, lr=REC_LR)
    losses = []
    for _ in range(REC_STEPS + 1):
        w = ops.skin_weights(xyz, sg, c, s).requires_grad_(True)
        pxyz = ops.lbs_cov(xyz, ls, rot, w, T)[0]
        loss = ((pxyz - target) ** 2).sum()
        losses.append(loss)
        if len(losses) == REC_STEPS + 1:
            break
        loss.backward()
        opt.step(ops.skin_grid_grad(xyz, sg, c, s, w.grad))
    rho = float(losses[-1]) / float(losses[0])
    print("FIGURE recovery rho_gpu %.4e  rho_ref %.4e  (loss0 gpu %.4e, cpu %.4e)" % (rho, ref["rho_ref"], float(losses[0]), ref["loss0"]))
    assert rho <= 2.0 * ref["rho_ref"], (rho, ref["rho_ref"])
    assert bool((sg.data[..., 21:] == 0).all()) and bool((sg.data >= 0).all())


# =================================================================================================================
# the reference-only report (no GPU)
# =================================================================================================================
if __name__ == "__main__":
    for B in SKIN_BONES:
        r = parity_reference(B)
        assert_caps(r)
        print("B=%2d  kept %d / %d  small S %.3f  near a node %.3f  e32 %.3e" % (B, r["keep"].numel(), SKIN_N, r["share_small"], r["share_near"],
                                                                                  row_rel_err(vox_rows(r["g32"]), vox_rows(r["g64"]))))
    for tag, inp in (("long segments", long_segment_inputs()), ("borders", border_inputs()), ("skip rule", skip_inputs())):
        _, small, near = kept_rows(inp)
        print("%-14s N %d  small S %.3f  near a node %.3f" % (tag, inp["xyz"].shape[0], small, near))
    print("recovery rho_ref %.4e" % recovery_reference()["rho_ref"])

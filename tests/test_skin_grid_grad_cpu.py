"""CPU: the checker and the inputs of tests/test_gpu_skin_grid_grad.py, and the host side of the skin-grid surface.

The fp64 oracle's grid gradient (oracle/torch_ref.skin_weights_from_grid with a grid that requires grad) against central
differences; the closed form of include/manus_hip.h, restated as a loop, against the oracle; why the skip rule exists; the
conditions the GPU file puts on its own inputs (share of Gaussians left out, the recovery checker's loss ratio);
`SkinGrid.dense()` / `version` and `SkinGridGrad.to_dense()` on CPU tensors."""
import numpy as np
import torch

import test_gpu_skin_grid_grad as G
from oracle import torch_ref as tr

F64 = torch.float64


def _small():
    g = torch.Generator().manual_seed(1)
    inp = G.grid_inputs(21, dims=(3, 4, 5), n=60, seed=2)
    return inp, g


def test_oracle_grid_gradient_equals_central_differences():
    inp, g = _small()
    g64 = G.grid_oracle(inp, F64)

    def loss(grid):
        return float((tr.skin_weights_from_grid(inp["xyz"], inp["center"], inp["scale"], grid) * inp["g_w"]).sum())

    flat = torch.nonzero(g64.reshape(-1).abs() > 0).reshape(-1)
    picks = flat[torch.randperm(flat.numel(), generator=g)[:12]]
    h = 1e-6
    for k in picks.tolist():
        up, dn = inp["grid"].clone(), inp["grid"].clone()
        up.reshape(-1)[k] += h
        dn.reshape(-1)[k] -= h
        fd = (loss(up) - loss(dn)) / (2 * h)
        an = float(g64.reshape(-1)[k])
        assert abs(fd - an) <= 1e-6 * max(abs(an), float(g64.abs().max()) * 1e-3), (k, fd, an)


def test_closed_form_equals_the_oracle():
    for inp in (_small()[0], G.grid_inputs(25, n=200, seed=9), G.border_inputs(8)):
        cf, listed = G.closed_form(inp)
        g64 = G.grid_oracle(inp, F64)
        assert G.row_rel_err(G.vox_rows(cf), G.vox_rows(g64)) < 1e-12
        touched = set(torch.nonzero(G.vox_rows(g64).abs().sum(1) > 0).reshape(-1).tolist())
        assert touched <= listed and all(0 <= v < g64.numel() // g64.shape[-1] for v in listed)


def test_skip_rule_keeps_the_shared_leaf_finite():
    inp = G.skip_inputs()
    n = inp["xyz"].shape[0]
    rows = torch.arange(n - 6)
    without = G.grid_oracle(inp, F64, rows)
    assert bool(torch.isfinite(without).all())
    # autograd with the six degenerate Gaussians: 0/0 lands in the leaf -- even with a zero dL/dw row for them
    assert bool(torch.isnan(G.grid_oracle(inp, F64)).any())
    zeroed = dict(inp, g_w=torch.cat([inp["g_w"][:-6], torch.zeros((6, inp["B"]), dtype=F64)]))
    assert bool(torch.isnan(G.grid_oracle(zeroed, F64)).any())
    # the closed form with the rule is the oracle without them, and lists nothing for them
    cf, listed = G.closed_form(inp)
    assert G.row_rel_err(G.vox_rows(cf), G.vox_rows(without)) < 1e-12
    assert listed == G.closed_form(inp, rows)[1]
    w = tr.skin_weights_from_grid(inp["xyz"][-6:], inp["center"], inp["scale"], inp["grid"])
    assert bool(torch.isnan(w).all())       # the forward's NaN rows are how a caller sees them


def test_input_caps_of_the_gpu_file():
    for B in G.SKIN_BONES:
        ref = G.parity_reference(B)
        G.assert_caps(ref)
        assert ref["keep"].numel() >= 0.9 * G.SKIN_N
        S, _, _ = G.raw_sum(ref["inp"])
        assert float(S.min()) > 0.0                      # strictly positive grid: no S is zero
    for inp in (G.long_segment_inputs(), G.border_inputs(), G.skip_inputs()):
        _, small, near = G.kept_rows(inp)
        assert small + near <= G.LEFT_OUT_CAP + 6.0 / inp["xyz"].shape[0], (small, near)
    for N in (1, 63, 64, 65, 257):
        for B in (21, 25):
            keep, _, _ = G.kept_rows(G.grid_inputs(B, n=N, seed=11 + N))
            assert keep.numel() >= max(1, int(0.9 * N))
    inp = G.long_segment_inputs()
    _, _, idx = G.raw_sum(inp)
    assert bool(((idx > 0) & (idx < 1)).all())           # one cell


def test_recovery_checker_converges():
    ref = G.recovery_reference()
    print("recovery rho_ref %.4e" % ref["rho_ref"])
    assert ref["rho_ref"] < 0.1


def test_skin_grid_dense_round_trip_and_version():
    from manus_amd import ops
    g = torch.Generator().manual_seed(4)
    for B in (1, 21, 24, 25, 32):
        grid = torch.rand((3, 4, 5, B), generator=g)
        sg = ops.SkinGrid(grid)
        assert sg.version == 0
        d = sg.dense()
        assert d.shape == grid.shape and d.is_contiguous() and torch.equal(d, grid)
        d.zero_()                                        # a copy: the grid is not touched
        assert torch.equal(sg.dense(), grid)
        sg.data[0, 0, 0, 0] = 2.0                        # a write torch sees counts by itself
        assert sg.version == 1 and float(sg.dense()[0, 0, 0, 0]) == 2.0
        sg.bump()                                        # a kernel's write through the pointer is reported
        assert sg.version == 2
        sg.data.copy_(torch.zeros_like(sg.data))
        assert sg.version == 3


def test_skin_grid_grad_to_dense():
    from manus_amd import ops
    voxel = torch.tensor([1, 7, 59, -7, -7], dtype=torch.int32)
    grad = torch.full((5, 24), 123.0)
    grad[:3] = 0.0
    grad[:3, :21] = torch.arange(63, dtype=torch.float32).reshape(3, 21) + 1.0
    d = ops.SkinGridGrad(voxel, grad, torch.tensor([3], dtype=torch.int32), (3, 4, 5, 21))
    v, g = d.rows()
    assert v.tolist() == [1, 7, 59] and g.shape == (3, 24)
    dense = d.to_dense()
    assert dense.shape == (3, 4, 5, 21)
    flat = dense.reshape(60, 21)
    assert torch.equal(flat[[1, 7, 59]], grad[:3, :21])
    rest = np.setdiff1d(np.arange(60), [1, 7, 59])
    assert bool((flat[rest] == 0).all())
    empty = ops.SkinGridGrad(voxel, grad, torch.tensor([0], dtype=torch.int32), (3, 4, 5, 21))
    assert bool((empty.to_dense() == 0).all())

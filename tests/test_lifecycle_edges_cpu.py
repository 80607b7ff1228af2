"""CPU: the references and input conditions of tests/test_gpu_lifecycle_edges.py (tests/lifecycle_ref.py).  Nothing here runs
a kernel: these tests prove that the committed inputs are what the GPU tests say they are -- every densify class and layout
is populated and gives the counts expected by construction, every tie row ties, the kNN cases reach the grid regime they
are named for and exclude at most 1 % of their rows as near-ties -- and that the fp64 references agree with torch itself."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as tr

import lifecycle_ref as L
from util import max_rel_err


# -- 1. Adam --------------------------------------------------------------------------------------------------------------
def test_adam_reference_is_torch_optim_adam():
    """torch_ref.adam_step through the skip schedule (lagging per-group step counts, groups without .grad) is
    torch.optim.Adam(eps=1e-15) in fp64: the fp64 reference of the GPU tests is pinned to torch, not only to a restatement."""
    st, grads = L.adam_state(), L.adam_grads()
    ref, t_ref = L.adam_schedule({k: v.double() for k, v in st.items()}, [{k: g.double() for k, g in gr.items()} for gr in grads],
                                 lambda k, p, g, m, v, lr, t: tr.adam_step(p, g, m, v, lr, t))
    opt, t_opt = L.adam_schedule_torch_optim(st, grads)
    assert t_ref == t_opt == {"xyz": 9, "f_dc": 10, "f_rest": 10, "opacity": 5, "scaling": 10, "rotation": 3}
    for k in L.LEAVES:
        for suf in ("", "_m", "_v"):
            assert max_rel_err(opt[k + suf].numpy(), ref[k + suf].numpy()) < 1e-13, k + suf
            assert float((opt[k + suf] - ref[k + suf]).abs().max()) <= 1e-13 * float(ref[k + suf].abs().max()), k + suf


def test_adam_per_element_bar_holds_for_fp32_torch():
    """The per-element bar of the GPU tests (2 ulp + 64 * 2^-24 of the un-cancelled update) is a rounding-count bound, not a
    measurement of the kernel: fp32 torch_ref.adam_step meets it against fp64 from the same fp32 inputs, at every group's step
    count of the schedule, and so does the project's per-tensor 2e-6 bar."""
    st, grads = L.adam_state(), L.adam_grads()
    worst = 0.0

    def step(k, p, g, m, v, lr, t):
        nonlocal worst
        p64, m64, v64 = L.adam_ref64(p, g, m, v, lr, t)
        p32, m32, v32 = tr.adam_step(p, g, m, v, lr, t)
        bound = L.adam_elem_bound(p64, m, g, v64, lr, t)
        ratio = float(((p32.double() - p64).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, t, ratio)
        for a, b in ((p32, p64), (m32, m64), (v32, v64)):
            assert max_rel_err(a.numpy(), b.numpy()) < 2e-6, k
        return p32, m32, v32

    L.adam_schedule(st, grads, step)
    print("fp32 torch uses %.3f of the per-element Adam bar" % worst)


def test_adam_element_ranges_are_the_stated_partition():
    n, cuts = L.ADAM_N, L.ADAM_CUTS
    off = {k: (a, b) for k, a, b in L.group_offsets(n)}
    # 3N, 6N, 51N and 55N break the 16-byte alignment of their groups (whole groups on the scalar path of k_adam); 52N is a
    # multiple of 4 for every N, so the scaling group keeps the vector path and both paths run in one launch
    assert [off[k][0] % 4 != 0 for k in L.LEAVES] == [False, True, True, True, False, True]
    assert cuts[0] == 0 and cuts[-1] == L.ADAM_TOTAL == 59 * n and list(cuts) == sorted(cuts) and len(cuts) == L.ADAM_K + 1
    assert L.ADAM_PADDED == 59 * n + 5
    assert any(c % 4 for c in cuts[1:-1])                                       # a cut that is no multiple of 4
    assert any(off["f_rest"][0] < c < off["f_rest"][1] for c in cuts)           # strictly inside _features_rest
    assert any(c in [a for a, _ in off.values()][1:] for c in cuts[1:-1])       # exactly on a group boundary
    assert any(cuts[i] == cuts[i + 1] for i in range(L.ADAM_K))                 # an empty range
    missed = [sum(1 for a, b in off.values() if min(hi, b) <= max(lo, a)) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
    assert 3 in missed                                                          # a range without any element of three groups
    # an aligned start in the middle of a group and misaligned ones: both paths of k_adam run in range mode too
    assert any(lo % 4 == 0 and lo > 0 for lo in cuts[:-1]) and any(max(lo, a) % 4 for lo in cuts[:-1] for a, _ in off.values())


# -- 2. densify / prune -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_thr", [None, 20])
@pytest.mark.parametrize("layout", L.DENS_LAYOUTS)
@pytest.mark.parametrize("n", L.DENS_SIZES)
def test_densify_layouts_give_the_counts_expected_by_construction(n, layout, size_thr):
    """The oracle on the committed layout returns exactly the counts the classes imply (so every row is in the class its
    construction names), and the random / runs layouts populate every class once they have the rows for it."""
    cls = L.dens_classes(n, layout)
    st, accum, denom = L.dens_state(cls)
    want = L.dens_expected(cls, size_thr)
    got = tr.densify_and_prune(st, accum.clone(), denom, L.MAX_GRAD, L.MIN_OPACITY, L.EXTENT, L.PERCENT_DENSE,
                               L.dens_noise(want["split_selected"]), max_screen_size=size_thr)
    assert got["xyz"].shape[0] == want["total"]
    grads = torch.nan_to_num(accum / denom, nan=0.0).reshape(-1)
    sel = (grads >= L.MAX_GRAD) & (st["scaling"].exp().max(1).values > L.PERCENT_DENSE * L.EXTENT)
    assert int(sel.sum()) == want["split_selected"] and torch.equal(sel, L.dens_flags(cls, size_thr)[2])
    if layout == "random" and n >= 1023 or layout == "runs" and n >= 2049:
        assert sorted(set(cls.tolist())) == list(range(len(L.CLASSES)))
    if layout == "all_pruned":
        assert want["total"] == 0 and (n < 4 or want["split_selected"] > 0)
    if layout in ("all_split", "all_clone"):
        assert want["total"] == 2 * n
    if (n, layout, size_thr) == (2049, "random", None):
        c = [int((cls == i).sum()) for i in range(len(L.CLASSES))]
        assert max(c) - min(c) <= 1                                            # every class as often as N allows
    if layout == "random" and n >= 1023:
        # the noise row of a child is its rank among the SELECTED rows, not among the kept ones: a third of the selected
        # rows (split_pruned) is not kept, so the two ranks differ for most children
        ks = L.dens_flags(cls, size_thr)[3]
        assert int((torch.cumsum(sel.long(), 0)[ks] != torch.cumsum(ks.long(), 0)[ks]).sum()) > 0.5 * int(ks.sum())


def test_runs_layout_starves_and_floods_waves_and_blocks():
    """In the runs layout at N = 4100 every one of the four scanned flags has a 64-row wave with none of it and a wave with
    nothing else, and a 1024-row block with none; the first block is all split (selected and children kept everywhere), the
    third all clones (keep-original and keep-clone everywhere)."""
    cls = L.dens_classes(4100, "runs")
    for f in L.dens_flags(cls, None):
        w = torch.nn.functional.pad(f.long(), (0, 4160 - 4100)).reshape(-1, 64).sum(1)[:64]     # the 64 full waves
        b = f.long()[:4096].reshape(4, 1024).sum(1)
        assert int(w.min()) == 0 and int(w.max()) == 64 and int(b.min()) == 0
    ko, kc, sel, ks = L.dens_flags(cls, None)
    assert bool(ko[2048:3072].all()) and bool(kc[2048:3072].all()) and bool(sel[:1024].all()) and bool(ks[:1024].all())
    assert all(length % 64 and length % 1024 for _, length in L._RUNS)


def test_nonfinite_rows_are_decided_by_the_oracle():
    """Each non-finite row is classified by the oracle as its comment says, with and without the size threshold."""
    st, accum, denom, rows = L.nonfinite_state()
    assert len(rows) == 8 and len(set(rows.values())) == 8
    n = L.NONFINITE_N
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    smax = st["scaling"].exp().max(1).values
    clone = (grads.reshape(-1).abs() >= L.MAX_GRAD) & (smax <= 0.005)
    split = (grads.reshape(-1) >= L.MAX_GRAD) & (smax > 0.005)
    want = {"clone:accum_inf": "clone", "split:accum_inf": "split", "clone:denom_zero": "clone", "clone:scale_pinf": "split",
            "keep:scale_pinf": "keep", "split:scale_ninf": "split", "clone:scale_ninf": "clone", "nan:nan_and_inf": "keep"}
    for kind, r in rows.items():
        got = "clone" if clone[r] else "split" if split[r] else "keep"
        assert got == want[kind], kind
    assert torch.isinf(grads[rows["clone:denom_zero"]]).all() and torch.isnan(smax[rows["nan:nan_and_inf"]])
    for thr in (None, 20):
        ns = int(split.sum())
        out = tr.densify_and_prune(st, accum.clone(), denom, L.MAX_GRAD, L.MIN_OPACITY, L.EXTENT, L.PERCENT_DENSE, L.dens_noise(ns),
                                   max_screen_size=thr)
        assert 0 < out["xyz"].shape[0] < 2 * n
        # the children of an infinite scale survive without the size threshold (inf is no NaN) and go with it
        assert int(torch.isinf(out["scaling"]).any(1).sum()) == (1 + 2 + 2 + 2 if thr is None else 2 + 2)


def test_prune_masks():
    for n in (1, 1025, 4100):
        assert L.mask_layout(n, "all").all() and not L.mask_layout(n, "none").any()
    m = L.mask_layout(4100, "runs")
    w = m[:4096].reshape(-1, 64).long().sum(1)
    assert int(w.min()) == 0 and int(w.max()) == 64 and 0 < int(m.sum()) < 4100
    assert bool(m[:1024].all()) and not bool(m[2048:3072].any())                # a block without survivors, a block of survivors only


# -- 3. small kernels -------------------------------------------------------------------------------------------------------
def test_reset_opacity_bar_holds_for_fp32_torch():
    """fp32 torch (torch_ref.reset_opacity, what the reference runs) against fp64: the same NaN and -inf rows, the derived bound
    on every row where both are finite -- and -inf for the logits below -88.7 (-100, -89), where exp(-x) overflows in fp32,
    sigmoid is 0 and log(0) = -inf, while fp64 returns about the logit.  That overflow is the reference's own fp32 behaviour;
    the GPU test pins the kernel to it."""
    op = L.reset_logits()
    ref64, bound = L.reset_bound(op)
    ref32 = L.reset_ref(op, torch.float32).double()
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isnan(ref32), torch.isnan(ref64)) and torch.equal(ref32[~fin & ~ref64.isnan()], ref64[~fin & ~ref64.isnan()])
    assert int((~fin).sum()) == 2                                            # NaN stays NaN, -inf stays -inf; +inf is clamped
    overflow = fin & ~torch.isfinite(ref32)
    assert torch.equal(overflow, (op.double() < -88.7) & fin) and int(overflow.sum()) == 2 and bool((ref32[overflow] == -float("inf")).all())
    assert abs(float(ref64[0]) + 100.0) < 1e-9 and abs(float(ref64[1]) + 89.0) < 1e-9
    fin = fin & ~overflow
    ratio = ((ref32 - ref64).abs() / bound)[fin]
    assert float(ratio.max()) <= 1.0, float(ratio.max())
    assert float(bound[fin].max()) < 1e-3 and float(bound[3:9].max()) < 1e-5   # loose only where sigmoid is subnormal (-88)
    clamp = float(np.log(0.01 / 0.99))
    assert abs(float(ref64[5]) - clamp) < 1e-6 and abs(float(ref64[4]) + 4.6) < 1e-6   # -4.59 is clamped, -4.6 is not


def test_sh_half_inputs_hold_the_rounding_cases():
    x = L.sh_half_inputs(5)
    h = x.half()
    assert torch.isnan(h).sum() == 2 and torch.isinf(h).sum() >= 2 * 5
    ties = x.reshape(-1)[:36]
    near = ties.half()
    bits = near.view(torch.int16).long()                                      # sign-magnitude: +1 is the next half away from zero
    away, toward = ((bits + d).to(torch.int16).view(torch.float16).float() for d in (1, -1))
    other = torch.where(near.float().abs() < ties.abs(), away, toward)
    # a tie: the fp32 value is no half, its two neighbouring halves are equally far, and torch picked the even one
    assert bool((near.float() != ties).all()) and torch.equal((near.float() - ties).abs(), (other - ties).abs())
    assert bool((bits % 2 == 0).all()) and bool((ties[:18] > 0).all()) and bool((ties[18:] < 0).all())
    assert int((bits & 0x7C00 == 0).sum()) >= 6                               # some of them among the subnormal halves
    flat, hf = x.reshape(-1), h.reshape(-1).float()
    assert float(flat[37]) == 65520.0 and torch.isinf(hf[37]) and float(hf[36]) == 65504.0
    assert float(hf[38]) == 65504.0                                          # just below the overflow threshold
    assert float(hf[41]) == 2.0 ** -24 and float(hf[42]) == 0.0 and float(hf[43]) == 0.0 and float(hf[44]) == 2.0 ** -24
    assert float(hf[45]) == 2.0 ** -23                                       # 1.5 quanta: up to the even neighbour
    assert L.sh_half_inputs(1).shape == (1, 45) and L.sh_half_inputs(1000).shape == (1000, 45)


@pytest.mark.parametrize("n", L.ISO_SIZES)
def test_isotropic_inputs_tie_where_they_say(n):
    ls, tied = L.iso_inputs(n)
    s = ls.exp()
    for i in range(n):
        kind = L.iso_kind(i)
        row = s[i]
        if kind == "all_equal":
            assert row[0] == row[1] == row[2] and tied[i].all()
        elif kind == "big88":
            assert torch.isfinite(row).all() and row.max() > 1e38 and not tied[i].any()
        elif kind is not None:
            j, k = int(kind[3]), int(kind[4])
            ext = row.max() if kind.startswith("max") else row.min()
            assert row[j] == row[k] == ext and row[3 - j - k] != ext and tied[i].tolist() == [x in (j, k) for x in range(3)]
        else:
            assert len(set(row.tolist())) == 3 and not tied[i].any()
    if n >= 255:
        assert {L.iso_kind(i) for i in range(n)} - {None} == set(L.ISO_KINDS)
    if n == 256:
        assert L.iso_kind(n - 1) == "all_equal"                              # the last row of a full workgroup
    if n in (1, 257, 1025):
        assert L.iso_kind(n - 1) == "max01"                                  # the single row of the last workgroup ties
    loss, grad = L.iso_ref64(ls)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()


# -- 4. kNN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.KNN_CASES)
def test_knn_cases_reach_their_regime(name):
    pts, rows = L.knn_case(name)
    n = pts.shape[0]
    ref, tie = L.knn_ref64(pts, rows)
    assert tie.mean() <= 0.01, tie.mean()                                    # near-tie exclusions: at most 1 % of the rows
    assert np.isfinite(ref).all() and (ref >= 0).all()
    lo, h, raw, dims, budget = L.knn_grid(pts)
    cells = L.knn_cells(pts, lo, h, dims)
    if name == "collinear":
        assert len(rows) == 64 and raw[0] > 2048 and dims.tolist() == [2048, 1, 1]
        order = np.argsort(pts[:, 0])
        assert order[0] in rows and order[-1] in rows
        unclamped = ((pts[rows, 0] - lo[0]) * np.float32(1.0 / h)).astype(np.int64)
        assert (unclamped >= 2048).sum() >= 15 and (unclamped < 2040).sum() >= 30
        assert (cells[:, 0] == 2047).sum() > 1000                              # the clamped last cell holds the overhang
    elif name == "coplanar":
        assert dims[1] == 1 and dims[0] > 8 and dims[2] > 8
    elif name == "outlier":
        flat = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
        assert np.bincount(flat).max() >= 0.95 * n and ref[n // 2] > 9e7
    elif name.startswith("tiny"):
        assert budget == (64 if n <= 64 else n) and int(dims.prod()) <= budget
        if n in (4, 5):
            assert int(dims.prod()) > n                                        # more cells than N: only the floor allows them
    elif name == "identical":
        assert (ref == 0).all() and dims.tolist() == [1, 1, 1]
    elif name == "offset":
        # the coordinates are what loses bits (ulp 6.1e-5 at 1e3 against a spread of 1e-2), not the reference: the fp64
        # distances are taken from the fp32 coordinates, and differences of fp32 neighbours are exact in fp32 as well
        assert np.spacing(np.float32(1e3)) > 1e-3 * pts.std(0).min()
        d32 = ((pts[:50, None, :] - pts[None, :50, :]).astype(np.float32) ** 2).sum(-1)
        d64 = ((pts[:50, None, :].astype(np.float64) - pts[None, :50, :]) ** 2).sum(-1)
        np.testing.assert_allclose(d32, d64, rtol=1e-6)
    elif name == "negative":
        assert (pts < 0).all()

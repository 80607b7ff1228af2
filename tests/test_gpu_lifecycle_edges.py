"""GPU: the kernels that run around the render step -- Adam, densify / prune / gather, opacity reset, the fp16 SH copy, the
isotropic regulariser (csrc/optim.hip) and distCUDA2 (csrc/knn.hip) -- at the edges their other tests do not reach, against
the plain fp64 references of tests/lifecycle_ref.py.  tests/test_lifecycle_edges_cpu.py proves on the CPU that the inputs
used here are what the docstrings below say they are."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr

import lifecycle_ref as L
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAVES, ATTR = L.LEAVES, L.ATTR


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _optimizer(st, skin=True, opts=None):
    """GaussianOptimizer over the leaves of `st` with its moments (and skin weights) installed."""
    from manus_amd.optim import GaussianOptimizer
    sk = st.get("skin") if skin else None
    go = GaussianOptimizer({ATTR[k]: st[k].to(DEV) for k in LEAVES}, opts=opts, skin_weights=None if sk is None else sk.to(DEV))
    for k in LEAVES:
        go.m[ATTR[k]].copy_(st[k + "_m"])
        go.v[ATTR[k]].copy_(st[k + "_v"])
    return go


def _snapshot(go):
    out = {}
    for k in LEAVES:
        out[k], out[k + "_m"], out[k + "_v"] = (s[ATTR[k]].detach().cpu().clone() for s in (go.p, go.m, go.v))
    return out


# =====================================================================================================================
# 1. Adam (mgr_adam_step_groups / k_adam)
# =====================================================================================================================
def _adam_optimizer(st):
    go = _optimizer(st, skin=False)
    go.group_step, go.lr = dict(L.ADAM_STEPS0), dict(L.ADAM_LRS)
    return go


def _check_adam_group(k, before, g, after, lr, t):
    """One stepped group against torch_ref.adam_step in fp64 from the same fp32 p, g, m, v: the project's per-tensor bar for
    fp32 Adam (max_rel_err < 2e-6 on p, m, v) and, because a wrong update of a few elements hides under a bar scaled by the
    tensor's maximum, the per-element bar of lifecycle_ref.adam_elem_bound on p (2 ulp + 64 * 2^-24 of the un-cancelled update;
    a rounding count that fp32 torch meets with a ratio of 0.25 on these inputs, see the CPU test -- not a measurement of the
    kernel)."""
    p64, m64, v64 = L.adam_ref64(before[k], g, before[k + "_m"], before[k + "_v"], lr, t)
    for suf, ref in (("", p64), ("_m", m64), ("_v", v64)):
        assert max_rel_err(after[k + suf].numpy(), ref.numpy()) < 2e-6, (k + suf, t)
    ratio = float(((after[k].double() - p64).abs() / L.adam_elem_bound(p64, before[k + "_m"], g, v64, lr, t)).max())
    print("adam %-8s t=%2d  per-element error / bar = %.3f" % (k, t, ratio))
    assert ratio <= 1.0, (k, t, ratio)


def test_adam_skipped_and_lagging_groups_match_fp64():
    """k_adam's group lookup and per-group bias correction: N = 1027 rows, non-zero moments, step counts {7,7,7,3,7,1}, distinct
    learning rates, three steps with skip = {}, {opacity}, {xyz, rotation} -- the last switches off the first and the last group,
    so the lookup has to pass switched-off groups at both ends.  A skipped group keeps p, m, v bit for bit and its step count;
    a stepped group is compared with fp64 at ITS t.  Every tensor is its own 16-byte-aligned allocation, so this is the vector
    path plus the tail of a count that is no multiple of 4 (3081 = 4 * 770 + 1)."""
    st, grads = L.adam_state(), L.adam_grads()
    go = _adam_optimizer(st)
    for gr, skip in zip(grads, L.ADAM_SKIPS):
        before, t0 = _snapshot(go), dict(go.group_step)
        go.step({ATTR[k]: gr[k].to(DEV) for k in LEAVES}, skip=skip)
        after = _snapshot(go)
        for k in LEAVES:
            if k in skip:
                assert go.group_step[k] == t0[k], k
                for suf in ("", "_m", "_v"):
                    assert _same_bits(after[k + suf], before[k + suf]), k + suf
            else:
                assert go.group_step[k] == t0[k] + 1, k
                _check_adam_group(k, before, gr[k], after, L.ADAM_LRS[k], t0[k] + 1)
    assert go.group_step == {"xyz": 9, "f_dc": 10, "f_rest": 10, "opacity": 5, "scaling": 10, "rotation": 3}


def test_adam_element_ranges_assemble_to_the_plain_step():
    """GaussianOptimizer.flatten + step_range (the sharded-optimizer mode) on sub-range pointers: K = 5 optimizers over clones of
    one state, flattened to 59 N + 5 floats, each stepping one range of the partition lifecycle_ref.ADAM_CUTS (a cut that is no
    multiple of 4, one inside _features_rest, one on a group boundary, an empty range, a range without three groups), with the
    skip sets of the test above.  Most ranges start misaligned, so whole groups take k_adam's scalar path; ranges 0 and 3 start
    aligned (vector path).
    (a) nothing outside an optimizer's range changes, bit for bit, in p, m, v (the 5 padding floats included);
    (b) the owned slices, assembled, are bit for bit a plain step() of an un-flattened optimizer: both run the same adam_one,
        and a dropped or double-stepped element at a range seam, or a group stepped with another group's bias correction, shows;
    (c) group_step advances once per non-skipped group on every optimizer, whether or not its range touches the group."""
    st, grads = L.adam_state(), L.adam_grads()
    n, T = L.ADAM_N, L.ADAM_TOTAL
    plain = _adam_optimizer(st)
    shards = [_adam_optimizer(st) for _ in range(L.ADAM_K)]
    for s in shards:
        s.flatten(L.ADAM_PADDED)
        assert s.pflat.numel() == L.ADAM_PADDED and s.p["_features_rest"].shape == (n, 15, 3)
    ranges = list(zip(L.ADAM_CUTS[:-1], L.ADAM_CUTS[1:]))
    offs = L.group_offsets(n)
    for gr, skip in zip(grads, L.ADAM_SKIPS):
        gflat = torch.cat([gr[k].reshape(-1) for k in LEAVES] + [torch.full((5,), 7.0)]).to(DEV)
        stepped = torch.zeros(L.ADAM_PADDED, dtype=torch.bool)
        for k, a, b in offs:
            stepped[a:b] = k not in skip
        t0 = dict(plain.group_step)
        plain.step({ATTR[k]: gr[k].to(DEV) for k in LEAVES}, skip=skip)
        want = {suf: torch.cat([s[ATTR[k]].reshape(-1) for k in LEAVES]).cpu() for suf, s in (("p", plain.p), ("m", plain.m), ("v", plain.v))}
        got = {suf: torch.zeros(T) for suf in "pmv"}
        for s, (lo, hi) in zip(shards, ranges):
            before = {"p": s.pflat.cpu().clone(), "m": s.mflat.cpu().clone(), "v": s.vflat.cpu().clone()}
            s.step_range(gflat, lo, hi, skip=skip)
            own = torch.zeros(L.ADAM_PADDED, dtype=torch.bool)
            own[lo:hi] = True
            own &= stepped
            for suf, flat in (("p", s.pflat), ("m", s.mflat), ("v", s.vflat)):
                after = flat.cpu()
                assert torch.equal(_bits(after)[~own], _bits(before[suf])[~own]), (suf, lo, hi)                      # (a)
                got[suf][lo:hi] = after[lo:hi]
            assert s.group_step == {k: t0[k] + (k not in skip) for k in LEAVES} == plain.group_step, (lo, hi)          # (c)
        for suf in "pmv":                                                                                             # (b)
            diff = _bits(got[suf]) != _bits(want[suf])
            assert not bool(diff.any()), "%s: %d elements differ from the plain step, first at %d" % (suf, int(diff.sum()), int(diff.nonzero()[0]))
        for s in shards:      # what the all-gather of a sharded step does: every rank sees the new parameters
            s.pflat[:T].copy_(got["p"])


def test_adam_raw_entry_with_an_empty_group_in_the_middle():
    """mgr_adam_step_groups with count == 0 and null pointers for a switched-ON group in the middle (legal by the argument
    check: what step_range would pass if it kept an untouched group on): the launch steps the other five groups exactly as a
    call that switches that group off, leaves its tensors alone, and the stepped groups meet the fp64 bars."""
    from manus_amd._lib import lib, ptr, stream
    st, gr = L.adam_state(), L.adam_grads()[0]
    t = {k: L.ADAM_STEPS0[k] + 1 for k in LEAVES}
    arr = lambda ts: (ctypes.c_void_p * 6)(*[None if x is None else ptr(x) for x in ts])
    outs = []
    for null_group in (True, False):
        dev = {k: v.to(DEV).contiguous() for k, v in st.items()}
        g = {k: gr[k].to(DEV).contiguous() for k in LEAVES}
        pick = lambda d, suf: [None if (null_group and k == "f_rest") else d[k + suf] for k in LEAVES]
        counts = (ctypes.c_int64 * 6)(*[0 if (null_group and k == "f_rest") else st[k].numel() for k in LEAVES])
        steps = (ctypes.c_int64 * 6)(*[t[k] if (null_group or k != "f_rest") else 0 for k in LEAVES])
        lrs = (ctypes.c_double * 6)(*[L.ADAM_LRS[k] for k in LEAVES])
        rc = lib().mgr_adam_step_groups(6, counts, arr(pick(dev, "")), arr(pick(g, "")), arr(pick(dev, "_m")), arr(pick(dev, "_v")), lrs,
                                        steps, 0.9, 0.999, 1e-15, stream())
        assert rc == 0
        outs.append({k: v.cpu() for k, v in dev.items()})
    a, b = outs
    for k in LEAVES:
        for suf in ("", "_m", "_v"):
            assert _same_bits(a[k + suf], b[k + suf]), k + suf
            if k == "f_rest":
                assert _same_bits(a[k + suf], st[k + suf]), k + suf
        if k != "f_rest":
            _check_adam_group(k, st, gr[k], a, L.ADAM_LRS[k], t[k])


# =====================================================================================================================
# 2. densify, prune, gather (k_dens_flags / k_dens_map / k_dens_apply / k_prune_flags / k_gather_rows)
# =====================================================================================================================
def _run_densify(st, accum, denom, size_thr, n_sel, skin=True):
    noise = L.dens_noise(n_sel)
    want = tr.densify_and_prune(st if skin else dict(st, skin=None), accum.clone(), denom.clone(), L.MAX_GRAD, L.MIN_OPACITY, L.EXTENT,
                                L.PERCENT_DENSE, noise, max_screen_size=size_thr)
    go = _optimizer(st, skin=skin, opts={"percent_dense": L.PERCENT_DENSE})
    go.xyz_gradient_accum, go.denom = accum.to(DEV), denom.to(DEV)
    go.max_radii2D = torch.full((accum.shape[0],), 30.0, device=DEV)
    info = go.densify_and_prune(L.MAX_GRAD, L.MIN_OPACITY, L.EXTENT, size_thr, noise=noise.to(DEV))
    return go, info, want, noise


def _check_copied_state(go, want, M, skin=True):
    """Shapes of all eighteen tensors and the skin weights (M = 0 included: (0, ...)); everything that is a copy or a zero is
    exact -- both moments, the skin weights, the four leaves a split does not recompute; the statistics are reset."""
    for k in LEAVES:
        for suf, store in (("", go.p), ("_m", go.m), ("_v", go.v)):
            assert tuple(store[ATTR[k]].shape) == (M,) + L.SHAPE[k] == tuple(want[k + suf].shape), k + suf
        assert _same_bits(go.m[ATTR[k]], want[k + "_m"]) and _same_bits(go.v[ATTR[k]], want[k + "_v"]), k
        if k not in ("xyz", "scaling"):
            assert _same_bits(go.p[ATTR[k]], want[k]), k
    if skin:
        assert tuple(go.skin_weights.shape) == (M, 21) and _same_bits(go.skin_weights, want["skin"])
    else:
        assert go.skin_weights is None
    assert go.xyz_gradient_accum.shape == (M, 1) and go.denom.shape == (M, 1) and go.max_radii2D.shape == (M,)
    assert not go.xyz_gradient_accum.any() and not go.denom.any() and not go.max_radii2D.any()
    assert go.replaced == frozenset(LEAVES) and go.N == M


def _check_densify(n, layout, size_thr, skin=True):
    cls = L.dens_classes(n, layout)
    st, accum, denom = L.dens_state(cls, skin_bones=21 if skin else 0)
    exp = L.dens_expected(cls, size_thr)
    go, info, want, noise = _run_densify(st, accum, denom, size_thr, exp["split_selected"], skin)
    assert info == exp, (info, exp)                                   # counts: exact, and those the classes imply
    M = exp["total"]
    _check_copied_state(go, want, M, skin)
    for k in ("xyz", "scaling"):
        got = go.p[ATTR[k]].cpu()
        assert M == 0 or max_rel_err(got.numpy(), want[k].numpy()) < 2e-6, k
        head = exp["kept"] + exp["cloned"]                             # kept originals and clones are copies
        assert _same_bits(got[:head], want[k][:head]), k
    # split children, row by row, against the fp64 formula: child c of the j-th SELECTED row reads noise[c * n_sel + j]
    _, _, sel, ks = L.dens_flags(cls, size_thr)
    sel_rows = torch.nonzero(sel)[:, 0]
    if sel_rows.numel() == 0:
        return
    xyz64, sc64, bar = L.split_children64(st, sel_rows, noise)
    kept = torch.nonzero(ks[sel_rows])[:, 0]
    nk, head = exp["split_kept"], exp["kept"] + exp["cloned"]
    got_xyz = go.p["_xyz"].cpu()[head:].reshape(2, nk, 3).double()
    got_sc = go.p["_scaling"].cpu()[head:].reshape(2, nk, 3).double()
    assert bool(((got_xyz - xyz64[:, kept]).abs() <= bar[:, kept]).all()), float(((got_xyz - xyz64[:, kept]).abs() / bar[:, kept]).max())
    ref_sc = sc64[kept][None].expand(2, nk, 3)
    assert bool(((got_sc - ref_sc).abs() <= 2.0 * L.ulp32(ref_sc).reshape(ref_sc.shape)).all())


@pytest.mark.parametrize("size_thr", [None, 20])
@pytest.mark.parametrize("layout", L.DENS_LAYOUTS)
@pytest.mark.parametrize("n", L.DENS_SIZES)
def test_densify_layouts_match_oracle(n, layout, size_thr):
    """densify_and_prune on rows whose fate is set by construction (lifecycle_ref.dens_state: 0/0 statistics, clone, split,
    children pruned, low opacity, NaN scale, clone that goes with its original, big parent with small children, big keeper),
    over one, two, three and five 1024-row blocks, with and without the size threshold (`if max_screen_size:`).  Layouts:
    `random` -- every class, a third of the selected rows not kept, so a child's noise row (rank among the SELECTED) differs
    from its output rank (among the KEPT); `runs` -- lengths that are no multiples of 64 or 1024, whole waves and blocks with
    none / only one kind (scan bases of k_dens_map); `all_pruned` -- M = 0 with rows selected for the split: shapes (0, ...)
    of everything, nothing skipped; `all_split` / `all_clone` -- M = 2N, the largest aux and noise indices and the full map.
    Against torch_ref.densify_and_prune with the same noise: counts exact, parameters max_rel_err < 2e-6 (the project's bar),
    copies and moments bit-exact, statistics reset; children row by row against the fp64 split formula: position within
    1e-6 (|xyz| + 3 max scale |noise|), log-scale within 2 ulp (bars from the operation count, see split_children64)."""
    _check_densify(n, layout, size_thr)


def test_densify_without_skin_weights():
    """The same with no skin weights (skin == NULL in k_dens_apply), on the two-block random layout."""
    _check_densify(1025, "random", 20, skin=False)


@pytest.mark.parametrize("size_thr", [None, 20])
def test_densify_non_finite_statistics_and_scales(size_thr):
    """k_dens_flags on single rows with accum = inf, denom = 0 under a positive accum, a log-scale of +inf (with and without
    gradient), of -inf (beside a split-size scale, and alone), and a NaN beside an inf (nan_row: neither cloned nor split,
    pruned): count and order equal the oracle's -- the pure-copy leaves, moments and skin weights are compared bit for bit,
    which fixes which source row every output row came from.  None of the listed kinds is left out: the oracle decides every
    one (torch.max over a row with a NaN is NaN).  A child of an infinite scale has a non-finite position on both sides (which
    of inf / NaN is an accident of the summation order); the finite rest meets the usual bar."""
    st, accum, denom, rows = L.nonfinite_state()
    grads = torch.nan_to_num(accum / denom, nan=0.0).reshape(-1)
    n_sel = int(((grads >= L.MAX_GRAD) & (st["scaling"].exp().max(1).values > L.PERCENT_DENSE * L.EXTENT)).sum())
    go, info, want, _ = _run_densify(st, accum, denom, size_thr, n_sel)
    M = want["xyz"].shape[0]
    assert info["total"] == M and info["split_selected"] == n_sel and info["kept"] + info["cloned"] + 2 * info["split_kept"] == M
    _check_copied_state(go, want, M)
    sc, wsc = go.p["_scaling"].cpu().double(), want["scaling"].double()
    fin = torch.isfinite(wsc)
    assert not wsc.isnan().any() and torch.equal(torch.isfinite(sc), fin) and torch.equal(sc[~fin], wsc[~fin])     # the same +-inf
    assert float((sc[fin] - wsc[fin]).abs().max()) < 2e-6 * float(wsc[fin].abs().max())
    xyz, wxyz = go.p["_xyz"].cpu().double(), want["xyz"].double()
    fin = torch.isfinite(wxyz).all(1)
    assert torch.equal(torch.isfinite(xyz).all(1), fin) and int((~fin).sum()) == (2 if size_thr is None else 0)
    assert float((xyz[fin] - wxyz[fin]).abs().max()) < 2e-6 * float(wxyz[fin].abs().max())


@pytest.mark.parametrize("layout", ["random", "runs", "all", "none"])
@pytest.mark.parametrize("n", [1, 1025, 4100])
def test_prune_points_is_boolean_mask_indexing(n, layout):
    """prune_points (k_prune_flags + k_dens_map + k_dens_apply with kind 0 everywhere + k_gather_rows): leaves, moments, skin
    weights, the three statistics and side arrays of widths 1, 2, 21, 45 and an int32 one equal boolean-mask indexing bit
    for bit (a gather has no rounding).  `runs`: a block without survivors and a block of survivors only.  `all`: 0 is
    returned, every tensor has shape (0, ...), and the emptied optimizer still takes a step."""
    cls = L.dens_classes(n, "random")
    st, accum, denom = L.dens_state(cls)
    g = torch.Generator().manual_seed(n)
    mask = L.mask_layout(n, layout)
    extra = {"w1": torch.randn(n, generator=g), "w2": torch.randn(n, 2, generator=g), "w21": torch.randn(n, 21, generator=g),
             "w45": torch.randn(n, 15, 3, generator=g), "i32": torch.arange(n, dtype=torch.int32)}
    maxr = torch.rand(n, generator=g) * 50
    go = _optimizer(st)
    go.xyz_gradient_accum, go.denom, go.max_radii2D = accum.to(DEV), denom.to(DEV), maxr.to(DEV)
    M = go.prune_points(mask.to(DEV), extra={k: v.to(DEV) for k, v in extra.items()})
    keep = ~mask
    assert M == int(keep.sum()) == go.N
    want = tr.prune_points(dict(st, accum=accum, denom=denom, maxrad=maxr, **extra), mask)
    for k in LEAVES:
        for suf, store in (("", go.p), ("_m", go.m), ("_v", go.v)):
            assert tuple(store[ATTR[k]].shape) == (M,) + L.SHAPE[k] and _same_bits(store[ATTR[k]], want[k + suf]), k + suf
    assert _same_bits(go.skin_weights, want["skin"]) and go.skin_weights.shape == (M, 21)
    assert _same_bits(go.xyz_gradient_accum, want["accum"]) and _same_bits(go.denom, want["denom"]) and _same_bits(go.max_radii2D, want["maxrad"])
    for k, v in extra.items():
        out = go.last_prune_extra[k]
        assert out.dtype == v.dtype and _same_bits(out, want[k]), k
    assert go.replaced == frozenset(LEAVES)
    if layout == "all":
        assert M == 0
        go.step({ATTR[k]: torch.zeros((0,) + L.SHAPE[k], device=DEV) for k in LEAVES}, skip=())
        assert go.N == 0 and all(t == 1 for t in go.group_step.values())


def test_prune_everything_through_the_raw_entries():
    """What prune_points relies on when nothing survives: mgr_prune_plan reports five zeros, and mgr_densify_apply and
    mgr_gather_rows with M = 0 return MGR_OK without writing a byte of their outputs."""
    from manus_amd._lib import lib, ptr, stream
    n = 1025
    st, _, _ = L.dens_state(L.dens_classes(n, "random"))
    dev = {k: v.to(DEV).contiguous() for k, v in st.items()}
    nbytes = int(lib().mgr_densify_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    counts = (ctypes.c_int64 * 5)(*[9] * 5)
    assert lib().mgr_prune_plan(n, ptr(torch.ones(n, dtype=torch.uint8, device=DEV)), ptr(ws), nbytes, counts, stream()) == 0
    assert list(counts) == [0, 0, 0, 0, 0]
    arr = lambda ts: (ctypes.c_void_p * 6)(*[ptr(x) for x in ts])
    new = {k + suf: torch.full((1,) + L.SHAPE[k], 123.0, device=DEV) for k in LEAVES for suf in ("", "_m", "_v")}
    new_skin, side = torch.full((1, 21), 123.0, device=DEV), torch.full((1, 45), 123.0, device=DEV)
    rc = lib().mgr_densify_apply(n, 0, 0, ptr(ws), arr([dev[k] for k in LEAVES]), arr([dev[k + "_m"] for k in LEAVES]),
                                 arr([dev[k + "_v"] for k in LEAVES]), arr([new[k] for k in LEAVES]), arr([new[k + "_m"] for k in LEAVES]),
                                 arr([new[k + "_v"] for k in LEAVES]), ptr(dev["skin"]), ptr(new_skin), 21, None, stream())
    assert rc == 0
    assert lib().mgr_gather_rows(n, 0, ptr(ws), ptr(dev["f_rest"]), ptr(side), 45, stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 123.0).all()) for t in list(new.values()) + [new_skin, side])


# =====================================================================================================================
# 3. small kernels
# =====================================================================================================================
def test_reset_opacity_extreme_logits():
    """k_reset_opacity on logits {-100, -89, -88, -20, -4.6, -4.59, 0, 20, 100, NaN, +-inf} and 1000 random ones, against
    torch_ref.reset_opacity in fp32 (what the reference runs) and in fp64.
    * non-finite rows are those of fp32 torch: NaN stays NaN (torch.min propagates it; the kernel's fminf used to turn a NaN
      logit into log(0.01 / 0.99) -- fixed in k_reset_opacity), -inf stays -inf, and -100 and -89 become -inf: below -88.7
      exp(-x) overflows in fp32, sigmoid is 0 and log(0) = -inf in torch's fp32 exactly as in the kernel (fp64 gives about the
      logit; the row is documented at mgr_reset_opacity in include/manus_hip.h and pinned here);
    * every other row is within lifecycle_ref.reset_bound of the fp64 result, a bound derived from the roundings of the fp32
      expression (and met by fp32 torch, see the CPU test): about 2e-6 for ordinary logits, wide only at -88 where the sigmoid
      is subnormal;
    * the moments of the opacity group are zero, every other group is untouched bit for bit, and the next step skips opacity."""
    op = L.reset_logits()
    n = op.shape[0]
    st = L.adam_state(n=n, seed=3)
    st["opacity"] = op
    go = _optimizer(st, skin=False)
    go.reset_opacity()
    after = _snapshot(go)
    assert not after["opacity_m"].any() and not after["opacity_v"].any() and "opacity" in go.replaced
    for k in LEAVES:
        if k != "opacity":
            for suf in ("", "_m", "_v"):
                assert _same_bits(after[k + suf], st[k + suf]), k + suf
    got = after["opacity"].double()
    ref32 = L.reset_ref(op, torch.float32).double()
    ref64, bound = L.reset_bound(op)
    fin = torch.isfinite(ref32)
    print("reset_opacity special rows:", got[:12, 0].tolist())
    assert torch.equal(torch.isnan(got), torch.isnan(ref32))
    assert torch.equal(torch.isfinite(got), fin) and torch.equal(got[~fin & ~ref32.isnan()], ref32[~fin & ~ref32.isnan()])
    assert got[:2, 0].tolist() == [-float("inf")] * 2 and int((~fin).sum()) == 4          # -100, -89, NaN, -inf
    ratio = ((got - ref64).abs() / bound)[fin]
    print("reset_opacity: error / bound = %.3f" % float(ratio.max()))
    assert float(ratio.max()) <= 1.0
    assert bool(((got - ref32).abs()[fin] <= 2.0 * bound[fin]).all())                     # both lie within the bound of fp64


@pytest.mark.parametrize("n", [1, 5, 1000])
def test_sh_to_half_rounds_like_torch(n):
    """mgr_sh_to_half against f_rest.reshape(N, 45).half(), bit for bit: values exactly halfway between two halves (ties to
    even, normal and subnormal, both signs), 65504, 65520 (the first value that rounds to inf), 1e5, 6e-8, 2^-25 (tie with
    zero), -0.0, +-inf; NaN must come out as a NaN (its payload is not part of the conversion's contract).  The three padding
    halves of every row are +0, and nothing is written past row N (canary-filled buffer two rows longer)."""
    from manus_amd._lib import lib, ptr, stream
    x = L.sh_half_inputs(n)
    out = torch.full(((n + 2) * 48,), 0x7B7B, dtype=torch.int16, device=DEV)
    assert lib().mgr_sh_to_half(n, ptr(x.reshape(n, 15, 3).to(DEV)), ptr(out), stream()) == 0
    out = out.cpu()
    rows = out[: n * 48].reshape(n, 48)
    assert bool((out[n * 48:] == 0x7B7B).all()) and bool((rows[:, 45:] == 0).all())
    want = x.half()
    nan = torch.isnan(want)
    got_h = rows[:, :45].contiguous().view(torch.float16)
    assert torch.equal(torch.isnan(got_h), nan)
    assert torch.equal(rows[:, :45][~nan], want.view(torch.int16)[~nan])


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n", L.ISO_SIZES)
def test_isotropic_reg_ties_overflow_and_seams(n, accumulate):
    """k_isotropic_reg against autograd of torch_ref.isotropic_reg in fp64, N at the 256-row workgroup seams, gradient written
    and accumulated: rows with all three scales equal, each two-way tie on the maximum and on the minimum, and a log-scale of
    88 (exp finite, its square not).  Value: the project's 2e-6 relative bar; gradient: max_rel_err < 2e-6 per tensor, with
    the tied entries of a row compared as their SUM (which index of a tie gets the gradient is a convention) -- and the kernel's
    documented convention asserted separately: the FIRST index attaining an extreme receives it, later tied ones exactly 0.
    The only row of N = 1 ties on its maximum; it is not an all-equal row, whose own gradient is a cancellation remainder
    (1e-8 / (s + 1e-8) of its two terms: 2 % off in fp32 on the GPU, absolute error 4e-8) that the per-tensor bar can judge
    only beside ordinary rows, as it does at the other sizes (see lifecycle_ref.iso_inputs)."""
    from manus_amd import ops
    ls, tied = L.iso_inputs(n)
    loss64, g64 = L.iso_ref64(ls)
    base = torch.randn(n, 3, generator=torch.Generator().manual_seed(n)) * float(g64.abs().max())
    loss, g = ops.isotropic_reg_grad(ls.to(DEV), 0.4, 1.0, grad_out=base.to(DEV).clone() if accumulate else None)
    got = g.cpu()
    assert abs(float(loss) - float(loss64)) <= 2e-6 * abs(float(loss64))
    delta = got.double() - base.double() if accumulate else got.double()
    ref = L.fold_ties(g64, tied)
    assert max_rel_err(L.fold_ties(delta, tied).numpy(), ref.numpy()) < 2e-6
    later = tied & (torch.cumsum(tied.long(), 1) > 1)              # tied entries after the first of their row
    assert int(later.sum()) >= (1 if n == 1 else 7)
    assert torch.equal(got[later], base[later] if accumulate else torch.zeros(int(later.sum())))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_add_densification_stats_small_sizes(n):
    """mgr_add_densification_stats at one row and either side of the 256-row workgroup: exactly the three torch updates."""
    st, _, _ = L.dens_state(L.dens_classes(n, "random"))
    go = _optimizer(st)
    g = torch.Generator().manual_seed(n)
    acc, den, mx = torch.zeros(n, 1), torch.zeros(n, 1), torch.zeros(n)
    for _ in range(3):
        g2 = torch.rand(n, generator=g) * (torch.rand(n, generator=g) < 0.4)
        vis = torch.randint(0, 9, (n,), generator=g).float()
        rad = torch.randint(0, 60, (n,), generator=g).to(torch.int32)
        acc += g2.reshape(-1, 1); den += vis.reshape(-1, 1); mx = torch.maximum(mx, rad.float())
        go.add_densification_stats(g2.to(DEV), vis.to(DEV), rad.to(DEV))
    assert torch.equal(go.xyz_gradient_accum.cpu(), acc) and torch.equal(go.denom.cpu(), den) and torch.equal(go.max_radii2D.cpu(), mx)


# =====================================================================================================================
# 4. kNN (distCUDA2 / csrc/knn.hip)
# =====================================================================================================================
@pytest.mark.parametrize("name", L.KNN_CASES)
def test_distcuda2_grid_regimes(name):
    """distCUDA2 against brute force in fp64 (from the fp32 coordinates, over ALL points, for the queried rows) at the existing
    bar rtol 2e-5, atol 1e-12, in the regimes of the grid the other kNN tests do not enter: collinear 40 000 (the 2048-cell
    clamp per axis; 64 rows with the first and last sorted point and rows inside the clamped last cell), coplanar (one
    degenerate axis), a cloud with one outlier at 1e4 (coarse grid, nearly everything in one cell; the outlier's own value),
    N = 4, 5, 63, 64, 65 (the floor of 64 cells), 100 identical points (zero extent: exactly 0), a cloud of spread 1e-2 around
    (1e3, -1e3, 1e3) (the cell coordinate loses bits), negative-only coordinates (the ordered-uint bounding box).  Rows whose
    third and fourth neighbour distances differ by less than 1e-5 relative are left out (the near-tie rule of
    tests/test_gpu_mano_init.py); the CPU test shows that this is at most 1 % of any case."""
    from simple_knn._C import distCUDA2
    pts, rows = L.knn_case(name)
    ref, tie = L.knn_ref64(pts, rows)
    got = distCUDA2(torch.tensor(pts, device=DEV)).cpu().numpy().astype(np.float64)
    assert got.shape == (pts.shape[0],) and np.isfinite(got).all() and (got >= 0).all()
    np.testing.assert_allclose(got[rows][~tie], ref[~tie], rtol=2e-5, atol=1e-12)
    if name == "identical":
        assert (got == 0).all()
    if name == "outlier":
        i = pts.shape[0] // 2
        assert not tie[i] and abs(got[i] - ref[i]) <= 2e-5 * ref[i] and ref[i] > 9e7

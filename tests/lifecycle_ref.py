"""Plain fp64 references and input builders for the optimizer / densification / kNN edge-case tests
(tests/test_lifecycle_edges_cpu.py proves the stated input conditions on the CPU, tests/test_gpu_lifecycle_edges.py runs
the kernels of csrc/optim.hip and csrc/knn.hip on them).  torch / numpy only; nothing here touches a GPU."""
import math

import numpy as np
import torch

from oracle import torch_ref as tr

LEAVES = tr.LEAVES
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}
SHAPE = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
WIDTH = {k: int(np.prod(s)) for k, s in SHAPE.items()}
ROW_FLOATS = sum(WIDTH.values())          # 59


def ulp32(x):
    """Spacing of fp32 at |x| (x: fp64 tensor or array), as fp64."""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# 1. Adam
# ---------------------------------------------------------------------------------------------------------------------
ADAM_N = 1027                              # odd: the flat offsets 3N, 6N, 51N, 55N are no multiples of 4 (52N always is)
ADAM_STEPS0 = {"xyz": 7, "f_dc": 7, "f_rest": 7, "opacity": 3, "scaling": 7, "rotation": 1}
ADAM_LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
ADAM_SKIPS = (frozenset(), frozenset({"opacity"}), frozenset({"xyz", "rotation"}))
ADAM_C = 64.0 * 2.0 ** -24                 # per-element bar: rounding count relative to the un-cancelled update
ADAM_K = 5
ADAM_TOTAL = ROW_FLOATS * ADAM_N
ADAM_PADDED = ADAM_TOTAL + 5
# cuts of [0, 59 N): 4107 is no multiple of 4 (inside f_dc); 30000 lies strictly inside _features_rest and is used twice, so
# the range between is empty; 52377 = 51 N is exactly the f_rest / opacity boundary; the last range [51 N, 59 N) holds no
# element of xyz, f_dc and f_rest.
ADAM_CUTS = (0, 4107, 30000, 30000, 51 * ADAM_N, ADAM_TOTAL)


def group_offsets(n):
    """[(name, first element, one past the last)] of the flat layout of GaussianOptimizer.flatten."""
    out, o = [], 0
    for k in LEAVES:
        out.append((k, o, o + WIDTH[k] * n))
        o += WIDTH[k] * n
    return out


def adam_state(n=ADAM_N, seed=0):
    """fp32 leaves with non-zero moments: {name: p, name_m, name_v}."""
    g = torch.Generator().manual_seed(seed)
    scale = {"xyz": 0.05, "f_dc": 1.0, "f_rest": 0.1, "opacity": 2.5, "scaling": 1.0, "rotation": 1.0}
    st = {}
    for k in LEAVES:
        shp = (n,) + SHAPE[k]
        st[k] = torch.randn(shp, generator=g) * scale[k] - (5.0 if k == "scaling" else 0.0)
        st[k + "_m"] = torch.randn(shp, generator=g) * 1e-3
        st[k + "_v"] = (torch.randn(shp, generator=g) * 1e-3) ** 2 + 1e-9
    return st


def adam_grads(n=ADAM_N, seed=0, steps=3):
    g = torch.Generator().manual_seed(1000 + seed)
    return [{k: torch.randn((n,) + SHAPE[k], generator=g) * 1e-3 for k in LEAVES} for _ in range(steps)]


def adam_ref64(p, g, m, v, lr, t):
    """torch_ref.adam_step in fp64 from fp32 inputs."""
    return tr.adam_step(p.double(), g.double(), m.double(), v.double(), lr, t)


def adam_elem_bound(p_ref64, m_old, g, v_new64, lr, t, c=ADAM_C, beta1=0.9, beta2=0.999, eps=1e-15):
    """|p_got - p_ref64| may be at most this, element by element: 2 ulp of the result plus c times the size the update
    would have without the cancellation in the first moment."""
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    upd = abs(lr / bc1) * (m_old.double().abs() + g.double().abs()) / (v_new64.sqrt() / math.sqrt(bc2) + eps)
    return 2.0 * ulp32(p_ref64).reshape(p_ref64.shape) + c * upd


def adam_schedule(state, grads, step_fn, steps0=ADAM_STEPS0, lrs=ADAM_LRS, skips=ADAM_SKIPS):
    """Run the skip schedule: step_fn(name, p, g, m, v, lr, t) -> (p, m, v) for every group not skipped, at the group's own
    step count.  Returns (final state, final step counts)."""
    st, t = dict(state), dict(steps0)
    for gr, skip in zip(grads, skips):
        for k in LEAVES:
            if k in skip:
                continue
            t[k] += 1
            st[k], st[k + "_m"], st[k + "_v"] = step_fn(k, st[k], gr[k], st[k + "_m"], st[k + "_v"], lrs[k], t[k])
    return st, t


def adam_schedule_torch_optim(state, grads, steps0=ADAM_STEPS0, lrs=ADAM_LRS, skips=ADAM_SKIPS):
    """The same schedule through torch.optim.Adam(eps=1e-15) in fp64 on the CPU: six groups, state seeded with the moments
    and per-parameter step counts, a skipped group has .grad = None (which Adam passes over)."""
    prm = {k: torch.nn.Parameter(state[k].double().clone()) for k in LEAVES}
    opt = torch.optim.Adam([{"params": [prm[k]], "lr": lrs[k], "name": k} for k in LEAVES], lr=0.0, eps=1e-15)
    for k in LEAVES:
        opt.state[prm[k]] = {"step": torch.tensor(float(steps0[k])), "exp_avg": state[k + "_m"].double().clone(),
                             "exp_avg_sq": state[k + "_v"].double().clone()}
    for gr, skip in zip(grads, skips):
        for k in LEAVES:
            prm[k].grad = None if k in skip else gr[k].double().clone()
        opt.step()
    out = {}
    for k in LEAVES:
        out[k], out[k + "_m"], out[k + "_v"] = prm[k].detach(), opt.state[prm[k]]["exp_avg"], opt.state[prm[k]]["exp_avg_sq"]
    return out, {k: int(opt.state[prm[k]]["step"]) for k in LEAVES}


# ---------------------------------------------------------------------------------------------------------------------
# 2. densify / prune
# ---------------------------------------------------------------------------------------------------------------------
DENS_SIZES = (1, 7, 1023, 1025, 2049, 4100)
EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY = 0.5, 0.01, 0.0002, 0.005      # dense limit 0.005, big limit 0.05
CLASSES = ("keep", "clone", "split", "split_pruned", "pruned", "nan", "clone_pruned", "split_big_parent", "keep_big")
C = {name: i for i, name in enumerate(CLASSES)}
_HIGH_GRAD = {"clone", "split", "split_pruned", "nan", "clone_pruned", "split_big_parent"}
_LOW_OP = {"split_pruned", "pruned", "clone_pruned"}
_SPECIAL_SCALE = {"split": -4.0, "split_pruned": -4.0, "split_big_parent": -2.8, "keep_big": -2.5, "nan": float("nan")}
# runs whose lengths are neither multiples of 64 nor of 1024: the first 1024-row block is all split, the 1400 clones cover the
# whole third block, and every class has appeared by row 1754
_RUNS = (("split", 1030), ("pruned", 70), ("clone", 1), ("keep_big", 45), ("split_pruned", 77), ("nan", 3), ("clone_pruned", 65),
         ("split_big_parent", 333), ("keep", 130), ("clone", 1400))
DENS_LAYOUTS = ("random", "runs", "all_pruned", "all_split", "all_clone")


def dens_classes(n, layout, seed=0):
    """(n,) int64 class of every row."""
    if layout == "random":     # every class as often as n allows, in seeded random order
        g = torch.Generator().manual_seed(77 + seed + n)
        return (torch.arange(n) % len(CLASSES))[torch.randperm(n, generator=g)]
    if layout == "runs":
        out = []
        while len(out) < n:
            for name, length in _RUNS:
                out += [C[name]] * length
        return torch.tensor(out[:n])
    if layout == "all_pruned":  # four ways to vanish: nothing survives, yet Gaussians are selected for the split
        gone = torch.tensor([C["pruned"], C["nan"], C["clone_pruned"], C["split_pruned"]])
        return gone[torch.arange(n) % 4]
    if layout == "all_split":
        return torch.full((n,), C["split"])
    if layout == "all_clone":
        return torch.full((n,), C["clone"])
    raise ValueError(layout)


def dens_state(cls, seed=0, skin_bones=21):
    """(state dict for torch_ref.densify_and_prune, accum, denom) with the rows built by class (ISSUE table):
    keep 0/0 statistics; clone high gradient + scales <= dense limit; split one log-scale at -4; *_pruned opacity logit -6;
    nan one NaN log-scale; split_big_parent one log-scale at -2.8 (parent 0.061 > 0.05, children 0.038 < 0.05); keep_big one
    log-scale at -2.5 with a low gradient."""
    n = cls.shape[0]
    g = torch.Generator().manual_seed(500 + seed + n)
    st = {"xyz": torch.randn(n, 3, generator=g) * 0.05, "f_dc": torch.randn(n, 1, 3, generator=g),
          "f_rest": torch.randn(n, 15, 3, generator=g) * 0.1, "rotation": torch.randn(n, 4, generator=g)}
    scaling = -7.5 + 1.5 * torch.rand(n, 3, generator=g)                      # exp <= 0.0025: below the dense limit
    col = torch.randint(0, 3, (n,), generator=g)
    opacity = torch.full((n, 1), 2.0) + 0.5 * torch.rand(n, 1, generator=g)
    accum, denom = torch.zeros(n, 1), torch.zeros(n, 1)
    for name, i in C.items():
        rows = torch.nonzero(cls == i)[:, 0]
        if name in _SPECIAL_SCALE:
            scaling[rows, col[rows]] = _SPECIAL_SCALE[name]
        if name in _LOW_OP:
            opacity[rows] = -6.0
        if name in _HIGH_GRAD:
            denom[rows] = torch.randint(1, 4, (rows.numel(), 1), generator=g).float()
            accum[rows] = denom[rows] * (5e-4 + 5e-4 * torch.rand(rows.numel(), 1, generator=g))
        elif name != "keep":                                                # low but finite gradient; keep stays 0/0
            denom[rows] = 1.0
            accum[rows] = 1e-5
    st["scaling"], st["opacity"] = scaling, opacity
    for k in LEAVES:                                                        # non-zero moments: copied rows keep them, new rows get zeros
        st[k + "_m"] = torch.randn(st[k].shape, generator=g) * 1e-3
        st[k + "_v"] = torch.rand(st[k].shape, generator=g) * 1e-6 + 1e-9
    if skin_bones:
        w = torch.rand(n, skin_bones, generator=g)
        st["skin"] = w / w.sum(1, keepdim=True)
    else:
        st["skin"] = None
    return st, accum, denom


def dens_flags(cls, size_thr):
    """The four per-row decisions by construction: (keep original, keep clone, selected for split, children kept)."""
    is_ = lambda *names: torch.isin(cls, torch.tensor([C[x] for x in names]))
    keep_orig = is_("keep", "clone") | (is_("keep_big") if not size_thr else torch.zeros_like(cls, dtype=torch.bool))
    return keep_orig, is_("clone"), is_("split", "split_pruned", "split_big_parent"), is_("split", "split_big_parent")


def dens_expected(cls, size_thr):
    ko, kc, sel, ks = (int(x.sum()) for x in dens_flags(cls, size_thr))
    return dict(kept=ko, cloned=kc, split_selected=sel, split_kept=ks, total=ko + kc + 2 * ks)


def dens_noise(n_sel, seed=0):
    return torch.randn(2 * n_sel, 3, generator=torch.Generator().manual_seed(900 + seed + n_sel))


def split_children64(st, sel_rows, noise):
    """fp64 evaluation of the split formula (gaussian.py:264-268) for the selected rows `sel_rows` (ascending):
    child c of the j-th selected row: xyz = R(q) (noise[c * n_sel + j] * exp(s)) + xyz, scaling = log(exp(s) / 1.6).
    Returns (xyz (2, n_sel, 3), scaling (n_sel, 3), position bar (2, n_sel, 1)): the bar is 1e-6 (|xyz| + 3 max scale |noise|)
    with max norms -- R comes out of a normalisation, six products and three sums (error < 1e-6 per entry), the offset is
    three products of those with |noise * scale| <= max scale |noise|, and the final add rounds at |xyz|."""
    ns = sel_rows.numel()
    s = st["scaling"][sel_rows].double().exp()
    R = tr._rot_from_raw_quat(st["rotation"][sel_rows].double())
    nz = noise.double().reshape(2, ns, 3)
    xyz0 = st["xyz"][sel_rows].double()
    xyz = torch.einsum("jab,cjb->cja", R, nz * s[None]) + xyz0[None]
    bar = 1e-6 * (xyz0.abs().max(1).values[None, :, None] + 3.0 * s.max(1).values[None, :, None] * nz.abs().max(2, keepdim=True).values)
    return xyz, torch.log(s / 1.6), bar


NONFINITE_N = 300


def nonfinite_state(seed=0):
    """A random-layout model of NONFINITE_N rows with single non-finite rows on top; returns (state, accum, denom, {kind: row}).
    Every kind is a row the oracle decides without ambiguity: torch.max over a row with a NaN is NaN whatever else the row
    holds, so `nan_and_inf` (a NaN and a +inf log-scale) is classified like any NaN row and none of the listed kinds is left
    out."""
    cls = dens_classes(NONFINITE_N, "random", seed=seed)
    st, accum, denom = dens_state(cls, seed=seed)
    rows = {}

    def take(kind, want):
        r = int(torch.nonzero(cls == C[want])[len([k for k in rows if k.startswith(want + ":")]), 0])
        rows[want + ":" + kind] = r
        return r

    accum[take("accum_inf", "clone")] = float("inf")                    # inf / finite: cloned
    accum[take("accum_inf", "split")] = float("inf")                    # inf / finite: split
    denom[take("denom_zero", "clone")] = 0.0                            # positive / 0 = inf: cloned
    r = take("scale_pinf", "clone"); st["scaling"][r, 1] = float("inf")  # high gradient + infinite scale: split, children inf
    r = take("scale_pinf", "keep"); st["scaling"][r, 2] = float("inf")   # no gradient: stays (goes with the size threshold)
    r = take("scale_ninf", "split")
    st["scaling"][r, (int(torch.argmax(st["scaling"][r])) + 1) % 3] = float("-inf")   # beside the -4: split, one child scale -inf
    r = take("scale_ninf", "clone"); st["scaling"][r, 0] = float("-inf")  # still below the dense limit: cloned
    r = take("nan_and_inf", "nan"); st["scaling"][r, (int(torch.nonzero(st["scaling"][r].isnan())[0, 0]) + 1) % 3] = float("inf")
    return st, accum, denom, rows


def mask_layout(n, layout, seed=0):
    """prune_points masks (True = remove): seeded random, runs, all, none."""
    if layout == "random":
        return torch.rand(n, generator=torch.Generator().manual_seed(31 + seed + n)) < 0.5
    if layout == "runs":
        m, o, v = torch.zeros(n, dtype=torch.bool), 0, True
        for length in [length for _, length in _RUNS] * 3:   # the first block goes entirely, the third stays entirely
            m[o:o + length] = v
            o, v = o + length, not v
        return m
    return torch.full((n,), layout == "all")


# ---------------------------------------------------------------------------------------------------------------------
# 3. small kernels
# ---------------------------------------------------------------------------------------------------------------------
RESET_SPECIAL = (-100.0, -89.0, -88.0, -20.0, -4.6, -4.59, 0.0, 20.0, 100.0, float("nan"), float("inf"), float("-inf"))


def reset_logits(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.tensor(RESET_SPECIAL), torch.randn(1000, generator=g) * 4.0]).reshape(-1, 1)


def reset_ref(op, dtype):
    return tr.reset_opacity({"opacity": op.to(dtype)})["opacity"]


def reset_bound(op):
    """Error an fp32 evaluation of log(s / (1 - s)), s = min(sigmoid(x), 0.01), may show against fp64: s carries four roundings
    (exp, add, divide, the quotient s / (1 - s)) relative to itself plus -- below 2^-126 -- two quanta of the subnormal grid,
    and d log(s / (1 - s)) / ds = 1 / (s (1 - s)); logf and the final rounding are 4 ulp of the result.  Returns (fp64 reference,
    bound); the bound is 0 where the reference is not finite.  It says nothing about logits below -88.7: there exp(-x) overflows
    in fp32, the fp32 expression gives sigmoid = 0 and log(0) = -inf where fp64 gives about the logit itself."""
    x = op.double()
    ref = reset_ref(op, torch.float64)
    s = torch.minimum(torch.sigmoid(x), torch.full_like(x, 0.01))
    fin = torch.isfinite(ref)
    b = torch.zeros_like(ref)
    b[fin] = 4.0 * ulp32(ref[fin]) + (4.0 * 2.0 ** -24 + 2.0 * 2.0 ** -149 / s[fin]) / (1.0 - s[fin])
    return ref, b


def sh_half_inputs(n, seed=0):
    """(n, 45) fp32: random values with, from the front, the rounding edge cases of fp32 -> fp16: values exactly halfway
    between two neighbouring halves (normal and subnormal, both parities, both signs), the overflow threshold, subnormals,
    signed zero, NaN, infinities."""
    g = torch.Generator().manual_seed(7 + seed + n)
    x = torch.randn(n * 45, generator=g)
    bits = torch.cat([torch.randint(0x0400, 0x7BFF, (12,), generator=g), torch.randint(0, 0x03FF, (6,), generator=g)])
    bits = torch.cat([bits, bits + 0x8000 - 0x10000])                       # the same magnitudes, negative (as int16)
    lo, hi = bits.to(torch.int16).view(torch.float16).float(), (bits + 1).to(torch.int16).view(torch.float16).float()
    special = torch.cat([(lo + hi) / 2, torch.tensor([65504.0, 65520.0, 65519.996, 1e5, -1e5, 6e-8, 5.96e-8 / 2, 2.0 ** -25, 2.0 ** -24,
                                                      1.5 * 2.0 ** -24, -0.0, 0.0, float("nan"), float("inf"), float("-inf")])])
    k = min(special.numel(), x.numel())
    x[:k] = special[:k]
    if n > 1:                                                               # and the same set at the tail of the last row
        x[-k:] = special[:k]
    return x.reshape(n, 45)


ISO_SIZES = (1, 255, 256, 257, 1025)
ISO_KINDS = ("all_equal", "max01", "max02", "max12", "min01", "min02", "min12", "big88")


def iso_kind(i):
    return ISO_KINDS[(i + 1) % 32] if (i + 1) % 32 < len(ISO_KINDS) else None


def iso_inputs(n, seed=0):
    """(log_scale (n,3) fp32, tied (n,3) bool: the indices that tie on an extreme of their row).  Row i is the special row
    iso_kind(i) = ISO_KINDS[(i + 1) % 32] where that exists: all three scales equal; each two-way tie on the maximum and on the
    minimum; one log-scale at 88 (exp just below the fp32 overflow).  256 and 1024 are multiples of 32, so the last row of a
    full 256-row workgroup is an all-equal row and the single row of the last workgroup of n = 257 and 1025 ties on its maximum;
    so does the only row of n = 1.  (Not an all-equal row there: its gradient is the remainder 1e-8 / (s + 1e-8) of two terms
    that cancel, which fp32 holds to a few per cent -- in any fp32 evaluation, torch's included -- and which a per-tensor bar
    can only judge beside ordinary rows.)"""
    g = torch.Generator().manual_seed(11 + seed + n)
    ls = -8.0 + 6.0 * torch.rand(n, 3, generator=g)
    tied = torch.zeros(n, 3, dtype=torch.bool)
    for i in range(n):
        kind = iso_kind(i)
        if kind is None:
            continue
        a, b, c = sorted(float(v) for v in ls[i])
        if kind == "all_equal":
            ls[i], tied[i] = b, True
        elif kind == "big88":
            ls[i, i % 3] = 88.0
        else:
            j, k = int(kind[3]), int(kind[4])
            other = 3 - j - k
            ls[i, j] = ls[i, k] = c if kind.startswith("max") else a
            ls[i, other] = b
            tied[i, j] = tied[i, k] = True
    return ls, tied


def iso_ref64(ls, cond=0.4, weight=1.0):
    x = ls.double().clone().requires_grad_(True)
    loss = weight * tr.isotropic_reg(x, cond)
    loss.backward()
    return loss.detach(), x.grad


def fold_ties(g, tied):
    """(n,4): the gradient with the tied entries of every row moved into a fourth column as their sum (which index of a tie
    receives the gradient is a convention; the sum is not)."""
    g = g.double()
    return torch.cat([torch.where(tied, torch.zeros_like(g), g), (g * tied).sum(1, keepdim=True)], 1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. kNN
# ---------------------------------------------------------------------------------------------------------------------
KNN_CASES = ("collinear", "coplanar", "outlier", "tiny4", "tiny5", "tiny63", "tiny64", "tiny65", "identical", "offset", "negative")


def knn_case(name):
    """(points (N,3) fp32, query rows (int64 array))."""
    g = np.random.default_rng(sum(map(ord, name)))
    if name == "collinear":
        n = 40000
        pts = np.zeros((n, 3), np.float32)
        pts[:, 0] = g.uniform(0, 1, n)
        order = np.argsort(pts[:, 0])
        clamped = order[pts[order, 0] > 0.97 * pts[:, 0].max()]           # beyond the 2048 cells the grid is clamped to
        inner = np.setdiff1d(g.permutation(n)[:200], np.concatenate([order[:1], order[-20:]]))[:43]
        rows = np.concatenate([order[:1], order[-1:], clamped[:: len(clamped) // 20][:19], inner])   # 1 + 1 + 19 + 43 = 64
        return pts, np.unique(rows)
    if name == "coplanar":
        n = 5000
        pts = g.normal(size=(n, 3)).astype(np.float32)
        pts[:, 1] = 0.25
    elif name == "outlier":
        n = 3000
        pts = g.normal(size=(n, 3)).astype(np.float32)
        pts[n // 2] = (1e4, 0, 0)
    elif name in ("tiny4", "tiny5"):   # every axis spans exactly [0, 1]: 2 x 2 x 2 cells, more than N, which only the floor of 64 allows
        pts = np.float32([[0, 0.3, 1], [1, 0, 0.2], [0.6, 1, 0], [0.2, 0.7, 0.45], [0.9, 0.4, 0.8]])[: int(name[4:])]
    elif name.startswith("tiny"):
        pts = g.normal(size=(int(name[4:]), 3)).astype(np.float32)
    elif name == "identical":
        pts = np.tile(np.float32([0.3, -1.7, 2.5]), (100, 1))
    elif name == "offset":
        pts = (np.float64([1e3, -1e3, 1e3]) + 1e-2 * g.normal(size=(2000, 3))).astype(np.float32)
    elif name == "negative":
        pts = (-1.0 - g.uniform(0, 3, size=(2000, 3))).astype(np.float32)
    else:
        raise ValueError(name)
    return pts, np.arange(pts.shape[0])


def knn_ref64(pts, rows, chunk=512):
    """Brute force in fp64 from the fp32 coordinates: (mean of the three smallest squared distances to the OTHER points,
    near_tie) for the queried rows; near_tie marks rows whose third and fourth neighbour distances differ by less than 1e-5
    relative (the rule of tests/test_gpu_mano_init.py)."""
    p = np.asarray(pts, np.float64)
    n = p.shape[0]
    out, tie = np.zeros(len(rows)), np.zeros(len(rows), bool)
    for s in range(0, len(rows), chunk):
        r = np.asarray(rows[s:s + chunk])
        d = ((p[r, None, :] - p[None, :, :]) ** 2).sum(-1)
        d[np.arange(len(r)), r] = np.inf
        k = min(4, n - 1)
        d = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
        out[s:s + chunk] = d[:, :3].mean(1)
        if k == 4:
            tie[s:s + chunk] = (d[:, 3] - d[:, 2]) < 1e-5 * d[:, 3]
    return out, tie


def knn_grid(pts):
    """The grid k_knn_setup (csrc/knn.hip) sizes for these points, restated in fp32 numpy: (lo, h, dims before the clamp to
    2048 per axis, dims, cell budget).  Used on the CPU to prove that a case reaches the regime it is named for."""
    f = np.float32
    p = np.asarray(pts, f)
    n = p.shape[0]
    lo, ext = p.min(0), (p.max(0) - p.min(0)).astype(f)
    emax = ext.max()
    vol = f(1)
    for k in range(3):
        vol = f(vol * max(ext[k], f(1e-3) * emax))
    h = f(np.cbrt(vol / f(max(1.0, n * 0.25)))) if vol > 0 else f(1)
    if not (h > 0 and np.isfinite(h)):
        h = f(1)
    budget = min(max(n, 64), 1 << 21)
    for _ in range(200):
        raw = np.floor(ext / h).astype(np.int64) + 1
        dims = np.clip(raw, 1, 2048)
        if int(dims.prod()) <= budget:
            break
        h = f(h * f(1.2))
    return lo, h, raw, dims, budget


def knn_cells(pts, lo, h, dims):
    p = np.asarray(pts, np.float32)
    c = ((p - lo) * np.float32(1.0 / h)).astype(np.int64)
    return np.clip(c, 0, dims - 1)

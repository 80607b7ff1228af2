"""Multi-view training step: V views batched per GPU, views sharded across GPUs,
ONE all-reduce of the per-Gaussian gradients per step (RCCL over xGMI via torch.distributed).

The reference trains one (frame, view) per step on one GPU (config/trainer/trainer.yaml:5,
main.py:84-87 DDP commented out).  "V views per iteration" is defined here as
    grad = (1/V) * sum_v grad(L_v)            (with V=1 it is the reference step)
and the densification statistics follow the reference's per-view rule
(src/models/gaussian.py:335-338, src/utils/gaussian_utils.py:469-471):
    xyz_gradient_accum += sum_v ||d L_v / d means2D[:, :2]||   (visible Gaussians only)
    denom              += sum_v visible_v
    max_radii2D         = max_v radii_v

Collectives per step: one SUM all-reduce of the flat buffer
    [ 59 N leaf gradients | N grad2d | N visibility counts | loss | overflow flag ]
which the backward kernels write in place (no packing copies).  max_radii2D needs a MAX, not a SUM; max is
associative and idempotent, so every rank keeps the running maximum over ITS views and the ranks are only
combined (one MAX all-reduce) right before the statistic is consumed, i.e. at a densification step.
"""
import ctypes
import functools
import os

import numpy as np
import torch
import torch.distributed as dist

from . import fused as fused_mod, losses, ops, rasterizer
from . import _lib
from ._lib import ManusHipError, check, lib, ptr, stream

# packed leaf-gradient layout: 59 floats per Gaussian
GRAD_LAYOUT = (("_xyz", 3), ("_features_dc", 3), ("_features_rest", 45), ("_opacity", 1),
               ("_scaling", 3), ("_rotation", 4))
GRAD_WIDTH = sum(w for _, w in GRAD_LAYOUT)
FLAT_TAIL = 2            # loss, overflow flag

# positions in the array mgr_raster_layout fills (byte offsets of the regions of a rasterizer workspace, in the order of
# MgrLayout) of the regions the Python side and tools/instr read
LAYOUT_TILE_START, LAYOUT_TILE_DONE = 7, 9
LAYOUT_FINAL_T, LAYOUT_N_CONTRIB, LAYOUT_INST_TAG = 16, 17, 22
LAYOUT_TILE_ZCUT, LAYOUT_TILE_ZUSED, LAYOUT_TILE_QEND = 26, 27, 28
LAYOUT_TILE_REP, LAYOUT_REP_UNIT, LAYOUT_REP_CNT, LAYOUT_TILE_ZWIN = 29, 30, 31, 32


def flat_size(N):
    return N * (GRAD_WIDTH + 2) + FLAT_TAIL


def shard_views(n_views, rank, world_size, weights=None):
    """View indices of `rank`.  Without weights: round-robin.  With weights (one cost per view, identical on every
    rank -- e.g. `view_costs` of the measured pair counts): greedy longest-processing-time assignment, the heaviest
    view first, each to the rank with the smallest load so far (ties: the lowest rank; views of a rank in ascending
    order), so that a rig whose cameras see the hand at very different sizes does not leave ranks idle (SURVEY.md 8e:
    "pad or balance by measured R per view")."""
    if weights is None:
        return list(range(rank, n_views, world_size))
    w = [float(x) for x in weights]
    assert len(w) == n_views
    load, mine = [0.0] * world_size, [[] for _ in range(world_size)]
    for v in sorted(range(n_views), key=lambda i: (-w[i], i)):
        r = min(range(world_size), key=lambda k: (load[k], k))
        load[r] += w[v]
        mine[r].append(v)
    return sorted(mine[rank])


def view_costs(pairs_per_view, n_gaussians):
    """Cost model of one view for `shard_views`: the blend / binning kernels scale with the view's (tile, Gaussian) pairs,
    the per-instance kernels with N.  Measured on the 300k / 1080p bench (profiles/): 0.16 ms per 2.6 M pairs against
    0.066 ms per 300k Gaussians, i.e. one Gaussian costs as much as 3.5 pairs."""
    return [float(p) + 3.5 * float(n_gaussians) for p in pairs_per_view]


def flat_views(flat, N):
    """Named views of the flat step buffer: one contiguous segment per leaf (GRAD_LAYOUT order), the two
    statistics, the loss and the overflow flag."""
    out, o = {}, 0
    for name, w in GRAD_LAYOUT:
        out[name] = flat[o:o + N * w]
        o += N * w
    out["grad2d"], out["vis"] = flat[o:o + N], flat[o + N:o + 2 * N]
    out["loss"], out["overflow"] = flat[o + 2 * N:o + 2 * N + 1], flat[o + 2 * N + 1:o + 2 * N + 2]
    return out


def pack_grads(grads, N, device, out=None):
    """Flat SoA buffer: one contiguous segment per leaf, in GRAD_LAYOUT order."""
    buf = out if out is not None else torch.empty(N * GRAD_WIDTH, dtype=torch.float32, device=device)
    o = 0
    for name, w in GRAD_LAYOUT:
        g = grads[name]
        seg = buf[o:o + N * w]
        if not (g.data_ptr() == seg.data_ptr() and g.is_contiguous()):   # already written in place (grad arena)
            seg.copy_(g.reshape(-1))
        o += N * w
    return buf


def unpack_grads(buf, shapes, N):
    out, o = {}, 0
    for name, w in GRAD_LAYOUT:
        out[name] = buf[o:o + N * w].reshape(shapes[name])
        o += N * w
    return out


class ViewShardedStep:
    """Runs `compute_fn(view_ids, scale)` on this rank's views and reduces across ranks.

    compute_fn returns a dict with
        grads      {leaf name: scale * sum over the given views of dL_v/dleaf}
        grad2d     (N,) sum over views of the visible 2D-gradient norms (unscaled)
        vis        (N,) number of views in which the Gaussian was visible
        radii      (N,) int32 max screen radius over views
        loss       scalar tensor, scale * sum of L_v
        overflow   optional scalar tensor, non-zero when the rasterizer ran out of pair capacity
    If compute_fn has a `grad_arena` attribute it is handed views of the step buffer and writes them in place.

    step() returns the reduced grads / grad2d / vis / loss / overflow (sums over all ranks) and the LOCAL radii
    (max over this rank's views); `reduce_max_radii` combines the ranks when the statistic is consumed.

    Reduction modes (world_size > 1):
        default        one SUM all-reduce of [59 N gradients | N grad2d | N vis | loss | overflow]
        compact=True   only the rows with a gradient on some rank travel (see `_compact_all_reduce`)
        scatter=True   sharded optimizer step: a reduce-scatter of the gradient part leaves every rank with the summed
                       slice it owns (`owned`, element range of the flat gradient buffer; the returned grads are then
                       only valid inside that slice) + one small all-reduce of the statistics; the caller updates the
                       parameters it owns and all-gathers them with `all_gather_params`.
    """

    def __init__(self, n_gaussians, shapes, compute_fn, n_views, rank=0, world_size=1, group=None, compact=False,
                 scatter=False, view_weights=None, force_collectives=False):
        self.N, self.shapes, self.compute_fn = n_gaussians, shapes, compute_fn
        self.n_views, self.rank, self.world, self.group = n_views, rank, world_size, group
        if world_size > 1 and getattr(compute_fn, "skin_grid_grad", False):
            # a sparse grid gradient has a different voxel list on every rank: nothing here reduces it
            raise ValueError("ViewShardedStep does not reduce the sparse skin-grid gradient across ranks: skin_grid_grad needs world_size == 1")
        self.local_views = shard_views(n_views, rank, world_size, view_weights)
        self.always_pack = False   # tests: take the packing path without a process group
        # force_collectives: issue every collective even in a world of one rank (a single-process "nccl" group on a one-GPU
        # box runs RCCL's all-reduce / reduce-scatter / all-gather code paths with the dtypes and in-place forms used here)
        self.force = bool(force_collectives)
        self.compact = bool(compact)
        self.scatter = bool(scatter) and (world_size > 1 or self.force)
        self.last_rows = None
        self._store = None
        n_g = self.N * GRAD_WIDTH
        self.padded_g = (n_g + world_size - 1) // world_size * world_size      # reduce-scatter needs equal slices
        c = self.padded_g // world_size
        self.owned = (rank * c, min((rank + 1) * c, n_g))
        dev = getattr(compute_fn, "device", None)
        if dev is not None and (world_size > 1 or self.force):
            self._alloc(dev)

    def _alloc(self, dev):
        # [ 59 N gradients | padding to a multiple of the world size | N grad2d | N vis | loss | overflow ]
        self._store = torch.zeros(self.padded_g + 2 * self.N + FLAT_TAIL, dtype=torch.float32, device=dev)

    @property
    def _flat(self):   # (tests look at the buffer the kernels write into)
        return self._store

    def _views(self):
        N, st = self.N, self._store
        out, o = {}, 0
        for name, w in GRAD_LAYOUT:
            out[name] = st[o:o + N * w]
            o += N * w
        o = self.padded_g
        out["grad2d"], out["vis"] = st[o:o + N], st[o + N:o + 2 * N]
        out["loss"], out["overflow"] = st[o + 2 * N:o + 2 * N + 1], st[o + 2 * N + 1:o + 2 * N + 2]
        return out

    def exchanged_rows(self):
        """Rows in the union of a recent compact exchange (the count reaches the host through an asynchronous copy behind the
        step: this waits for the one in flight, if any).  None before the first compact step."""
        sc = getattr(self, "_xch", None)
        if sc is not None and sc.get("ev") is not None:
            sc["ev"].synchronize()
            self.last_rows, sc["ev"] = int(sc["host"][0]), None
            sc["cap_rows"] = min(self.N, int(self.last_rows * 1.25) + 1024)
        return self.last_rows

    def reduce_max_radii(self, radii):
        """MAX over ranks of a per-Gaussian radius statistic (in place; any integer or float dtype)."""
        if self.world > 1 or self.force:
            dist.all_reduce(radii, op=dist.ReduceOp.MAX, group=self.group)
        return radii

    def all_gather_params(self, store):
        """In place on a parameter buffer laid out like the gradient part (`padded_g` floats): every rank contributes
        the slice it owns."""
        c = self.padded_g // self.world
        mine = store[self.rank * c:(self.rank + 1) * c]
        if dist.get_backend(self.group) == "gloo":      # (CPU / single-GPU tests; RCCL takes the one-call form)
            parts = [torch.empty_like(mine) for _ in range(self.world)]
            dist.all_gather(parts, mine.clone(), group=self.group)
            for r, t in enumerate(parts):
                store[r * c:(r + 1) * c].copy_(t)
        else:
            dist.all_gather_into_tensor(store, mine, group=self.group)

    def step(self):
        # compute_fn folds the 1/V of "grad = (1/V) sum_v grad L_v" into the loss scale
        N = self.N
        packed = self.world > 1 or self.always_pack or self.force
        if packed and self._store is not None and hasattr(self.compute_fn, "grad_arena"):
            # the backward kernels write straight into the step buffer (no packing copies): one view per leaf
            self.compute_fn.grad_arena = self._views()
        out = self.compute_fn(self.local_views, 1.0 / float(self.n_views))
        dev = out["grad2d"].device
        radii = out["radii"].to(torch.int32)
        if not packed:
            res = dict(grads=out["grads"], grad2d=out["grad2d"], vis=out["vis"], radii=radii, loss=out["loss"],
                       overflow=out.get("overflow"))
            # (one rank, nothing to reduce: what the compute object returned beside the reduced quantities travels as it is)
            for name in ("loss_lpips", "loss_ssim", "d_transforms", "d_exposure", "d_skin_grid", "loss_mask", "loss_depth"):
                if name in out:
                    res[name] = out[name]
            return res
        if self._store is None or self._store.device != dev:
            self._alloc(dev)
        st, n_g = self._store, N * GRAD_WIDTH
        fv = self._views()
        pack_grads(out["grads"], N, dev, out=st[:n_g])
        for name in ("grad2d", "vis"):
            if out[name].data_ptr() != fv[name].data_ptr():
                fv[name].copy_(out[name])
        fv["loss"].copy_(out["loss"].reshape(1))
        ovf = out.get("overflow")
        if ovf is None:
            fv["overflow"].zero_()
        else:
            fv["overflow"].copy_(ovf.reshape(1).to(torch.float32))
        if self.scatter:
            c = self.padded_g // self.world
            mine = st[self.rank * c:(self.rank + 1) * c]
            if dist.get_backend(self.group) == "gloo":      # gloo has no reduce-scatter: same sums, more bytes
                dist.all_reduce(st[:self.padded_g], op=dist.ReduceOp.SUM, group=self.group)
            else:
                dist.reduce_scatter_tensor(mine, st[:self.padded_g], op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(st[self.padded_g:], op=dist.ReduceOp.SUM, group=self.group)    # 2 N + 2 floats
        elif self.world > 1 or self.force or (self.always_pack and self.compact):
            if self.compact:
                self._compact_all_reduce(st, fv, active=getattr(self.compute_fn, "last_active", None))
            else:
                dist.all_reduce(st, op=dist.ReduceOp.SUM, group=self.group)   # the step's ONE collective
        grads = unpack_grads(st[:n_g], self.shapes, N)
        return dict(grads=grads, grad2d=fv["grad2d"], vis=fv["vis"], radii=radii, loss=fv["loss"][0],
                    overflow=fv["overflow"][0])


def _row_mask(fv, N):
    """Rows with any non-zero gradient entry (uint8).  Exact by construction: a row outside the mask is all zeros."""
    m = fv["grad2d"] != 0
    for name, w in GRAD_LAYOUT:
        m = m | (fv[name].view(N, w).abs().amax(dim=1) > 0)
    return m.to(torch.uint8)


_XCH_SEGS = list(GRAD_LAYOUT) + [("grad2d", 1)]


def _compact_all_reduce(self, flat, fv, active=None):
    """Two collectives: (1) one byte-sized SUM all-reduce of [row mask | visibility count] (2 N bytes: the visibility
    count is needed for every Gaussian -- a hidden Gaussian still counts as visible, gaussian.py:335-338 -- but it is
    at most the number of views, so a byte carries it); (2) the SUM all-reduce of the 60 floats (59 gradients + the
    2D-gradient norm) of the rows that are active on some rank.

    On the GPU everything around the two collectives is five launches of the library (csrc/exchange.hip): the mask -- from
    the fused backward's own list of the Gaussians that received a gradient when the compute function hands it over
    (`active`), otherwise from the rows --, the ordered row list (two launches), one pack, one unpack.  The host reads
    NOTHING in the middle of the step (round 6): the second collective is sized by a row capacity chosen beforehand -- the
    union's size of the step before + 25 % (+ 1024; all N rows the first time), the same on every rank --, the pack / unpack kernels take the actual
    count from the device, rows between count and capacity travel as zeros, and a union that outgrows the capacity adds to
    the step's overflow word (summed over the ranks: `Trainer._run_step` runs the step again, by which time the count has
    arrived on the host through an asynchronous copy and the capacity has grown).  `self.last_rows`: the count of the step before.  Tensors on the CPU (the gloo tests of the rank logic, where a CPU stand-in
    computes the gradients) take the same steps in torch."""
    N = self.N
    if self.n_views > 255:
        raise ValueError("compact all-reduce carries the visibility count in one byte: at most 255 views per step (use the dense mode)")
    live = self.world > 1 or self.force
    if flat.is_cuda:
        L = lib()
        dev = flat.device
        nseg = len(_XCH_SEGS)
        base = flat.data_ptr()
        offs = (ctypes.c_int64 * nseg)(*[(fv[name].data_ptr() - base) // 4 for name, _ in _XCH_SEGS])
        widths = (ctypes.c_int * nseg)(*[w for _, w in _XCH_SEGS])
        vis_off, tail_off = (fv["vis"].data_ptr() - base) // 4, (fv["loss"].data_ptr() - base) // 4
        sc = getattr(self, "_xch", None)
        if sc is None or sc["small"].device != dev:
            sc = self._xch = dict(small=torch.empty(2 * N, dtype=torch.uint8, device=dev), idx=torch.empty(N, dtype=torch.int32, device=dev),
                                  count=torch.zeros(1, dtype=torch.int32, device=dev),
                                  ws=torch.empty(L.mgr_exchange_index_workspace_bytes(N), dtype=torch.uint8, device=dev),
                                  host=torch.zeros(1, dtype=torch.int32).pin_memory(), buf=None, ev=None, cap_rows=N)
        small, idx, count = sc["small"], sc["idx"], sc["count"]
        if sc["ev"] is not None:          # the count of the step before: the capacity follows it
            # (waited for, never queried: the capacity sizes a collective, and a choice that depended on timing could give two
            # ranks different sizes for the same all-reduce.  Under Trainer the copy is complete by now -- it reads the step's
            # overflow word on the host -- so the wait costs nothing there.)
            sc["ev"].synchronize()
            n_seen = int(sc["host"][0])
            self.last_rows, sc["ev"] = n_seen, None
            sc["cap_rows"] = min(N, int(n_seen * 1.25) + 1024)
        cap_rows = int(getattr(self, "row_capacity", None) or sc["cap_rows"])      # (row_capacity: a test's fixed capacity)
        lst, cnt = active if active is not None else (None, None)
        check(L.mgr_exchange_mask(N, ptr(flat), nseg, offs, widths, vis_off, lst, cnt, ptr(small), stream()), "mgr_exchange_mask")
        if live:
            dist.all_reduce(small, op=dist.ReduceOp.SUM, group=self.group)
        check(L.mgr_exchange_index(N, ptr(small), ptr(idx), ptr(count), ptr(sc["ws"]), sc["ws"].numel(), stream()), "mgr_exchange_index")
        need = cap_rows * (GRAD_WIDTH + 1) + FLAT_TAIL
        if sc["buf"] is None or sc["buf"].numel() < need:
            sc["buf"] = torch.empty(need + 64, dtype=torch.float32, device=dev)
        buf = sc["buf"][:need]
        check(L.mgr_exchange_pack_rows(N, cap_rows, ptr(count), ptr(idx), ptr(flat), nseg, offs, widths, tail_off, ptr(buf), stream()),
              "mgr_exchange_pack_rows")
        if live:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
        check(L.mgr_exchange_unpack_rows(N, cap_rows, ptr(count), ptr(idx), ptr(flat), nseg, offs, widths, tail_off, ptr(buf),
                                         small[N:].data_ptr(), vis_off, stream()), "mgr_exchange_unpack_rows")
        if sc["ev"] is None:                                   # the count travels to the host behind the step (read by a later one)
            sc["host"].copy_(count, non_blocking=True)
            sc["ev"] = torch.cuda.Event()
            sc["ev"].record()
        self.last_cap_rows = cap_rows
        return
    small = torch.cat([_row_mask(fv, N), fv["vis"].to(torch.uint8)])
    if live:
        dist.all_reduce(small, op=dist.ReduceOp.SUM, group=self.group)
    fv["vis"].copy_(small[N:])
    idx = torch.nonzero(small[:N], as_tuple=False)[:, 0]                     # (host sync: the collective's size)
    n = idx.shape[0]
    self.last_rows = n
    width = GRAD_WIDTH + 1
    buf = torch.empty(n * width + FLAT_TAIL, dtype=torch.float32, device=flat.device)
    o, segs = 0, []
    for name, w in _XCH_SEGS:
        seg = buf[o:o + n * w].view(n, w)
        torch.index_select(fv[name].view(N, w), 0, idx, out=seg)
        segs.append((name, w, seg))
        o += n * w
    buf[o:o + FLAT_TAIL].copy_(flat[-FLAT_TAIL:])   # (loss, overflow: the last two floats of the step buffer)
    if live:
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
    for name, w, seg in segs:                                                # rows outside the union are zero everywhere
        fv[name].view(N, w).index_copy_(0, idx, seg)
    flat[-FLAT_TAIL:].copy_(buf[o:o + FLAT_TAIL])


ViewShardedStep._compact_all_reduce = _compact_all_reduce


class _DepthCut:
    """The depth-cut hints of one `HipViewCompute` and the policy of using them (fused step only).

    Every forward leaves, per tile whose pixels all saturated, the depth in front of which they had stopped (+ a margin);
    the next forward of the SAME views leaves the instances behind it out of that tile's list (mgr_views_forward, MGR_FWD_DEPTH_CUT)
    -- the binning kernels then handle a fraction of the pairs, the image and the gradients stay bit for bit those of the full
    lists (a cut list that runs out under an unsaturated pixel is flagged like a pair-capacity overflow and the step is run
    again without the cut).  The hints live in the workspace; when the view set changes they are parked per view set
    (`max_sets` sets of 4 bytes per tile and view, at most MAX_HINT_BYTES) and brought back when it returns -- a training
    run revisits its (frame, camera) pairs every epoch.  OFF by default (`HipViewCompute.depth_cut`): it pays only while the
    model stands still between two forwards of its views (fwd+bwd loops without an optimizer, evaluation sweeps); under a
    moving model it is a wash.

    A flagged forward costs a whole step, and with the optimizer in the loop no margin prevents them all: a pixel whose
    transmittance ends just under the threshold needs many more entries after the slightest change (measured on the bench
    scene with Adam at the reference's learning rates: a flagged forward every ~30 steps at 4x the margins).  So the cut backs
    off: a flagged forward doubles the margins (every clean one takes 2 % off again, 1x .. 32x the library's defaults),
    restricts the hints to interior tiles, and suspends the cut for `backoff` forwards -- 4, then 8, ... up to 512; 32 clean
    forwards in a row halve it again.  A model that stands still between two forwards of its views (fwd+bwd benchmarks,
    evaluation sweeps, several losses on one state) keeps the cut on; one that moves every step ends up trying it every few
    hundred steps, at a cost below the run-to-run noise.  Hints that have seen more than `max_age` parameter updates are not
    used at all (a dataset of thousands of views revisits each once per epoch: the forward then simply runs uncut and leaves
    fresh hints).

    With the on-device repair (round 6, `HipViewCompute.cut_repair`) tiles whose cut list runs out are completed on the device
    (MGR_FWD_REPAIR) -- no flagged forward, no re-run, no back-off: a flagged forward is then a capacity matter, rare, and
    the margins need neither widening nor the interior-only rule (the library's per-tile countdown keeps the repeat offenders
    out).  `margin` scales the library's default margins there, `penalty` = forwards a tile that ran out goes without a hint.

    `decide` is the policy: host arithmetic on this object's counters, no tensor and no library call.  `flag` is the workspace
    part: it names the views in the workspace, sets the library's margins and parks / restores the hint tables."""

    MAX_HINT_BYTES = 64 << 20

    def __init__(self, max_hints=1024):
        self.gen = 0              # model generation (`new_generation`)
        self.clock = 0            # parameter updates so far
        self.born = {}            # hint key -> clock at the last forward of those views
        self.max_age = 16
        self.scale = 1.0          # margin scale of the legacy mode
        self.seen = 0             # the context's count of flagged forwards at the last launch
        self.pause = 0            # forwards still to go without the cut
        self.backoff = 4          # the pause the next flagged forward starts
        self.clean = 0            # forwards with the cut in a row
        self.store = {}           # hint key -> parked hint tables
        self.max_sets = int(max_hints)
        self.bit = 0              # MGR_FWD_* flags of the step's current forward

    def new_generation(self):
        self.gen += 1
        self.store.clear()
        self.born.clear()

    def decide(self, key, cut_retries, cut_block, repair, margin=1.0):
        """(0, MGR_FWD_DEPTH_CUT or MGR_FWD_DEPTH_CUT | MGR_FWD_REPAIR; arguments of mgr_raster_set_cut_margin) for a forward of the views `key`.  cut_retries:
        the context's count of flagged forwards; cut_block: the previous forward on the workspace was flagged (this one
        rebuilds the hints from full lists)."""
        if cut_retries != self.seen:          # a forward of ours was flagged since the last launch
            self.seen, self.scale = cut_retries, min(32.0, self.scale * 2.0)
            self.pause, self.backoff, self.clean = self.backoff, min(512, self.backoff * 2), 0
        else:
            self.scale = max(1.0, self.scale * 0.98)
        k = self.scale
        if repair:
            margins = (0.125 * margin, int(64 * margin), 0.0625 * margin, 2.0e-4 * margin, 0)
        else:
            margins = (min(4.0, 0.125 * k), int(64 * k), min(4.0, 0.0625 * k), 2.0e-4 * k, 1 if k > 1.0 else 0)
        born, self.born[key] = self.born.get(key), self.clock
        if len(self.born) > 4 * self.max_sets:     # view sets not seen for max_age updates have no usable hints
            self.born = {k_: b_ for k_, b_ in self.born.items() if self.clock - b_ <= self.max_age}
        if cut_block or born is None or self.clock - born > self.max_age:
            return 0, margins
        if self.pause > 0:     # backing off after a flagged forward (repair: one of its capacities was exceeded -- a few forwards
            self.pause = (min(self.pause, 4) if repair else self.pause) - 1       # on full lists, no escalation)
            return 0, margins
        if repair:
            return _lib.MGR_FWD_DEPTH_CUT | _lib.MGR_FWD_REPAIR, margins
        self.clean += 1
        if self.clean >= 32:
            self.clean, self.backoff = 0, max(4, self.backoff // 2)
        return _lib.MGR_FWD_DEPTH_CUT, margins

    def flag(self, ws, view_ids, cut_retries, hint_offsets, hint_bytes, repair, margin, penalty):
        """MGR_FWD_* flags of mgr_views_forward for this forward on `ws`: MGR_FWD_DEPTH_CUT when the workspace holds the hints of exactly these
        views (left by the previous forward, or parked earlier and brought back here) and `decide` lets them be used.
        hint_offsets, hint_bytes: the hints (tile_zcut) and the repair's depth windows that belong to them (tile_zwin) in `ws.buf`."""
        key = (id(self), self.gen, tuple(view_ids))
        prev, ws.hint_key = ws.prev_hint_key, key
        cut_block, ws.cut_block = ws.cut_block, False
        bits, margins = self.decide(key, cut_retries, cut_block, repair, margin)
        lib().mgr_raster_set_cut_margin(*margins)
        if repair:
            lib().mgr_raster_set_cut_penalty(int(penalty))
        if prev != key:
            regions = [ws.buf[o: o + hint_bytes] for o in hint_offsets]
            nbytes = sum(r.numel() for r in regions)
            if prev is not None and prev[:2] == key[:2]:      # park the hints of the views rendered last
                max_sets = max(1, min(self.max_sets, self.MAX_HINT_BYTES // max(1, nbytes)))
                while len(self.store) >= max_sets:
                    self.store.pop(next(iter(self.store)))
                self.store[prev] = torch.cat(regions)
            saved = self.store.pop(key, None)
            if saved is not None and saved.numel() == nbytes:
                for r, part in zip(regions, saved.split(hint_bytes)):
                    r.copy_(part)
            else:
                for r in regions:
                    r.zero_()                                       # no hints for these views yet
        return bits


class _KeptBuffers:
    """The gradient, statistics and image tensors a `HipViewCompute` with persistent_grads keeps from step to step (fused
    step, no grad_arena): the leaf gradients, the skin-weight gradient, the statistics and the image are written into these
    buffers (see HipViewCompute's docstring).  The backward then zeroes only the rows that were written by the previous step
    and get nothing now, instead of every row of every gradient every step (mgr_views_backward, MGR_BWD_OUTPUTS_KEPT: 97 MB of stores
    per bench step), and the forward writes the background only into empty tiles that held something else
    (mgr_views_forward, MGR_FWD_IMAGE_KEPT).  Both need the workspace's row / tile state to describe THESE buffers: `grad_ws` and
    `image_ws` name the workspace whose last backward / forward wrote them, None when nobody's does."""

    def __init__(self):
        self.key = None           # (N, n_art, device) the tensors were made for
        self.device = None
        self.tensors = {}         # name -> tensor
        self.versions = {}        # name -> torch version counter as of the end of the last step
        self.grad_ws = None
        self.image_ws = None

    def begin(self, N, n_art, device):
        """Start of a step: new tensors when the model or the device changed; full fills when somebody wrote into them."""
        if self.key != (N, n_art, str(device)):
            self.key, self.device, self.tensors, self.versions = (N, n_art, str(device)), device, {}, {}
            self.invalidate()
        elif self.touched():
            self.invalidate()

    def get(self, shape, name, zeroed=True):
        t = self.tensors.get(name)
        if t is None:
            t = self.tensors[name] = (torch.zeros if zeroed else torch.empty)(shape, dtype=torch.float32, device=self.device)
        return t

    def touched(self):
        """Somebody wrote into a buffer since it was handed out (torch bumps a tensor's version counter on every in-place op,
        also through views): it no longer holds what the row / tile bookkeeping says."""
        return any(self.tensors[n]._version != ver for n, ver in self.versions.items() if n in self.tensors)

    def handed_out(self, ws):
        """End of a backward on `ws`: its row state is ours, and the tensors go to the caller as they are now."""
        self.grad_ws = ws
        self.versions = {n: t._version for n, t in self.tensors.items()}

    def invalidate(self):
        self.grad_ws = self.image_ws = None


def _arena_tensor(arena, device, shape, name):
    """The arena's buffer of that name viewed as `shape` if it fits, else a fresh tensor."""
    t = arena.get(name)
    n = 1
    for d in shape:
        n *= d
    if t is not None and t.numel() == n and t.is_contiguous() and t.dtype == torch.float32 and t.device == device:
        return t.view(shape)
    return torch.empty(shape, dtype=torch.float32, device=device)


class HipViewCompute:
    """compute_fn over the HIP kernels: skin weights once, LBS per pose, SH colour and rasterisation per view,
    image loss (rgb_loss / ssim_loss of src/modules/base.py:323-365), backward to the six leaf tensors.  All local
    views go through every kernel launch together.

    scene["kind"]: "hand" (every Gaussian skinned, hand_dynamic.py:86-137), "object" (static, object.py:32-41) or
    "composite" (the first scene["n_hand"] Gaussians skinned, the rest static with the identity transform,
    composite.py:50-59).  fused=True runs the fused kernels through direct C-ABI calls (no autograd graph); fused=False
    the modular operators under autograd (the reference-shaped path).

    ONE set of defaults for the step, shared by `Trainer`, `bench.py` and a hand-built object: depth cut off, gradient /
    image buffers kept (`persistent_grads`).  With kept buffers the tensors in a step's output dict (`grads`, `grad2d`,
    `vis`) and `last_image` are the SAME storage every step, like `.grad` tensors: they hold the latest step's values --
    clone what must outlive the next call, or construct with persistent_grads=False for fresh tensors per call.  Writing
    into them is allowed: every step compares the tensors' torch version counters with those it recorded when it handed
    them out, and a buffer touched in between (any in-place torch op on it or on a view of it) is filled in full again
    instead of row- / tile-selectively (tests/test_gpu_fused.py::test_kept_buffers_survive_a_caller_writing_into_them).
    Writes torch cannot see (raw pointers, `.data`) are the caller's to avoid.

    The image loss of the fused step ("l1+ssim") has four routes, chosen per step from plain attributes (settable after
    construction; the MANUS_* environment switches set their defaults for A/B runs):
      sparse_loss   the forward's tile-list offsets go to the image loss, which then settles the spans under empty tiles from
                    the target alone (exact: the rasterizer writes the background colour there) and leaves their gradient
                    unwritten (the backward never reads it).  False: the loss reads both images everywhere.
      target_map    the span list is derived from column masks "target differs from the background here", which the list
                    kernel otherwise recomputes from the full target images every step (0.2 GB at 8 views of 1080p).  A
                    target is a constant of its view: the masks are computed once per view (1 bit per pixel column and row
                    pair, 130 KB per 1080p view) and the list is built from them, in-stream, in a few microseconds -- no
                    second stream, no forward split at the blend.  Same list, same loss and gradients.  MANUS_TARGET_MAP=0.
      attach_list   that mapped list is built by the forward's last kernel (mgr_views_forward_attach_loss_list) instead of a
                    launch of its own.  MANUS_LOSS_LIST_ATTACH=0.
      overlap_loss  without target maps: the span list is built on a second stream while the forward blend runs (forward split
                    at the blend, MGR_FWD_NO_BLEND / MGR_FWD_BLEND_ONLY).  MANUS_OVERLAP_LOSS=0.

    SSIM statistic (`ssim`; a plain attribute, "rows" or "spatial", anything else raises ValueError at the step): "rows"
    (default) is the reference's ssim() on its HWC images, the window over the (W,3) plane of every image row -- the step without
    the keyword, bit for bit.  "spatial" with loss="l1+ssim": the image term of both routes is w_rgb * mean|d| + w_ssim * (1 - mean S) of
    the standard 2-D SSIM (`ops.image_loss2d_grad`, csrc/ssim2d.hip) on the same scales; the fused step then takes the plain
    route (no span list, dL/dimage written in full) and LPIPS, the map terms, pose_grad and skin_grid_grad work behind it
    unchanged.  The output dict gains "loss_ssim": the unweighted sum over the views of 1 - mean S_v on the step's scale (one
    rank only, like "loss_lpips").  With loss="l1" the attribute has no effect.

    Map supervision (`mask_targets`, `w_mask`, `depth_targets`, `w_depth`; plain attributes, settable after construction): with
    `mask_targets` (V_all,H,W) and a non-zero weight the step adds, per view,
        w_mask * mean|alpha - mask| + w_depth * mean(mask * |depth - depth_target|)
    on the accumulated-opacity and expected-depth maps of the view (`rasterizer.blend_features`), on the scale convention of the
    image term (`scale` * sum over the views).  The depth term needs `depth_targets` (V_all,H,W) as well.  Fused: feature render
    on the step's lists, mgr_map_loss, mgr_views_maps_backward adding into the step's gradient buffers; modular: the same loss
    through `rasterize_views_features` and `losses.map_loss` under autograd.  The output dict gains "loss_mask" / "loss_depth"
    (the unweighted terms on that scale) and "loss" includes the weighted sum.  With a term on, the fused step fills its
    gradient buffers in full every step (no MGR_BWD_OUTPUTS_KEPT), `last_active` is None, and grad2d / vis / radii stay the
    COLOUR loss's statistics (the modular route's grad2d includes the map term: DESIGN.md section 9).  Not combined with
    depth_cut (ValueError).  With pose_grad, "d_transforms" includes the map terms (fused: mgr_views_maps_backward_pose adds
    them to the colour backward's); with skin_grid_grad, "d_skin_grid" is formed from the summed skin-weight gradient over its
    non-zero rows (up to 8 views; all rows beyond).  With both weights zero or no mask the step is exactly the step without
    these arguments.

    LPIPS (`lpips`, `w_lpips`, `lpips_on`; plain attributes): with a VGG `manus_amd.lpips.LPIPS` and a non-zero weight the step
    adds scale * w_lpips * sum over the views of d(render_v, target_v), the reference's lpips_loss term (base.py:333-341), on the
    scale of the image loss and the map terms.  Its gradient travels through the image on both routes (mgr_lpips adds it to
    dL/dimage before the backward), so grad2d / vis see the term, unlike the map terms.  `lpips_on` gates it per step (a Trainer
    sets it from start_lpips_iter); the output dict gains "loss_lpips" (the unweighted term on that scale) and `last_lpips`
    holds it (None with the term off).  Off -- no network, weight zero or lpips_on False -- the step is exactly the step without
    these arguments.

    LPIPS windows (`lpips_rects`, `lpips_norm`, `lpips_cache_targets`; plain attributes): `lpips_rects` is a HOST table (V_all,4)
    of ints x0, y0, w, h indexed by view id like `targets` (the caller's, or `frames.FrameStore.load_step(lpips_rects=True)`'s;
    never found on the device); with it view v's term is the LPIPS of the CROPS of render and target at its rectangle
    (`LPIPS.values_grad(rects=)`: the crop's own zero padding and spatial means, not the full-frame value restricted to the
    region), only the rectangle is convolved (times: DESIGN.md section 6), and the gradient is zero outside it.  An empty rectangle turns a
    view's term off.  `lpips_norm`: "frame" (default) multiplies view v's value and gradient by (w h) / (W H), which keeps
    `w_lpips` on the scale of the full-frame term -- an APPROXIMATION: the full-frame spatial mean is diluted by the background
    where both images agree, but the crop's padding and the features near its edge differ from the frame's; "window" applies no
    factor (full-frame rects then give the step without rects, bit for bit).  `lpips_cache_targets` True keeps the target
    tower's taps of the step's view set beside the other per-view constants (`LPIPS.target_taps`; same bits, the target
    tower skipped, 122 floats per window pixel and view of memory): dropped with them -- `view_constants_changed()`, a version-counter
    change of `targets` -- and on new rects.  None (default): exactly the step above.  `lpips_batch` (a plain attribute like the
    others): the most views per launch of the windowed term and of the cached taps build (`LPIPS.values_grad(batch=)`,
    `LPIPS.target_taps(batch=)`): views whose rectangles share a size run as one chain of launches, the same bits (so it is no
    part of the window cache's key); `FrameStore.lpips_fit` gives a drawn step such rectangles.  0 (default) is the step above.

    Per-camera exposure (`exposure`, `exposure_ids`, `exposure_on`; plain attributes): `exposure` is a (C,3,4) fp32 device table
    E, one affine colour transform per camera (csrc/exposure.hip), used as it is -- never copied, so whoever steps it
    (`exposure.ExposureRefiner`) is seen by the next step; `exposure_ids` a HOST int sequence over all view rows giving each
    view's table row (default: the view id itself, which needs C == V_all; a row outside [0,C) leaves the view uncorrected).
    With a table and `exposure_on` true both routes apply E to the render (`mgr_exposure_apply`), take every image term -- L1,
    either SSIM, LPIPS full-frame, windowed or batched -- on the corrected image out', DENSE (no span list: under empty tiles
    out' is the corrected background, not the target), send dL/dout' through `mgr_exposure_backward` in place and hand the
    rasterizer's backward the raw render and dL/drender.  Map terms are untouched.  The output dict gains "d_exposure" (V,3,4)
    by position, on the scale of `grads`; `last_image` stays the raw render, `last_corrected` holds out' (None with the
    correction off).  `_step_direct(g_img=...)` is a gradient with respect to the render and bypasses the correction.  No
    reference counterpart.  None, or `exposure_on` False: exactly the step without these arguments."""

    # per-view target maps kept (130 KB per 1080p view)
    MAX_TARGET_MAPS = 4096

    def __init__(self, scene, targets, cam_table, loss_weight=1.0, fused=True, loss="l1", w_rgb=0.8, w_ssim=0.2,
                 sh_storage="fp32", sparse_loss=True, overlap_loss=True, depth_cut=False, max_cut_hints=1024,
                 persistent_grads=True, pose_grad=False, skin_grid_grad=False, mask_targets=None, w_mask=0.0, depth_targets=None,
                 w_depth=0.0, lpips=None, w_lpips=0.0, lpips_rects=None, lpips_norm="frame", lpips_cache_targets=False,
                 lpips_batch=0, ssim="rows", exposure=None, exposure_ids=None):
        if sh_storage not in ("fp32", "fp16"):
            raise ValueError("sh_storage must be 'fp32' or 'fp16'")
        if loss not in ("l1", "l1+ssim"):
            raise ValueError("loss must be 'l1' or 'l1+ssim'")
        self.ssim = ssim                # "rows" | "spatial" (class docstring); a plain attribute, asked again at every step
        self._loss_ssim = None          # "spatial": the step's unweighted SSIM term
        self._ssim_mode()
        env = os.environ.get
        self.ops, self.rz, self.fz, self.fused = ops, rasterizer, fused_mod, fused
        # -- scene and per-view constants
        self.s = scene
        self.kind = scene["kind"]
        self._cache = {}                # per-view-set gathers (`_select`)
        self._const_stamp = None
        self._tmaps = {}                # per-view target maps (`_target_map`)
        self.targets = targets          # (V_all,3,H,W) on the GPU (a property: replacing it drops what was derived from it)
        self.cams = cam_table           # (V_all,40)
        # -- map supervision (class docstring): (V_all,H,W) masks / depth targets and their weights
        self._mask_targets = self._depth_targets = None
        self._map_bufs = {}             # fused route: maps, their gradients and the scratch of the map chain, kept across steps
        self.w_mask, self.w_depth = float(w_mask), float(w_depth)
        # -- LPIPS term (class docstring)
        if lpips is not None and getattr(lpips, "net", None) != "vgg":
            raise ValueError("lpips: the training term takes a VGG manus_amd.lpips.LPIPS (the AlexNet network is forward only)")
        self.lpips, self.w_lpips, self.lpips_on = lpips, float(w_lpips), True
        self.last_lpips = None
        if lpips_norm not in ("frame", "window"):
            raise ValueError("lpips_norm must be 'frame' or 'window' (got %r)" % (lpips_norm,))
        self.lpips_rects, self.lpips_norm, self.lpips_cache_targets = lpips_rects, lpips_norm, bool(lpips_cache_targets)
        self.lpips_batch = int(lpips_batch)
        # -- model
        self.params = {k: v.detach().clone().requires_grad_(True) for k, v in scene["params"].items()}
        N = self.params["_xyz"].shape[0]
        has_grid = scene.get("grid") is not None
        self.n_art = N if (self.kind == "hand" and has_grid) else (int(scene["n_hand"]) if (self.kind == "composite" and has_grid) else 0)
        self.is_hand = self.n_art > 0
        self.device = self.params["_xyz"].device
        # -- pose_grad True: the step's output dict gains "d_transforms" (len(view_ids), B, 4, 4) = dL/d(bone transforms of the
        # view's pose), on the scale of `grads` (fused: mgr_views_backward_pose; modular: autograd with the transforms a leaf of
        # the step).  No reference counterpart (its pose optimizer was never released); `manus_amd.pose` builds on it.
        self.pose_grad = bool(pose_grad)
        if self.pose_grad and not self.is_hand:
            raise ValueError("pose_grad needs articulated Gaussians: a %r scene without a skin grid has no bone transforms" % self.kind)
        self.grid = ops.SkinGrid(scene["grid"], scene["grid"].device) if self.is_hand else None
        # -- skin_grid_grad True: the step's output dict gains "d_skin_grid", the sparse dL/d(skin-weight grid) (`ops.SkinGridGrad`,
        # on the scale of `grads`) of `self.grid` -- one mgr_skin_grid_bwd behind the skin-weight backward, on its list (fused) or
        # on all articulated rows (modular, and fused beyond 8 views).  `optim.SkinGridAdam(self.grid, ...)` steps the grid on it.
        self.skin_grid_grad = bool(skin_grid_grad)
        if self.skin_grid_grad and not self.is_hand:
            raise ValueError("skin_grid_grad needs articulated Gaussians: a %r scene without a skin grid has nothing to differentiate" % self.kind)
        self._sg_kept = {}              # fused route: outputs and workspace of mgr_skin_grid_bwd, kept across steps
        self._skin_w = None             # modular route with skin_grid_grad: the step's skin weights, kept for their gradient
        self.last_skin_w_grad = None    # with skin_grid_grad: dL/dw (n_art,B) of the last step, what "d_skin_grid" was formed from
        self._w_cache = None            # forward-only skin weights of the current model state (forward_views_fused under no_grad)
        # -- image loss.  "l1": mean|render - gt| (rgb_loss alone); "l1+ssim": w_rgb * rgb_loss + w_ssim * ssim_loss, the image
        # terms of config/HAND_GAUSSIAN.yaml:22-23 (src/modules/base.py:323-365), one fused kernel.  Routes: class docstring.
        self.loss = loss
        self.loss_weight = loss_weight
        self.w_rgb = w_rgb
        self.w_ssim = w_ssim
        self.sparse_loss = bool(sparse_loss)
        self.target_map = env("MANUS_TARGET_MAP", "1") != "0"
        self.attach_list = env("MANUS_LOSS_LIST_ATTACH", "1") != "0"
        self.overlap_loss = bool(overlap_loss) and env("MANUS_OVERLAP_LOSS", "1") != "0"
        self._lws = {}                  # (V,H,W) -> kept workspace of the mapped span list
        self._side = None               # second stream of the overlap route
        self._ts_off = {}               # (V,N,W,H,capacity) -> mgr_raster_layout offsets (`_layout`)
        # -- depth cut (`_DepthCut`).  MANUS_DEPTH_CUT=0 in the environment forces it off; MANUS_CUT_REPAIR=0: the round-5
        # behaviour without the on-device repair (A/B)
        self.depth_cut = bool(depth_cut) and env("MANUS_DEPTH_CUT", "1") != "0"
        self.cut_repair = env("MANUS_CUT_REPAIR", "1") != "0"
        self.cut_margin = float(env("MANUS_CUT_MARGIN", "1.0"))
        self.cut_penalty = int(env("MANUS_CUT_PENALTY", "16"))
        self._cut = _DepthCut(max_cut_hints)
        # -- gradient outputs: kept buffers (`_KeptBuffers`), or the arena a ViewShardedStep sets (preallocated views of its
        # step buffer; fused path only), or fresh tensors
        self.persistent_grads = bool(persistent_grads)
        self._kept = _KeptBuffers()
        self.grad_arena = None
        self._pose_ws = None            # partial slots of mgr_views_backward_pose (kept across steps)
        self._map_pose_ws = None        # partial slots of mgr_views_maps_backward_pose (kept across steps)
        self._sg_rows = None            # fused route, skin_grid_grad with a map term: mask / list / count / workspace of `_d_w_rows`
        # -- sh_storage "fp16" (BASELINE config 5): the fused kernels read an fp16 copy of _features_rest (96 B instead of
        # 180 B per Gaussian and view group); arithmetic, gradients and the optimizer's master copy stay fp32.  The copy
        # is refreshed lazily after the leaves changed (`mark_params_changed`).  The reference has no fp16 mode:
        # parity is judged with "fp32".
        self.sh_half = sh_storage == "fp16"
        self._sh_copy = None
        self._sh_dirty = True
        # -- sync_check True: every fused forward reads the pair count back and retries on overflow (like the drop-in
        # operator).  A Trainer sets it False on ITS compute object: no host sync, the forward leaves an overflow fence
        # that Trainer._run_step polls.  (The device-wide policy of rasterizer.set_sync_policy is left alone.)
        self.sync_check = True
        self.mask_targets = mask_targets
        self.depth_targets = depth_targets
        self._map_terms()               # (the combinations a map term refuses)
        # -- per-camera exposure (class docstring): the table, each view row's table row, the per-step switch
        self.exposure, self.exposure_ids, self.exposure_on = exposure, exposure_ids, True
        self.last_corrected = None
        self._exp_rows = None           # (host rows of the last corrected step, their device vector)
        self._exp_ws = None             # workspace of mgr_exposure_backward, kept across steps
        self._exposure_table()

    def _exposure_table(self):
        """The exposure table of the step about to run (None: no correction); ValueError for a table or an id list the step
        cannot use.  Asked at construction and again at every step: the three are plain attributes."""
        E = self.exposure
        if E is None:
            return None
        V_all = int(self.cams.shape[0])
        if not torch.is_tensor(E) or E.dim() != 3 or tuple(E.shape[1:]) != (3, 4) or E.shape[0] < 1:
            raise ValueError("exposure must be a (C,3,4) tensor (got %s)" % (tuple(E.shape) if torch.is_tensor(E) else type(E),))
        if E.dtype != torch.float32 or not E.is_contiguous():
            raise ValueError("exposure must be a contiguous float32 table (got %s)" % (E.dtype,))
        if E.device != self.cams.device:
            raise ValueError("exposure is on %s, the step's views are on %s" % (E.device, self.cams.device))
        if self.exposure_ids is None:
            if E.shape[0] != V_all:
                raise ValueError("exposure has %d rows for %d views: pass exposure_ids (one table row per view row)" % (E.shape[0], V_all))
        elif len(self.exposure_ids) != V_all:
            raise ValueError("exposure_ids has %d entries for %d view rows" % (len(self.exposure_ids), V_all))
        return E if self.exposure_on else None

    def _exposure_rows(self, view_ids):
        """Device int32 vector: the table row of every view of the step (kept while the host rows stay the same)."""
        ids = self.exposure_ids
        rows = tuple(int(v) if ids is None else int(ids[v]) for v in view_ids)
        if self._exp_rows is None or self._exp_rows[0] != rows or self._exp_rows[1].device != self.device:
            self._exp_rows = (rows, torch.tensor(rows, dtype=torch.int32, device=self.device))
        return self._exp_rows[1]

    def _exposure_loss(self, img, E, sel, view_ids, scale):
        """The image terms of a corrected step: E applied to the raw render `img` (detached), `_image_loss` and `_lpips_term` on
        the corrected image -- dense: under empty tiles it is not the target --, the exposure backward in place.
        -> (loss, dL/dimg, LPIPS term or None, d_exposure (V,3,4) by position)."""
        rows = self._exposure_rows(view_ids)
        tgt = sel["targets"]
        corr = self.ops.exposure_forward(img, E, rows)
        loss, g = self._image_loss(corr, tgt, scale)
        lp = self._lpips_term(corr, tgt, scale, g, sel, view_ids)
        nbytes = int(lib().mgr_exposure_workspace_bytes(*[int(x) for x in (img.shape[0], img.shape[2], img.shape[3])]))
        if self._exp_ws is None or self._exp_ws.numel() < nbytes or self._exp_ws.device != img.device:
            self._exp_ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        g, d_E = self.ops.exposure_backward(img, E, rows, g, inplace=True, workspace=self._exp_ws)
        self.last_corrected = corr
        return loss, g, lp, d_E

    def _map_target(self, t, what):
        """A (V_all,H,W) float map on the step's device, or None; ValueError otherwise."""
        if t is None:
            return None
        shape = (self.cams.shape[0], int(self.s["height"]), int(self.s["width"]))
        if not torch.is_tensor(t) or tuple(t.shape) != shape or not t.is_floating_point():
            raise ValueError("%s must be a float tensor (V_all,H,W) = %s (got %s)" % (what, shape, tuple(t.shape) if torch.is_tensor(t) else type(t)))
        if t.device != self.cams.device:
            raise ValueError("%s is on %s, the step's views are on %s" % (what, t.device, self.cams.device))
        return t

    @property
    def mask_targets(self):
        return self._mask_targets

    @mask_targets.setter
    def mask_targets(self, t):
        self._mask_targets = self._map_target(t, "mask_targets")
        self._drop_view_constants()

    @property
    def depth_targets(self):
        return self._depth_targets

    @depth_targets.setter
    def depth_targets(self, t):
        self._depth_targets = self._map_target(t, "depth_targets")
        self._drop_view_constants()

    def _map_terms(self):
        """(mask term on, depth term on) of the step about to run; ValueError for a combination the map chain does not serve."""
        if self._mask_targets is None:
            return False, False
        depth = self.w_depth != 0.0 and self._depth_targets is not None
        mask = self.w_mask != 0.0
        if mask or depth:
            if getattr(self, "depth_cut", False):      # (the depth cut shortens the lists the maps are rendered on)
                raise ValueError("a map term (mask_targets with w_mask / w_depth) cannot be combined with depth_cut=True")
            for name in ("pose_grad", "skin_grid_grad"):
                # (the constructor's refusal, asked again at the step: the flags are plain attributes)
                if getattr(self, name, False) and not self.is_hand:
                    raise ValueError("%s=True needs articulated Gaussians: a %r scene without a skin grid has none (asked with a map term on)"
                                     % (name, self.kind))
        return mask, depth

    def _map_sel(self, sel, view_ids, depth):
        """The step's views of the mask (and depth) targets, cached with the other per-view constants."""
        if "masks" not in sel:
            sel["masks"] = self._mask_targets[list(view_ids)].float().contiguous()
        if depth and "depths" not in sel:
            sel["depths"] = self._depth_targets[list(view_ids)].float().contiguous()
        return sel["masks"], sel.get("depths") if depth else None

    @property
    def _pg_ws(self):      # (bench.py and the tests ask whether the selective fills are in use)
        return self._kept.grad_ws

    @property
    def _pimg_ws(self):
        return self._kept.image_ws

    @property
    def targets(self):
        return self._targets

    @targets.setter
    def targets(self, t):
        self._targets = t
        self._drop_view_constants()

    def _drop_view_constants(self):
        """Forget everything derived from the per-view constants (targets, background, cameras, poses)."""
        self._cache = {}
        self._tmaps.clear()
        self._const_stamp = None

    def view_constants_changed(self):
        """Someone wrote into `targets`, `mask_targets`, `depth_targets`, `cams` or the scene's transforms in a way torch's
        version counters do not see (a kernel given the raw pointer: `frames.FrameStore`): everything derived from them is
        rebuilt by the next step, and the depth-cut hints of the views rendered so far are dropped."""
        self._drop_view_constants()
        self._cut.new_generation()

    def gathered_transforms(self, view_ids):
        """The contiguous (len(view_ids),B+1,4,4) copy of the transforms the kernels read for exactly this view set, when one is
        cached and still valid; else None (the next step gathers it from the table)."""
        if not self.is_hand:
            return None
        self._check_view_constants()
        c = self._cache.get(tuple(view_ids))
        return None if c is None else c.get("T")

    def transforms_changed(self, written=None):
        """ONLY the scene's transforms moved, written through a raw pointer (`pose.PoseRefiner.apply`): the gathered transforms
        of the cached view set are refreshed from the table -- unless it is the view set `written`, whose gathered copy
        (`gathered_transforms`) the writer has filled itself -- and the depth-cut hints of the views rendered so far are
        dropped.  Everything that depends on the targets alone is kept: the gathered targets and cameras, target maps, mask and
        depth gathers, LPIPS windows and the cached target taps.  (`view_constants_changed()` drops all of it.)"""
        if self.is_hand:
            self._check_view_constants()
            skip = None if written is None else tuple(written)
            for key, c in self._cache.items():
                if key != skip and c.get("T") is not None:
                    c["T"].copy_(self.s["transforms"][list(key)])
        self._cut.new_generation()

    def _check_view_constants(self):
        """The target maps and the per-view-set gathers are functions of `targets`, `s["bg"]`, `cams` and the transforms:
        when one of those tensors was replaced or written in place (torch version counter) they are rebuilt."""
        s = self.s
        tfm = s.get("transforms") if self.is_hand else None
        stamp = tuple((id(t), t._version) if t is not None else None for t in (self._targets, s.get("bg"), self.cams, tfm, self._mask_targets, self._depth_targets))
        if stamp != self._const_stamp:
            if self._const_stamp is not None:
                self._drop_view_constants()
            self._const_stamp = stamp

    def set_params(self, params, n_art=None):
        """Re-point at new leaf tensors (after densification / pruning changed N)."""
        self.params = {k: v.detach().requires_grad_(True) for k, v in params.items()}
        if n_art is not None:
            self.n_art = int(n_art)
        elif self.kind == "hand" and self.is_hand:
            self.n_art = self.params["_xyz"].shape[0]
        self.grad_arena = None
        self._sh_dirty = True
        self._cut.new_generation()  # rows were added / removed: the hints of the old model are dropped

    def mark_params_changed(self):
        """The leaves were updated in place (optimizer step): derived storage copies are stale."""
        self._sh_dirty = True
        self._cut.clock += 1

    def _sh_storage(self, f_rest):
        """(pointer source tensor, sh_half flag) for the fused kernels."""
        if not self.sh_half:
            return f_rest, 0
        N = f_rest.shape[0]
        if self._sh_copy is None or self._sh_copy.shape[0] != N:
            self._sh_copy, self._sh_dirty = torch.empty((N, 48), dtype=torch.float16, device=f_rest.device), True
        if self._sh_dirty:
            check(lib().mgr_sh_to_half(N, ptr(f_rest), ptr(self._sh_copy), stream()), "mgr_sh_to_half")
            self._sh_dirty = False
        return self._sh_copy, 1

    def _select(self, view_ids):
        """Per-view constants for a set of views (cached: no per-step gather copies)."""
        self._check_view_constants()
        key = tuple(view_ids)
        c = self._cache.get(key)
        if c is None:
            idx = list(view_ids)
            c = dict(cams=self.cams[idx].contiguous(), targets=self.targets[idx].contiguous(),
                     T=self.s["transforms"][idx].contiguous() if self.is_hand else None)
            self._cache = {key: c}
        return c

    # -- modular, reference-shaped path (autograd) -------------------------------------------------
    def _posed(self, T):
        """posed means / covariances / transforms of all Gaussians for the poses T (P,B,4,4): LBS for the first
        n_art rows, identity for the rest."""
        p, ops = self.params, self.ops
        N, na = p["_xyz"].shape[0], self.n_art
        if na == 0:
            _, pcov1, _ = ops.lbs_cov(p["_xyz"], p["_scaling"], p["_rotation"], None, None)
            return p["_xyz"], pcov1[0], None
        w = ops.skin_weights(p["_xyz"][:na], self.grid, self.s["grid_center"], self.s["grid_scale"])
        if self.skin_grid_grad and w.requires_grad:
            w.retain_grad()
            self._skin_w = w
        pxyz, pcov, tf = ops.lbs_cov(p["_xyz"][:na], p["_scaling"][:na], p["_rotation"][:na], w, T)
        if na < N:   # composite.py:50-59: concat, identity tf for the object
            P = T.shape[0]
            _, ocov, otf = ops.lbs_cov(p["_xyz"][na:], p["_scaling"][na:], p["_rotation"][na:], None, None)
            pxyz = torch.cat([pxyz, p["_xyz"][na:][None].expand(P, -1, -1)], dim=1)
            pcov = torch.cat([pcov, ocov.expand(P, -1, -1)], dim=1)
            tf = torch.cat([tf, otf.expand(P, -1, -1)], dim=1)
        return pxyz, pcov, tf

    def forward_views(self, view_ids, T=None, maps=None):
        """T: the bone transforms to pose with instead of the scene's (the pose-gradient step passes a leaf).  maps = (alpha,
        depth) booleans: a fourth result, the differentiable maps of `rasterize_views_features`."""
        s, p, ops = self.s, self.params, self.ops
        sel = self._select(view_ids)
        cams = sel["cams"]
        V = len(view_ids)
        feats = torch.cat([p["_features_dc"], p["_features_rest"]], dim=1)
        opac = torch.sigmoid(p["_opacity"])
        pxyz, pcov, tf = self._posed(sel["T"] if T is None else T)   # one pose per view (the reference trains one (frame, view) per step)
        col = ops.sh_colors(feats, p["_xyz"], tf, cams)
        N = p["_xyz"].shape[0]
        means2D = torch.zeros((V, N, 3), dtype=torch.float32, device=cams.device, requires_grad=True)
        if maps is not None:
            img, radii, extras = self.rz.rasterize_views_features(cams, pxyz, means2D, col, opac, pcov, s["bg"], s["width"], s["height"],
                                                                  depth=bool(maps[1]), alpha=bool(maps[0]))
            return img, radii, means2D, extras
        img, radii = self.rz.rasterize_views(cams, pxyz, means2D, col, opac, pcov, s["bg"], s["width"], s["height"])
        return img, radii, means2D

    def forward_views_fused(self, view_ids, stats=None, grad2d_scale=1.0):
        """The fused kernels behind the autograd node `fused.render_views`."""
        s, p, ops = self.s, self.params, self.ops
        sel = self._select(view_ids)
        na = self.n_art
        w = None
        if na and not torch.is_grad_enabled():
            # forward only (evaluation sweeps, target rendering): the skin weights depend on `_xyz` alone, so they are kept per
            # model state -- (generation, parameter-update clock, the leaf's storage and version) -- instead of gathered from
            # the grid again for every batch of views (0.04 ms for 300 k Gaussians: 13 % of a one-view forward).  Training
            # steps always recompute them (their gradient flows back into `_xyz`).
            key = (self._cut.gen, self._cut.clock, p["_xyz"].data_ptr(), p["_xyz"]._version, na, id(self.grid), self.grid.version)
            if self._w_cache is None or self._w_cache[0] != key:
                self._w_cache = (key, ops.skin_weights(p["_xyz"][:na], self.grid, s["grid_center"], s["grid_scale"]))
            w = self._w_cache[1]
        elif na:
            w = ops.skin_weights(p["_xyz"][:na], self.grid, s["grid_center"], s["grid_scale"])
        return self.fz.render_views(p["_xyz"], p["_scaling"], p["_rotation"], p["_opacity"], p["_features_dc"],
                                    p["_features_rest"], w, sel["T"], sel["cams"], s["bg"], s["width"], s["height"],
                                    stats=stats, grad2d_scale=grad2d_scale, grad_arena=self.grad_arena)

    def _ssim_mode(self):
        """`self.ssim`, or ValueError for anything but "rows" / "spatial"."""
        if self.ssim not in ("rows", "spatial"):
            raise ValueError("ssim must be 'rows' or 'spatial' (got %r)" % (self.ssim,))
        return self.ssim

    def _loss_scales(self, img, scale):
        """(k, const) of the image-loss kernels for scale * sum over the views of the per-view loss of `img` (V,3,H,W):
        the factor on the per-pixel terms, and the "1 -" of 1 - ssim, once per view."""
        k = self.loss_weight * scale / img[0].numel()
        return k, self.w_ssim * self.loss_weight * scale * img.shape[0]

    def _lpips_term(self, img, tgt, scale, g_img, sel=None, view_ids=None):
        """The LPIPS term of the step: mgr_lpips ADDS the gradient of scale * w_lpips * sum_v d_v to g_img (V,3,H,W) and returns
        scale * sum_v d_v; None with the term off.  On the fused route g_img is unwritten under empty background tiles (the image
        loss leaves it so); the backward never reads there, so adding to whatever it holds is harmless.  With `lpips_rects` the
        views are windowed (class docstring): d_v is the crops' distance times the view's norm factor."""
        self.last_lpips = None
        if self.lpips is None or self.w_lpips == 0.0 or not self.lpips_on:
            return None
        if self.lpips_rects is None:
            vals, _ = self.lpips.values_grad(img.detach(), tgt, need_grad=True, grad_scale=scale * self.w_lpips, out_grad=g_img, accumulate=True)
            self.last_lpips = vals.sum() * scale
            return self.last_lpips
        win = self._lpips_window(sel, view_ids, tgt)
        k = scale * self.w_lpips
        vals, _ = self.lpips.values_grad(img.detach(), tgt, need_grad=True, out_grad=g_img, accumulate=True, rects=win["rects"],
                                         grad_scales=[k] * len(view_ids) if win["factors"] is None else [k * f for f in win["factors"]],
                                         target_taps=win["taps"], batch=self.lpips_batch)
        if win["factors"] is not None:
            vals = vals * win["factors_dev"]
        self.last_lpips = vals.sum() * scale
        return self.last_lpips

    def _lpips_window(self, sel, view_ids, tgt):
        """The windows of the step's views, kept with the other per-view constants of the view set: their rects, the norm
        factors (w h) / (W H) of lpips_norm = "frame" (host floats and a device vector; None for "window") and, with
        lpips_cache_targets, the target tower's taps.  Rebuilt when the rects of these views, the norm, the network or the
        cache switch differ from what the entry was built with; dropped with `sel` by `_drop_view_constants`."""
        if self.lpips_norm not in ("frame", "window"):
            raise ValueError("lpips_norm must be 'frame' or 'window' (got %r)" % (self.lpips_norm,))
        table = np.asarray(self.lpips_rects)
        if table.ndim != 2 or table.shape != (self.cams.shape[0], 4):
            raise ValueError("lpips_rects must be (V_all,4) = (%d,4) host ints x0, y0, w, h (got %s)" % (self.cams.shape[0], table.shape))
        rects = np.ascontiguousarray(table[list(view_ids)].astype(np.int32))
        cache = bool(self.lpips_cache_targets)
        key = (rects.tobytes(), self.lpips_norm, id(self.lpips), cache)
        win = sel.get("lpips")
        if win is None or win["key"] != key:
            factors = factors_dev = None
            if self.lpips_norm == "frame":
                area = float(int(self.s["width"]) * int(self.s["height"]))
                factors = [float(int(r[2]) * int(r[3])) / area for r in rects]
                factors_dev = torch.tensor(factors, dtype=torch.float32, device=self.device)
            win = sel["lpips"] = dict(key=key, rects=rects, factors=factors, factors_dev=factors_dev,
                                      taps=self.lpips.target_taps(tgt, rects, batch=self.lpips_batch) if cache else None)
        return win

    def _image_loss(self, img, tgt, scale, tiles=None):
        """(loss value, dL/dimg) of scale * sum over the views of the per-view image loss.  tiles = (bg, device address
        of the tile-list offsets of the forward that rendered img): spans under empty tiles are not read (ops.image_loss_grad)."""
        k, const = self._loss_scales(img, scale)
        if self.loss == "l1":
            loss_sum, g = self.ops.l1_loss_grad(img, tgt, scale=k)
            return loss_sum[0] * k, g
        if self._ssim_mode() == "spatial":
            # the standard 2-D SSIM (mgr_image_loss2d): the same scales, no span list, the gradient written in full
            sums, _, g = self.ops.image_loss2d_grad(img, tgt, self.w_rgb, self.w_ssim, k, const)
            self._loss_ssim = scale * (img.shape[0] - sums[1] / img[0].numel())
            return sums[2], g
        bg, ts = tiles if (tiles is not None and self.sparse_loss) else (None, None)
        sums, g = self.ops.image_loss_grad(img, tgt, self.w_rgb, self.w_ssim, k, const, bg=bg, tile_start_ptr=ts)
        return sums[2], g

    def _layout(self, ws, V, N, W, H):
        """Byte offsets of the regions of `ws.buf` (indexed by the LAYOUT_* constants)."""
        key = (V, N, W, H, ws.cap)
        off = self._ts_off.get(key)
        if off is None:
            arr = (ctypes.c_size_t * 40)()
            lib().mgr_raster_layout(V, N, W, H, ws.cap, arr, 40)
            off = self._ts_off[key] = [int(x) for x in arr]
        return off

    def _target_map(self, view_ids, sel, bg):
        """(V, rows / 2, ceil(W / 32)) int32: the target-vs-background column masks of the views (computed once per view)."""
        m = sel.get("tmap")
        if m is None:
            H, W = int(self.s["height"]), int(self.s["width"])
            per = int(lib().mgr_image_loss_target_map_words(1, H, W))
            rows = []
            for k, v in enumerate(view_ids):
                t = self._tmaps.get(v)
                if t is None:
                    t = torch.empty(per, dtype=torch.int32, device=self.device)
                    check(lib().mgr_image_loss_target_map(1, H, W, ptr(sel["targets"][k]), ptr(bg), ptr(t), stream()),
                          "mgr_image_loss_target_map")
                    while len(self._tmaps) >= self.MAX_TARGET_MAPS:
                        self._tmaps.pop(next(iter(self._tmaps)))
                    self._tmaps[v] = t
                rows.append(t)
            m = sel["tmap"] = torch.stack(rows).contiguous()
        return m

    def _tile_start_ptr(self, ws, V, N, W, H):
        return ws.buf.data_ptr() + self._layout(ws, V, N, W, H)[LAYOUT_TILE_START]

    def _cut_flag(self, ws, view_ids, V, N, W, H):
        """Depth-cut flags of mgr_views_forward for this forward on `ws` (`_DepthCut.flag`); 0 with the cut off."""
        ctx = self.rz.context(self.device)
        if not self.depth_cut or not ctx.fenced(self.sync_check):
            return 0      # (with a host sync per forward the split forward would need a second one after the blend: not worth it)
        lay = self._layout(ws, V, N, W, H)
        T = ((W + 15) // 16) * ((H + 15) // 16)
        return self._cut.flag(ws, view_ids, ctx.cut_retries, (lay[LAYOUT_TILE_ZCUT], lay[LAYOUT_TILE_ZWIN]), 4 * V * T,
                              self.cut_repair, self.cut_margin, self.cut_penalty)

    # -- fused path, direct C-ABI calls ------------------------------------------------------------
    def _step_direct(self, view_ids, scale, g_img=None):
        """skin weights -> mgr_views_forward -> image loss -> mgr_views_backward -> skin-weight backward, every
        gradient written straight into the arena (the all-reduce buffer) when one is set.  g_img: optional dL/dimage
        (V,3,H,W) used instead of the image loss (parity tests)."""
        s, p = self.s, {k: v.detach() for k, v in self.params.items()}
        sel = self._select(view_ids)
        dev = self.device
        N, na, V = p["_xyz"].shape[0], self.n_art, len(view_ids)
        W, H = int(s["width"]), int(s["height"])
        kept = self._kept if (self.persistent_grads and not self.grad_arena and self.fused) else None
        if kept is not None:
            kept.begin(N, na, dev)
        map_on = self._map_terms()
        w, B = self._skin_weights(p["_xyz"], na)
        if kept is not None:      # the image too is a kept buffer (MGR_FWD_IMAGE_KEPT)
            out = kept.get((V, 3, H, W), ("image", V, H, W), zeroed=False)
        else:
            out = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((V, N), dtype=torch.int32, device=dev)
        f_rest, sh_half = self._sh_storage(p["_features_rest"])
        # the leading arguments mgr_views_forward and mgr_views_backward share
        head = (V, N, B, na, sh_half, W, H, ptr(sel["cams"]), ptr(s["bg"]), ptr(p["_xyz"]), ptr(p["_scaling"]), ptr(p["_rotation"]),
                ptr(p["_opacity"].reshape(-1)), ptr(p["_features_dc"]), ptr(f_rest), ptr(w), ptr(sel["T"]))
        fwd = (head, out, radii, kept)
        # route of the image loss (class docstring): "mapped" / "overlap" span lists, or None = plain / g_img given
        self._loss_ssim = None
        self.last_corrected = None
        # (a given g_img is a gradient with respect to the render: it bypasses the correction)
        E = self._exposure_table() if g_img is None else None
        listed = g_img is None and E is None and self.loss == "l1+ssim" and self.sparse_loss and self._ssim_mode() == "rows"
        route = None if not listed else "mapped" if self.target_map else "overlap" if self.overlap_loss else None
        loss_list = self._mapped_loss_list(view_ids, sel, V, H, W) if route == "mapped" else None
        ctx = self.rz.context(dev)
        ws = None
        try:
            ws, _ = ctx.forward(V, N, W, H, self._forward_launch(fwd, view_ids, loss_list, _lib.MGR_FWD_NO_BLEND if route == "overlap" else 0),
                                sync_check=self.sync_check, defer_fence=True)
            if route != "overlap" and ctx.fenced(self.sync_check):
                ctx.fence(ws)
            given = g_img is not None
            d_E = None
            if E is not None:
                loss, g_img, lp, d_E = self._exposure_loss(out, E, sel, view_ids, scale)
            else:
                loss, g_img = self._loss(ctx, ws, fwd, sel, scale, g_img, route, loss_list)
                lp = None if given else self._lpips_term(out, sel["targets"], scale, g_img, sel, view_ids)
            grads, d_w, st_g, st_v, st_r, d_T = self._backward(ws, fwd, g_img, scale, full_rows=any(map_on))
            map_out = self._map_chain(ws, head, sel, view_ids, scale, map_on, grads, d_w, d_T) if any(map_on) else None
            active = self._skin_backward(ws, head, p["_xyz"], d_w, grads["_xyz"], full_rows=any(map_on))
            d_grid = self._skin_grid_backward(head, p["_xyz"], d_w, active, rows_of_d_w=any(map_on)) if self.skin_grid_grad else None
            overflow = ws.buf[4:8].view(torch.int32)
        except BaseException:
            # a call that failed between the loss's list and finish passes -- the forward included: its last kernel builds the
            # attached list -- leaves the kept loss workspace with a non-zero span count (the finish pass is what resets it) and
            # the kept buffers in an unknown state: start over
            self._lws.pop((V, H, W), None)
            self._kept.invalidate()
            raise
        finally:
            if ws is not None:
                ws.busy = False
        self.last_image, self.last_radii = out, radii
        self.last_active = active      # (device pointers into the workspace of this step: valid until the next forward on it)
        res = dict(grads=grads, grad2d=st_g, vis=st_v, radii=st_r, loss=loss, overflow=overflow)
        if map_out is not None:
            res["loss"] = loss + map_out[0]
            res["loss_mask"], res["loss_depth"] = map_out[1], map_out[2]
        if lp is not None:
            res["loss"] = res["loss"] + self.w_lpips * lp
            res["loss_lpips"] = lp
        if self._loss_ssim is not None:
            res["loss_ssim"] = self._loss_ssim
        if d_T is not None:
            res["d_transforms"] = d_T
        if d_E is not None:
            res["d_exposure"] = d_E
        if d_grid is not None:
            res["d_skin_grid"] = d_grid
        return res

    def _skin_weights(self, xyz, na):
        """(skin weights (na,B) of the articulated rows, B); (None, 0) without any."""
        if not na:
            return None, 0
        s, sg = self.s, self.grid
        w = torch.empty((na, sg.B), dtype=torch.float32, device=self.device)
        check(lib().mgr_skin_weights_fwd(na, ptr(xyz), ptr(sg.data), sg.D, sg.H, sg.W, sg.B, sg.stride,
                                         ptr(s["grid_center"]), ptr(s["grid_scale"]), ptr(w), stream()),
              "mgr_skin_weights_fwd")
        return w, sg.B

    def _mapped_loss_list(self, view_ids, sel, V, H, W):
        """(workspace, target maps, workspace bytes) of the mapped span list.  The workspace is kept across steps, zero-filled
        once: list / finish pairs leave it clean."""
        nbytes = int(lib().mgr_image_loss_workspace_bytes(V, H, W))
        lws = self._lws.get((V, H, W))
        if lws is None:
            lws = self._lws[(V, H, W)] = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return lws, self._target_map(view_ids, sel, self.s["bg"]), nbytes

    def _views_forward(self, ws, fwd, phase):
        """One mgr_views_forward on `ws`.  phase: 0 whole, MGR_FWD_NO_BLEND up to the blend, MGR_FWD_BLEND_ONLY the blend."""
        head, out, radii, kept = fwd
        # kept image: a tile that held the background after the previous forward on the same workspace and is empty again is not
        # written again (MGR_FWD_IMAGE_KEPT)
        bits = phase | self._cut.bit | ws.skip_bits() | (_lib.MGR_FWD_IMAGE_KEPT if (kept is not None and kept.image_ws is ws) else 0)
        check(lib().mgr_views_forward(*head, ptr(out), ptr(radii), ptr(ws.buf), ws.nbytes, ws.cap, bits, stream()), "mgr_views_forward")
        if kept is not None:
            kept.image_ws = ws

    def _forward_launch(self, fwd, view_ids, loss_list, phase):
        """What `RasterContext.forward` runs on the workspace it chose -- again after a capacity / tier retry: the depth-cut
        decision and the forward, with the mapped span list of the loss attached to it when there is one (extra workgroups of
        the forward's last kernel, attached per launch)."""
        V, N, W, H = fwd[0][0], fwd[0][1], fwd[0][5], fwd[0][6]
        launches = [0]

        def launch(ws):
            self._cut.bit = self._cut_flag(ws, view_ids, V, N, W, H)
            if loss_list is None or not self.attach_list:
                return self._views_forward(ws, fwd, phase)
            lws, tmap, nbytes = loss_list
            if launches[0]:          # a forward of this step ran before (capacity / tier retry): its list was never finished
                lws.zero_()
            launches[0] += 1
            check(lib().mgr_views_forward_attach_loss_list(ptr(ws.buf), V, H, W, ptr(tmap), ptr(lws), nbytes),
                  "mgr_views_forward_attach_loss_list")
            try:
                self._views_forward(ws, fwd, 0)
            except Exception:        # (a forward that failed before its last kernel leaves the attachment pending: withdraw it)
                lib().mgr_views_forward_attach_loss_list(ptr(ws.buf), V, H, W, None, None, 0)
                raise

        return launch

    def _loss(self, ctx, ws, fwd, sel, scale, g_img, route, loss_list):
        """(loss, dL/dimage) of the forward on `ws` by the step's route."""
        head, out = fwd[0], fwd[1]
        V, N, W, H = head[0], head[1], head[5], head[6]
        tgt, bg = sel["targets"], self.s["bg"]
        if route is None:
            if g_img is not None:
                return (out * g_img).sum(), g_img.contiguous()
            return self._image_loss(out, tgt, scale, tiles=(bg, self._tile_start_ptr(ws, V, N, W, H)))
        if route == "mapped":
            lws, tmap, nbytes = loss_list
            if not self.attach_list:      # the list in a launch of its own
                check(lib().mgr_image_loss_tiles_list_mapped(V, H, W, ptr(tmap), ptr(bg), ctypes.c_void_p(self._tile_start_ptr(ws, V, N, W, H)),
                                                             ptr(lws), nbytes, 1, stream()), "mgr_image_loss_tiles_list_mapped")
        else:
            # overlap: the span list needs the forward's tile offsets but not its image -- it is built on a second stream while
            # the forward blend runs
            nbytes = int(lib().mgr_image_loss_workspace_bytes(V, H, W))
            lws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            cur = torch.cuda.current_stream(self.device)
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                check(lib().mgr_image_loss_tiles_list(V, H, W, ptr(tgt), ptr(bg), ctypes.c_void_p(self._tile_start_ptr(ws, V, N, W, H)),
                                                      ptr(lws), nbytes, stream()), "mgr_image_loss_tiles_list")
            self._views_forward(ws, fwd, _lib.MGR_FWD_BLEND_ONLY)   # the blend, next to the list
            if ctx.fenced(self.sync_check):
                ctx.fence(ws)                           # (after the blend: it is the blend that raises the depth-cut flag)
            cur.wait_stream(self._side)
            lws.record_stream(self._side)
        k, const = self._loss_scales(out, scale)
        g_img = torch.empty_like(out)
        sums = torch.empty(3, dtype=torch.float32, device=self.device)
        check(lib().mgr_image_loss_tiles_finish(V, H, W, ptr(out), ptr(tgt), self.w_rgb, self.w_ssim, k, const, ptr(g_img),
                                                ptr(sums), ptr(lws), nbytes, stream()), "mgr_image_loss_tiles_finish")
        return sums[2], g_img

    def _map_chain(self, ws, head, sel, view_ids, scale, map_on, grads, d_w, d_T=None):
        """The map terms of the fused step, behind the colour backward: feature render (C = 0) of alpha and, with the depth term,
        the expected depth on the step's lists -> mgr_map_loss -> mgr_views_maps_backward ADDING to the leaf gradients and the
        skin-weight gradient the colour backward has just written.  d_T (pose_grad): mgr_views_maps_backward_pose instead, which
        also adds the map terms' pose gradient to the colour backward's d_transforms.  -> (weighted loss, mask term, depth term)
        on the step's scale (`scale` * sum over the views).  A forward that overflowed its pair capacity leaves no complete
        lists: the chain is skipped (zeros; d_T stays the colour term's) -- the step's overflow word tells the caller to run it
        again."""
        V, N, B, na, _, W, H = head[:7]
        cams, xyz, ls, rot, op, w, T = head[7], head[9], head[10], head[11], head[12], head[15], head[16]
        dev, L = self.device, lib()
        masks, depths = self._map_sel(sel, view_ids, map_on[1])
        key = (V, N, W, H, ws.cap, bool(map_on[1]))
        mb = self._map_bufs.get(key)
        if mb is None:
            e = functools.partial(torch.empty, dtype=torch.float32, device=dev)
            n_loss, n_scr = int(L.mgr_map_loss_workspace_bytes(V, H, W)), int(L.mgr_views_maps_backward_workspace_bytes(V, N, W, H, ws.cap))
            mb = dict(alpha=e((V, H, W)), g_alpha=e((V, H, W)), depth=e((V, 1, H, W)) if map_on[1] else None,
                      g_depth=e((V, 1, H, W)) if map_on[1] else None,
                      loss_ws=torch.empty(n_loss, dtype=torch.uint8, device=dev), scratch=torch.empty(n_scr, dtype=torch.uint8, device=dev))
            self._map_bufs = {key: mb}
        sums = torch.empty(3, dtype=torch.float32, device=dev)
        rc = L.mgr_raster_blend_features(V, N, 0, W, H, None, 0, None, int(map_on[1]), ptr(mb["depth"]), ptr(mb["alpha"]), ptr(ws.buf),
                                         ws.nbytes, ws.cap, stream())
        if rc == _lib.MGR_ESTATE and int(ws.buf[4:8].view(torch.int32).item()) != 0:
            z = torch.zeros((), dtype=torch.float32, device=dev)
            return z, z, z
        check(rc, "mgr_raster_blend_features")
        k = scale * V      # scale * sum over the views of a per-view mean = scale * V * the mean over all V H W elements
        check(L.mgr_map_loss(V, H, W, ptr(mb["alpha"]), ptr(masks), ptr(mb["depth"]), ptr(depths), self.w_mask,
                             self.w_depth if map_on[1] else 0.0, k, ptr(mb["g_alpha"]), ptr(mb["g_depth"]), ptr(sums), ptr(mb["loss_ws"]),
                             mb["loss_ws"].numel(), stream()), "mgr_map_loss")
        args = (V, N, B, na, W, H, cams, xyz, ls, rot, op, w, T, ptr(mb["alpha"]), ptr(mb["depth"]), ptr(mb["g_alpha"]), ptr(mb["g_depth"]), 1,
                ptr(grads["_xyz"]), ptr(grads["_scaling"]), ptr(grads["_rotation"]), ptr(grads["_opacity"]), ptr(d_w), ptr(ws.buf),
                ws.nbytes, ws.cap, ptr(mb["scratch"]), mb["scratch"].numel(), 0)
        if d_T is not None:
            nbytes = int(L.mgr_views_maps_pose_workspace_bytes(V, N, B))
            if self._map_pose_ws is None or self._map_pose_ws.numel() < nbytes:
                self._map_pose_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(L.mgr_views_maps_backward_pose(*args, 1, ptr(d_T), ptr(self._map_pose_ws), self._map_pose_ws.numel(), stream()),
                  "mgr_views_maps_backward_pose")
        else:
            check(L.mgr_views_maps_backward(*args, stream()), "mgr_views_maps_backward")
        return sums[2] * k, sums[0] * k, sums[1] * k

    def _backward(self, ws, fwd, g_img, scale, full_rows=False):
        """mgr_views_backward into the kept buffers, the arena or fresh tensors: (leaf gradients, skin-weight gradient,
        grad2d, vis, radii, dL/dtransforms or None).  full_rows: every row is filled (a map term adds rows behind this call that
        the library's row state does not know about)."""
        head, out, radii, kept = fwd
        V, N, B, na = head[:4]
        dev = self.device
        e = kept.get if kept is not None else functools.partial(_arena_tensor, self.grad_arena or {}, dev)
        grads = {name: e(shape, name) for name, shape in (("_xyz", (N, 3)), ("_scaling", (N, 3)), ("_rotation", (N, 4)), ("_opacity", (N, 1)),
                                                           ("_features_dc", (N, 1, 3)), ("_features_rest", (N, 15, 3)))}
        st_g, st_v = e((N,), "grad2d"), e((N,), "vis")
        st_r = torch.empty(N, dtype=torch.int32, device=dev)
        d_w = e((na, B), "_skin_w") if na else None
        # the buffers are those of the previous backward on this very workspace, untouched since: the library may skip the
        # zero fill of the rows it knows to be zero (it checks that its row state is that call's)
        bits = _lib.MGR_BWD_OUTPUTS_KEPT if (kept is not None and kept.grad_ws is ws and V <= 8 and not full_rows) else 0
        self._kept.grad_ws = None
        args = (*head, ptr(radii), ptr(out), ptr(g_img), 1.0 / scale, *[ptr(g) for g in grads.values()],
                ptr(d_w), ptr(st_g), ptr(st_v), ptr(st_r), ptr(ws.buf), ws.nbytes, ws.cap, bits)
        d_T = None
        if self.pose_grad:
            d_T = torch.empty((V, B, 4, 4), dtype=torch.float32, device=dev)
            nbytes = int(lib().mgr_views_pose_workspace_bytes(V, N, B))
            if self._pose_ws is None or self._pose_ws.numel() < nbytes:
                self._pose_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(lib().mgr_views_backward_pose(*args, ptr(d_T), ptr(self._pose_ws), self._pose_ws.numel(), stream()),
                  "mgr_views_backward_pose")
        else:
            check(lib().mgr_views_backward(*args, stream()), "mgr_views_backward")
        if kept is not None:
            kept.handed_out(ws)
            if full_rows:
                kept.grad_ws = None
        return grads, d_w, st_g, st_v, st_r, d_T

    def _skin_backward(self, ws, head, xyz, d_w, d_xyz, full_rows=False):
        """The backward's list of the Gaussians that received a gradient (device pointers: list, length; None beyond 8 views)
        and, through it, d xyz += d w . d(trilinear weights)/d xyz (the leaf is used twice: gaussian_utils.py:167-196).
        full_rows: no list, every articulated row (a map term wrote d_w rows outside the colour backward's list)."""
        V, N, _, na, _, W, H = head[:7]
        active = None
        if V <= 8 and N > 0 and not full_rows:
            lst, cnt = ctypes.c_void_p(), ctypes.c_void_p()
            check(lib().mgr_views_active_list(ptr(ws.buf), V, N, W, H, ws.cap, ctypes.byref(lst), ctypes.byref(cnt)),
                  "mgr_views_active_list")
            active = (lst, cnt)
        if not na:
            return active
        s, sg = self.s, self.grid
        grid = (na, ptr(xyz), ptr(sg.data), sg.D, sg.H, sg.W, sg.B, sg.stride, ptr(s["grid_center"]), ptr(s["grid_scale"]), ptr(d_w), ptr(d_xyz))
        if active is not None:      # for the Gaussians that received a gradient only (the others' d_w rows are zero)
            check(lib().mgr_skin_weights_bwd_indexed(*grid, lst, cnt, N, stream()), "mgr_skin_weights_bwd_indexed")
        else:
            check(lib().mgr_skin_weights_bwd(*grid, 1, stream()), "mgr_skin_weights_bwd")
        return active

    def _d_w_rows(self, d_w):
        """(list, count) device pointers: the rows of d_w (na,B) that are not all zero, ascending -- the modular route's
        `(w.grad != 0).any(1)`, formed on the device: a row mask (mgr_skin_rows_mask), then the exchange's ordered index of
        a mask (mgr_exchange_index).  Deterministic: a scan, no atomics."""
        na, B = d_w.shape
        L, dev = lib(), d_w.device
        r = self._sg_rows
        if r is None or r["idx"].numel() != na or r["idx"].device != dev:
            r = self._sg_rows = dict(mask=torch.empty(na, dtype=torch.uint8, device=dev), idx=torch.empty(na, dtype=torch.int32, device=dev),
                                     count=torch.zeros(1, dtype=torch.int32, device=dev),
                                     ws=torch.empty(L.mgr_exchange_index_workspace_bytes(na), dtype=torch.uint8, device=dev))
        check(L.mgr_skin_rows_mask(na, B, ptr(d_w), ptr(r["mask"]), stream()), "mgr_skin_rows_mask")
        check(L.mgr_exchange_index(na, ptr(r["mask"]), ptr(r["idx"]), ptr(r["count"]), ptr(r["ws"]), r["ws"].numel(), stream()), "mgr_exchange_index")
        return ptr(r["idx"]), ptr(r["count"])

    def _skin_grid_backward(self, head, xyz, d_w, active, rows_of_d_w=False):
        """Sparse dL/d(grid) from the skin-weight gradient the backward wrote: on the active list up to 8 views (the other
        rows of d_w are zero), on all articulated rows beyond.  rows_of_d_w (a map term added rows the active list does not
        know): up to 8 views, on the list of the rows of the summed d_w that are not all zero -- SkinGridAdam steps every LISTED
        voxel, so the list must be the modular route's."""
        V, N, _, na = head[:4]
        s = self.s
        lst, cnt = active if active is not None else (None, None)
        self.last_skin_w_grad = d_w
        if rows_of_d_w and V <= 8 and na:
            lst, cnt = self._d_w_rows(d_w)
            return self.ops._skin_grid_grad(na, xyz, self.grid, s["grid_center"], s["grid_scale"], d_w, lst, cnt, na,
                                            kept=self._sg_kept if self.persistent_grads else None)
        # (outputs and workspace kept across steps like the gradient buffers: "d_skin_grid" is valid until the next step)
        return self.ops._skin_grid_grad(na, xyz, self.grid, s["grid_center"], s["grid_scale"], d_w, lst, cnt, N if active is not None else na,
                                        kept=self._sg_kept if self.persistent_grads else None)

    def __call__(self, view_ids, scale=1.0):
        if self.fused:
            return self._step_direct(view_ids, scale)
        self.last_active = None
        self._loss_ssim = None
        self._ssim_mode()
        for v in self.params.values():
            v.grad = None
        sel = self._select(view_ids)
        T = sel["T"].detach().requires_grad_(True) if self.pose_grad else None     # a leaf for this step
        map_on = self._map_terms()
        tgt = sel["targets"]
        map_out = None
        self.last_corrected = None
        E, d_E = self._exposure_table(), None

        def image_terms(img):
            # (loss, dL/dimg, LPIPS term); corrected: the terms on E applied to the render, the gradient sent back through it
            nonlocal d_E
            if E is not None:
                self.last_image = img.detach()
                loss, g, lp, d_E = self._exposure_loss(self.last_image, E, sel, view_ids, scale)
                return loss, g, lp
            loss, g = self._image_loss(img, tgt, scale)
            return loss, g, self._lpips_term(img, tgt, scale, g, sel, view_ids)

        if any(map_on):
            img, radii, means2D, extras = self.forward_views(view_ids, T=T, maps=(True, map_on[1]))
            loss, g, lp = image_terms(img)
            masks, depths = self._map_sel(sel, view_ids, map_on[1])
            k = scale * len(view_ids)
            ml, sums = losses.map_loss(extras["alpha"], masks, self.w_mask, extras["depth"] if map_on[1] else None, depths,
                                       self.w_depth if map_on[1] else 0.0)
            torch.autograd.backward([img, ml * k], [g, None])
            map_out = (sums[2] * k, sums[0] * k, sums[1] * k)
            loss = loss + map_out[0]
        else:
            img, radii, means2D = self.forward_views(view_ids, T=T)
            loss, g, lp = image_terms(img)
            img.backward(g)
        vis = radii > 0
        g2 = means2D.grad[..., :2].norm(dim=-1) * (1.0 / scale)
        res = dict(grads={n: v.grad for n, v in self.params.items()},
                   grad2d=(g2 * vis).sum(0), vis=vis.sum(0).float(),
                   radii=radii.max(dim=0).values, loss=loss)
        if map_out is not None:
            res["loss_mask"], res["loss_depth"] = map_out[1], map_out[2]
        if lp is not None:
            res["loss"] = res["loss"] + self.w_lpips * lp
            res["loss_lpips"] = lp
        if self._loss_ssim is not None:
            res["loss_ssim"] = self._loss_ssim
        if T is not None:
            res["d_transforms"] = T.grad
        if d_E is not None:
            res["d_exposure"] = d_E
        if self.skin_grid_grad:
            w, self._skin_w = self._skin_w, None
            if w is None or w.grad is None:
                raise ManusHipError("skin_grid_grad: the step formed no skin-weight gradient (do the leaves require grad?)")
            self.last_skin_w_grad = w.grad
            # only the Gaussians that received a gradient, as the fused route's active list: the row Adam steps every LISTED voxel
            # (SparseAdam's semantics), so voxels under all-zero rows must not be listed on one route and left out on the other
            live = torch.nonzero((w.grad != 0).any(1)).reshape(-1).to(torch.int32)
            res["d_skin_grid"] = self.ops.skin_grid_grad(self.params["_xyz"].detach()[:self.n_art], self.grid, self.s["grid_center"],
                                                         self.s["grid_scale"], w.grad, index=live)
        return res

    def pairs_per_view(self, view_ids=None, group=8):
        """Surviving (tile, Gaussian) pairs of every view (forward only, in groups of `group` views): the weights of the
        balanced view assignment.  Deterministic, so every rank computes the same list."""
        ids = list(range(self.cams.shape[0])) if view_ids is None else list(view_ids)
        W, H = int(self.s["width"]), int(self.s["height"])
        T = ((W + 15) // 16) * ((H + 15) // 16)
        N = self.params["_xyz"].shape[0]
        out = []
        ctx = self.rz.context(self.device)
        with torch.no_grad():
            for k in range(0, len(ids), group):
                part = ids[k:k + group]
                for attempt in range(4):
                    self.forward_views_fused(part)
                    try:    # (the autograd node's forward follows the device's sync policy: whatever that is, the tile offsets
                        ctx.check_overflow()    # read below come from a forward that did not overflow its pair capacity)
                        break
                    except ManusHipError:
                        if attempt == 3:
                            raise
                ws = ctx.last_ws
                o = self._layout(ws, len(part), N, W, H)[LAYOUT_TILE_START]
                ts = ws.buf[o: o + 4 * (len(part) * T + 1)].view(torch.int32)[::T].cpu().tolist()
                out += [int(b - a) for a, b in zip(ts[:-1], ts[1:])]
        return out

    # -- inputs of the pruning tests (on_after_backward) ---------------------------------------------
    def prune_views(self, view_ids):
        """One dict per view for `density.DensityController`: camera (K, extr), mask, posed means of the view's
        pose and its keypoints.  Views without a mask / keypoints in the scene are skipped by the controller."""
        s = self.s
        with torch.no_grad():
            if self.is_hand:
                pxyz, _, _ = self._posed(self._select(view_ids)["T"])
            else:
                pxyz = None
        out = []
        masks, keyp = s.get("masks"), s.get("keypoints")
        for k, v in enumerate(view_ids):
            out.append(dict(camera=s["cameras"][v], mask=masks[v] if masks is not None else None,
                            posed_xyz=(pxyz[k, : self.n_art] if pxyz is not None else self.params["_xyz"].detach()),
                            keypoints=keyp[v] if keyp is not None else None))
        return out


class FrameSchedule:
    """Which items of a `frames.FrameStore` a step looks at: epoch e is a permutation of the store's items drawn from
    numpy.random.default_rng((seed, e)) ("shuffle") or their stored order ("sequential"), consumed `views_per_step` at a time; a
    tail shorter than that is dropped.  `items(step)` is a pure function of (seed, step).  The reference trains one shuffled
    (frame, view) per step (its DataLoader shuffles the items); this is that order, batched build-side."""

    def __init__(self, store, views_per_step, seed=0, order="shuffle"):
        if order not in ("shuffle", "sequential"):
            raise ValueError("order must be 'shuffle' or 'sequential' (got %r)" % (order,))
        self.store, self.views_per_step, self.seed, self.order = store, int(views_per_step), int(seed), order
        self.pool = [int(i) for i in store.items]
        if self.views_per_step < 1 or len(self.pool) < self.views_per_step:
            raise ValueError("FrameSchedule: %d items cannot fill a step of %d views" % (len(self.pool), self.views_per_step))
        self.steps_per_epoch = len(self.pool) // self.views_per_step
        self._epoch = None          # (e, its item list)

    def epoch(self, e):
        """The items of epoch e in the order they are consumed (the dropped tail included)."""
        if self._epoch is None or self._epoch[0] != e:
            import numpy as np
            n = len(self.pool)
            perm = np.arange(n) if self.order == "sequential" else np.random.default_rng((self.seed, int(e))).permutation(n)
            self._epoch = (e, [self.pool[int(j)] for j in perm])
        return list(self._epoch[1])

    def items(self, step):
        e, k = divmod(int(step), self.steps_per_epoch)
        return self.epoch(e)[k * self.views_per_step:(k + 1) * self.views_per_step]


class Trainer:
    """One optimisation step in the reference's order (src/modules/hand_dynamic.py:230-282 + Lightning's hooks):

        training_step      render the views, loss, backward (+ the all-reduce)                at global_step g
        on_after_backward  pruning tests + density_update(g)   hand_dynamic.py:193-224 / object.py:66-81
        on_before_optimizer_step   xyz learning rate = schedule(g)   hand_dynamic.py:226-228
        optimizer.step()   Adam; leaves that density_update has just replaced carry no gradient and are skipped
        global_step += 1

    After a densification / pruning the parameter tensors are new (different N): the compute object is re-pointed
    at them and the rasterizer workspaces of the old size are released.  The rasterizer runs without host
    synchronisation; every step is fenced (`rasterizer.poll`: waits for the forward only) and re-run with a larger
    pair capacity if it overflowed, so no update is ever made from a truncated image.
    Multi-GPU: every rank must draw the same split noise, so rank 0's is broadcast; the pruning masks are OR-ed
    over the ranks; max_radii2D is MAX-reduced before it is consumed.

    Drawn frames and pose refinement (one rank; both None: exactly the step above on the fixed views 0 .. n_views - 1).
    frames: a `FrameSchedule` of n_views views per step -- before the step, the rows 0 .. n_views - 1 of the compute object's
    tables are pointed at `frames.items(global_step)` (`FrameStore.load_step`; `last_items` keeps the list).  pose: a
    `pose.PoseRefiner` or a `pose.KinematicPoseRefiner` (joint angles through forward kinematics: bone lengths stay fixed) -- the
    Trainer uses nothing but their common surface, `frames_of`, `apply`, `hold`, `step`, `steps` and `last_prior` -- at the global steps g >= pose_from_iter with (g - pose_from_iter) % pose_every == 0 the corrected
    transforms of the step's frames are written before the step (`PoseRefiner.apply`) and the corrections take their own Adam
    step on `out["d_transforms"]` behind the Gaussians' optimizer step (`PoseRefiner.step`); a re-run after an overflow uses
    the same items and transforms.  Without `frames`, pose_frames gives the frame row of each of the fixed views.  On a step
    at which the corrections are NOT applied (before pose_from_iter, between pose_every steps) the two modes differ: with
    `frames`, `load_step` has just written the items' UNCORRECTED transforms, so the Gaussians train on those; on a fixed view
    set the table keeps the transforms of the last `apply`.  pose_hold=True closes that gap: on every step g >= pose_from_iter
    that is OFF the pose_every schedule the corrected transforms of the step's frames are written before the step
    (`PoseRefiner.hold`) and no correction step follows, so the Gaussians never see a frame at two poses; a re-run after an
    overflow uses the same transforms, and before pose_from_iter nothing is applied in either mode.  The default False is the
    Trainer described above, bit for bit.  When the refiner has priors, `out["loss_pose_prior"]` is its `last_prior` on the
    steps at which the corrections took their step (a device scalar, not read here and not added to `out["loss"]`).
    The pruning tests (`compute.prune_views`) keep testing against the DATASET's keypoints, not the corrected ones; their masks and cameras are those of the drawn items
    (`load_step(scene_masks=True)`), with or without a mask table on the compute object.

    Skin-weight grid refinement (one rank; None: the step above, bit for bit).  skin_grid: an `optim.SkinGridRefiner` on
    `compute.grid`, the compute object built with skin_grid_grad=True -- at the global steps g >= skin_grid_from_iter with
    (g - skin_grid_from_iter) % skin_grid_every == 0 the grid takes its step (prior, row Adam, clamp, projection) on
    `out["d_skin_grid"]` behind the Gaussians' optimizer step and the pose corrections', on both branches of `train_step`, on the
    final run of an overflow re-run and on steps whose leaves densify / prune replaced; `out["loss_skin_prior"]` is then the
    refiner's `last_prior` (a device scalar, not read here).  Off schedule the gradient is still formed and ignored.

    Per-camera exposure (one rank; None: the step above, bit for bit).  exposure: an `exposure.ExposureRefiner`, attached to the
    compute object here unless it already is (`ExposureRefiner.attach`: one table row per view row; with `frames` every row
    starts at -1).  `compute.exposure_on` is set to g >= exposure_from_iter before every step -- before that the step is the
    step without the keyword --, with `frames` the table rows of the drawn items (`ExposureRefiner.rows_of`) are written into
    `compute.exposure_ids` beside `load_step`, and at the global steps g >= exposure_from_iter with (g - exposure_from_iter) %
    exposure_every == 0 the table takes its step on `out["d_exposure"]` behind the Gaussians' optimizer step, the pose
    corrections' and the skin grid's, on both branches of `train_step`.  Off schedule the gradient is formed and ignored.  The
    refiner's state travels through `checkpoint.save_checkpoint(extra_state=)`."""

    def __init__(self, compute, n_views, extent, opts=None, spatial_lr_scale=1.0, rank=0, world_size=1, group=None,
                 bg_white=True, kind=None, compact_allreduce=False, sharded_adam=False, view_weights=None, depth_cut=False,
                 sort_rows=False, persistent_grads=True, start_lpips_iter=1000, frames=None, pose=None, pose_from_iter=0,
                 pose_every=1, pose_frames=None, skin_grid=None, skin_grid_from_iter=0, skin_grid_every=1, pose_hold=False,
                 exposure=None, exposure_from_iter=0, exposure_every=1):
        if exposure is not None:
            if world_size > 1:
                raise ValueError("Trainer(exposure=...) needs world_size == 1: d_exposure is not reduced across ranks")
            if int(exposure_every) < 1:
                raise ValueError("exposure_every must be at least 1")
            if not hasattr(compute, "exposure_on"):
                raise ValueError("Trainer(exposure=...) needs a compute object with an exposure table (HipViewCompute)")
            if frames is not None and getattr(frames.store, "camera_keys", None) is None:
                raise ValueError("Trainer(exposure=..., frames=...) needs the camera keys of a store built by FrameStore.from_dataset")
            if getattr(compute, "exposure", None) is not exposure.E:
                # with frames the rows of the drawn items are written before every step; until then no view is corrected
                exposure.attach(compute, [-1] * int(compute.cams.shape[0]) if frames is not None else None)
        self.exposure, self.exposure_from_iter, self.exposure_every = exposure, int(exposure_from_iter), int(exposure_every)
        if frames is not None:
            if world_size > 1:
                raise ValueError("Trainer(frames=...) needs world_size == 1: the frame pool is one rank's")
            if frames.views_per_step != n_views:
                raise ValueError("Trainer: the schedule draws %d views per step, n_views is %d" % (frames.views_per_step, n_views))
        if pose is not None:
            if not getattr(compute, "pose_grad", False):
                raise ValueError("Trainer(pose=...) needs a compute object with pose_grad=True (its step returns d_transforms)")
            if world_size > 1:
                raise ValueError("Trainer(pose=...) needs world_size == 1: d_transforms is not reduced across ranks")
            if int(pose_every) < 1:
                raise ValueError("pose_every must be at least 1")
            if frames is None and (pose_frames is None or len(pose_frames) != n_views):
                raise ValueError("Trainer(pose=...) without frames needs pose_frames: one frame row per view of the fixed set")
        if skin_grid is not None:
            if not getattr(compute, "skin_grid_grad", False):
                raise ValueError("Trainer(skin_grid=...) needs a compute object with skin_grid_grad=True (its step returns d_skin_grid)")
            if skin_grid.sg is not getattr(compute, "grid", None):
                raise ValueError("Trainer(skin_grid=...): the refiner steps another grid than compute.grid, the one the step differentiates")
            if world_size > 1:
                raise ValueError("Trainer(skin_grid=...) needs world_size == 1: d_skin_grid is not reduced across ranks")
            if int(skin_grid_every) < 1:
                raise ValueError("skin_grid_every must be at least 1")
        self.frames, self.pose, self.pose_from_iter, self.pose_every = frames, pose, int(pose_from_iter), int(pose_every)
        self.skin_grid, self.skin_grid_from_iter, self.skin_grid_every = skin_grid, int(skin_grid_from_iter), int(skin_grid_every)
        self.pose_frames = None if pose_frames is None else [int(f) for f in pose_frames]
        self.pose_hold = bool(pose_hold)
        self.last_items = None          # with frames: the dataset items of the last step
        # sharded_adam (world_size > 1): reduce-scatter of the gradients -> every rank takes the Adam step on the 1/world
        # of the parameter elements it owns -> all-gather of the parameters.  The same bytes on the wire as the
        # all-reduce (which is a reduce-scatter followed by an all-gather), 1/world of the optimizer work per rank.
        # sort_rows: after a densification / pruning has rebuilt the tensors, put the rows in Z-order of their positions
        # (GaussianOptimizer.sort_rows: the same model up to the permutation; every rank computes the same one)
        self.sort_rows = bool(sort_rows)
        # start_lpips_iter: the LPIPS term of the compute object (if it has a network) is on from this global step
        # (base.py:334, scripts/train/train_hands.sh:40)
        self.start_lpips_iter = int(start_lpips_iter)
        # persistent_grads (one rank): the compute object keeps the gradient buffers (HipViewCompute's own default): the
        # tensors in a step's `out["grads"]` are overwritten by the next step -- the optimizer has consumed them by then
        # (see train_step).  False: fresh tensors every step.
        # (only ever narrowed: a compute object built with persistent_grads=False keeps handing out fresh tensors)
        if hasattr(compute, "persistent_grads"):
            compute.persistent_grads = bool(compute.persistent_grads) and bool(persistent_grads) and world_size == 1
        self.compact_allreduce = compact_allreduce and not sharded_adam
        self.sharded_adam = bool(sharded_adam) and world_size > 1
        from .density import DensityController
        from .optim import GaussianOptimizer
        global ALL_GROUPS
        from .optim import ALL_GROUPS
        self.compute, self.n_views, self.extent, self.bg_white = compute, n_views, float(extent), bg_white
        self.view_weights = view_weights   # per-view costs for the balanced assignment (shard_views); None = round-robin
        self.rank, self.world, self.group = rank, world_size, group
        self.opt = GaussianOptimizer(compute.params, opts=opts, spatial_lr_scale=spatial_lr_scale, adopt=True)
        # A composite scene (hand + object in one launch) has no density control in the reference: composite.py has no
        # on_after_backward / density_update and its training_step is `pass` (composite.py:80-81); the two models are
        # densified by their own modules.  The Trainer therefore only renders, reduces and takes the Adam step there --
        # decided here, before any state exists, and independent of `opts` (densify_from_step etc. are ignored).
        self.density_enabled = getattr(compute, "kind", "hand") != "composite"
        kind = kind or ("object" if getattr(compute, "kind", "hand") == "object" else "hand")
        self.density = DensityController(self.opt, extent, kind=kind, bg_white=bg_white)
        self.global_step = 0
        self.retries = 0
        self._rz = rasterizer
        if getattr(compute, "fused", False) and hasattr(compute, "sync_check"):
            compute.sync_check = False      # this trainer's forwards are fenced and polled in _run_step (no global policy flip)
        # depth_cut: a Trainer moves the model every step, and under a moving model the depth cut of the fused forward is a
        # wash at best (flagged forwards are run twice; measured 567 against 578 iters/s with its back-off): off
        # -- HipViewCompute's own default -- unless asked for here.
        if hasattr(compute, "depth_cut"):
            compute.depth_cut = bool(depth_cut) and os.environ.get("MANUS_DEPTH_CUT", "1") != "0"
        self._rebuild_step()

    def _rebuild_step(self):
        if hasattr(self.compute, "grad_arena"):
            self.compute.grad_arena = None   # views of the previous step object's buffer (possibly another N)
        p = self.compute.params
        shapes = {k: v.shape for k, v in p.items()}
        self.stepper = ViewShardedStep(p["_xyz"].shape[0], shapes, self.compute, self.n_views, rank=self.rank,
                                       world_size=self.world, group=self.group, compact=self.compact_allreduce,
                                       scatter=self.sharded_adam, view_weights=self.view_weights)
        if self.sharded_adam:   # leaves and moments as views of flat buffers laid out like the gradient buffer
            self.opt.flatten(self.stepper.padded_g)
            self.compute.set_params(self.opt.parameters())
            self.opt.p = {k: v.detach() for k, v in self.compute.params.items()}

    def _split_noise(self, n_rows, device):
        noise = torch.randn((2 * n_rows, 3), dtype=torch.float32, device=device)
        if self.world > 1:
            dist.broadcast(noise, src=0, group=self.group)
        return noise

    def _run_step(self):
        """Forward + backward (+ all-reduce) with the overflow fence; re-runs the step after an overflow."""
        for _ in range(4):
            out = self.stepper.step()
            local_bad = False
            if torch.cuda.is_available() and getattr(self.compute, "fused", False):
                try:
                    self._rz.poll(getattr(self.compute, "device", None))
                except RuntimeError:
                    local_bad = True
            bad = local_bad
            if self.world > 1 and out.get("overflow") is not None:
                bad = float(out["overflow"]) > 0.0     # summed over the ranks by the all-reduce: the same on all of them
            if not bad:
                return out
            self.retries += 1
        raise RuntimeError("rasterizer pair capacity still exceeded after 4 attempts")

    def gather_moments(self):
        """Sharded optimizer step: each rank keeps only the Adam moments of the elements it owns up to date.  Before
        the rows move (prune / densify: ownership is by element range, so it moves with them), and before a checkpoint,
        the ranks exchange their slices."""
        if self.sharded_adam:
            self.stepper.all_gather_params(self.opt.mflat)
            self.stepper.all_gather_params(self.opt.vflat)

    def validate(self, view_ids, masks=None, validator=None, group=8, lpips=None, ssim="rows", exposure=False):
        """The validation pass over the views `view_ids` of the compute object (validation_step / on_validation_epoch_end,
        src/modules/base.py:112-188): rendered under no_grad with `forward_views` in groups of `group` views (the group
        size of `HipViewCompute.pairs_per_view`), compared with `compute.targets` by `ops.eval_views` / `ops.eval_triptych`
        on the whole group, ONE host synchronisation per group (the read-back of its metrics; the render runs fenced and
        is rendered again with more room should its pairs not have fitted).  masks: (len(view_ids),H,W), possibly fractional, or None
        (ones).  validator: a `validation.Validator` that receives every view (metrics, its share of the group's render
        time, triptych); the caller brackets the pass with its start() / end(global_step).  lpips: a `manus_amd.lpips.LPIPS`
        (the reference's is AlexNet, loss_utils.py:19): its per-view value on the masked images, render * mask against
        target * mask, goes to the validator's CSV column and to the result's "lpips" list.  ssim: "rows" (default; the
        reference's statistic on HWC images, from `ops.eval_views`) or "spatial" (the standard 2-D SSIM of the masked images,
        `validation.spatial_ssim`): which one fills the result's "ssim" list and the CSV column; anything else raises ValueError.
        exposure: True takes metrics, LPIPS and the triptych on the render corrected by the compute object's exposure table
        (`compute.exposure`, rows `compute.exposure_ids`; a view whose row is -1 is taken as it is) -- what the training loss saw;
        False (default) on the raw render, every output as without the keyword.

        Returns dict(psnr, ssim: per-view lists; psnr_mean, ssim_mean; ssim_kind; render_time: seconds from the start of each
        group's render to the end of its last kernel, summed (two events on the stream: the group's host work included,
        no extra synchronisation);
        images: (len(view_ids),3H,W,3) uint8 on the device).

        The training state is left as it was: the renders run in a rasterizer context of their own (workspace pool,
        learnt capacities, fences and sync policy of the training context are not touched), the compute object's cache of
        per-view constants is put back, nothing is written into the kept gradient / image / loss buffers, and
        `global_step` does not move -- a train_step after a validate computes what it would have without it."""
        from .validation import check_ssim_kind, psnr_from_sums, spatial_ssim
        check_ssim_kind(ssim)
        c = self.compute
        ids = list(view_ids)
        dev = getattr(c, "device", None)
        if masks is not None and (masks.dim() != 3 or masks.shape[0] != len(ids)):
            raise ValueError("validate: masks must be (len(view_ids),H,W)")
        exp_table = exp_ids = None
        if exposure:
            if getattr(c, "exposure", None) is None:
                raise ValueError("validate(exposure=True): the compute object has no exposure table")
            on, c.exposure_on = c.exposure_on, True       # (the table's own checks, whatever the training schedule says)
            try:
                exp_table = c._exposure_table()
            finally:
                c.exposure_on = on
            exp_ids = c.exposure_ids if c.exposure_ids is not None else range(int(c.cams.shape[0]))
        idx = self._rz.context(dev).device.index
        train_ctx = self._rz._CONTEXTS[idx]
        if getattr(self, "_val_ctx", None) is None or self._val_ctx.device != train_ctx.device:
            self._val_ctx = self._rz.RasterContext(train_ctx.device)
            self._val_ctx.sync_every_forward = False     # (of the private context: the training context keeps its policy)
        n_now = c.params["_xyz"].shape[0]
        if any(key[1] != n_now for key in self._val_ctx.pool):      # a densification changed N: the old workspaces are of no use
            self._val_ctx.clear()
        saved_cache, saved_stamp = c._cache, c._const_stamp
        psnrs, ssims, lps, images, render_time = [], [], [], [], 0.0
        self._rz._CONTEXTS[idx] = self._val_ctx
        try:
            with torch.no_grad():
                for k in range(0, len(ids), group):
                    part = ids[k:k + group]
                    m = masks[k:k + group] if masks is not None else None
                    for attempt in range(4):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        img, _, _ = c.forward_views(part)       # no host read: the private context runs fenced
                        e1.record()
                        if exp_table is not None:
                            img = ops.exposure_forward(img, exp_table, [exp_ids[v] for v in part])
                        tgt = c._select(part)["targets"]
                        sq, ss, gmax = ops.eval_views(img, tgt, m)
                        trip = ops.eval_triptych(img, tgt, gmax)
                        n = float(img[0].numel())
                        rows = [psnr_from_sums(sq, n), spatial_ssim(img, tgt, m) if ssim == "spatial" else ss / n]
                        if lpips is not None:
                            rows.append(lpips.values_grad(img, tgt, m, need_grad=False)[0])
                        both = torch.stack(rows).cpu()      # the group's one synchronisation
                        try:
                            self._val_ctx.poll()                # the render's fence (long complete): did its pairs fit?
                            break
                        except ManusHipError:                   # no: the capacity was enlarged, render the group again
                            if attempt == 3:
                                raise
                    dt = e0.elapsed_time(e1) * 1e-3
                    render_time += dt
                    psnrs += both[0].tolist()
                    ssims += both[1].tolist()
                    if lpips is not None:
                        lps += both[2].tolist()
                    images.append(trip)
                    if validator is not None:
                        host = trip.cpu().numpy()
                        for j in range(len(part)):
                            validator.add(float(both[0, j]), float(both[1, j]), dt / len(part), host[j],
                                          lpips=float(both[2, j]) if lpips is not None else None)
        finally:
            self._rz._CONTEXTS[idx] = train_ctx
            c._cache, c._const_stamp = saved_cache, saved_stamp
        import numpy as np
        res = dict(psnr=psnrs, ssim=ssims, psnr_mean=float(np.mean(psnrs)) if psnrs else float("nan"),
                   ssim_mean=float(np.mean(ssims)) if ssims else float("nan"), ssim_kind=ssim, render_time=render_time,
                   images=torch.cat(images) if images else None)
        if lpips is not None:
            res["lpips"] = lps
        return res

    def _point_views(self, gs):
        """Before the step at global step gs: the drawn items into the compute object's rows, then the pose corrections into
        its transforms.  -> (view ids, frame rows) when the corrections were applied (they take their step behind this one's
        backward), else None -- also where `pose_hold` wrote the corrected transforms of an off-schedule step, which no
        correction step follows."""
        c, ids = self.compute, list(self.stepper.local_views)
        if self.frames is not None:
            self.last_items = self.frames.items(gs)
            # (scene_masks: without a mask table the pruning masks of the scene still follow the drawn items)
            self.frames.store.load_step(c, self.last_items, masks=c.mask_targets is not None, lpips_rects=c.lpips_rects is not None,
                                        scene_masks=True)
            if self.exposure is not None:      # the table rows follow the drawn items (slots 0 .. n_views - 1, as load_step's)
                table = list(c.exposure_ids)
                table[:len(self.last_items)] = self.exposure.rows_of(self.frames.store, self.last_items)
                c.exposure_ids = table
        if self.pose is None or gs < self.pose_from_iter:
            return None
        due = (gs - self.pose_from_iter) % self.pose_every == 0
        if not due and not self.pose_hold:
            return None
        rows = self.pose.frames_of(self.frames.store, self.last_items) if self.frames is not None else self.pose_frames
        if not due:
            self.pose.hold(c, ids, rows)
            return None
        self.pose.apply(c, ids, rows)
        return ids, rows

    def _pose_step(self, out, posed_step):
        """Behind the Gaussians' optimizer step: the corrections' own step when `_point_views` applied them, and the value of
        the refiner's prior (if it has one) on the rows that moved."""
        if posed_step is None:
            return
        before = self.pose.steps
        self.pose.step(out["d_transforms"], *posed_step)
        if self.pose.steps != before and getattr(self.pose, "last_prior", None) is not None:
            out["loss_pose_prior"] = self.pose.last_prior

    def _skin_grid_step(self, gs, out):
        """Behind the Gaussians' optimizer step (and the pose corrections'): the skin-weight grid's own step on the step's
        `out["d_skin_grid"]` -- the gradient of the parameters the step rendered, also where densify / prune has just replaced the
        leaves (the grid tensor is never replaced) -- at the scheduled global steps; off schedule the gradient is formed and ignored."""
        r = self.skin_grid
        if r is None or gs < self.skin_grid_from_iter or (gs - self.skin_grid_from_iter) % self.skin_grid_every != 0:
            return
        r.step(out["d_skin_grid"])
        out["loss_skin_prior"] = r.last_prior

    def _exposure_step(self, gs, out):
        """Behind the Gaussians' optimizer step, the pose corrections' and the skin grid's: the exposure table's own step on the
        step's `out["d_exposure"]` at the scheduled global steps; off schedule the gradient is formed and ignored."""
        r = self.exposure
        if r is None or gs < self.exposure_from_iter or (gs - self.exposure_from_iter) % self.exposure_every != 0:
            return
        ids = list(self.stepper.local_views)
        r.step(out["d_exposure"], ids, [self.compute.exposure_ids[v] for v in ids])

    def train_step(self, views=None):
        """One optimisation step; returns the step's output dict (loss, statistics) plus "changed".
        views: optional list of per-view dicts for the pruning tests (default: `compute.prune_views`).

        ALIASING: with kept buffers (the default at one rank) `out["grads"]`, `out["grad2d"]`, `out["vis"]` and
        `compute.last_image` are the same storage every step, like `.grad` tensors -- they hold THIS step's values until the
        next call; clone what is logged or compared across steps (or construct the Trainer with persistent_grads=False).
        Writing into them is safe (HipViewCompute notices by the tensors' version counters and refills them in full)."""
        o, gs = self.opt.opts, self.global_step
        if getattr(self.compute, "lpips", None) is not None:
            self.compute.lpips_on = gs >= self.start_lpips_iter
        if self.exposure is not None:
            self.compute.exposure_on = gs >= self.exposure_from_iter
        posed_step = self._point_views(gs) if (self.frames is not None or self.pose is not None) else None
        out = self._run_step()
        if not self.density_enabled:     # composite: render + reduce + Adam only (see __init__)
            self.opt.update_learning_rate(gs)
            if self.sharded_adam:
                lo, hi = self.stepper.owned
                self.opt.step_range(self.stepper._store, lo, hi)
                self.stepper.all_gather_params(self.opt.pflat)
            else:
                self.opt.step(out["grads"])
            if hasattr(self.compute, "mark_params_changed"):
                self.compute.mark_params_changed()
            self._pose_step(out, posed_step)
            self._skin_grid_step(gs, out)
            self._exposure_step(gs, out)
            self.global_step += 1
            out["changed"] = False
            return out
        # ---- on_after_backward ----
        needs_tests = self.density.kind == "hand" and (gs < o["remove_seg_end"] or gs % 100 == 0) or \
            self.density.kind == "object" and gs < o["remove_seg_end"]
        if views is None and needs_tests and hasattr(self.compute, "prune_views"):
            views = self.compute.prune_views(self.stepper.local_views)
        mask = self.density.prune_mask(gs, views) if needs_tests else None
        if self.world > 1 and needs_tests:   # every rank tested its own views: OR them
            m8 = (mask if mask is not None else torch.zeros(self.opt.N, dtype=torch.bool, device=self.opt.device)).to(torch.uint8)
            dist.all_reduce(m8, op=dist.ReduceOp.MAX, group=self.group)
            mask = m8.bool() if bool(m8.any()) else None
        will_densify = mask is None and gs < o["densify_until_step"] and gs > o["densify_from_step"] and \
            gs % o["densification_interval"] == 0
        stats = dict(grad2d=out["grad2d"], vis=out["vis"], radii=out["radii"])
        noise = None
        if will_densify and self.world > 1:
            # the selection count is only known inside the plan: draw the worst case on rank 0 and broadcast
            noise = self._split_noise(self.opt.N, self.opt.device)
        n_before = self.opt.N
        if self.sharded_adam and (mask is not None or will_densify):
            self.gather_moments()     # rows are about to move: every rank needs the moments of every row
        if mask is not None:
            changed = self.opt.density_update(stats, self.extent, gs, self.bg_white, mask_to_prune=mask)
        else:
            if will_densify and self.world > 1:
                # max_radii2D is a running maximum over this rank's views; combine the ranks before it is consumed
                self.opt.add_densification_stats(out["grad2d"], out["vis"], out["radii"])
                self.stepper.reduce_max_radii(self.opt.max_radii2D)
                stats = dict(grad2d=torch.zeros_like(out["grad2d"]), vis=torch.zeros_like(out["vis"]),
                             radii=torch.zeros_like(out["radii"]))
            changed = self.opt.density_update(stats, self.extent, gs, self.bg_white, noise=noise,
                                              noise_is_pool=noise is not None)
        if changed:
            self.density.on_train_epoch_start()
        resized = changed and (self.opt.N != n_before or self.opt.replaced == ALL_GROUPS)   # new leaf tensors
        if resized and self.sort_rows and self.opt.replaced == ALL_GROUPS:
            na = getattr(self.compute, "n_art", 0)
            out["row_perm"] = self.opt.sort_rows(n_art=na if 0 < na < n_before and getattr(self.compute, "kind", "") == "composite" else None)
        # ---- on_before_optimizer_step + optimizer.step() ----
        self.opt.update_learning_rate(gs)
        if self.sharded_adam:
            if self.opt.replaced == ALL_GROUPS:
                self.opt.replaced = frozenset()          # every leaf is new: no gradient, no step (like opt.step)
            else:
                lo, hi = self.stepper.owned
                self.opt.step_range(self.stepper._store, lo, hi)
                self.stepper.all_gather_params(self.opt.pflat)
        else:
            self.opt.step(out["grads"])   # skips the groups replaced above (all of them after a densify / prune)
        if hasattr(self.compute, "mark_params_changed"):
            self.compute.mark_params_changed()
        self._pose_step(out, posed_step)
        self._skin_grid_step(gs, out)
        self._exposure_step(gs, out)
        self.global_step += 1
        if resized:
            self.compute.set_params(self.opt.parameters(), None)
            self.opt.p = {k: v.detach() for k, v in self.compute.params.items()}
            if torch.cuda.is_available():
                self._rz.context(getattr(self.compute, "device", None)).clear()
            self._rebuild_step()
        out["changed"] = changed
        if changed and getattr(self.opt, "last_densify", None) is not None and will_densify:
            out["densify"] = self.opt.last_densify
        return out

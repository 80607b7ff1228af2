"""Drop-in operator surface of `diff_gaussian_rasterization` on MI355X.

Mirrors the interface MANUS imports at src/utils/gaussian_utils.py:18-21 and calls
at :378-416 (reference tree brown-ivl/manus):

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg,
        scale_modifier, viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None,
        colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None)
        -> (color (3,H,W), radii (N,) int32)

Everything is computed by hand-written HIP kernels through the C ABI of
libmanus_hip.so; there is no PyTorch fallback.  `rasterize_views` is the
multi-view batched form (V cameras in every launch) used by the training engine.
"""
from typing import NamedTuple

import ctypes
import os
import time
import weakref

import torch
import torch.nn as nn

from . import _lib
from ._lib import (check, f32c, lib, ptr, stream, MGR_FWD_RANK_LARGE, MGR_FWD_SKIP_BOX_LARGE, MGR_FWD_SKIP_BOX_MID, MGR_FWD_SKIP_SORT_BEHIND,
                   MGR_FWD_SPREAD, MGR_OVF_CUT, MGR_OVF_FLAGS_MASK, MGR_OVF_PAIRS, MGR_OVF_REPAIRED_SHIFT, MGR_OVF_TIER, MGR_TIERS_BEYOND_SMALL_MASK,
                   MGR_TIERS_BEYOND_SMALL_SHIFT, MGR_TIERS_BOX_LARGE, MGR_TIERS_BOX_MID, MGR_TIERS_NEAR_LARGE_SHIFT, MGR_TIERS_NEAR_MASK,
                   MGR_TIERS_NEAR_SMALL_SHIFT, MGR_TIERS_WIDE_RECT)
from .ops import lbs_cov, sh_colors


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


# ---------------------------------------------------------------------------
# per-device context: workspace pool, learnt pair capacities, overflow fences
# ---------------------------------------------------------------------------
class RasterWorkspace:
    """One opaque byte tensor that links a forward to its backward."""
    # sort items with a single depth bucket beyond the light launch's LDS that the light launch may take on itself: none --
    # such a bucket goes through its global-memory fallback, ~90 us, which with one view on the GPU is the whole kernel
    # (measured: 0.039 -> 0.093 ms)
    SORT_BIG_MAX = int(os.environ.get("MANUS_SORT_BIG_MAX", "0"))

    def __init__(self, device, V, N, W, H, cap):
        self.key = (V, N, W, H)
        self.cap = int(cap)
        self.nbytes = int(lib().mgr_raster_workspace_bytes(V, N, W, H, self.cap))
        # zero-filled once: pair tags start at 0 = "never written"
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.busy = False
        # depth cut (mgr_views_forward, MGR_FWD_DEPTH_CUT): whose views the per-tile hints in this workspace describe (set by
        # the caller that opts in), and "the last forward with the cut was flagged: run the next one without it"
        self.hint_key = self.prev_hint_key = None
        self.cut_block = False
        self.mirror = None
        # binning tiers: the MGR_TIERS_* word of the most recent forward whose status was read (None: unknown, launch everything)
        self.tiers = None
        # set by a forward that runs without a host read but promises the caller a complete result (the operator route's
        # automatic fences): launches whose absence would have to be answered by a re-run are then never skipped
        self.no_flagging_skips = False

    def skip_bits(self):
        """MGR_FWD_* flags that spare the forward the binning launches its views did not need last time (verified on the device:
        a view that needs a skipped launch flags the forward, MGR_OVF_TIER, which is then run again with all of them)."""
        t = self.tiers
        if t is None:
            return 0
        # sort items beyond MGR_DB_RANK_MAX keys met (a dense depth slice): ~4 us in k_dbin_rank's large instantiation, 33 us behind it
        large = (t >> MGR_TIERS_BEYOND_SMALL_SHIFT) & MGR_TIERS_BEYOND_SMALL_MASK
        # ... and no item near the LDS of the instantiation this forward asks for: skip the launch behind it
        near = (t >> (MGR_TIERS_NEAR_LARGE_SHIFT if large else MGR_TIERS_NEAR_SMALL_SHIFT)) & MGR_TIERS_NEAR_MASK
        bits = ((MGR_FWD_RANK_LARGE if large else 0) | (MGR_FWD_SPREAD if t & MGR_TIERS_WIDE_RECT else 0))
        if not self.no_flagging_skips:
            bits |= ((0 if t & MGR_TIERS_BOX_LARGE else MGR_FWD_SKIP_BOX_LARGE) | (0 if t & MGR_TIERS_BOX_MID else MGR_FWD_SKIP_BOX_MID)
                     | (MGR_FWD_SKIP_SORT_BEHIND if near <= RasterWorkspace.SORT_BIG_MAX else 0))
        return bits


def default_pair_capacity(V, N):
    return max(4096, 8 * V * max(N, 1))


class RasterContext:
    """All host-side rasterizer state of ONE device (SURVEY.md 8b "Threading": one host thread per device, re-entrant
    across devices): the workspace pool, the pair capacity learnt per (V,N,W,H), the sync policy and the overflow
    fences of forwards that ran without a host synchronisation."""

    MAX_FENCES = 64
    # Operator route (`GaussianRasterizer` under autograd, sync policy left at its default): after this many consecutive
    # forwards of one (V, N, W, H) whose pair count fitted the learnt capacity, the blocking read of the pair count per forward
    # (upstream's cudaMemcpy; 0.23 ms of a 1.47 ms step at 1280x720, profiles/r05_other_configs/dropin_c*) is replaced by a
    # fence that the NEXT forward of the context resolves -- by then it has long been written.  The capacity keeps its 25 %
    # headroom; should a forward outgrow it all the same, the next forward (or `poll()`) raises ManusHipError (the step before
    # it used an incomplete image) and the context returns to the blocking mode.  0 = never switch; a densification (new N)
    # starts over.  Two kinds of forward always read the count back, because nothing after them would report an overflow:
    # one that builds no autograd graph (an evaluation render under no_grad), and one whose packed camera table -- the same
    # tensor object at the same version while the caller's camera tensors are unmodified (_lib.cached_pack) -- has not been
    # through a synchronous forward of this (V, N, W, H): a new camera may need far more pairs than the capacity learnt so far.
    AUTO_FENCE_AFTER = int(os.environ.get("MANUS_AUTO_FENCE_AFTER", "8"))

    def __init__(self, device):
        self.device = torch.device(device)
        self.pool = {}
        self.cap_hint = {}
        self.sync_every_forward = True
        self.last_ws = None
        self._fences = []        # (workspace, pinned int32[2], event) per unsynchronised forward, oldest first
        self._free_pinned = []
        self._evicted_overflow = False   # an overflow seen while retiring old fences: raised by the next poll()
        self.cut_retries = 0             # forwards flagged MGR_OVF_CUT (each is answered by a forward without the depth cut)
        self.cut_repairs = 0             # (tile, quadrant) units repaired on the device by forwards with the depth cut (MGR_FWD_REPAIR)
        self._clean = {}                 # (V, N, W, H) -> consecutive synchronised forwards that fitted their capacity
        self._seen = {}                  # (V, N, W, H) -> {id: (weak reference, version)} of the camera tables read back synchronously
        self.auto_fenced = 0             # forwards that ran on an automatic fence instead of the blocking read
        self.tier_retries = 0            # forwards flagged MGR_OVF_TIER (answered by a forward with every binning launch)

    # -- pool ---------------------------------------------------------------------------------
    def acquire(self, V, N, W, H, min_cap):
        lst = self.pool.setdefault((V, N, W, H), [])
        for ws in lst:
            if not ws.busy and ws.cap >= min_cap:
                ws.busy = True
                return ws
        lst[:] = [w for w in lst if w.busy]   # drop idle smaller workspaces before growing
        ws = RasterWorkspace(self.device, V, N, W, H, min_cap)
        ws.busy = True
        lst.append(ws)
        return ws

    def clear(self):
        """Forget pooled workspaces and learnt capacities (e.g. after densification changed N)."""
        if self._fences:                        # the forwards' last kernels write into the pinned words: wait before recycling
            torch.cuda.synchronize(self.device)
        for ws, pinned, ev in self._fences:
            if pinned is not None:
                self._free_pinned.append(pinned)
        for lst in self.pool.values():          # withdraw mirrors that no forward took
            for ws in lst:
                if ws.mirror is not None:
                    lib().mgr_raster_set_status_mirror(ptr(ws.buf), None)
                    self._free_pinned.append(ws.mirror)
                    ws.mirror = None
        self.pool.clear()
        self.cap_hint.clear()
        self._fences.clear()
        self._evicted_overflow = False
        self.last_ws = None
        self._clean.clear()
        self._seen.clear()

    # -- status of a forward --------------------------------------------------------------------
    # Where the three callers of _digest differ (kept as found, listed in LAB.md): (learn the capacity from a flagged forward
    # too, MGR_OVF_* bits that hide MGR_OVF_CUT, bits that hide MGR_OVF_TIER -- a hidden flag blocks / counts nothing)
    _SYNC = (False, MGR_OVF_PAIRS, MGR_OVF_PAIRS | MGR_OVF_CUT)   # forward(): acts on the return code = the first flag set; its retry learns
    _FENCE = (True, 0, 0)                                         # _resolve(): every flag on its own
    _RECHECK = (True, MGR_OVF_PAIRS, 0)                           # check_overflow(): the cut by the return code, the tiers by the flag

    def _read_header(self, ws):
        """Blocking read of the status in the workspace header: (return code, pair count, overflow word, tiers word)."""
        npairs, ovf, tiers = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
        rc = lib().mgr_raster_status_tiers_sync(ptr(ws.buf), ctypes.byref(npairs), ctypes.byref(ovf), ctypes.byref(tiers), stream())
        return rc, int(npairs.value), int(ovf.value), int(tiers.value)

    def _digest(self, ws, npairs, word, tiers, route):
        """All the context keeps of one forward's status words, whatever they were read from: the learnt capacity, the tiers
        for the next forward's skip_bits(), the depth-cut block, the counters.  Returns the MGR_OVF_* flags."""
        learn_flagged, cut_hidden_by, tier_hidden_by = route
        ovf = word & MGR_OVF_FLAGS_MASK
        self.cut_repairs += word >> MGR_OVF_REPAIRED_SHIFT   # quadrants repaired on the device (no re-run); the mirror's word alone carries them
        if learn_flagged or not ovf:    # the capacity of the next forwards of these sizes: 25 % of headroom
            self.cap_hint[ws.key] = max(self.cap_hint.get(ws.key, 0), int(npairs * 1.25) + 4096)
        ws.tiers = None if ovf & MGR_OVF_TIER else tiers          # flagged: the next forward runs every binning launch
        if ovf & MGR_OVF_CUT and not ovf & cut_hidden_by:         # ... and must not use the hints
            ws.cut_block = True
            self.cut_retries += 1
        if ovf & MGR_OVF_TIER and not ovf & tier_hidden_by:
            self.tier_retries += 1
        return ovf

    # -- forward driver -------------------------------------------------------------------------
    def _seen_cams(self, key, cams):
        ent = self._seen.get(key, {}).get(id(cams))
        return ent is not None and ent[0]() is cams and ent[1] == cams._version

    def _see_cams(self, key, cams):
        seen = self._seen.setdefault(key, {})
        if len(seen) >= 256:
            seen.clear()
        seen[id(cams)] = (weakref.ref(cams), cams._version)

    def forward(self, V, N, W, H, launch, sync_check=True, defer_fence=False, auto_fence=False, cams=None):
        """Run `launch(ws)` (which enqueues one forward on the current stream) with a workspace large enough for
        the pairs it produces.  sync policy True: read the pair count back (one host sync, like upstream) and
        retry with a larger workspace on overflow; False: no host sync, an overflow fence is recorded instead
        (`poll()` / `check_overflow()`).  Returns (workspace, pair count or None).  defer_fence: the caller records the
        fence itself (`fence(ws)`) once everything that can raise a flag is queued -- a forward split at the blend raises
        the depth-cut flag in its second half."""
        key = (V, N, W, H)
        cap = max(self.cap_hint.get(key, 0), default_pair_capacity(V, N))
        # auto_fence (the operator route, False for a forward without autograd graph): see AUTO_FENCE_AFTER; cams: its camera table
        auto = (bool(auto_fence) and sync_check and self.sync_every_forward and 0 < self.AUTO_FENCE_AFTER <= self._clean.get(key, 0)
                and cams is not None and self._seen_cams(key, cams))
        if auto:
            try:
                self.poll()              # the automatic fences of the forwards before (complete by now)
            except _lib.ManusHipError:
                self._clean[key] = 0
                raise _lib.ManusHipError("an unsynchronised forward of the previous step outgrew its pair capacity: its image and "
                                         "gradients were incomplete.  The capacity was enlarged and this context reads the pair count "
                                         "back again; set MANUS_AUTO_FENCE_AFTER=0 to keep every forward synchronous.")
        while True:
            ws = self.acquire(V, N, W, H, cap)
            # whoever launches may claim the depth-cut hints of the forward before (prev_hint_key) and name the views of
            # this one; a launch that does neither leaves hints nobody may use
            ws.prev_hint_key, ws.hint_key = ws.hint_key, None
            fenced = auto or not (sync_check and self.sync_every_forward)
            ws.no_flagging_skips = auto
            if fenced:
                self._arm_mirror(ws)
            launch(ws)
            self.last_ws = ws
            if fenced:
                if auto:
                    self.auto_fenced += 1
                if not defer_fence:
                    self._fence(ws)
                return ws, None
            rc, npairs, word, tiers = self._read_header(ws)
            self._digest(ws, npairs, word, tiers, self._SYNC)
            if rc == _lib.MGR_OK:
                self._clean[key] = self._clean.get(key, 0) + 1
                if auto_fence and cams is not None:
                    self._see_cams(key, cams)
                return ws, npairs
            self._clean[key] = 0
            # MGR_ETIER: a skipped binning launch was needed; MGR_ECUT: the depth-cut hints no longer fit -- the same workspace again,
            # with all launches / without the cut (_digest has seen to both)
            if rc not in (_lib.MGR_ETIER, _lib.MGR_ECUT):
                if rc != _lib.MGR_EOVERFLOW:
                    check(rc, "mgr_raster_status_sync")
                cap = int(npairs * 1.5) + 4096   # overflow: retry with room for the observed count
            ws.busy = False

    # -- overflow fences ------------------------------------------------------------------------
    def fence(self, ws):
        self._fence(ws)

    def fenced(self, sync_check=True):
        """True when forwards run without a host synchronisation (fences instead)."""
        return not (sync_check and self.sync_every_forward)

    def _arm_mirror(self, ws):
        """Before an unsynchronised forward: four pinned words the forward's last kernel writes its status to
        (mgr_raster_set_status_mirror) -- the fence is then an event only, no device-to-host copy on the stream."""
        while len(self._fences) >= self.MAX_FENCES:
            _, ovf = self._resolve(self._fences.pop(0))
            self._evicted_overflow = self._evicted_overflow or bool(ovf)
        pinned = self._free_pinned.pop() if self._free_pinned else torch.zeros(4, dtype=torch.int32).pin_memory()
        pinned[3] = 0
        rc = lib().mgr_raster_set_status_mirror(ptr(ws.buf), ctypes.c_void_p(pinned.data_ptr()))
        ws.mirror = pinned if rc == _lib.MGR_OK else None      # (not mappable: the fence falls back to a blocking read)

    def _fence(self, ws):
        """Remember the forward just queued: the host can later wait for THIS forward only, while the kernels queued after
        it keep the GPU busy.  With a mirror armed nothing at all goes onto the stream -- the forward's last kernel writes
        the status words and then their valid flag into pinned memory, and the host waits on that flag (an event behind
        the forward costs ~6 us of idle GPU: the next kernel does not start until it has signalled).  Without a mirror:
        an event."""
        mirror, ev = ws.mirror, None
        if mirror is None:
            ev = torch.cuda.Event()
            ev.record()
        self._fences.append((ws, mirror, ev))
        ws.mirror = None

    @staticmethod
    def _wait_flag(pinned, seconds=5.0):
        """Spin (politely) until the device has written the valid flag of a status mirror."""
        t0, n = time.perf_counter(), 0
        while int(pinned[3]) != 1:
            n += 1
            if n > 200:
                time.sleep(0.00005)
            if time.perf_counter() - t0 > seconds:
                return False
        return True

    def _resolve(self, fence):
        ws, pinned, ev = fence
        if ev is not None:
            ev.synchronize()
        elif pinned is not None and not self._wait_flag(pinned):
            torch.cuda.synchronize(self.device)      # (a forward whose blend never ran: nothing will write the flag)
        if pinned is not None and int(pinned[3].item()) == 1:
            npairs, word, tiers = int(pinned[0].item()) & 0xFFFFFFFF, int(pinned[1].item()) & 0xFFFFFFFF, int(pinned[2].item())
        else:   # (a forward that did not run its blend, or no mirror: read the header -- valid if nothing ran on ws since)
            _, npairs, word, tiers = self._read_header(ws)
        if pinned is not None:
            self._free_pinned.append(pinned)
        return npairs, self._digest(ws, npairs, word, tiers, self._FENCE)   # (flagged: the caller re-runs the step)

    def poll(self):
        """Wait for the forwards recorded so far (not for what was queued after them) and raise ManusHipError if one
        of them overflowed its pair capacity -- its image and gradients are incomplete; the capacity hint has been
        enlarged, so re-running the step succeeds.  Returns the pair count of the most recent forward."""
        last, bad = 0, self._evicted_overflow
        self._evicted_overflow = False
        while self._fences:
            npairs, ovf = self._resolve(self._fences.pop(0))
            last, bad = npairs, bad or bool(ovf)
        if bad:
            raise _lib.ManusHipError("rasterizer forward incomplete: pair capacity exceeded or depth-cut hints outdated "
                                     "(retry: the capacity hint was enlarged / the next forward runs without the cut)")
        return last

    def check_overflow(self):
        """Blocking check of every forward since the last check (fences) and of the most recent workspace; returns
        the most recent pair count, raises ManusHipError on overflow (after enlarging the capacity hint)."""
        polled = self.poll()
        ws = self.last_ws
        if ws is None:
            return polled
        rc, npairs, word, tiers = self._read_header(ws)
        self._digest(ws, npairs, word, tiers, self._RECHECK)
        check(rc, "rasterizer overflow check (retry: capacity hint was enlarged)")
        return npairs


_CONTEXTS = {}


def context(device=None):
    """The RasterContext of `device` (default: the current device)."""
    idx = torch.cuda.current_device() if device is None else (torch.device(device).index
                                                              if torch.device(device).index is not None
                                                              else torch.cuda.current_device())
    ctx = _CONTEXTS.get(idx)
    if ctx is None:
        ctx = _CONTEXTS[idx] = RasterContext(torch.device("cuda", idx))
    return ctx


def set_sync_policy(sync_every_forward, device=None):
    """True (default, drop-in behaviour): every forward reads back the pair count
    (one host sync, like the upstream extension) and transparently retries with a
    larger workspace on overflow.  False (training engine): no host sync; the
    capacity learnt so far is used and `poll()` / `check_overflow()` report overflows."""
    context(device).sync_every_forward = bool(sync_every_forward)


def check_overflow(device=None):
    return context(device).check_overflow()


def poll(device=None):
    return context(device).poll()


class _Lease:
    """Releases the workspace when the autograd graph that needs it is freed."""

    def __init__(self, ws):
        self.ws = ws

    def __del__(self):
        self.ws.busy = False


def _run_forward(cams, V, N, W, H, bg, means3D, cov3D, colors, opacity, debug, sync_check=True, graph=True):
    dev = means3D.device
    out = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((V, N), dtype=torch.int32, device=dev)
    s_m = means3D.stride(0) if means3D.dim() == 3 else 0
    s_c = cov3D.stride(0) if cov3D.dim() == 3 else 0
    s_col = colors.stride(0) if colors.dim() == 3 else 0
    s_o = opacity.stride(0) if opacity.dim() == 2 else 0

    def launch(ws):
        check(lib().mgr_raster_forward(V, N, W, H, ptr(cams), ptr(bg), ptr(means3D), s_m, ptr(cov3D), s_c,
                                       ptr(colors), s_col, ptr(opacity), s_o, ptr(out), ptr(radii),
                                       ptr(ws.buf), ws.nbytes, ws.cap, (_lib.MGR_FWD_CHECK if debug else 0) | ws.skip_bits(), stream()),
              "mgr_raster_forward")

    ws, npairs = context(dev).forward(V, N, W, H, launch, sync_check, auto_fence=graph, cams=cams)
    return out, radii, ws, npairs


def _opacity_layout(op, V, N):
    """(N,1)/(N,) -> shared (N); (V,N,1)/(V,N) -> per view (V,N)."""
    if op.dim() == 3:
        return op.reshape(V, N)
    if op.dim() == 2 and op.shape[1] == 1:
        return op.reshape(N)
    if op.dim() == 2:
        return op.reshape(V, N)
    return op.reshape(N)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, colors, opacities, cov3D, cams, bg, W, H, debug, graph=True, share=None):
        V = cams.shape[0]
        means3D, colors, cov3D = f32c(means3D), f32c(colors), f32c(cov3D)
        opac = f32c(opacities)
        N = means3D.shape[-2]
        opac = _opacity_layout(opac, V, N)
        bg = f32c(bg).reshape(-1)
        out, radii, ws, npairs = _run_forward(cams, V, N, W, H, bg, means3D, cov3D, colors, opac, debug, graph=graph)
        ctx.lease = _Lease(ws)
        if share is not None:      # (rasterize_views_features: a second graph node on the same workspace holds the same lease)
            share.lease = ctx.lease
        ctx.meta = (V, N, W, H, bool(debug), means2D.shape, opacities.shape)
        ctx.num_rendered = npairs
        ctx.save_for_backward(means3D, colors, opac, cov3D, cams, bg, out)
        ctx.mark_non_differentiable(radii)
        return out, radii

    @staticmethod
    def backward(ctx, g_color, _g_radii):
        means3D, colors, opac, cov3D, cams, bg, out = ctx.saved_tensors
        V, N, W, H, debug, m2d_shape, op_shape = ctx.meta
        ws = ctx.lease.ws
        dev = means3D.device
        g_color = f32c(g_color)
        d_m3 = torch.empty((V, N, 3), dtype=torch.float32, device=dev)
        d_m2 = torch.empty((V, N, 3), dtype=torch.float32, device=dev)
        d_col = torch.empty((V, N, 3), dtype=torch.float32, device=dev)
        d_op = torch.empty((V, N), dtype=torch.float32, device=dev)
        d_cov = torch.empty((V, N, 6), dtype=torch.float32, device=dev)
        s_m = means3D.stride(0) if means3D.dim() == 3 else 0
        s_c = cov3D.stride(0) if cov3D.dim() == 3 else 0
        s_col = colors.stride(0) if colors.dim() == 3 else 0
        s_o = opac.stride(0) if opac.dim() == 2 else 0
        check(lib().mgr_raster_backward(V, N, W, H, ptr(cams), ptr(bg), ptr(means3D), s_m, ptr(cov3D), s_c,
                                        ptr(colors), s_col, ptr(opac), s_o, ptr(out), ptr(g_color), ptr(d_m3), ptr(d_m2),
                                        ptr(d_col), ptr(d_op), ptr(d_cov), ptr(ws.buf), ws.nbytes, ws.cap,
                                        _lib.MGR_BWD_CHECK if debug else 0, stream()), "mgr_raster_backward")

        def fold(g, shared, shape=None):
            # inputs shared by all views receive the sum over views
            if shared:
                g = g.sum(0) if V > 1 else g[0]
            return g.reshape(shape) if shape is not None else g

        g_m3 = fold(d_m3, means3D.dim() == 2)
        g_m2 = fold(d_m2, len(m2d_shape) == 2, m2d_shape)
        g_col = fold(d_col, colors.dim() == 2)
        g_op = fold(d_op, opac.dim() == 1, op_shape)
        g_cov = fold(d_cov, cov3D.dim() == 2)
        return g_m3, g_m2, g_col, g_op, g_cov, None, None, None, None, None, None, None


def _builds_graph(*tensors):
    """True when autograd records the operator (a backward will follow); False for an evaluation render."""
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def rasterize_views(cams, means3D, means2D, colors, opacities, cov3D, bg, W, H, debug=False):
    """V views in one call.  cams (V,40) from `_lib.pack_cameras`; per-Gaussian
    inputs are (N,..) shared by all views or (V,N,..).  Returns color (V,3,H,W),
    radii (V,N)."""
    return _RasterizeGaussians.apply(means3D, means2D, colors, opacities, cov3D, cams, bg, int(W), int(H), debug,
                                     _builds_graph(means3D, means2D, colors, opacities, cov3D))


MAX_FEATURE_CHANNELS = 32


def _feature_request(features, bg, depth, alpha):
    """The checks of a feature render that need no device: (C, bg as a flat fp32 tensor or None).  ManusHipError on a request
    the library would refuse for its shape alone."""
    C = 0
    if features is not None:
        if not torch.is_tensor(features) or features.dim() not in (2, 3):
            raise _lib.ManusHipError("features must be a tensor (N,C), shared by the views, or (V,N,C)")
        C = int(features.shape[-1])
        if not 1 <= C <= MAX_FEATURE_CHANNELS:
            raise _lib.ManusHipError("features carry %d channels; 1 .. %d are supported" % (C, MAX_FEATURE_CHANNELS))
    if C == 0 and not depth and not alpha:
        raise _lib.ManusHipError("nothing to render: no features, no depth, no alpha")
    if bg is not None:
        bg = torch.as_tensor(bg, dtype=torch.float32).reshape(-1)
        if bg.numel() != C:
            raise _lib.ManusHipError("bg has %d values for %d feature channels" % (bg.numel(), C))
    return C, bg


def blend_features(features=None, bg=None, depth=False, alpha=False, device=None):
    """Composite other per-Gaussian values over the tile lists of the context's LAST forward (mgr_raster_blend_features): no
    projection, no sort, no binning, and exactly the contributions of that forward's image.  features (N,C) shared by the
    views or (V,N,C), 1 <= C <= 32 (a non-contiguous tensor is copied); bg: C values (None: zeros).  Returns
    {"features": (V,C,H,W), "depth": (V,H,W), "alpha": (V,H,W)}, None for what was not asked for.  `depth` is the EXPECTED
    depth sum_i w_i z_i (not divided by alpha, background 0), `alpha` the accumulated opacity 1 - T.  Forward only: no
    gradient flows through it.  ManusHipError when the context has no forward, or its last forward left no complete lists
    (stopped before the blend, depth cut applied, overflow raised)."""
    C, bg = _feature_request(features, bg, depth, alpha)
    with torch.no_grad():
        ctx = context(device)
        ws = ctx.last_ws
        if ws is None:
            raise _lib.ManusHipError("blend_features: no forward has run on this context")
        V, N, W, H = ws.key
        dev = ws.buf.device
        s_f = 0
        if features is not None:
            if features.shape[-2] != N or (features.dim() == 3 and features.shape[0] != V):
                raise _lib.ManusHipError("features %s do not fit the last forward's %d views of %d Gaussians" % (tuple(features.shape), V, N))
            features = f32c(features.detach().to(dev))
            s_f = N * C if features.dim() == 3 else 0
        if bg is not None:
            bg = bg.to(dev).contiguous()
        n_out = C + (1 if depth else 0)
        out = torch.empty((V, n_out, H, W), dtype=torch.float32, device=dev) if n_out else None
        out_a = torch.empty((V, H, W), dtype=torch.float32, device=dev) if alpha else None
        check(lib().mgr_raster_blend_features(V, N, C, W, H, ptr(features), s_f, ptr(bg), int(bool(depth)), ptr(out), ptr(out_a),
                                              ptr(ws.buf), ws.nbytes, ws.cap, stream()), "mgr_raster_blend_features")
        return {"features": out[:, :C] if C else None, "depth": out[:, C] if depth else None, "alpha": out_a}


class _LeaseShare:
    """Carries the colour node's lease out of _RasterizeGaussians.forward."""
    lease = None


def _forward_seq(ws):
    """The workspace's forward sequence number (one blocking read)."""
    seq = ctypes.c_uint32(0)
    check(lib().mgr_raster_forward_seq_sync(ptr(ws.buf), ctypes.byref(seq), stream()), "mgr_raster_forward_seq_sync")
    return int(seq.value)


class _BlendFeatures(torch.autograd.Function):
    """Feature, depth and alpha maps over the lists of the forward that holds `lease`, with their backward
    (mgr_raster_blend_features_backward).  The node notes the workspace's forward sequence number and refuses a backward
    once another forward has used the workspace."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, cov3D, features, cams, bg, lease, depth, alpha, debug):
        # opacities: laid out (N) or (V,N) by the caller; like means2D it is here for its gradient only (the workspace holds the values)
        ws = lease.ws
        V, N, W, H = ws.key
        dev = ws.buf.device
        means3D, cov3D = f32c(means3D), f32c(cov3D)
        C, s_f = 0, 0
        if features is not None:
            features = f32c(features)
            C = int(features.shape[-1])
            s_f = N * C if features.dim() == 3 else 0
        n_out = C + (1 if depth else 0)
        out = torch.empty((V, n_out, H, W), dtype=torch.float32, device=dev) if n_out else None
        out_a = torch.empty((V, H, W), dtype=torch.float32, device=dev) if alpha else None
        check(lib().mgr_raster_blend_features(V, N, C, W, H, ptr(features), s_f, ptr(bg), int(bool(depth)), ptr(out), ptr(out_a),
                                              ptr(ws.buf), ws.nbytes, ws.cap, stream()), "mgr_raster_blend_features")
        ctx.lease = lease
        ctx.seq = _forward_seq(ws)
        ctx.meta = (C, s_f, bool(depth), bool(debug), means2D.shape, opacities.shape, opacities.dim(), n_out > 0, bool(alpha))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(means3D, cov3D, features, cams, bg, out, out_a)
        empty = torch.empty(0, device=dev)
        outs = (out if out is not None else empty, out_a if out_a is not None else empty)
        if out is None:
            ctx.mark_non_differentiable(outs[0])
        if out_a is None:
            ctx.mark_non_differentiable(outs[1])
        return outs

    @staticmethod
    def backward(ctx, g_out, g_alpha):
        means3D, cov3D, features, cams, bg, out, out_a = ctx.saved_tensors
        C, s_f, depth, debug, m2d_shape, op_shape, op_dim, has_out, has_alpha = ctx.meta
        ws = ctx.lease.ws
        V, N, W, H = ws.key
        dev = ws.buf.device
        g_out = f32c(g_out) if (g_out is not None and has_out) else None
        g_alpha = f32c(g_alpha) if (g_alpha is not None and has_alpha) else None
        if g_out is None and g_alpha is None:
            return (None,) * 11
        if _forward_seq(ws) != ctx.seq:
            raise _lib.ManusHipError("rasterize_views_features: another forward has used this workspace since the maps were "
                                     "rendered (forward %d then); their tile lists are gone" % ctx.seq)
        d_m3 = torch.empty((V, N, 3), dtype=torch.float32, device=dev)
        d_m2 = torch.empty((V, N, 3), dtype=torch.float32, device=dev)
        d_op = torch.empty((V, N), dtype=torch.float32, device=dev)
        d_cov = torch.empty((V, N, 6), dtype=torch.float32, device=dev)
        d_f = torch.empty((V, N, C), dtype=torch.float32, device=dev) if C else None
        nbytes = int(lib().mgr_raster_feat_backward_workspace_bytes(V, N, C, W, H, ws.cap))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s_m = means3D.stride(0) if means3D.dim() == 3 else 0
        s_c = cov3D.stride(0) if cov3D.dim() == 3 else 0
        check(lib().mgr_raster_blend_features_backward(V, N, C, W, H, ptr(cams), ptr(means3D), s_m, ptr(cov3D), s_c, ptr(features), s_f,
                                                       ptr(bg), int(depth), ptr(out), ptr(out_a), ptr(g_out), ptr(g_alpha), ptr(d_m3),
                                                       ptr(d_m2), ptr(d_op), ptr(d_cov), ptr(d_f), ptr(ws.buf), ws.nbytes, ws.cap,
                                                       ptr(scratch), nbytes, _lib.MGR_BWD_CHECK if debug else 0, stream()),
              "mgr_raster_blend_features_backward")

        def fold(g, shared, shape=None):   # as _RasterizeGaussians.backward: inputs shared by the views receive the sum
            if shared:
                g = g.sum(0) if V > 1 else g[0]
            return g.reshape(shape) if shape is not None else g

        return (fold(d_m3, means3D.dim() == 2), fold(d_m2, len(m2d_shape) == 2, m2d_shape), fold(d_op, op_dim == 1, op_shape),
                fold(d_cov, cov3D.dim() == 2), fold(d_f, features.dim() == 2) if C else None, None, None, None, None, None, None)


def rasterize_views_features(cams, means3D, means2D, colors, opacities, cov3D, bg, W, H, features=None, feature_bg=None,
                             depth=False, alpha=False, debug=False):
    """`rasterize_views` plus differentiable feature / depth / alpha maps of the same forward: -> (color (V,3,H,W), radii (V,N),
    extras), extras = {"features": (V,C,H,W), "depth": (V,H,W), "alpha": (V,H,W)}, None for what was not asked for (the maps of
    `blend_features`).  The maps carry gradient to features, means3D, means2D, opacities and cov3D (inputs shared by the
    views receive the sum over views); their backward walks the colour forward's tile lists, so both graph nodes hold ONE lease
    on the workspace, and the maps' backward raises ManusHipError if another forward has used the workspace in between."""
    C, fbg = _feature_request(features, feature_bg, depth, alpha)
    if not (torch.is_tensor(means3D) and means3D.is_cuda):
        raise _lib.ManusHipError("rasterize_views_features needs GPU tensors; there is no CPU fallback")
    V, N = cams.shape[0], means3D.shape[-2]
    if features is not None and (features.shape[-2] != N or (features.dim() == 3 and features.shape[0] != V)):
        raise _lib.ManusHipError("features %s do not fit %d views of %d Gaussians" % (tuple(features.shape), V, N))
    dev = means3D.device
    share = _LeaseShare()
    graph = _builds_graph(means3D, means2D, colors, opacities, cov3D, features)
    color, radii = _RasterizeGaussians.apply(means3D, means2D, colors, opacities, cov3D, cams, bg, int(W), int(H), debug, graph, share)
    if features is not None:
        features = features.to(dev)
    if fbg is not None:
        fbg = fbg.to(dev).contiguous()
    opac = _opacity_layout(opacities, V, N)      # (a view: the gradient finds its way back to `opacities`)
    out, out_a = _BlendFeatures.apply(means3D, means2D, opac, cov3D, features, cams, fbg, share.lease, bool(depth), bool(alpha),
                                      bool(debug))
    return color, radii, {"features": out[:, :C] if C else None, "depth": out[:, C] if depth else None,
                          "alpha": out_a if alpha else None}


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """In-frustum mask (view-space z > 0.2), as the upstream helper."""
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix.reshape(4, 4).to(positions)
            z = positions @ vm[:3, 2] + vm[3, 2]
            return z > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        dev = means3D.device
        if not means3D.is_cuda:
            raise _lib.ManusHipError("GaussianRasterizer needs GPU tensors; there is no CPU fallback")
        cams = _lib.pack_cameras(rs.tanfovx, rs.tanfovy, rs.viewmatrix, rs.projmatrix, rs.campos, dev)
        if cov3D_precomp is None:
            _, cov, _ = lbs_cov(means3D, torch.log(scales * rs.scale_modifier), rotations, None, None)
            cov3D_precomp = cov[0]
        if colors_precomp is None:
            K = (rs.sh_degree + 1) ** 2
            sh = shs
            if sh.shape[1] < 16 or K < 16:
                full = torch.zeros((sh.shape[0], 16, 3), dtype=sh.dtype, device=dev)
                k = min(K, sh.shape[1])
                full[:, :k] = sh[:, :k]
                sh = full
            colors_precomp = sh_colors(sh, means3D, None, cams)[0]
        color, radii = _RasterizeGaussians.apply(means3D, means2D, colors_precomp, opacities, cov3D_precomp,
                                                 cams, rs.bg, int(rs.image_width), int(rs.image_height),
                                                 bool(rs.debug), _builds_graph(means3D, means2D, colors_precomp, opacities,
                                                                               cov3D_precomp))
        return color[0], radii[0]

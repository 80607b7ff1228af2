"""LPIPS over the HIP kernels of csrc/lpips.hip (`mgr_lpips`): the reference's fourth loss term, `lpips.LPIPS(net="vgg")`
(src/modules/hand_dynamic.py:59, base.py:333-341), and the LPIPS-AlexNet value of its validation pass (loss_utils.py:19,
111-117).

No weight file ships with this package and none is fetched: the user supplies torchvision's `vgg16` / `alexnet` checkpoint
(keys `features.{i}.weight` / `features.{i}.bias`) and the `lpips` package's `weights/v0.1/{vgg,alex}.pth` (keys
`lin{k}.model.1.weight`, shape (1,C,1,1)); INTEGRATION.md says where.  The weights are frozen.  GPU tensors only; there is
no CPU fallback.

`operands="bf16"` runs every convolution, forward and data gradient, on the bf16 matrix pipe: input values and weights are
rounded to bf16 (round to nearest even), the products summed in fp32; everything else stays fp32 (include/manus_hip.h).  The
default, "fp32", is the k-ordered fp32 chain.

`storage="bf16"` (with `operands="bf16"` only; the `mgr_lpips*_st` entries) also STORES every tensor of the chain -- activations,
taps, pool outputs, gradients -- as bf16, channel-blocked [ceil(C/8)][h][w][8] with zero pad lanes: half the workspace and the
cached taps, one rounding at each store, pool ties to the first position (include/manus_hip.h has the rules).  The scaled image
and the gradient that leaves the chain stay fp32.  `pack_blocked` / `unpack_blocked` convert between (C,h,w) fp32 and those
bytes.  The default, "fp32", is the code without the mode, bit for bit.

Windows (`values_grad(rects=)`, `target_taps`, `fit_rects`): the distance of view v on the rectangle rects[v] = (x0, y0, w, h)
of its frame is the LPIPS of the two crops -- the plain call on contiguous copies of that rectangle, bit for bit, with the
crop's own zero padding and spatial means -- not the full-frame value restricted to a region.  Only the window is convolved
(DESIGN.md section 6 has the times: below about 768^2 they fall more slowly than the area).  A target is a constant of its view: `target_taps` keeps the target tower's five taps of
a window, and a call given them skips that tower (the same bits).

Batches (`values_grad(rects=, batch=B)`, `target_taps(batch=B)`): with B >= 2 the views of a call that share a window size run
as chunks of at most min(B, LP_MAX_BATCH) views, one chain of launches per chunk (`mgr_lpips_roi_batch_op`), bit for bit the
sequential call; the kept workspace grows to the largest chunk's.  `fit_rects(quantum=, common=)` gives a view set windows of a
shared size -- larger windows, and so other values than the tight ones.  The default, batch=0, is the sequential call.
"""
import ctypes
import functools

import numpy as np
import torch

from ._lib import (LP_MAX_BATCH, MGR_LPIPS_BF16, MGR_LPIPS_F32, MGR_LPIPS_STORE_BF16, MGR_LPIPS_STORE_F32, ManusHipError, check, f32c, lib,
                   ptr, stream)

NETS = {"vgg": 0, "alex": 1}
OPERANDS = {"fp32": MGR_LPIPS_F32, "bf16": MGR_LPIPS_BF16}
STORAGES = {"fp32": MGR_LPIPS_STORE_F32, "bf16": MGR_LPIPS_STORE_BF16}
# torchvision `features` indices of the convolutions, (Cout, Cin, K) of each, and the tap channels
CONV_INDEX = {"vgg": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28), "alex": (0, 3, 6, 8, 10)}
CONV_SHAPE = {"vgg": ((64, 3, 3), (64, 64, 3), (128, 64, 3), (128, 128, 3), (256, 128, 3), (256, 256, 3), (256, 256, 3), (512, 256, 3),
                      (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3)),
              "alex": ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))}
TAP_CHANNELS = {"vgg": (64, 128, 256, 512, 512), "alex": (64, 192, 384, 256, 256)}
# which convolution (in layer order) each tap is the output of
TAP_CONV = {"vgg": (1, 3, 6, 9, 12), "alex": (0, 1, 2, 3, 4)}


def _operands(operands, who):
    if operands not in OPERANDS:
        raise ManusHipError("%s: operands must be 'fp32' or 'bf16' (got %r)" % (who, operands))
    return OPERANDS[operands]


def _storage(storage, operands, who):
    """The storage keyword as the C ABI's value; bf16 storage goes with bf16 operands only."""
    if not isinstance(storage, str) or storage not in STORAGES:
        raise ManusHipError("%s: storage must be 'fp32' or 'bf16' (got %r)" % (who, storage))
    if storage == "bf16" and operands != "bf16":
        raise ManusHipError("%s: storage='bf16' needs operands='bf16' (got operands=%r)" % (who, operands))
    return STORAGES[storage]


def pack_blocked(t):
    """fp32 (C,h,w) -> the bytes of bf16 storage: uint8 of 2 * pad8(C) * h * w, laid out [ceil(C/8)][h][w][8], values rounded to
    nearest even, pad lanes zero.  Any device."""
    t = t.detach().to(torch.float32)
    C, h, w = t.shape
    nb = (C + 7) // 8
    full = torch.zeros((nb * 8, h, w), dtype=torch.bfloat16, device=t.device)
    full[:C] = t.to(torch.bfloat16)
    return full.reshape(nb, 8, h, w).permute(0, 2, 3, 1).contiguous().view(torch.uint8).reshape(-1)


def unpack_blocked(buf, C, h, w, pads=False):
    """The bytes of bf16 storage -> fp32 (C,h,w), exactly; pads=True returns all pad8(C) channels (the pad lanes last)."""
    nb = (C + 7) // 8
    n = nb * 8 * h * w * 2
    full = buf.reshape(-1)[:n].view(torch.bfloat16).reshape(nb, h, w, 8).permute(0, 3, 1, 2).reshape(nb * 8, h, w).to(torch.float32)
    return full if pads else full[:C].contiguous()


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def layout(net, H, W, need_grad=True, storage="fp32"):
    """Byte offsets of `mgr_lpips_layout` (`mgr_lpips_layout_st` for storage="bf16"): {"act": pred's convolution outputs, "tap":
    the target's taps, "scratch": (a, b), "part", "total"}."""
    n_conv = len(CONV_INDEX[net])
    buf = (ctypes.c_size_t * (n_conv + 9))()
    st = _storage(storage, "bf16", "layout")
    if st == MGR_LPIPS_STORE_F32:
        rc = lib().mgr_lpips_layout(NETS[net], int(H), int(W), int(bool(need_grad)), buf, len(buf))
    else:
        rc = lib().mgr_lpips_layout_st(NETS[net], int(H), int(W), int(bool(need_grad)), buf, len(buf), st)
    if rc < 0:
        check(rc, "mgr_lpips_layout")
    v = list(buf)
    return {"act": v[:n_conv], "tap": v[n_conv:n_conv + 5], "scratch": (v[n_conv + 5], v[n_conv + 6]), "part": v[n_conv + 7],
            "total": v[n_conv + 8]}


@functools.lru_cache(maxsize=None)
def min_size(net):
    """The smallest height (= width) at which the deepest tap of `net` has a pixel, asked of the library's layer tables."""
    m = 1
    while not lib().mgr_lpips_workspace_bytes(NETS[net], m, m, 0):
        m += 1
    return m


def _rects(rects, V=None):
    """(V,4) int32 host array of x0, y0, w, h."""
    r = np.ascontiguousarray(np.asarray(rects, dtype=np.int64).reshape(-1, 4).astype(np.int32))
    if V is not None and r.shape[0] != V:
        raise ManusHipError("LPIPS: rects must be (V,4) = (%d,4) ints (got %s)" % (V, r.shape))
    return r


def _fit_span(a, n, margin, m, F):
    """The span [a, a + n) grown by `margin`, clamped to [0, F), then grown (evenly, shifted at a border) to m pixels."""
    lo, hi = max(a - margin, 0), min(a + n + margin, F)
    if hi <= lo:
        return 0, 0
    if hi - lo < m:
        lo = min(max(lo - (m - (hi - lo)) // 2, 0), F - m)
        hi = lo + m
    return lo, hi - lo


def _widen_span(a, n, to, F):
    """The span [a, a + n) of a frame side F widened to min(to, F) pixels: grown to the right, shifted left at the border."""
    to = min(int(to), F)
    return min(a, F - to), to


def fit_rects(rects, H, W, net, margin=0, quantum=0, common=False):
    """Rectangles (x0, y0, w, h) made fit for a windowed call on an H x W frame: every non-empty one grown by `margin` on all
    sides, clamped to the frame, then grown or shifted inside the frame to the network's minimum size (`min_size`).  An empty
    rectangle (w or h zero, or nothing left inside the frame) comes back as (0,0,0,0).  Pure host arithmetic; (V,4) int32.
    ValueError for a negative size, margin or quantum, or a frame smaller than the minimum.

    For a batched call (`values_grad(batch=)`), which groups views by window size: quantum > 0 then rounds w and h up to a
    multiple of `quantum`, capped at the frame's side; common=True then gives every non-empty rectangle the largest w and the
    largest h of the set, so that the whole set is one group.  Either keeps the origin and shifts the rectangle at the right /
    bottom border so that it stays inside the frame and contains the rectangle fitted so far.  Both off is the fitting above."""
    m = min_size(net)
    if H < m or W < m:
        raise ValueError("fit_rects: a %dx%d frame is smaller than the %dx%d minimum of the %s network" % (W, H, m, m, net))
    if margin < 0:
        raise ValueError("fit_rects: negative margin")
    if quantum < 0:
        raise ValueError("fit_rects: negative quantum")
    quantum = int(quantum)
    src = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    out = np.zeros(src.shape, np.int32)
    for j, (x0, y0, w, h) in enumerate(src.tolist()):
        if w < 0 or h < 0:
            raise ValueError("fit_rects: rectangle %d has a negative size" % j)
        if w == 0 or h == 0:
            continue
        fx, fw = _fit_span(x0, w, int(margin), m, W)
        fy, fh = _fit_span(y0, h, int(margin), m, H)
        if fw and fh:
            if quantum > 0:
                fx, fw = _widen_span(fx, fw, -(-fw // quantum) * quantum, W)
                fy, fh = _widen_span(fy, fh, -(-fh // quantum) * quantum, H)
            out[j] = (fx, fy, fw, fh)
    if common and out[:, 2].any():
        cw, ch = int(out[:, 2].max()), int(out[:, 3].max())
        for j in range(out.shape[0]):
            if out[j, 2]:
                fx, fw = _widen_span(int(out[j, 0]), int(out[j, 2]), cw, W)
                fy, fh = _widen_span(int(out[j, 1]), int(out[j, 3]), ch, H)
                out[j] = (fx, fy, fw, fh)
    return out


def _batch(batch, who):
    """The `batch` keyword as the C ABI's max_batch: 0 (and 1) is the sequential call."""
    b = int(batch)
    if b < 0:
        raise ManusHipError("%s: batch must be 0 (sequential) or the most views per launch (got %r)" % (who, batch))
    return b


class TargetTaps:
    """The target tower's five taps of each view's window (`LPIPS.target_taps`): one device buffer per view (None for an empty
    view), and what they were built with -- a call with other rects, frame size, network, operand mode, storage or normalize /
    mask flags refuses them."""

    def __init__(self, bufs, rects, frame, net, operands, normalize, masked, storage="fp32"):
        self.bufs, self.rects, self.frame = bufs, rects, frame
        self.net, self.operands, self.normalize, self.masked = net, operands, bool(normalize), bool(masked)
        self.storage = storage

    @property
    def nbytes(self):
        return sum(int(b.numel()) for b in self.bufs if b is not None)

    def matches(self, rects, frame, net, operands, normalize, masked, storage="fp32"):
        return (self.frame == frame and self.net == net and self.operands == operands and self.storage == storage
                and self.normalize == bool(normalize)
                and self.masked == bool(masked) and self.rects.shape == rects.shape and bool((self.rects == rects).all()))


class _Lpips(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1, model, normalize):
        need = ctx.needs_input_grad[0]
        vals, g = model.values_grad(in0.detach(), in1.detach(), normalize=normalize, need_grad=need)
        ctx.save_for_backward(g)
        return vals.reshape(-1, 1, 1, 1)

    @staticmethod
    def backward(ctx, go):
        (g,) = ctx.saved_tensors
        if g is None:
            return None, None, None, None
        return g * go.reshape(-1, 1, 1, 1), None, None, None


class LPIPS:
    """`lpips.LPIPS(net=...)` in eval mode with frozen weights.  Build with `from_state_dicts` or `load`."""

    def __init__(self, net="vgg", operands="fp32", storage="fp32"):
        if net not in NETS:
            raise ManusHipError("LPIPS: net must be 'vgg' or 'alex' (got %r)" % (net,))
        self._op = _operands(operands, "LPIPS")
        self._st = _storage(storage, operands, "LPIPS")
        self.net = net
        self.operands = operands
        self.storage = storage
        self.blob = None
        self._ws = None

    # ---- weights
    @classmethod
    def from_state_dicts(cls, backbone_sd, lin_sd, net="vgg", device="cuda", operands="fp32", storage="fp32"):
        """backbone_sd: torchvision's `vgg16` / `alexnet` state dict; lin_sd: the lpips package's linear layers."""
        self = cls(net, operands, storage)
        ws, bs, lins = [], [], []
        for i, (co, ci, k) in zip(CONV_INDEX[net], CONV_SHAPE[net]):
            for kind, shape, out in (("weight", (co, ci, k, k), ws), ("bias", (co,), bs)):
                key = "features.%d.%s" % (i, kind)
                if key not in backbone_sd:
                    raise ManusHipError("LPIPS(%s): the backbone state dict has no key %r" % (net, key))
                t = backbone_sd[key]
                if tuple(t.shape) != shape:
                    raise ManusHipError("LPIPS(%s): %s has shape %s, expected %s" % (net, key, tuple(t.shape), shape))
                out.append(t)
        for k, c in enumerate(TAP_CHANNELS[net]):
            key = "lin%d.model.1.weight" % k
            if key not in lin_sd:
                raise ManusHipError("LPIPS(%s): the linear-layer state dict has no key %r" % (net, key))
            t = lin_sd[key]
            if tuple(t.shape) != (1, c, 1, 1):
                raise ManusHipError("LPIPS(%s): %s has shape %s, expected %s" % (net, key, tuple(t.shape), (1, c, 1, 1)))
            lins.append(t)
        dev = torch.device(device)
        ws, bs, lins = ([f32c(t.detach().to(dev)) for t in grp] for grp in (ws, bs, lins))
        nbytes = int(lib().mgr_lpips_net_bytes_op(NETS[net], self._op))
        blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for t in ws + bs + lins:
            ptr(t)      # (raises for CPU tensors: there is no CPU fallback)
        check(lib().mgr_lpips_net_pack_op(NETS[net], _ptr_array(ws), _ptr_array(bs), _ptr_array(lins), ptr(blob), nbytes, stream(),
                                          self._op), "mgr_lpips_net_pack_op")
        torch.cuda.current_stream().synchronize()       # the sources may die now
        self.blob = blob
        return self

    @classmethod
    def load(cls, backbone_path, lin_path, net="vgg", device="cuda", operands="fp32", storage="fp32"):
        """torch.load of the two user-supplied files (see the module docstring)."""
        return cls.from_state_dicts(torch.load(backbone_path, map_location="cpu"), torch.load(lin_path, map_location="cpu"), net, device,
                                    operands, storage)

    # ---- the call
    def workspace(self, H, W, need_grad):
        """The kept workspace of one view (mgr_lpips_workspace_bytes, or its _st form for bf16 storage); grown, never shrunk."""
        n = int(self._ws_bytes(H, W, need_grad))
        if n == 0:
            raise ManusHipError("LPIPS(%s): a %dx%d image is too small for the deepest tap to have one pixel" % (self.net, W, H))
        if self._ws is None or self._ws.numel() < n or self._ws.device != self.blob.device:
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.blob.device)
        return self._ws

    @property
    def _blocked(self):
        return self._st == MGR_LPIPS_STORE_BF16

    # the size queries of the model's storage
    def _ws_bytes(self, H, W, need_grad):
        if self._blocked:
            return lib().mgr_lpips_workspace_bytes_st(NETS[self.net], int(H), int(W), int(bool(need_grad)), self._st)
        return lib().mgr_lpips_workspace_bytes(NETS[self.net], int(H), int(W), int(bool(need_grad)))

    def _taps_bytes(self, h, w):
        if self._blocked:
            return lib().mgr_lpips_taps_bytes_st(NETS[self.net], int(h), int(w), self._st)
        return lib().mgr_lpips_taps_bytes(NETS[self.net], int(h), int(w))

    def _grow(self, n):
        if self._ws is None or self._ws.numel() < n or self._ws.device != self.blob.device:
            self._ws = torch.empty(max(int(n), 1), dtype=torch.uint8, device=self.blob.device)
        return self._ws

    def values_grad(self, pred, target, mask=None, normalize=False, need_grad=True, grad_scale=1.0, out_grad=None, accumulate=False,
                    rects=None, grad_scales=None, target_taps=None, batch=0):
        """values (V,) and the gradient of grad_scale * sum(values) w.r.t. pred (V,3,H,W) in one pass (`mgr_lpips`).  `out_grad`:
        write (or, with accumulate, add) the gradient there instead of a new tensor.

        rects: (V,4) host ints x0, y0, w, h -- the windowed call (`mgr_lpips_roi_op`, module docstring): view v is the LPIPS of
        the crops at rects[v]; its gradient is the crop's inside the rectangle and, outside it, zero (or, with accumulate,
        untouched).  An empty rectangle gives the value 0 and no gradient.  grad_scales: V floats, one per view, instead of the
        one grad_scale.  target_taps: a `TargetTaps` of `target_taps(...)` on the same rects, mask and flags: the target tower
        is skipped, `target` may then be None.  rects=None is the plain call.  batch: the most views per launch; 0 or 1 is the
        sequential call, >= 2 runs the views that share a window size as chunks of that many (at most LP_MAX_BATCH) on
        `mgr_lpips_roi_batch_op` -- the same bits, a kept workspace of the largest chunk.  A full-frame batch is rects = the
        frame: batch without rects is refused."""
        if self.blob is None:
            raise ManusHipError("LPIPS: no weights (build with LPIPS.from_state_dicts or LPIPS.load)")
        if rects is not None:
            return self._values_grad_roi(pred, target, mask, normalize, need_grad, grad_scale, out_grad, accumulate, rects, grad_scales,
                                         target_taps, _batch(batch, "LPIPS"))
        if _batch(batch, "LPIPS"):
            raise ManusHipError("LPIPS: batch belongs to the windowed call (rects=); a full-frame batch is rects = the frame")
        if grad_scales is not None or target_taps is not None:
            raise ManusHipError("LPIPS: grad_scales and target_taps belong to the windowed call (rects=)")
        pred, target = f32c(pred), f32c(target)
        if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != target.shape:
            raise ManusHipError("LPIPS: images are (N,3,H,W), both of one shape (got %s, %s)" % (tuple(pred.shape), tuple(target.shape)))
        V, _, H, W = pred.shape
        if mask is not None:
            mask = f32c(mask)
            if tuple(mask.shape) != (V, H, W):
                raise ManusHipError("LPIPS: mask must be (N,H,W)")
        g = None
        if need_grad:
            g = out_grad if out_grad is not None else torch.empty_like(pred)
            if g.shape != pred.shape or g.dtype != torch.float32:
                raise ManusHipError("LPIPS: out_grad must be fp32 of pred's shape")
        ws = self.workspace(H, W, need_grad)
        vals = torch.empty(V, dtype=torch.float32, device=pred.device)
        if self._blocked:
            check(lib().mgr_lpips_st(NETS[self.net], V, H, W, ptr(pred), ptr(target), ptr(mask), ptr(self.blob), self.blob.numel(),
                                     int(bool(normalize)), float(grad_scale), ptr(vals), ptr(g), int(bool(accumulate)), ptr(ws), ws.numel(),
                                     stream(), self._op, self._st), "mgr_lpips_st")
            return vals, g
        check(lib().mgr_lpips_op(NETS[self.net], V, H, W, ptr(pred), ptr(target), ptr(mask), ptr(self.blob), self.blob.numel(),
                                 int(bool(normalize)), float(grad_scale), ptr(vals), ptr(g), int(bool(accumulate)), ptr(ws), ws.numel(),
                                 stream(), self._op), "mgr_lpips_op")
        return vals, g

    def _frames(self, pred, target, mask):
        """The checked frames of a windowed call: (pred, target or None, mask or None, V, H, W)."""
        pred = f32c(pred)
        if pred.dim() != 4 or pred.shape[1] != 3:
            raise ManusHipError("LPIPS: images are (N,3,H,W) (got %s)" % (tuple(pred.shape),))
        if target is not None:
            target = f32c(target)
            if target.shape != pred.shape:
                raise ManusHipError("LPIPS: images are (N,3,H,W), both of one shape (got %s, %s)" % (tuple(pred.shape), tuple(target.shape)))
        V, _, H, W = pred.shape
        if mask is not None:
            mask = f32c(mask)
            if tuple(mask.shape) != (V, H, W):
                raise ManusHipError("LPIPS: mask must be (N,H,W)")
        return pred, target, mask, V, H, W

    def _values_grad_roi(self, pred, target, mask, normalize, need_grad, grad_scale, out_grad, accumulate, rects, grad_scales, taps,
                         batch=0):
        if target is None and taps is None:
            raise ManusHipError("LPIPS: a windowed call needs target or target_taps")
        pred, target, mask, V, H, W = self._frames(pred, target, mask)
        rects = _rects(rects, V)
        tap_ptrs = None
        if taps is not None:
            if not isinstance(taps, TargetTaps) or not taps.matches(rects, (H, W), self.net, self.operands, normalize, mask is not None,
                                                                    self.storage):
                raise ManusHipError("LPIPS: target_taps were built with other rects, frame size, network, operand mode, storage or "
                                    "normalize / mask flags than this call's")
            tap_ptrs = (ctypes.c_void_p * V)(*[None if b is None else ptr(b) for b in taps.bufs])
        scales = [float(grad_scale)] * V if grad_scales is None else [float(x) for x in grad_scales]
        if len(scales) != V:
            raise ManusHipError("LPIPS: grad_scales must hold one float per view")
        g = None
        if need_grad:
            g = out_grad if out_grad is not None else torch.empty_like(pred)
            if g.shape != pred.shape or g.dtype != torch.float32:
                raise ManusHipError("LPIPS: out_grad must be fp32 of pred's shape")
        rp = rects.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        # (0 where a rectangle is refused: the call below says which and why)
        vals = torch.empty(V, dtype=torch.float32, device=pred.device)
        if self._blocked:
            # (max_batch = 1 is the sequential windowed call)
            mb = max(batch, 1)
            ws = self._grow(lib().mgr_lpips_roi_batch_workspace_bytes_st(NETS[self.net], V, rp, int(bool(need_grad)), mb, self._st))
            check(lib().mgr_lpips_roi_batch_st(NETS[self.net], V, H, W, rp, ptr(pred), ptr(target), ptr(mask), ptr(self.blob),
                                               self.blob.numel(), int(bool(normalize)), (ctypes.c_float * V)(*scales), ptr(vals), ptr(g),
                                               int(bool(accumulate)), tap_ptrs, ptr(ws), ws.numel(), stream(), self._op, mb, self._st),
                  "mgr_lpips_roi_batch_st")
            return vals, g
        if batch >= 2:
            ws = self._grow(lib().mgr_lpips_roi_batch_workspace_bytes(NETS[self.net], V, rp, int(bool(need_grad)), batch))
            check(lib().mgr_lpips_roi_batch_op(NETS[self.net], V, H, W, rp, ptr(pred), ptr(target), ptr(mask), ptr(self.blob),
                                               self.blob.numel(), int(bool(normalize)), (ctypes.c_float * V)(*scales), ptr(vals), ptr(g),
                                               int(bool(accumulate)), tap_ptrs, ptr(ws), ws.numel(), stream(), self._op, batch),
                  "mgr_lpips_roi_batch_op")
            return vals, g
        ws = self._grow(lib().mgr_lpips_roi_workspace_bytes(NETS[self.net], V, rp, int(bool(need_grad))))
        check(lib().mgr_lpips_roi_op(NETS[self.net], V, H, W, rp, ptr(pred), ptr(target), ptr(mask), ptr(self.blob), self.blob.numel(),
                                     int(bool(normalize)), (ctypes.c_float * V)(*scales), ptr(vals), ptr(g), int(bool(accumulate)),
                                     tap_ptrs, ptr(ws), ws.numel(), stream(), self._op), "mgr_lpips_roi_op")
        return vals, g

    def target_taps(self, target, rects, mask=None, normalize=False, batch=0):
        """The target tower's taps of every view's window (`mgr_lpips_roi_taps_op`), for `values_grad(target_taps=)`: a
        `TargetTaps` holding mgr_lpips_taps_bytes per non-empty view.  target (V,3,H,W), mask (V,H,W) or None, rects (V,4).
        batch >= 2: the views that share a window size are built as chunks of that many (`mgr_lpips_roi_taps_batch_op`); the
        buffers are the same, bit for bit."""
        if self.blob is None:
            raise ManusHipError("LPIPS: no weights (build with LPIPS.from_state_dicts or LPIPS.load)")
        target, _, mask, V, H, W = self._frames(target, None, mask)
        rects = _rects(rects, V)
        net, bufs = NETS[self.net], []
        batch = _batch(batch, "LPIPS.target_taps")
        if batch >= 2 or self._blocked:
            # (0 bytes where a rectangle is refused: the call says which and why)
            bufs = [None if rects[v, 2] == 0 or rects[v, 3] == 0 else
                    torch.empty(max(int(self._taps_bytes(rects[v, 3], rects[v, 2])), 1), dtype=torch.uint8, device=target.device)
                    for v in range(V)]
            rp = rects.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
            if self._blocked:
                # (max_batch = 1 builds the taps view by view)
                mb = max(batch, 1)
                ws = self._grow(lib().mgr_lpips_roi_batch_workspace_bytes_st(net, V, rp, 0, mb, self._st))
                check(lib().mgr_lpips_roi_taps_batch_st(net, V, H, W, rp, ptr(target), ptr(mask), ptr(self.blob), self.blob.numel(),
                                                        int(bool(normalize)),
                                                        (ctypes.c_void_p * V)(*[None if b is None else ptr(b) for b in bufs]), mb, ptr(ws),
                                                        ws.numel(), stream(), self._op, self._st), "mgr_lpips_roi_taps_batch_st")
                return TargetTaps(bufs, rects.copy(), (H, W), self.net, self.operands, normalize, mask is not None, self.storage)
            ws = self._grow(lib().mgr_lpips_roi_batch_workspace_bytes(net, V, rp, 0, batch))
            check(lib().mgr_lpips_roi_taps_batch_op(net, V, H, W, rp, ptr(target), ptr(mask), ptr(self.blob), self.blob.numel(),
                                                    int(bool(normalize)), (ctypes.c_void_p * V)(*[None if b is None else ptr(b) for b in bufs]),
                                                    batch, ptr(ws), ws.numel(), stream(), self._op), "mgr_lpips_roi_taps_batch_op")
            return TargetTaps(bufs, rects.copy(), (H, W), self.net, self.operands, normalize, mask is not None, self.storage)
        for v in range(V):
            x0, y0, w, h = (int(t) for t in rects[v])
            if w == 0 or h == 0:
                bufs.append(None)
                continue
            # (0 bytes where the rectangle is refused: the call says why)
            buf = torch.empty(max(int(lib().mgr_lpips_taps_bytes(net, h, w)), 1), dtype=torch.uint8, device=target.device)
            ws = self._grow(lib().mgr_lpips_workspace_bytes(net, h, w, 0))
            check(lib().mgr_lpips_roi_taps_op(net, H, W, rects[v].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ptr(target[v]),
                                              None if mask is None else ptr(mask[v]), ptr(self.blob), self.blob.numel(),
                                              int(bool(normalize)), ptr(buf), ptr(ws), ws.numel(), stream(), self._op),
                  "mgr_lpips_roi_taps_op")
            bufs.append(buf)
        return TargetTaps(bufs, rects.copy(), (H, W), self.net, self.operands, normalize, mask is not None, self.storage)

    def __call__(self, in0, in1, normalize=False):
        """d(in0, in1) of shape (N,1,1,1) for (N,3,H,W) images, differentiable in in0 (VGG only)."""
        if in0.dim() == 3:
            in0, in1 = in0[None], in1[None]
        return _Lpips.apply(in0, in1, self, bool(normalize))


def conv2d(x, w, bias=None, stride=1, pad=0, relu=True, gate=None, transposed=False, operands="fp32", x_storage="fp32", y_storage="fp32",
           raw=False):
    """One convolution of the backbones on its own (`mgr_lpips_conv_op`, or `mgr_lpips_conv_st` where a storage is "bf16"; tests
    and tools).  x (Cin,H,W), w (Cout,Cin,K,K).  x_storage="bf16": x and gate reach the kernel as `pack_blocked` of the fp32
    tensors given (so rounded to bf16).  y_storage="bf16": the kernel writes blocked bf16; the result is `unpack_blocked` of it,
    or with raw=True the bytes themselves."""
    op = _operands(operands, "conv2d")
    xs, ys = _storage(x_storage, operands, "conv2d"), _storage(y_storage, operands, "conv2d")
    x, w = f32c(x), f32c(w)
    co, ci, kh, kw = w.shape
    cx, H, W = x.shape
    if cx != (co if transposed else ci):
        raise ManusHipError("conv2d: x has %d channels" % cx)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    cy = ci if transposed else co
    if ys == MGR_LPIPS_STORE_BF16:
        y = torch.empty(((cy + 7) // 8) * 8 * Ho * Wo * 2, dtype=torch.uint8, device=x.device)
    else:
        y = torch.empty((cy, Ho, Wo), dtype=torch.float32, device=x.device)
    n = int(lib().mgr_lpips_conv_scratch_bytes_op(ci, co, kh, kw, op))
    scratch = torch.empty(n, dtype=torch.uint8, device=x.device)
    gate = None if gate is None else f32c(gate)
    if xs == MGR_LPIPS_STORE_BF16:
        x, gate = pack_blocked(x), None if gate is None else pack_blocked(gate)
    if xs == MGR_LPIPS_STORE_F32 and ys == MGR_LPIPS_STORE_F32:
        check(lib().mgr_lpips_conv_op(ci, co, H, W, kh, kw, int(stride), int(pad), ptr(x), ptr(gate), ptr(w),
                                      ptr(None if bias is None else f32c(bias)), int(bool(relu)), int(bool(transposed)), ptr(y), ptr(scratch),
                                      n, stream(), op), "mgr_lpips_conv_op")
        return y
    check(lib().mgr_lpips_conv_st(ci, co, H, W, kh, kw, int(stride), int(pad), ptr(x), ptr(gate), ptr(w),
                                  ptr(None if bias is None else f32c(bias)), int(bool(relu)), int(bool(transposed)), ptr(y), ptr(scratch), n,
                                  stream(), op, xs, ys), "mgr_lpips_conv_st")
    if ys == MGR_LPIPS_STORE_BF16 and not raw:
        return unpack_blocked(y, cy, Ho, Wo)
    return y

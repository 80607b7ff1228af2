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
"""
import ctypes

import torch

from ._lib import MGR_LPIPS_BF16, MGR_LPIPS_F32, ManusHipError, check, f32c, lib, ptr, stream

NETS = {"vgg": 0, "alex": 1}
OPERANDS = {"fp32": MGR_LPIPS_F32, "bf16": MGR_LPIPS_BF16}
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


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def layout(net, H, W, need_grad=True):
    """Byte offsets of `mgr_lpips_layout`: {"act": pred's convolution outputs, "tap": the target's taps, "scratch": (a, b),
    "part", "total"}."""
    n_conv = len(CONV_INDEX[net])
    buf = (ctypes.c_size_t * (n_conv + 9))()
    rc = lib().mgr_lpips_layout(NETS[net], int(H), int(W), int(bool(need_grad)), buf, len(buf))
    if rc < 0:
        check(rc, "mgr_lpips_layout")
    v = list(buf)
    return {"act": v[:n_conv], "tap": v[n_conv:n_conv + 5], "scratch": (v[n_conv + 5], v[n_conv + 6]), "part": v[n_conv + 7],
            "total": v[n_conv + 8]}


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

    def __init__(self, net="vgg", operands="fp32"):
        if net not in NETS:
            raise ManusHipError("LPIPS: net must be 'vgg' or 'alex' (got %r)" % (net,))
        self._op = _operands(operands, "LPIPS")
        self.net = net
        self.operands = operands
        self.blob = None
        self._ws = None

    # ---- weights
    @classmethod
    def from_state_dicts(cls, backbone_sd, lin_sd, net="vgg", device="cuda", operands="fp32"):
        """backbone_sd: torchvision's `vgg16` / `alexnet` state dict; lin_sd: the lpips package's linear layers."""
        self = cls(net, operands)
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
    def load(cls, backbone_path, lin_path, net="vgg", device="cuda", operands="fp32"):
        """torch.load of the two user-supplied files (see the module docstring)."""
        return cls.from_state_dicts(torch.load(backbone_path, map_location="cpu"), torch.load(lin_path, map_location="cpu"), net, device,
                                    operands)

    # ---- the call
    def workspace(self, H, W, need_grad):
        """The kept workspace of one view (mgr_lpips_workspace_bytes); grown, never shrunk."""
        n = int(lib().mgr_lpips_workspace_bytes(NETS[self.net], int(H), int(W), int(bool(need_grad))))
        if n == 0:
            raise ManusHipError("LPIPS(%s): a %dx%d image is too small for the deepest tap to have one pixel" % (self.net, W, H))
        if self._ws is None or self._ws.numel() < n or self._ws.device != self.blob.device:
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.blob.device)
        return self._ws

    def values_grad(self, pred, target, mask=None, normalize=False, need_grad=True, grad_scale=1.0, out_grad=None, accumulate=False):
        """values (V,) and the gradient of grad_scale * sum(values) w.r.t. pred (V,3,H,W) in one pass (`mgr_lpips`).  `out_grad`:
        write (or, with accumulate, add) the gradient there instead of a new tensor."""
        if self.blob is None:
            raise ManusHipError("LPIPS: no weights (build with LPIPS.from_state_dicts or LPIPS.load)")
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
        check(lib().mgr_lpips_op(NETS[self.net], V, H, W, ptr(pred), ptr(target), ptr(mask), ptr(self.blob), self.blob.numel(),
                                 int(bool(normalize)), float(grad_scale), ptr(vals), ptr(g), int(bool(accumulate)), ptr(ws), ws.numel(),
                                 stream(), self._op), "mgr_lpips_op")
        return vals, g

    def __call__(self, in0, in1, normalize=False):
        """d(in0, in1) of shape (N,1,1,1) for (N,3,H,W) images, differentiable in in0 (VGG only)."""
        if in0.dim() == 3:
            in0, in1 = in0[None], in1[None]
        return _Lpips.apply(in0, in1, self, bool(normalize))


def conv2d(x, w, bias=None, stride=1, pad=0, relu=True, gate=None, transposed=False, operands="fp32"):
    """One convolution of the backbones on its own (`mgr_lpips_conv_op`; tests and tools).  x (Cin,H,W), w (Cout,Cin,K,K)."""
    op = _operands(operands, "conv2d")
    x, w = f32c(x), f32c(w)
    co, ci, kh, kw = w.shape
    cx, H, W = x.shape
    if cx != (co if transposed else ci):
        raise ManusHipError("conv2d: x has %d channels" % cx)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    y = torch.empty((ci if transposed else co, Ho, Wo), dtype=torch.float32, device=x.device)
    n = int(lib().mgr_lpips_conv_scratch_bytes_op(ci, co, kh, kw, op))
    scratch = torch.empty(n, dtype=torch.uint8, device=x.device)
    check(lib().mgr_lpips_conv_op(ci, co, H, W, kh, kw, int(stride), int(pad), ptr(x), ptr(None if gate is None else f32c(gate)), ptr(w),
                                  ptr(None if bias is None else f32c(bias)), int(bool(relu)), int(bool(transposed)), ptr(y), ptr(scratch),
                                  n, stream(), op), "mgr_lpips_conv_op")
    return y

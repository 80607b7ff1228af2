"""The bf16 operand mode of LPIPS (mgr_lpips_op with MGR_LPIPS_BF16) restated on the CPU, for the tests.  tests/lpips_ref.py is
imported and left as it is.

    rb(t) = t.float().bfloat16().double()        round to nearest even, as v_cvt_pk_bf16_f32

Two references:
  * `conv` / `conv_data_grad`: ONE convolution (or its data gradient) in fp64 on rb(input), rb(weight): what the kernel computes
    up to the order of its fp32 sums (a product of two bf16 values is exact in fp32);
  * the EMULATION of the whole chain: lpips_ref's features / backward with rb applied to every convolution's input (after the
    gate) and weight, every pre-activation rounded to fp32, everything else in fp64.  Its distance to the fp64 restatement of
    lpips_ref is what the mode costs; the GPU bars of tests/test_gpu_lpips_bf16.py are multiples of it.
"""
import functools

import torch
import torch.nn.functional as F

import lpips_ref as R

# (W, H, seed) of the end-to-end tests: lpips_ref.GRAD_CASES and one more; stand-in weights of seed 0
CASES = tuple(R.GRAD_CASES) + ((40, 24, 9),)
WEIGHT_SEED = 0


def rb(t):
    return t.float().bfloat16().double()


def conv(x, w, b=None, stride=1, pad=0, relu=True, dtype=torch.float64):
    """[relu](conv(rb(x), rb(w)) + b) at `dtype`; x (Cin,H,W), w (Cout,Cin,K,K)."""
    y = F.conv2d(rb(x).to(dtype)[None], rb(w).to(dtype), None if b is None else b.to(dtype), stride=stride, padding=pad)[0]
    return torch.relu(y) if relu else y


def conv_data_grad(g, w, pad, gate=None, dtype=torch.float64):
    """The data gradient of a stride-1 layer w (Cout,Cin,K,K): g (Cout,H,W), zeroed where gate <= 0 BEFORE the rounding."""
    if gate is not None:
        g = g * (gate > 0)
    return F.conv_transpose2d(rb(g).to(dtype)[None], rb(w).to(dtype), stride=1, padding=pad)[0]


def _r32(t):
    return t.float().double()


def features(net, wts, x, decisions=None):
    """lpips_ref.features with bf16 operands: x the scaled image (3,H,W) in fp64."""
    out = {"pre": [], "act": [], "tap": [None] * 5, "win": []}
    cur, ci, pi = _r32(x), 0, 0
    for op in R.OPS[net]:
        if op[0] == "c":
            _, _, _, k, s, p, tap = op
            pre = _r32(F.conv2d(rb(cur)[None], rb(wts["w"][ci]), wts["b"][ci].double(), stride=s, padding=p)[0])
            cur = torch.relu(pre) if decisions is None else pre * decisions["relu"][ci].double()
            out["pre"].append(pre)
            out["act"].append(cur)
            if tap >= 0:
                out["tap"][tap] = cur
            ci += 1
        else:
            k = op[1]
            if k == 2:
                v = R.windows2(cur)
                out["win"].append(v)
                if decisions is None:
                    cur = F.max_pool2d(cur[None], 2, 2)[0]
                else:
                    cur = torch.gather(v, -1, decisions["pool"][pi][..., None])[..., 0]
            else:
                out["win"].append(None)
                cur = F.max_pool2d(cur[None], k, 2)[0]
            pi += 1
    return out


def forward(net, wts, x0, x1, mask=None, normalize=False, decisions=None):
    """lpips_ref.forward with bf16 operands: (value, features of x0, features of x1)."""
    dt = torch.float64
    a = features(net, wts, R.scaled(x0, mask, normalize, dt), decisions)
    b = features(net, wts, R.scaled(x1, mask, normalize, dt))
    val = sum(R.head(a["tap"][k], b["tap"][k], wts["lin"][k], dt) for k in range(5))
    return val, a, b


def backward(net, wts, fa, fb, decisions, mask=None, normalize=False):
    """lpips_ref.backward with bf16 operands in every data gradient (the gated gradient is rounded, as the kernel stages it)."""
    assert net == "vgg"
    dt = torch.float64
    ops = R.OPS[net]
    ci, pi = sum(1 for op in ops if op[0] == "c"), sum(1 for op in ops if op[0] == "p")
    g = None
    for op in reversed(ops):
        if op[0] == "c":
            ci -= 1
            tap = op[6]
            if tap >= 0:
                hg = _r32(R.head_grad(fa["tap"][tap], fb["tap"][tap], wts["lin"][tap], dt))
                g = hg if g is None else _r32(g + hg)
            g = g * decisions["relu"][ci].double()
            g = _r32(F.conv_transpose2d(rb(g)[None], rb(wts["w"][ci]), stride=1, padding=op[5])[0])
        else:
            pi -= 1
            idx = decisions["pool"][pi]
            C, Ho, Wo = idx.shape
            src = fa["act"][ci - 1]
            full = torch.zeros((C, Ho, Wo, 4), dtype=dt).scatter_(-1, idx[..., None], g[..., None])
            gi = torch.zeros((C,) + tuple(src.shape[1:]), dtype=dt)
            gi[:, :2 * Ho, :2 * Wo] = full.reshape(C, Ho, Wo, 2, 2).permute(0, 1, 3, 2, 4).reshape(C, 2 * Ho, 2 * Wo)
            g = gi
    g = g / torch.tensor(R.SCALE, dtype=dt)[:, None, None]
    if normalize:
        g = g * 2
    if mask is not None:
        g = g * mask.double()[None]
    return g


def cosine(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a * b).sum() / (a.norm() * b.norm()))


def grad64(wts, pred, target, dec, H, W):
    """The fp64 chain's gradient for the decisions `dec` (lpips_ref, unchanged)."""
    _, fz, fzb = R.forward("vgg", wts, pred, target, decisions=dec)
    return R.backward("vgg", wts, fz, fzb, dec, (H, W))


@functools.lru_cache(maxsize=None)
def weights(net="vgg"):
    return R.make_weights(net, WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def case(W, H, seed):
    """Everything the tests need of one committed VGG case, computed once: the fp64 restatement, the emulation, and the
    emulation's distances to the restatement (value: relative; act: lpips_ref.rel_err per layer; grad: max_rel_err and cosine,
    both gradients for the emulation's own decisions)."""
    wts = weights()
    pred, target, _ = R.images(seed, 1, H, W)
    v64, fa, fb = R.forward("vgg", wts, pred[0], target[0])
    ve, ea, eb = forward("vgg", wts, pred[0], target[0])
    dec = R.decisions_of("vgg", ea["act"])
    g64 = grad64(wts, pred[0], target[0], dec, H, W)
    ge = backward("vgg", wts, ea, eb, dec)
    return {"pred": pred, "target": target, "value64": float(v64), "value_emul": float(ve), "f64": fa, "f64_target": fb, "emul": ea,
            "value_err": abs(float(ve) - float(v64)) / abs(float(v64)),
            "act_err": [R.rel_err(e, r) for e, r in zip(ea["act"], fa["act"])],
            "grad_err": float((ge - g64).abs().max() / g64.abs().max()), "grad_cos": cosine(ge, g64)}

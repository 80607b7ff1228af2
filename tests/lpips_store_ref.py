"""The bf16 storage mode of LPIPS (the mgr_lpips*_st entries with MGR_LPIPS_STORE_BF16) restated on the CPU, for the tests:
tests/lpips_bf16_ref.py with rb applied ONCE to every stored tensor.  lpips_ref.py and lpips_bf16_ref.py are imported and left
as they are.

    stored activation   rb(relu(fp32(conv(stored input, rb(w)) + b)))         (the stored input IS the operand: rb(rb(t)) = rb(t))
    pool                the maximum of the stored values; the winner is the first maximum among the STORED values
    head gradient       rb(head_grad(stored taps))
    head + deeper       rb(stored g + head_grad)          one rounding of the fp32 sum
    data gradient       rb(fp32(conv_transpose(stored g * gate, rb(w)))), the gate being `stored activation > 0`;
                        layer 0's, dL/d(scaled image), is NOT rounded (it is stored fp32)

Everything else (the scaled image, the heads' values, the means) is lpips_bf16_ref's.
"""
import functools

import torch
import torch.nn.functional as F

import lpips_bf16_ref as B
import lpips_ref as R

rb = B.rb
CASES = B.CASES


def conv_shapes(net, H, W):
    """(C, h, w) of every convolution output in layer order, and the index of the convolution each tap is."""
    shapes, taps, h, w = [], [None] * 5, H, W
    for op in R.OPS[net]:
        if op[0] == "c":
            _, _, co, k, s, p, tap = op
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            if tap >= 0:
                taps[tap] = len(shapes)
            shapes.append((co, h, w))
        else:
            h, w = (h - op[1]) // 2 + 1, (w - op[1]) // 2 + 1
    return shapes, taps


def features(net, wts, x, decisions=None):
    """lpips_bf16_ref.features with every convolution output rounded once at the store; x the scaled image (3,H,W) in fp64."""
    out = {"pre": [], "act": [], "tap": [None] * 5, "win": []}
    cur, ci, pi = B._r32(x), 0, 0
    for op in R.OPS[net]:
        if op[0] == "c":
            _, _, _, k, s, p, tap = op
            pre = B._r32(F.conv2d(rb(cur)[None], rb(wts["w"][ci]), wts["b"][ci].double(), stride=s, padding=p)[0])
            cur = rb(torch.relu(pre) if decisions is None else pre * decisions["relu"][ci].double())
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
    """(value, features of x0, features of x1) in the storage mode."""
    dt = torch.float64
    a = features(net, wts, R.scaled(x0, mask, normalize, dt), decisions)
    b = features(net, wts, R.scaled(x1, mask, normalize, dt))
    val = sum(R.head(a["tap"][k], b["tap"][k], wts["lin"][k], dt) for k in range(5))
    return val, a, b


def backward(net, wts, fa, fb, decisions, mask=None, normalize=False):
    """lpips_bf16_ref.backward with every gradient buffer rounded once at its store; the final 3-channel gradient is not."""
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
                hg = B._r32(R.head_grad(fa["tap"][tap], fb["tap"][tap], wts["lin"][tap], dt))
                g = rb(hg) if g is None else rb(B._r32(g + hg))
            g = g * decisions["relu"][ci].double()
            g = B._r32(F.conv_transpose2d(rb(g)[None], rb(wts["w"][ci]), stride=1, padding=op[5])[0])
            if ci > 0:
                g = rb(g)
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


@functools.lru_cache(maxsize=None)
def case(W, H, seed):
    """lpips_bf16_ref.case for the storage emulation: its distances to the fp64 restatement, in the same units."""
    c = B.case(W, H, seed)
    wts = B.weights()
    pred, target = c["pred"], c["target"]
    ve, ea, eb = forward("vgg", wts, pred[0], target[0])
    dec = R.decisions_of("vgg", ea["act"])
    g64 = B.grad64(wts, pred[0], target[0], dec, H, W)
    ge = backward("vgg", wts, ea, eb, dec)
    return {"pred": pred, "target": target, "value64": c["value64"], "value_emul": float(ve), "f64": c["f64"], "emul": ea, "emul_target": eb,
            "value_err": abs(float(ve) - c["value64"]) / abs(c["value64"]),
            "act_err": [R.rel_err(e, r) for e, r in zip(ea["act"], c["f64"]["act"])],
            "grad_err": float((ge - g64).abs().max() / g64.abs().max()), "grad_cos": B.cosine(ge, g64), "operand": c}

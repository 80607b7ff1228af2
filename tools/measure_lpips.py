#!/usr/bin/env python3
"""Time the LPIPS term (csrc/lpips.hip, manus_amd/lpips.py).

    python tools/measure_lpips.py [--out FILE.json] [--quick] [--operands bf16] [--storage bf16]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats).  Stand-in
weights (seeded randn * sqrt(2 / fan_in)): no weight file ships, and the convolutions are dense, so their time does not depend
on the values.
With --operands bf16 every row of the three tables is run in BOTH operand modes, fp32 first, in this one process (a bf16 time
is only ever read beside the fp32 time of the same run); the result's "modes" then has both, and "speedup" their ratios.
With --storage bf16 (which needs --operands bf16) a third mode, "bf16_store", is bf16 operands with bf16 channel-blocked storage
(the mgr_lpips*_st entries; the convolutions alone through mgr_lpips_conv_st, blocked in and out, layer 0 fp32 in); every row
has it as one more column, with the workspace and taps bytes, and "storage_speedup" is its ratio to "bf16".  The modes of a row
alternate sample by sample.
  * every VGG convolution alone (mgr_lpips_conv_op: one launch of the weight pack + k_lp_conv; the pack's own time is reported
    next to it and subtracted) at 1280x720 and 1920x1080, one view: time and achieved TF/s (2 Cin Cout 9 Ho Wo flop), and the
    ratio to the 122 TF of an untuned fp32-MFMA GEMM at 4096^3;
  * the whole call (mgr_lpips, VGG, one view) forward only and with the gradient, and AlexNet forward only;
  * the bench step (bench.py's scene and targets: 300k hand Gaussians, 8 views of 1920x1080, loss l1+ssim) with the term off
    and on.
Needs a GPU; there is no fallback."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import statistics  # noqa: E402

from measure_feature_render import timed  # noqa: E402


def timed_alt(fns, repeats, samples=5):
    """`timed` of every function of the dict `fns`, their samples alternating: sample j of every function before sample j + 1
    of any."""
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeats):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / repeats)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), repeats=repeats) for k, v in out.items()}

GEMM_TF = 122.0      # untuned LDS-tiled mfma_f32_32x32x2f32 GEMM at 4096^3 on this device class


def stand_in(net, dev, operands="fp32", storage="fp32"):
    from manus_amd.lpips import CONV_INDEX, CONV_SHAPE, LPIPS, TAP_CHANNELS
    g = torch.Generator().manual_seed(0)
    sd, lin = {}, {}
    for i, (co, ci, k) in zip(CONV_INDEX[net], CONV_SHAPE[net]):
        sd["features.%d.weight" % i] = torch.randn((co, ci, k, k), generator=g) * math.sqrt(2.0 / (ci * k * k))
        sd["features.%d.bias" % i] = torch.randn(co, generator=g)
    for k, c in enumerate(TAP_CHANNELS[net]):
        lin["lin%d.model.1.weight" % k] = torch.randn((1, c, 1, 1), generator=g).abs()
    return LPIPS.from_state_dicts(sd, lin, net=net, device=dev, operands=operands, storage=storage), sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--no-step", action="store_true", help="skip the bench step")
    ap.add_argument("--operands", default="fp32", choices=("fp32", "bf16"), help="bf16: measure both modes, fp32 beside bf16")
    ap.add_argument("--storage", default="fp32", choices=("fp32", "bf16"), help="bf16: a third mode, bf16 operands with bf16 storage")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_lpips.py needs a GPU"
    assert a.storage == "fp32" or a.operands == "bf16", "--storage bf16 needs --operands bf16"
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.lpips import CONV_INDEX, CONV_SHAPE, OPERANDS, STORAGES, pack_blocked
    dev = "cuda:0"
    modes = ("fp32",) if a.operands == "fp32" else ("fp32", "bf16") + (("bf16_store",) if a.storage == "bf16" else ())
    OPS = {"fp32": ("fp32", "fp32"), "bf16": ("bf16", "fp32"), "bf16_store": ("bf16", "bf16")}      # mode -> (operands, storage)
    res = {"device": torch.cuda.get_device_name(0), "modes": {m: {"conv": {}, "call": {}, "step": {}} for m in modes}}
    nets = {m: (stand_in("vgg", dev, *OPS[m]), stand_in("alex", dev, *OPS[m])[0]) for m in modes}
    sizes = [(1280, 720), (1920, 1080)] if not a.quick else [(96, 64)]
    pools_before = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
    L = lib()
    for W, H in sizes:
        rows, total_ms, total_flop = {m: [] for m in modes}, dict.fromkeys(modes, 0.0), 0.0
        for li, (i, (co, ci, k)) in enumerate(zip(CONV_INDEX["vgg"], CONV_SHAPE["vgg"])):
            h, w = H >> pools_before[li], W >> pools_before[li]
            sd = nets["fp32"][0][1]
            x = torch.randn((ci, h, w), device=dev)
            wt, b = sd["features.%d.weight" % i].to(dev), sd["features.%d.bias" % i].to(dev)
            y = torch.empty((co, h, w), device=dev)
            xs, ys = torch.randn((ci, 1, 32), device=dev), torch.empty((co, 1, 32), device=dev)
            flop = 2.0 * ci * co * 9 * h * w
            total_flop += flop
            # blocked twins for the storage mode: layer 0 reads the fp32 scaled image in both storages
            xst = STORAGES["fp32" if li == 0 else "bf16"]
            xb, xsb = (x, xs) if li == 0 else (pack_blocked(x), pack_blocked(xs))
            yb, ysb = torch.empty((co + 7) // 8 * 16 * h * w, dtype=torch.uint8, device=dev), torch.empty((co + 7) // 8 * 16 * 32, dtype=torch.uint8, device=dev)
            f_all, f_pack, keep = {}, {}, []

            def conv_fn(op, xin, yout, hh, ww, scratch, n, xs_, ys_):
                if ys_ == STORAGES["fp32"]:
                    return lambda: check(L.mgr_lpips_conv_op(ci, co, hh, ww, 3, 3, 1, 1, ptr(xin), None, ptr(wt), ptr(b), 1, 0, ptr(yout),
                                                             ptr(scratch), n, stream(), op), "mgr_lpips_conv_op")
                return lambda: check(L.mgr_lpips_conv_st(ci, co, hh, ww, 3, 3, 1, 1, ptr(xin), None, ptr(wt), ptr(b), 1, 0, ptr(yout),
                                                         ptr(scratch), n, stream(), op, xs_, ys_), "mgr_lpips_conv_st")

            for m in modes:
                op = OPERANDS[OPS[m][0]]
                n = int(L.mgr_lpips_conv_scratch_bytes_op(ci, co, 3, 3, op))
                scratch = torch.empty(n, dtype=torch.uint8, device=dev)
                keep.append(scratch)
                if m == "bf16_store":
                    f_all[m] = conv_fn(op, xb, yb, h, w, scratch, n, xst, STORAGES["bf16"])
                    # the pack alone: the same call on a 1x32 image (one workgroup row of the convolution)
                    f_pack[m] = conv_fn(op, xsb, ysb, 1, 32, scratch, n, xst, STORAGES["bf16"])
                else:
                    f_all[m] = conv_fn(op, x, y, h, w, scratch, n, 0, 0)
                    f_pack[m] = conv_fn(op, xs, ys, 1, 32, scratch, n, 0, 0)
            ts_all, ts_pack = timed_alt(f_all, 3), timed_alt(f_pack, 3)
            for m in modes:
                t_all, t_pack = ts_all[m], ts_pack[m]
                ms = t_all["median_ms"] - t_pack["median_ms"]
                row = dict(layer=i, cin=ci, cout=co, h=h, w=w, ms=ms, ms_with_pack=t_all["median_ms"], min_ms=t_all["min_ms"],
                           max_ms=t_all["max_ms"], pack_ms=t_pack["median_ms"], tflops=flop / (ms * 1e9),
                           ratio_to_gemm=flop / (ms * 1e9) / GEMM_TF)
                rows[m].append(row)
                total_ms[m] += ms
                print("conv %s %dx%d" % (m, W, H), json.dumps(row), flush=True)
        pred, target = torch.rand((1, 3, H, W), device=dev), torch.rand((1, 3, H, W), device=dev)
        for m in modes:
            r = res["modes"][m]
            r["conv"]["%dx%d" % (W, H)] = dict(layers=rows[m], total_ms=total_ms[m], tflops=total_flop / (total_ms[m] * 1e9),
                                               ratio_to_gemm=total_flop / (total_ms[m] * 1e9) / GEMM_TF)
            print("conv %s %dx%d total" % (m, W, H), total_ms[m], "ms", total_flop / (total_ms[m] * 1e9), "TF/s", flush=True)
        for key, call in (("vgg_forward", lambda n_: n_[0][0].values_grad(pred, target, need_grad=False)),
                          ("vgg_value_and_gradient", lambda n_: n_[0][0].values_grad(pred, target, need_grad=True)),
                          ("alex_forward", lambda n_: n_[1].values_grad(pred, target, need_grad=False))):
            ts = timed_alt({m: (lambda m=m: call(nets[m])) for m in modes}, 2)
            for m in modes:
                res["modes"][m]["call"]["%s %dx%d" % (key, W, H)] = ts[m]
                print("call %s %s %dx%d" % (m, key, W, H), json.dumps(ts[m]), flush=True)
        for m in modes:
            st = STORAGES[OPS[m][1]]
            res["modes"][m]["call"]["workspace_bytes %dx%d" % (W, H)] = int(L.mgr_lpips_workspace_bytes_st(0, H, W, 1, st))
            res["modes"][m]["call"]["workspace_taps_bytes %dx%d" % (W, H)] = int(L.mgr_lpips_taps_bytes_st(0, H, W, st))
            print("bytes %s %dx%d workspace %d taps %d" % (m, W, H, res["modes"][m]["call"]["workspace_bytes %dx%d" % (W, H)],
                                                           res["modes"][m]["call"]["workspace_taps_bytes %dx%d" % (W, H)]), flush=True)

    if not a.no_step:
        from manus_amd import rasterizer as rz
        from manus_amd.engine import HipViewCompute
        from manus_amd.synthetic import camera_table, make_scene
        V, N, W, H = (8, 300000, 1920, 1080) if not a.quick else (3, 5000, 96, 64)
        scene = make_scene(n_gaussians=N, kind="hand", seed=0, n_cameras=V, width=W, height=H, device=dev,
                           **({} if not a.quick else dict(grid_res=24, cam_radius=0.5, sigma_range=(2e-3, 8e-3))))
        ct = camera_table(scene["cameras"], dev)
        g = torch.Generator(device="cpu").manual_seed(123)
        pert = dict(scene)
        pert["params"] = {k: (v + 0.01 * v.abs().mean() * torch.randn(v.shape, generator=g).to(dev)) for k, v in scene["params"].items()}
        ids = list(range(V))
        with torch.no_grad():
            hp = HipViewCompute(pert, torch.zeros((V, 3, H, W), device=dev), ct)
            targets = hp.forward_views_fused(ids)[0].contiguous().clone()
            del hp
        rz.context(dev).clear()
        off = HipViewCompute(scene, targets, ct, loss="l1+ssim")
        for m in modes:
            steps = {"off": off, "on": HipViewCompute(scene, targets, ct, loss="l1+ssim", lpips=nets[m][0][0], w_lpips=0.1)}
            for key in ("off", "on", "off_again", "on_again"):
                hc = steps[key.replace("_again", "")]
                res["modes"][m]["step"][key] = timed(lambda: hc(ids, 1.0 / V), 20 if key.startswith("off") and not a.quick else 2)
                print("step %s %s" % (m, key), json.dumps(res["modes"][m]["step"][key]), flush=True)
    if len(modes) >= 2:
        f, h16 = res["modes"]["fp32"], res["modes"]["bf16"]
        res["speedup"] = {"conv": {sz: [dict(layer=a_["layer"], cin=a_["cin"], cout=a_["cout"], fp32_ms=a_["ms"], bf16_ms=b_["ms"],
                                             ratio=a_["ms"] / b_["ms"]) for a_, b_ in zip(f["conv"][sz]["layers"], h16["conv"][sz]["layers"])]
                                        for sz in f["conv"]},
                          "call": {k: f["call"][k]["median_ms"] / h16["call"][k]["median_ms"] for k in f["call"] if not k.startswith("workspace")},
                          "step": {k: f["step"][k]["median_ms"] / h16["step"][k]["median_ms"] for k in f["step"]}}
        print("speedup", json.dumps(res["speedup"]), flush=True)
    if "bf16_store" in modes:
        f, h16 = res["modes"]["bf16"], res["modes"]["bf16_store"]
        res["storage_speedup"] = {"conv": {sz: [dict(layer=a_["layer"], cin=a_["cin"], cout=a_["cout"], fp32_storage_ms=a_["ms"],
                                                     bf16_storage_ms=b_["ms"], ratio=a_["ms"] / b_["ms"])
                                                for a_, b_ in zip(f["conv"][sz]["layers"], h16["conv"][sz]["layers"])] for sz in f["conv"]},
                                  "call": {k: f["call"][k]["median_ms"] / h16["call"][k]["median_ms"] for k in f["call"]
                                           if not k.startswith("workspace")},
                                  "step": {k: f["step"][k]["median_ms"] / h16["step"][k]["median_ms"] for k in f["step"]}}
        print("storage_speedup", json.dumps(res["storage_speedup"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

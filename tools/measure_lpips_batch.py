#!/usr/bin/env python3
"""Time a step's equal-size LPIPS windows as one batched call (mgr_lpips_roi_batch_op, mgr_lpips_roi_taps_batch_op;
`LPIPS.values_grad(rects=, batch=)`, `LPIPS.target_taps(batch=)`, `HipViewCompute(lpips_batch=)`) beside the sequential call.

    python tools/measure_lpips_batch.py [--out FILE.json] [--quick] [--no-step] [--views 8] [--batch 8] [--storage bf16] [--modes bf16,bf16_store]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats); the
sequential and the batched call ALTERNATE sample by sample, so that both see the same box.  Stand-in weights as
tools/measure_lpips.py.  Per operand mode (fp32, then bf16), VGG, V = 8 views of 1920x1080 with equal windows of 256^2, 512^2,
768^2 (each view at its own offset) and the full frame given as a rectangle:
  * value and gradient without and with the target's cached taps, batch 0 against 8; the workspace bytes of both;
  * the taps build alone, batch 0 against 8;
  * the outputs of the two calls compared bit for bit at the sizes timed ("equal");
  * the bench step (bench.py's scene: 300k hand Gaussians, 8 views of 1920x1080, loss l1+ssim) on such rects, without and with
    `lpips_cache_targets`, `lpips_batch` 0 against 8.
With --storage bf16 a third mode, "bf16_store" (bf16 operands, bf16 channel-blocked storage: the mgr_lpips*_st entries), gets
every row, its workspace and taps bytes from the _st queries, and a "storage" table times the batched calls of "bf16" and
"bf16_store" against each other, the two alternating sample by sample.  --modes restricts the run to some of the modes.
No speed-up is fixed in advance.  One condition is checked and reported under "conditions" (exit status 1 when it fails): at
256^2 and 512^2 every batched row is faster than the sequential row of the same run.  The 768^2 and full-frame rows carry no
condition.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from measure_lpips import stand_in  # noqa: E402


def timed_pair(fns, repeats, samples=5):
    """{name: median / min / max ms} of the named calls, their samples alternating."""
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


def spread(V, side_w, side_h, W, H):
    """V windows of one size, every view at its own offset inside the frame."""
    w, h = min(side_w, W), min(side_h, H)
    return [((v * 97) % (W - w + 1), (v * 61) % (H - h + 1), w, h) for v in range(V)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--no-step", action="store_true", help="skip the bench step")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--storage", default="fp32", choices=("fp32", "bf16"), help="bf16: a third mode, bf16 operands with bf16 storage")
    ap.add_argument("--modes", default=None, help="comma-separated subset of fp32,bf16,bf16_store to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_lpips_batch.py needs a GPU"
    import ctypes
    from manus_amd._lib import lib
    from manus_amd.lpips import STORAGES
    dev = "cuda:0"
    OPS = {"fp32": ("fp32", "fp32"), "bf16": ("bf16", "fp32"), "bf16_store": ("bf16", "bf16")}      # mode -> (operands, storage)
    modes = ("fp32", "bf16") + (("bf16_store",) if a.storage == "bf16" else ())
    if a.modes:
        assert all(m in modes for m in a.modes.split(",")), "--modes: a subset of %s" % (modes,)
        modes = tuple(m for m in modes if m in a.modes.split(","))
    V, B = a.views, a.batch
    W, H = (1920, 1080) if not a.quick else (96, 64)
    sides = (256, 512, 768) if not a.quick else (16, 32, 48)
    judged = ["%dx%d" % (s, s) for s in sides[:2]]
    windows = [("%dx%d" % (s, s), spread(V, s, s, W, H)) for s in sides] + [("frame", [(0, 0, W, H)] * V)]
    res = {"device": torch.cuda.get_device_name(0), "frame": [W, H], "views": V, "batch": B,
           "modes": {m: {"call": {}, "taps": {}, "bytes": {}, "equal": {}, "step": {}} for m in modes}, "conditions": {}}
    nets = {m: stand_in("vgg", dev, *OPS[m])[0] for m in modes}
    L = lib()
    g = torch.Generator().manual_seed(5)
    pred, target = torch.rand((V, 3, H, W), generator=g).to(dev), torch.rand((V, 3, H, W), generator=g).to(dev)
    grad = torch.empty_like(pred)
    ok = True
    for m in modes:
        vgg, r = nets[m], res["modes"][m]
        cond = {}
        for name, rects in windows:
            area = rects[0][2] * rects[0][3]
            reps = max(1, min(8, (W * H) // (8 * area))) * (1 if m == "fp32" else 2)
            vgg._ws = None          # (the kept workspace of the last window is dropped before the next one's is made)
            ra = np.ascontiguousarray(np.asarray(rects, np.int32))
            rp = ra.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
            st = STORAGES[OPS[m][1]]
            r["bytes"][name] = dict(sequential=int(L.mgr_lpips_roi_batch_workspace_bytes_st(0, V, rp, 1, 1, st)),
                                    batched=int(L.mgr_lpips_roi_batch_workspace_bytes_st(0, V, rp, 1, B, st)),
                                    taps=V * int(L.mgr_lpips_taps_bytes_st(0, rects[0][3], rects[0][2], st)))
            # the same bits at the sizes timed
            v0, g0 = vgg.values_grad(pred, target, need_grad=True, rects=rects)
            v0, g0 = v0.clone(), g0.clone()
            v1, g1 = vgg.values_grad(pred, target, need_grad=True, rects=rects, batch=B)
            r["equal"][name] = bool(torch.equal(v0, v1) and torch.equal(g0, g1))
            del v0, g0, v1, g1
            taps = vgg.target_taps(target, rects, batch=B)
            rows = {"": dict(sequential=lambda: vgg.values_grad(pred, target, need_grad=True, out_grad=grad, rects=rects),
                             batched=lambda: vgg.values_grad(pred, target, need_grad=True, out_grad=grad, rects=rects, batch=B)),
                    " cached taps": dict(sequential=lambda: vgg.values_grad(pred, None, need_grad=True, out_grad=grad, rects=rects, target_taps=taps),
                                         batched=lambda: vgg.values_grad(pred, None, need_grad=True, out_grad=grad, rects=rects, target_taps=taps,
                                                                         batch=B))}
            for suffix, fns in rows.items():
                t = r["call"][name + suffix] = timed_pair(fns, reps)
                print("call %s %s%s" % (m, name, suffix), json.dumps(t), flush=True)
                if name in judged:
                    cond[name + suffix + ": batched faster"] = t["batched"]["median_ms"] < t["sequential"]["median_ms"]
            del taps
            t = r["taps"][name] = timed_pair(dict(sequential=lambda: vgg.target_taps(target, rects),
                                                  batched=lambda: vgg.target_taps(target, rects, batch=B)), reps)
            print("taps %s %s" % (m, name), json.dumps(t), flush=True)
            if name in judged:
                cond[name + " taps build: batched faster"] = t["batched"]["median_ms"] < t["sequential"]["median_ms"]
            vgg._ws = None
            torch.cuda.empty_cache()
        res["conditions"][m] = cond
        ok = ok and all(cond.values()) and all(r["equal"].values())
        print("equal %s" % m, json.dumps(r["equal"]), flush=True)
        print("bytes %s" % m, json.dumps(r["bytes"]), flush=True)
        print("conditions %s" % m, json.dumps(cond), flush=True)

    if "bf16" in modes and "bf16_store" in modes:
        # the two storages of bf16 operands against each other, batched, alternating
        res["storage"] = {}
        for name, rects in windows:
            area = rects[0][2] * rects[0][3]
            reps = 2 * max(1, min(8, (W * H) // (8 * area)))
            taps = {m: nets[m].target_taps(target, rects, batch=B) for m in ("bf16", "bf16_store")}
            for suffix, cached in (("", False), (" cached taps", True)):
                fns = {m: (lambda m=m: nets[m].values_grad(pred, None if cached else target, need_grad=True, out_grad=grad, rects=rects,
                                                           target_taps=taps[m] if cached else None, batch=B)) for m in ("bf16", "bf16_store")}
                t = res["storage"][name + suffix] = timed_pair(fns, reps)
                t["ratio"] = t["bf16"]["median_ms"] / t["bf16_store"]["median_ms"]
                print("storage %s%s" % (name, suffix), json.dumps(t), flush=True)
            del taps
            for m in ("bf16", "bf16_store"):
                nets[m]._ws = None
            torch.cuda.empty_cache()

    if not a.no_step:
        from manus_amd import rasterizer as rz
        from manus_amd.engine import HipViewCompute
        from manus_amd.synthetic import camera_table, make_scene
        N = 300000 if not a.quick else 5000
        scene = make_scene(n_gaussians=N, kind="hand", seed=0, n_cameras=V, width=W, height=H, device=dev,
                           **({} if not a.quick else dict(grid_res=24, cam_radius=0.5, sigma_range=(2e-3, 8e-3))))
        ct = camera_table(scene["cameras"], dev)
        g = torch.Generator(device="cpu").manual_seed(123)
        pert = dict(scene)
        pert["params"] = {k: (v + 0.01 * v.abs().mean() * torch.randn(v.shape, generator=g).to(dev)) for k, v in scene["params"].items()}
        ids = list(range(V))
        del pred, target, grad
        with torch.no_grad():
            hp = HipViewCompute(pert, torch.zeros((V, 3, H, W), device=dev), ct)
            targets = hp.forward_views_fused(ids)[0].contiguous().clone()
            del hp
        rz.context(dev).clear()
        for m in modes:
            st, cond = res["modes"][m]["step"], res["conditions"][m]
            seq = HipViewCompute(scene, targets, ct, loss="l1+ssim", lpips=nets[m], w_lpips=0.1)
            bat = HipViewCompute(scene, targets, ct, loss="l1+ssim", lpips=nets[m], w_lpips=0.1, lpips_batch=B)
            for name, rects in windows:
                for cache in (False, True):
                    for hc in (seq, bat):
                        hc.lpips_rects, hc.lpips_cache_targets = rects, cache
                    key = name + (" cached taps" if cache else "")
                    st[key] = timed_pair(dict(sequential=lambda: seq(ids, 1.0 / V), batched=lambda: bat(ids, 1.0 / V)), 2)
                    print("step %s %s" % (m, key), json.dumps(st[key]), flush=True)
                    if name in judged:
                        cond["step " + key + ": batched faster"] = st[key]["batched"]["median_ms"] < st[key]["sequential"]["median_ms"]
            for hc in (seq, bat):
                hc.lpips_rects, hc.lpips_cache_targets = None, False
                hc._drop_view_constants()
            del seq, bat
            nets[m]._ws = None
            torch.cuda.empty_cache()
            ok = ok and all(cond.values())
            print("conditions %s" % m, json.dumps(cond), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not ok:
        print("a condition failed", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()

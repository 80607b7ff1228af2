#!/usr/bin/env python3
"""Time the windowed LPIPS term (mgr_lpips_roi_op, `LPIPS.values_grad(rects=)`, `LPIPS.target_taps`) beside the full-frame call.

    python tools/measure_lpips_roi.py [--out FILE.json] [--quick] [--no-step]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats); stand-in
weights as tools/measure_lpips.py.  Per operand mode (fp32, then bf16), VGG, one view of 1920x1080, value and gradient:
  * the plain full-frame call (twice: the second run gives the run-to-run spread);
  * the windowed call on a centred 256^2, 512^2 and 768^2 rectangle and on the full frame given as a rectangle, each without
    and with the target's cached taps; workspace and taps bytes of each;
  * the bench step (bench.py's scene: 300k hand Gaussians, 8 views of 1920x1080, loss l1+ssim) with the term off, on
    full-frame, and on with rects of those sizes, without and with `lpips_cache_targets`.
No ratio is fixed in advance.  Two conditions are checked and reported under "conditions" (exit status 1 when one fails):
every window smaller than the frame, and every cached-taps call, is faster than the full-frame call of the same run; the
full-frame rectangle is within the run-to-run spread of the plain call (its min - max range meets that of the two plain runs).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from measure_feature_render import timed  # noqa: E402
from measure_lpips import stand_in  # noqa: E402


def centred(side, W, H):
    w, h = min(side, W), min(side, H)
    return ((W - w) // 2, (H - h) // 2, w, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--no-step", action="store_true", help="skip the bench step")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_lpips_roi.py needs a GPU"
    from manus_amd._lib import lib
    dev = "cuda:0"
    modes = ("fp32", "bf16")
    W, H = (1920, 1080) if not a.quick else (96, 64)
    sides = (256, 512, 768) if not a.quick else (16, 32, 48)
    windows = [("%dx%d" % (s, s), centred(s, W, H)) for s in sides] + [("frame", (0, 0, W, H))]
    res = {"device": torch.cuda.get_device_name(0), "frame": [W, H], "modes": {m: {"call": {}, "bytes": {}, "step": {}} for m in modes},
           "conditions": {}}
    nets = {m: stand_in("vgg", dev, m)[0] for m in modes}
    L = lib()
    pred, target = torch.rand((1, 3, H, W), device=dev), torch.rand((1, 3, H, W), device=dev)
    grad = torch.empty_like(pred)
    ok = True
    for m in modes:
        vgg, r = nets[m], res["modes"][m]

        def row(key, fn, repeats):
            r["call"][key] = timed(fn, repeats)
            print("call %s %s" % (m, key), json.dumps(r["call"][key]), flush=True)
            return r["call"][key]

        reps = 2 if m == "fp32" else 4
        plain = row("plain", lambda: vgg.values_grad(pred, target, need_grad=True, out_grad=grad), reps)
        r["bytes"]["plain"] = dict(workspace=int(L.mgr_lpips_workspace_bytes(0, H, W, 1)), taps=0)
        for name, rect in windows:
            taps = vgg.target_taps(target, [rect])
            r["bytes"][name] = dict(workspace=int(L.mgr_lpips_workspace_bytes(0, rect[3], rect[2], 1)), taps=taps.nbytes)
            n = reps * max(1, min(16, (W * H) // (4 * rect[2] * rect[3])))
            row(name, lambda: vgg.values_grad(pred, target, need_grad=True, out_grad=grad, rects=[rect]), n)
            row(name + " cached taps", lambda: vgg.values_grad(pred, None, need_grad=True, out_grad=grad, rects=[rect], target_taps=taps), n)
            del taps
        again = row("plain again", lambda: vgg.values_grad(pred, target, need_grad=True, out_grad=grad), reps)
        full = max(plain["median_ms"], again["median_ms"])
        cond = {}
        for name, _ in windows:
            if name != "frame":
                cond[name + " faster than the frame"] = r["call"][name]["median_ms"] < full
            cond[name + " cached taps faster than the frame"] = r["call"][name + " cached taps"]["median_ms"] < full
        lo, hi = min(plain["min_ms"], again["min_ms"]), max(plain["max_ms"], again["max_ms"])
        fr = r["call"]["frame"]
        cond["frame rectangle within the plain call's spread"] = fr["min_ms"] <= hi and fr["max_ms"] >= lo
        res["conditions"][m] = cond
        ok = ok and all(cond.values())
        print("conditions %s" % m, json.dumps(cond), flush=True)

    if not a.no_step:
        from manus_amd import rasterizer as rz
        from manus_amd.engine import HipViewCompute
        from manus_amd.synthetic import camera_table, make_scene
        V, N = (8, 300000) if not a.quick else (3, 5000)
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
            st = res["modes"][m]["step"]
            st["off"] = timed(lambda: off(ids, 1.0 / V), 20 if not a.quick else 2)
            print("step %s off" % m, json.dumps(st["off"]), flush=True)
            hc = HipViewCompute(scene, targets, ct, loss="l1+ssim", lpips=nets[m], w_lpips=0.1)
            for name, rect in [("plain", None)] + windows:
                for cache in (False, True) if rect is not None else (False,):
                    hc.lpips_rects, hc.lpips_cache_targets = (None if rect is None else [rect] * V), cache
                    key = name + (" cached taps" if cache else "")
                    st[key] = timed(lambda: hc(ids, 1.0 / V), 2)
                    print("step %s %s" % (m, key), json.dumps(st[key]), flush=True)
            hc.lpips_rects, hc.lpips_cache_targets = None, False
            hc._drop_view_constants()
            del hc
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not ok:
        print("a condition failed", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the per-camera exposure of the fused step (HipViewCompute(exposure=...)).

    python tools/measure_exposure.py [--out FILE.json] [--quick]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats), on the bench
step (bench.py's scene and targets: 300k hand Gaussians, 8 views of 1920x1080, loss l1+ssim, targets = the model perturbed by
1 %):
  * the step with exposure off (today's step: the span list of the sparse loss), the same step with sparse_loss=False alone
    (what the correction forgoes), and the step with exposure on (a table of I + 0.15 N(0,1), b ~ 0.05 N(0,1)), alternated;
  * the three entries alone with their achieved GB/s: mgr_exposure_apply (24 B per pixel: 3 floats read, 3 written),
    mgr_exposure_backward in place (36 B per pixel: 6 floats read, 3 written; its fold kernel included) and
    mgr_exposure_adam.  The images of 8 views of 1080p are 199 MB each: more than the last-level cache holds, so the rates
    are memory rates;
  * the kernels' own times from the library's HIP-event profile.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from measure_feature_render import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_exposure.py needs a GPU"
    from manus_amd import _lib, ops, rasterizer as rz
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table, make_scene
    dev = "cuda:0"
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
    E = torch.zeros((V, 3, 4), device=dev)
    E[:, :, :3] = torch.eye(3, device=dev) + 0.15 * torch.randn((V, 3, 3), generator=g).to(dev)
    E[:, :, 3] = 0.05 * torch.randn((V, 3), generator=g).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "sizes": dict(V=V, N=N, W=W, H=H), "step": {}, "calls": {}, "kernels": {}}
    steps = {"off": HipViewCompute(scene, targets, ct, loss="l1+ssim"),
             "dense": HipViewCompute(scene, targets, ct, loss="l1+ssim", sparse_loss=False),
             "exposure": HipViewCompute(scene, targets, ct, loss="l1+ssim", exposure=E)}
    rep = 20 if not a.quick else 3
    for key in ("off", "dense", "exposure", "off_again", "dense_again", "exposure_again"):
        hc = steps[key.replace("_again", "")]
        res["step"][key] = timed(lambda: hc(ids, 1.0 / V), rep)
        print("step %s" % key, json.dumps(res["step"][key]), flush=True)
    off, dense, on = (min(res["step"][k]["median_ms"], res["step"][k + "_again"]["median_ms"]) for k in ("off", "dense", "exposure"))
    res["step"]["increase_ms"] = dict(total=on - off, dense_loss=dense - off, exposure_kernels=on - dense)
    print("increase", json.dumps(res["step"]["increase_ms"]), flush=True)

    # the three entries alone, on images of the step's size
    img = steps["exposure"].last_image.clone()
    grad = torch.randn((V, 3, H, W), generator=g).to(dev) / float(H * W)
    out = torch.empty_like(img)
    dE = torch.empty((V, 3, 4), device=dev)
    cov = torch.arange(V, dtype=torch.int32, device=dev)
    L = lib()
    nbytes = int(L.mgr_exposure_workspace_bytes(V, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tab, m, v = E.clone(), torch.zeros_like(E), torch.zeros_like(E)
    px = float(V * H * W)
    calls = (("apply", 24.0 * px, lambda: check(L.mgr_exposure_apply(V, H, W, V, ptr(cov), ptr(E), ptr(img), ptr(out), stream()), "mgr_exposure_apply")),
             ("backward_in_place", 36.0 * px, lambda: check(L.mgr_exposure_backward(V, H, W, V, ptr(cov), ptr(E), ptr(img), ptr(grad), ptr(grad), ptr(dE),
                                                                                    ptr(ws), nbytes, stream()), "mgr_exposure_backward")),
             ("adam", None, lambda: check(L.mgr_exposure_adam(V, V, ptr(cov), V, ptr(cov), ptr(dE), ptr(tab), ptr(m), ptr(v), 0.01, 0.9, 0.999, 1e-8, 1,
                                                              stream()), "mgr_exposure_adam")))
    res["calls"]["workspace_bytes"] = nbytes
    res["calls"]["block"] = ops.exposure_block()
    for key, moved, fn in calls:
        t = timed(fn, 20 if not a.quick else 2)
        if moved is not None:
            t["bytes"] = moved
            t["GBps"] = moved / (t["median_ms"] * 1e-3) / 1e9
        res["calls"][key] = t
        print("call %s" % key, json.dumps(t), flush=True)

    # the kernels' own times (HIP events around every launch of the library)
    for key in ("dense", "exposure"):
        _lib.profile_enable(True)
        _lib.profile_report()
        for _ in range(5):
            steps[key](ids, 1.0 / V)
        rp = _lib.profile_report()
        _lib.profile_enable(False)
        res["kernels"][key] = {k: dict(launches=c, mean_ms=ms / max(c, 1)) for k, (c, ms) in rp.items()
                               if k.startswith("k_exposure") or k.startswith("k_image_loss") or k in ("k_blend_bwd", "k_blend_fwd")}
        print("kernels %s" % key, json.dumps(res["kernels"][key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

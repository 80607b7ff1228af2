#!/usr/bin/env python3
"""Time the pose gradient of the map terms on the fused step (HipViewCompute(mask_targets=..., w_mask=..., pose_grad=True)).

    python tools/measure_map_pose.py [--out FILE.json] [--quick]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats), on the bench
step (the scene, targets and mask targets of tools/measure_map_loss.py: 300k hand Gaussians, 8 views of 1920x1080, loss l1+ssim):
  * the step with the mask term on, pose_grad off and on, alternated (and with skin_grid_grad as well);
  * mgr_views_maps_backward and mgr_views_maps_backward_pose alone on the workspace of a step, alternated -- the figure to hold
    against DESIGN.md section 6, "Map supervision on the fused step" (each call includes its blocking read of the header);
  * the kernels' own times from the library's HIP-event profile (k_blend_feat_bwd, k_views_feat_gather,
    k_views_feat_gather_pose, k_pose_fold).
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
    assert torch.cuda.is_available(), "measure_map_pose.py needs a GPU"
    from manus_amd import _lib, rasterizer as rz
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
        mask = rz.blend_features(alpha=True, device=dev)["alpha"].clone()
        del hp
    rz.context(dev).clear()
    res = {"device": torch.cuda.get_device_name(0), "sizes": dict(V=V, N=N, W=W, H=H), "step": {}, "calls": {}, "kernels": {}}
    kw = dict(loss="l1+ssim", mask_targets=mask, w_mask=0.1)
    steps = {"mask": HipViewCompute(scene, targets, ct, **kw),
             "mask+pose": HipViewCompute(scene, targets, ct, pose_grad=True, **kw),
             "mask+pose+grid": HipViewCompute(scene, targets, ct, pose_grad=True, skin_grid_grad=True, **kw)}
    rep = 20 if not a.quick else 3
    for key in ("mask", "mask+pose", "mask_again", "mask+pose_again", "mask+pose+grid"):
        hc = steps[key.replace("_again", "")]
        res["step"][key] = timed(lambda: hc(ids, 1.0 / V), rep)
        print("step %s" % key, json.dumps(res["step"][key]), flush=True)

    # the two entries alone, on the workspace of a step of the "mask+pose" object
    hc = steps["mask+pose"]
    hc(ids, 1.0 / V)
    torch.cuda.synchronize()
    ws = rz.context(dev).last_ws
    mb = next(iter(hc._map_bufs.values()))
    p = {k: v.detach() for k, v in hc.params.items()}
    w, B = hc._skin_weights(p["_xyz"], hc.n_art)
    sel = hc._select(ids)
    outs = [torch.zeros(s, device=dev) for s in ((N, 3), (N, 3), (N, 4), (N, 1), (hc.n_art, B))]
    d_T = torch.zeros((V, B, 4, 4), device=dev)
    L = lib()
    pose_ws = torch.empty(int(L.mgr_views_maps_pose_workspace_bytes(V, N, B)), dtype=torch.uint8, device=dev)
    args = (V, N, B, hc.n_art, W, H, ptr(sel["cams"]), ptr(p["_xyz"]), ptr(p["_scaling"]), ptr(p["_rotation"]), ptr(p["_opacity"].reshape(-1)),
            ptr(w), ptr(sel["T"]), ptr(mb["alpha"]), None, ptr(mb["g_alpha"]), None, 1, *[ptr(t) for t in outs], ptr(ws.buf), ws.nbytes, ws.cap,
            ptr(mb["scratch"]), mb["scratch"].numel(), 0)
    plain = lambda: check(L.mgr_views_maps_backward(*args, stream()), "mgr_views_maps_backward")
    pose = lambda: check(L.mgr_views_maps_backward_pose(*args, 1, ptr(d_T), ptr(pose_ws), pose_ws.numel(), stream()), "mgr_views_maps_backward_pose")
    res["calls"]["pose_workspace_bytes"] = int(pose_ws.numel())
    for key, fn in (("maps_backward", plain), ("maps_backward_pose", pose), ("maps_backward_again", plain), ("maps_backward_pose_again", pose)):
        res["calls"][key] = timed(fn, 5 if not a.quick else 2)
        print("call %s" % key, json.dumps(res["calls"][key]), flush=True)

    # the kernels' own times (HIP events around every launch of the library)
    for key in ("mask", "mask+pose"):
        _lib.profile_enable(True)
        _lib.profile_report()
        for _ in range(5):
            steps[key](ids, 1.0 / V)
        rp = _lib.profile_report()
        _lib.profile_enable(False)
        res["kernels"][key] = {k: dict(launches=c, mean_ms=ms / max(c, 1)) for k, (c, ms) in rp.items()
                               if k in ("k_blend_feat_bwd", "k_views_feat_gather", "k_views_feat_gather_pose", "k_pose_fold", "k_inst_bwd_pose",
                                        "k_pose_part_views")}
        print("kernels %s" % key, json.dumps(res["kernels"][key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

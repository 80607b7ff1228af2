#!/usr/bin/env python3
"""Time the bench step (300 k Gaussians, 8 views, 1920x1080, hand scene, l1+ssim) with the pose gradient off and on.

    python tools/measure_pose_grad.py [--out FILE.json] [--quick]

One process, HIP events around a batch of steps, every shape warmed, median of 5 samples with min and max; the two settings
alternate (off, on, off again) so that a drift of the clocks shows.  Also prints the per-kernel HIP-event times of the
backward's per-instance kernel, the partial kernel and the fold with the gradient on, and -- as a check of the reduction at full
size, where a workgroup takes several chunks -- the identity  sum_v sum_b <dT[v][b][:3,:], T[v][b][:3,:]> = sum_n sum_b w_nb d_skin_w[n][b]
(both sides contract the same per-lane values).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, repeats, samples=5):
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / repeats)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_pose_grad.py needs a GPU"
    from manus_amd import _lib, ops, rasterizer
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table, make_scene
    dev = "cuda:0"
    N, V, W, H = (300000, 8, 1920, 1080) if not a.quick else (3000, 8, 96, 64)
    scene = make_scene(n_gaussians=N, kind="hand", seed=0, n_cameras=V, width=W, height=H, device=dev, cam_radius=1.2,
                       **({} if not a.quick else dict(grid_res=24, cam_radius=0.5, sigma_range=(2e-3, 8e-3))))
    ct = camera_table(scene["cameras"], dev)
    g = torch.Generator(device="cpu").manual_seed(123)      # targets as in bench.py: the scene perturbed by 1 %
    pert = dict(scene)
    pert["params"] = {k: (v + 0.01 * v.abs().mean() * torch.randn(v.shape, generator=g).to(dev)) for k, v in scene["params"].items()}
    ids = list(range(V))
    with torch.no_grad():
        targets = HipViewCompute(pert, torch.zeros((V, 3, H, W), device=dev), ct).forward_views_fused(ids)[0].contiguous()
    rasterizer.context(dev).clear()
    off = HipViewCompute(scene, targets, ct, loss="l1+ssim")
    on = HipViewCompute(scene, targets, ct, loss="l1+ssim", pose_grad=True)
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(N=N, V=V, W=W, H=H)}
    reps = 20
    for name, hc in (("off", off), ("on", on), ("off_again", off), ("on_again", on)):
        res[name] = timed(lambda: hc(ids, 1.0 / V), reps)
        print("step, pose_grad %-9s %s" % (name, json.dumps(res[name])), flush=True)
    # the two kernels behind the figure
    out = on(ids, 1.0 / V)
    _lib.profile_enable(True)
    for _ in range(10):
        on(ids, 1.0 / V)
    rep_on = _lib.profile_report()
    for _ in range(10):
        off(ids, 1.0 / V)
    rep_off = _lib.profile_report()
    _lib.profile_enable(False)
    res["kernels_ms"] = {"k_inst_bwd_pose": rep_on["k_inst_bwd_pose"][1] / rep_on["k_inst_bwd_pose"][0], "k_pose_fold": rep_on["k_pose_fold"][1] / rep_on["k_pose_fold"][0],
                         "k_pose_part_views": rep_on["k_pose_part_views"][1] / rep_on["k_pose_part_views"][0],
                         "k_inst_bwd": rep_off["k_inst_bwd"][1] / rep_off["k_inst_bwd"][0]}
    print("kernels (ms per launch):", json.dumps(res["kernels_ms"]), flush=True)
    # the identity, accumulated in fp64
    d_w = on._kept.tensors["_skin_w"].double()
    with torch.no_grad():
        w = ops.skin_weights(on.params["_xyz"].detach(), on.grid, scene["grid_center"], scene["grid_scale"]).double()
    lhs = float((out["d_transforms"].double()[:, :, :3, :] * scene["transforms"][ids].double()[:, :, :3, :]).sum())
    rhs = float((w * d_w).sum())
    res["identity"] = dict(lhs=lhs, rhs=rhs, rel=abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300), terms=float((w * d_w).abs().sum()))
    print("identity:", json.dumps(res["identity"]), flush=True)
    # the leaf gradients do not depend on the setting
    o_off, o_on = off(ids, 1.0 / V), on(ids, 1.0 / V)
    res["leaf_grads_bit_equal"] = all(torch.equal(o_off["grads"][k], o_on["grads"][k]) for k in o_off["grads"])
    print("leaf gradients bit-equal off / on:", res["leaf_grads_bit_equal"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

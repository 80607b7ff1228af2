#!/usr/bin/env python3
"""Time pose refinement on the bench step (300 k Gaussians, 8 views, 1920x1080, hand scene, l1+ssim, one frame per view):

    plain        the step alone, pose_grad off and on (no chain)
    host chain   the step with pose_grad on, driven by the host loop of tests/test_gpu_pose_grad.py::test_pose_recovery_end_to_end:
                 PoseCorrection.forward per view, bone_transforms, an in-place write of the table, pose_backward and an autograd
                 backward per view, torch.optim.Adam
    device chain the same step driven by pose.PoseRefiner (mgr_pose_apply, the step, mgr_pose_backward, mgr_pose_adam)
    entries      the three entries alone
    --prior      also: the device chain with the priors on (PoseRefiner(w_mag_*, w_smooth_*): mgr_pose_backward_prior in place of
                 mgr_pose_backward, the eight frames one take) beside the chain without, and the new entry alone

    python tools/measure_pose_refine.py [--out FILE.json] [--quick] [--prior]

One process, HIP events around a batch of steps (a step that waits for the host shows as a longer step), every shape warmed,
median of 5 samples with min and max; host and device chain alternate so that a drift of the clocks shows.  Needs a GPU; there
is no fallback."""
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
    ap.add_argument("--prior", action="store_true", help="also time the chain and the backward entry with the priors on")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_pose_refine.py needs a GPU"
    from manus_amd import rasterizer
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.engine import HipViewCompute
    from manus_amd.pose import PoseCorrection, PoseRefiner, pose_backward
    from manus_amd.synthetic import camera_table, make_scene
    from manus_amd.transforms import bone_transforms
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
    rest, posed = scene["rest"], scene["posed"]
    nb = rest.shape[0]
    off = HipViewCompute(scene, targets, ct, loss="l1+ssim")
    on = HipViewCompute(scene, targets, ct, loss="l1+ssim", pose_grad=True)
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(N=N, V=V, W=W, H=H, B=nb)}
    reps = 20

    corr = PoseCorrection(V, nb, device=dev)
    opt = torch.optim.Adam(corr.parameters(), lr=1e-4)

    def host_step():
        opt.zero_grad()
        corrected = [corr(posed[v], v) for v in ids]
        with torch.no_grad():
            scene["transforms"][ids] = torch.stack([bone_transforms(c, rest) for c in corrected])
        out = on(ids, 1.0 / V)
        for v in ids:
            corrected[v].backward(pose_backward(out["d_transforms"][v], corrected[v], rest))
        opt.step()

    ref = PoseRefiner([("capture", v) for v in ids], nb, rest, 1e-4, 1e-4, device=dev)

    def device_step():
        ref.apply(on, ids, ids)
        out = on(ids, 1.0 / V)
        ref.step(out["d_transforms"], ids, ids)

    weights = dict(w_mag_rot=1e-3, w_smooth_rot=1e-2, w_mag_trans=1e-3, w_smooth_trans=1e-2)
    ref_p = PoseRefiner([("capture", v) for v in ids], nb, rest, 1e-4, 1e-4, device=dev, **weights)

    def device_step_prior():
        ref_p.apply(on, ids, ids)
        out = on(ids, 1.0 / V)
        ref_p.step(out["d_transforms"], ids, ids)

    runs = [("plain_pose_grad_off", lambda: off(ids, 1.0 / V)), ("plain_pose_grad_on", lambda: on(ids, 1.0 / V)),
            ("host_chain", host_step), ("device_chain", device_step), ("host_chain_again", host_step),
            ("device_chain_again", device_step), ("plain_pose_grad_off_again", lambda: off(ids, 1.0 / V))]
    if a.prior:      # off and on alternate, so that a drift of the clocks shows
        runs += [("device_chain_prior", device_step_prior), ("device_chain_off", device_step),
                 ("device_chain_prior_again", device_step_prior), ("device_chain_off_again", device_step)]
    for name, fn in runs:
        res[name] = timed(fn, reps)
        print("%-26s %s" % (name, json.dumps(res[name])), flush=True)

    # the three entries alone, on the tables of the last step
    out = on(ids, 1.0 / V)
    d_T = out["d_transforms"].clone()
    rows, fov, listed_t, listed = ref._device_lists(ids, ids)[:4]
    U, F = len(listed), ref.n_frames
    g_r, g_t = torch.zeros((U, nb, 3), device=dev), torch.zeros((U, nb, 3), device=dev)
    gathered = on.gathered_transforms(ids)
    L = lib()
    entries = {
        "mgr_pose_apply": lambda: check(L.mgr_pose_apply(V, nb, F, ptr(rows), ptr(fov), ptr(posed), ptr(ref.rest), ptr(ref.rotvec), ptr(ref.trans),
                                                         ptr(scene["transforms"]), ptr(gathered), stream()), "mgr_pose_apply"),
        "mgr_pose_backward": lambda: check(L.mgr_pose_backward(V, nb, F, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(posed), ptr(ref.rest),
                                                               ptr(ref.rotvec), ptr(ref.trans), ptr(d_T), ptr(g_r), ptr(g_t), stream()),
                                           "mgr_pose_backward"),
        "mgr_pose_adam": lambda: check(L.mgr_pose_adam(U, nb, ptr(listed_t), ptr(g_r), ptr(g_t), ptr(ref.rotvec), ptr(ref.trans), ptr(ref.m_r),
                                                       ptr(ref.v_r), ptr(ref.m_t), ptr(ref.v_t), 1e-4, 1e-4, 0.9, 0.999, 1e-8, ref.steps + 1, stream()),
                                       "mgr_pose_adam"),
    }
    if a.prior:
        value = torch.zeros((), dtype=torch.float64, device=dev)
        ws = torch.empty(max(int(L.mgr_pose_prior_workspace_bytes(U, nb)), 8), dtype=torch.uint8, device=dev)
        w = [weights[k] for k in ("w_mag_rot", "w_smooth_rot", "w_mag_trans", "w_smooth_trans")]
        entries["mgr_pose_backward_prior"] = lambda: check(
            L.mgr_pose_backward_prior(V, nb, F, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(posed), ptr(ref.rest), ptr(ref.rotvec), ptr(ref.trans),
                                      ptr(d_T), ptr(g_r), ptr(g_t), ptr(ref_p.neighbours), *w, ptr(value), ptr(ws), ws.numel(), stream()),
            "mgr_pose_backward_prior")
        entries["mgr_pose_backward_again"] = entries["mgr_pose_backward"]
    for name, fn in entries.items():
        res[name] = timed(fn, 200)
        print("%-26s %s" % (name, json.dumps(res[name])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time kinematic pose refinement on the bench step (300 k Gaussians, 8 views, 1920x1080, hand scene, l1+ssim, one frame per
view, 20 bones in five chains of four, the hand's 23 free angles plus the global rotation and translation):

    plain        the step alone, pose_grad off and on (no chain)
    host chain   the step with pose_grad on, driven by host torch on the device: `transforms.euler_angles_to_armature_space`
                 (the tree loop with a `linalg.inv` per bone), `base` in front and inv(rest) behind, an in-place write of the table,
                 an autograd backward, the mask, torch.optim.Adam and the clamp to the joint limits
    device chain the same step driven by pose.KinematicPoseRefiner (mgr_fk_apply, the step, mgr_fk_backward, mgr_fk_adam)
    entries      the three entries alone

    python tools/measure_fk_refine.py [--out FILE.json] [--quick]

One process, HIP events around a batch of steps (a step that waits for the host shows as a longer step), every shape warmed,
median of 5 samples with min and max; host and device chain alternate so that a drift of the clocks shows.  Needs a GPU; there
is no fallback."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from measure_pose_refine import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_fk_refine.py needs a GPU"
    from manus_amd import rasterizer
    from manus_amd import transforms as T
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.engine import HipViewCompute
    from manus_amd.pose import KinematicPoseRefiner, dof_mask, joint_limits
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
    rest, posed = scene["rest"], scene["posed"]
    J = rest.shape[0]
    assert J == 20, "the hand scene has 20 bones"
    names = ["bone_%d" % i for i in range(J)]
    parents = [-1 if i % 4 == 0 else i - 1 for i in range(J)]
    kintree = {str(i): p for i, p in enumerate(parents)}
    mask, (lo, hi) = dof_mask(names, True, True), joint_limits(names)
    off = HipViewCompute(scene, targets, ct, loss="l1+ssim")
    on = HipViewCompute(scene, targets, ct, loss="l1+ssim", pose_grad=True)
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(N=N, V=V, W=W, H=H, J=J, free=int(mask.sum()))}
    reps = 20

    # the angles start at zero (FK gives the rest pose) with base aligning the first root to the scene's posed matrices: the
    # images differ from the targets more than a capture's would, which the time of a step does not see
    ref = KinematicPoseRefiner([("capture", v) for v in ids], rest, parents, torch.zeros((V, J + 2, 3)), 1e-4, 1e-4, mask=mask,
                               limits=(lo, hi), device=dev)
    ref.fit_base(posed[ids])

    theta = torch.zeros((V, J + 2, 3), device=dev, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=1e-4)
    base_d, mask_d, lo_d, hi_d = ref.base.clone(), mask.to(dev), lo.to(dev), hi.to(dev)
    inv_rest = torch.linalg.inv(rest)
    eye = torch.eye(4, device=dev).expand(V, 1, 4, 4)

    def host_step():
        opt.zero_grad()
        M = base_d[:, None] @ T.euler_angles_to_armature_space(theta[:, :J + 1], kintree, rest, theta[:, J + 1])
        Tm = torch.cat([M @ inv_rest, eye], 1)
        with torch.no_grad():
            scene["transforms"][ids] = Tm
        out = on(ids, 1.0 / V)
        Tm.backward(out["d_transforms"])
        theta.grad.mul_(mask_d)
        opt.step()
        with torch.no_grad():
            theta.copy_(torch.where(mask_d != 0, torch.minimum(torch.maximum(theta, lo_d), hi_d), theta))

    def device_step():
        ref.apply(on, ids, ids)
        out = on(ids, 1.0 / V)
        ref.step(out["d_transforms"], ids, ids)

    runs = [("plain_pose_grad_off", lambda: off(ids, 1.0 / V)), ("plain_pose_grad_on", lambda: on(ids, 1.0 / V)),
            ("host_chain", host_step), ("device_chain", device_step), ("host_chain_again", host_step),
            ("device_chain_again", device_step), ("plain_pose_grad_off_again", lambda: off(ids, 1.0 / V))]
    for name, fn in runs:
        res[name] = timed(fn, reps)
        print("%-26s %s" % (name, json.dumps(res[name])), flush=True)

    # the three entries alone, on the tables of the last step
    out = on(ids, 1.0 / V)
    d_T = out["d_transforms"].clone()
    rows, fov, listed_t, listed = ref._device_lists(ids, ids)[:4]
    U, F = len(listed), ref.n_frames
    d_theta = torch.zeros((U, J + 2, 3), device=dev)
    gathered = on.gathered_transforms(ids)
    L = lib()
    entries = {
        "mgr_fk_apply": lambda: check(L.mgr_fk_apply(V, J, F, ptr(rows), ptr(fov), ptr(posed), ptr(ref.rest), ptr(ref.local), ptr(ref.parents),
                                                     ptr(ref.base), ptr(ref.theta), ptr(scene["transforms"]), ptr(gathered), None, stream()),
                                      "mgr_fk_apply"),
        "mgr_fk_backward": lambda: check(L.mgr_fk_backward(V, J, F, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(ref.rest), ptr(ref.local),
                                                           ptr(ref.parents), ptr(ref.base), ptr(ref.theta), ptr(ref.mask), ptr(d_T), ptr(d_theta),
                                                           stream()), "mgr_fk_backward"),
        "mgr_fk_adam": lambda: check(L.mgr_fk_adam(U, J, ptr(listed_t), ptr(d_theta), ptr(ref.theta), ptr(ref.m), ptr(ref.v), ptr(ref.mask),
                                                   ptr(ref.lo), ptr(ref.hi), 1e-4, 1e-4, 0.9, 0.999, 1e-8, ref.steps + 1, stream()), "mgr_fk_adam"),
    }
    for name, fn in entries.items():
        res[name] = timed(fn, 200)
        print("%-26s %s" % (name, json.dumps(res[name])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

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
    python tools/measure_fk_refine.py --terms [--out FILE.json]      the backward entry with the terms on the angles (deviation,
                 smoothness, keypoints) against the plain one, and `fit_keypoints` against a host torch loop; renders nothing

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


def terms_main(a):
    """--terms: the backward entry with the terms on the angles (mgr_fk_backward_terms: deviation, smoothness, 21 keypoints) against
    the plain mgr_fk_backward on the same tables -- 8 listed frames of the 20-bone hand, 8 views, a random dL/dT --, and
    `KinematicPoseRefiner.fit_keypoints(100)` against the same 100 Adam steps as host torch on the device (autograd through
    `transforms.euler_angles_to_armature_space`, torch.optim.Adam).  No scene is rendered."""
    from manus_amd import transforms as T
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.pose import KinematicPoseRefiner, dof_mask
    dev = "cuda:0"
    V = F = 8
    J, parents = 20, [-1 if i % 4 == 0 else i - 1 for i in range(20)]
    g = torch.Generator().manual_seed(5)
    rest = torch.eye(4).repeat(J, 1, 1)
    rest[:, :3, :3] = T.euler_angles_to_matrix(torch.randn((J, 3), generator=g), "XYZ")
    rest[:, :3, 3] = 0.05 * torch.randn((J, 3), generator=g)
    mask = dof_mask(["bone_%d" % i for i in range(J)], True, True)
    bones = [0] + list(range(J))
    K = len(bones)
    off = 0.03 * torch.randn((K, 3), generator=g)
    ref = KinematicPoseRefiner([("capture", f) for f in range(F)], rest, parents, 0.3 * mask * torch.randn((F, J + 2, 3), generator=g), 0.02,
                               0.002, mask=mask, device=dev, w_dev_rot=0.5, w_smooth_rot=0.25, w_dev_trans=2.0, w_smooth_trans=1.0, w_kp=10.0)
    target = 0.1 * torch.randn((F, K, 3), generator=g)
    ref.set_keypoints(bones, off, target)
    ids = list(range(V))
    rows, fov, listed_t, listed = ref._device_lists(ids, ids)[:4]
    U = len(listed)
    d_T = torch.randn((V, J + 1, 4, 4), generator=g).to(dev)
    d_theta = torch.zeros((U, J + 2, 3), device=dev)
    values = torch.zeros(4, dtype=torch.float64, device=dev)
    L = lib()
    ws = torch.empty(int(L.mgr_fk_terms_workspace_bytes(U, J, K)), dtype=torch.uint8, device=dev)
    kp = ref.kp

    def terms(weights, w_kp, chain=True):
        check(L.mgr_fk_backward_terms(V if chain else 0, J, F, U, ptr(listed_t), ptr(rows) if chain else None, ptr(fov) if chain else None,
                                      ptr(ref.rest), ptr(ref.local), ptr(ref.parents), ptr(ref.base), ptr(ref.theta), ptr(ref.mask),
                                      ptr(d_T) if chain else None, ptr(d_theta), ptr(ref.theta_ref), ptr(ref.neighbours), *weights, K, ptr(kp[0]),
                                      ptr(kp[1]), ptr(kp[2]), ptr(kp[3]), w_kp, ptr(values), ptr(ws), ws.numel(), stream()), "mgr_fk_backward_terms")

    def plain():
        check(L.mgr_fk_backward(V, J, F, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(ref.rest), ptr(ref.local), ptr(ref.parents), ptr(ref.base),
                                ptr(ref.theta), ptr(ref.mask), ptr(d_T), ptr(d_theta), stream()), "mgr_fk_backward")
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(V=V, F=F, U=U, J=J, K=K)}
    entries = [("mgr_fk_backward", plain), ("terms_all_on", lambda: terms(ref.weights, ref.w_kp)), ("terms_zero_weights", lambda: terms((0.0,) * 4, 0.0)),
               ("terms_priors_only", lambda: terms(ref.weights, 0.0)), ("terms_keypoints_only", lambda: terms((0.0,) * 4, ref.w_kp)),
               ("terms_without_d_transforms", lambda: terms(ref.weights, ref.w_kp, chain=False)), ("mgr_fk_backward_again", plain)]
    for name, fn in entries:
        res[name] = timed(fn, 200)
        print("%-28s %s" % (name, json.dumps(res[name])), flush=True)

    steps = 100 if not a.quick else 10
    start = ref.theta.clone()
    kintree = {str(i): p for i, p in enumerate(parents)}
    rest_d, mask_d, ref_d, tgt, off_h = ref.rest, ref.mask, ref.theta_ref, kp[2], torch.cat([kp[1], torch.ones((K, 1), device=dev)], 1)
    wd = torch.tensor([0.5] * (J + 1) + [2.0], device=dev)[:, None] * mask_d
    wsm = torch.tensor([0.25] * (J + 1) + [1.0], device=dev)[:, None] * mask_d

    def host_fit():
        theta = start.clone().requires_grad_(True)
        opt = torch.optim.Adam([theta], lr=0.02)
        for _ in range(steps):
            opt.zero_grad()
            M = T.euler_angles_to_armature_space(theta[:, :J + 1], kintree, rest_d, theta[:, J + 1])
            p = (M[:, bones] @ off_h[None, :, :, None])[:, :, :3, 0]
            e = 10.0 * ((p - tgt) ** 2).sum() + (wd * (theta - ref_d) ** 2).sum() + (wsm * (theta[:-1] - theta[1:]) ** 2).sum()
            e.backward()
            theta.grad.mul_(mask_d)
            opt.step()

    def device_fit():
        ref.theta.copy_(start)
        ref.fit_keypoints(steps)
    for name, fn in (("fit_keypoints_device", device_fit), ("fit_keypoints_host_torch", host_fit), ("fit_keypoints_device_again", device_fit)):
        res[name] = timed(fn, 2)
        res[name]["steps"] = steps
        print("%-28s %s" % (name, json.dumps(res[name])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--terms", action="store_true", help="time mgr_fk_backward_terms against mgr_fk_backward, and fit_keypoints against host torch")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_fk_refine.py needs a GPU"
    if a.terms:
        return terms_main(a)
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

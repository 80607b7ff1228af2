#!/usr/bin/env python3
"""Time the multi-view 2-D keypoint term of kinematic pose refinement (mgr_fk_backward_terms2d, csrc/fk.hip) at the hand's J = 20,
K = 21 with C = 8 and C = 53 cameras, on U = 8 listed frames (a training step) and U = 512 (a fit); nothing is rendered:

    terms2d_2d_only        the new entry with the 2-D term alone (Huber), no d_transforms
    terms2d_2d_and_3d      the new entry with the 2-D and the 3-D term
    terms2d_with_dist      the 2-D term alone with kp2d_dist written
    terms_3d_only          mgr_fk_backward_terms with the 3-D term alone at the same shape
    host_torch_loss_grad   one evaluation of the same 2-D loss and its gradient as host torch autograd on the device
    fit_keypoints_device   `KinematicPoseRefiner.fit_keypoints(steps)` with the 2-D term alone
    fit_keypoints_host     the same Adam steps as host torch on the device (autograd, torch.optim.Adam)

    python tools/measure_fk_kp2d.py [--out FILE.json] [--quick]

One process, HIP events around a batch of calls, every shape warmed, median of 5 samples with min and max (`measure_pose_refine.timed`).
Needs a GPU; there is no fallback."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from measure_pose_refine import timed  # noqa: E402


def cameras(C, centre, radius, g):
    """(C,3,4) fp64 pixel projections of C cameras on a sphere around `centre`, looking at it: focal 500, centre (320, 240)."""
    i = torch.arange(C, dtype=torch.float64) + 0.5
    phi, z = math.pi * (1 + 5 ** 0.5) * i, 1 - 2 * i / C
    r = (1 - z * z).sqrt()
    dirs = torch.stack([r * phi.cos(), r * phi.sin(), z], 1)
    Kin = torch.tensor([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    out = []
    for d in dirs:
        zc = -d
        up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64) if abs(float(zc[2])) < 0.9 else torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
        x = torch.linalg.cross(up, zc)
        x = x / x.norm()
        Rm = torch.stack([x, torch.linalg.cross(zc, x), zc])
        out.append(Kin @ torch.cat([Rm, -(Rm @ (centre + radius * d))[:, None]], 1))
    return torch.stack(out)


def measure(C, U, a, res):
    from manus_amd import transforms as T
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.pose import KinematicPoseRefiner, dof_mask, project_keypoints
    dev = "cuda:0"
    F = U
    J, parents = 20, [-1 if i % 4 == 0 else i - 1 for i in range(20)]
    g = torch.Generator().manual_seed(5)
    rest = torch.eye(4).repeat(J, 1, 1)
    rest[:, :3, :3] = T.euler_angles_to_matrix(torch.randn((J, 3), generator=g), "XYZ")
    rest[:, :3, 3] = 0.05 * torch.randn((J, 3), generator=g)
    mask = dof_mask(["bone_%d" % i for i in range(J)], True, True)
    bones = [0] + list(range(J))
    K = len(bones)
    off = 0.03 * torch.randn((K, 3), generator=g)
    theta0 = 0.3 * mask * torch.randn((F, J + 2, 3), generator=g)
    delta, w2d = 5.0, 0.01
    ref = KinematicPoseRefiner([("capture", f) for f in range(F)], rest, parents, theta0, 0.02, 0.002, mask=mask, device=dev, w_kp=10.0,
                               w_kp2d=w2d, kp2d_delta=delta)
    true = theta0 + 0.1 * mask * torch.randn((F, J + 2, 3), generator=g)
    M = ref.fk_host(true)
    hom = torch.cat([off.double(), torch.ones((K, 1), dtype=torch.float64)], 1)
    p = (M[:, bones] @ hom[None, :, :, None])[:, :, :3, 0]
    proj = cameras(C, p.reshape(-1, 3).mean(0), 1.0, g).float()
    target = project_keypoints(proj, p) + 2.0 * torch.randn((F, C, K, 2), generator=g, dtype=torch.float64)
    conf = 0.5 + 0.5 * torch.rand((F, C, K), generator=g)
    ref.set_keypoints(bones, off, p)
    ref.set_keypoints_2d(proj, target, conf)
    listed_t = torch.arange(U, dtype=torch.int32, device=dev)
    d_theta = torch.zeros((U, J + 2, 3), device=dev)
    values = torch.zeros(5, dtype=torch.float64, device=dev)
    dist = torch.zeros((U, C, K), device=dev)
    L = lib()
    ws = torch.empty(int(L.mgr_fk_terms2d_workspace_bytes(U, J, K, C)), dtype=torch.uint8, device=dev)
    kp, kp2 = ref.kp, ref.kp2d
    zero = (0.0,) * 4

    def terms2d(w_kp, w_kp2d, d=None):
        check(L.mgr_fk_backward_terms2d(0, J, F, U, ptr(listed_t), None, None, ptr(ref.rest), ptr(ref.local), ptr(ref.parents), ptr(ref.base),
                                        ptr(ref.theta), ptr(ref.mask), None, ptr(d_theta), None, None, *zero, K, ptr(kp[0]), ptr(kp[1]), ptr(kp[2]),
                                        ptr(kp[3]), w_kp, C, ptr(kp2[0]), ptr(kp2[1]), ptr(kp2[2]), w_kp2d, delta, 1e-2, ptr(d), ptr(values), ptr(ws),
                                        ws.numel(), stream()), "mgr_fk_backward_terms2d")

    def terms3d():
        check(L.mgr_fk_backward_terms(0, J, F, U, ptr(listed_t), None, None, ptr(ref.rest), ptr(ref.local), ptr(ref.parents), ptr(ref.base),
                                      ptr(ref.theta), ptr(ref.mask), None, ptr(d_theta), None, None, *zero, K, ptr(kp[0]), ptr(kp[1]), ptr(kp[2]),
                                      ptr(kp[3]), 10.0, ptr(values), ptr(ws), ws.numel(), stream()), "mgr_fk_backward_terms")

    kintree = {str(i): q for i, q in enumerate(parents)}
    off_h = torch.cat([kp[1], torch.ones((K, 1), device=dev)], 1)
    P, tgt, s, mask_d, rest_d = kp2[0], kp2[1], kp2[2], ref.mask, ref.rest

    def loss_of(theta):
        Mh = T.euler_angles_to_armature_space(theta[:, :J + 1], kintree, rest_d, theta[:, J + 1])
        x = (Mh[:, bones] @ off_h[None, :, :, None])[:, :, :3, 0]
        q = torch.einsum("cij,fkj->fcki", P[:, :, :3], x) + P[:, None, :, 3]
        r = q[..., :2] / q[..., 2:] - tgt
        d2 = (r * r).sum(-1)
        d = d2.clamp_min(1e-20).sqrt()
        return w2d * (s * torch.where(d <= delta, d2, 2 * delta * d - delta * delta)).sum()

    start = ref.theta.clone()

    def host_grad():
        theta = start.clone().requires_grad_(True)
        loss_of(theta).backward()
        theta.grad.mul_(mask_d)

    key = "C%d_U%d" % (C, U)
    out = res.setdefault(key, {"shape": dict(J=J, K=K, C=C, U=U, F=F)})
    reps = 200 if U <= 8 else 50
    for name, fn, n in (("terms_3d_only", terms3d, reps), ("terms2d_2d_only", lambda: terms2d(0.0, w2d), reps),
                        ("terms2d_2d_and_3d", lambda: terms2d(10.0, w2d), reps), ("terms2d_with_dist", lambda: terms2d(0.0, w2d, dist), reps),
                        ("terms_3d_only_again", terms3d, reps), ("host_torch_loss_grad", host_grad, 3)):
        out[name] = timed(fn, n)
        print("%-10s %-24s %s" % (key, name, json.dumps(out[name])), flush=True)

    steps = 30 if not a.quick else 3
    ref.w_kp = 0.0                                   # the fit: the 2-D term alone

    def device_fit():
        ref.theta.copy_(start)
        ref.fit_keypoints(steps)

    def host_fit():
        theta = start.clone().requires_grad_(True)
        opt = torch.optim.Adam([theta], lr=0.02)
        for _ in range(steps):
            opt.zero_grad()
            loss_of(theta).backward()
            theta.grad.mul_(mask_d)
            opt.step()
    for name, fn in (("fit_keypoints_device", device_fit), ("fit_keypoints_host", host_fit), ("fit_keypoints_device_again", device_fit)):
        out[name] = timed(fn, 2)
        out[name]["steps"] = steps
        print("%-10s %-24s %s" % (key, name, json.dumps(out[name])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_fk_kp2d.py needs a GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    for C, U in (((8, 8), (53, 8), (8, 512), (53, 512)) if not a.quick else ((8, 8),)):
        measure(C, U, a, res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

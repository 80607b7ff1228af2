#!/usr/bin/env python3
"""Time the spatial image loss (mgr_image_loss2d, csrc/ssim2d.hip) and the step that uses it.

    python tools/measure_ssim2d.py [--out FILE.json] [--quick] [--no-step] [--no-torch]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats), at 8 views of
1920x1080 on the bench scene (bench.py's: 300k hand Gaussians, targets = the model perturbed by 1 %):
  * the call dense (MGR_IL2D_DENSE: every block runs the heavy kernel) on the scene's render against its targets;
  * the call with settling on the same inputs (and the share of blocks it listed);
  * the forward-only masked call (the validation metric);
  * the torch composition on the same inputs: L1 + SSIM as five grouped F.conv2d under autograd, value and gradient -- what a
    user would write without the kernel;
  * mgr_image_loss, the rows kernel, on the same inputs (its plain entry: both images read everywhere);
  * the bench step with ssim "rows" and "spatial", alternated.
Needs a GPU; there is no fallback."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from measure_feature_render import timed  # noqa: E402


def torch_composition(pred, target, w_l1, w_ssim, scale):
    """w_l1 sum|d| - w_ssim sum S (times scale) and its gradient w.r.t. pred, in plain torch."""
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2.0 * 1.5 * 1.5)) for i in range(11)], dtype=torch.float32, device=pred.device)
    g = g / g.sum()
    win = (g[:, None] @ g[None, :]).expand(3, 1, 11, 11).contiguous()
    x = pred.detach().requires_grad_(True)

    def conv(a):
        return F.conv2d(a, win, padding=5, groups=3)

    mu1, mu2 = conv(x), conv(target)
    s11, s22, s12 = conv(x * x) - mu1 * mu1, conv(target * target) - mu2 * mu2, conv(x * target) - mu1 * mu2
    S = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    loss = scale * (w_l1 * (x - target).abs().sum() - w_ssim * S.sum())
    loss.backward()
    return loss.detach(), x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--no-step", action="store_true", help="skip the two bench steps")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_ssim2d.py needs a GPU"
    from manus_amd import ops, rasterizer as rz
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
        mask = rz.blend_features(depth=False, alpha=True, device=dev)["alpha"].clone()
        del hp
        rz.context(dev).clear()
        hc = HipViewCompute(scene, targets, ct)
        render = hc.forward_views_fused(ids)[0].contiguous().clone()
        del hc
    rz.context(dev).clear()
    n = float(3 * H * W)
    res = {"device": torch.cuda.get_device_name(0), "sizes": dict(V=V, N=N, W=W, H=H), "block": ops.image_loss2d_block(), "calls": {}, "step": {}}
    bw, bh = ops.image_loss2d_block()
    d = (render != targets).any(1).float()[:, None]
    listed = F.max_pool2d(F.max_pool2d(d, 21, 1, 10), (bh, bw), (bh, bw), ceil_mode=True)      # an upper estimate: dilated by 10, per block
    res["listed_block_share"] = float(listed.mean())
    rep = 5 if not a.quick else 2
    calls = [("dense", lambda: ops.image_loss2d_grad(render, targets, 0.8, 0.2, 1.0 / n, dense=True)),
             ("settling", lambda: ops.image_loss2d_grad(render, targets, 0.8, 0.2, 1.0 / n)),
             ("forward_only_masked", lambda: ops.image_loss2d_grad(render, targets, 0.0, 1.0, mask=mask, need_grad=False)),
             ("forward_only_masked_dense", lambda: ops.image_loss2d_grad(render, targets, 0.0, 1.0, mask=mask, need_grad=False, dense=True)),
             ("rows_kernel", lambda: ops.image_loss_grad(render, targets, 0.8, 0.2, 1.0 / n))]
    if not a.no_torch:
        calls.append(("torch_composition", lambda: torch_composition(render, targets, 0.8, 0.2, 1.0 / n)))
    for key, fn in calls:
        res["calls"][key] = timed(fn, rep if key != "torch_composition" else 2)
        print("call %s" % key, json.dumps(res["calls"][key]), flush=True)
    if "torch_composition" in res["calls"]:
        t = res["calls"]["torch_composition"]["median_ms"]
        res["torch_over_dense"] = t / res["calls"]["dense"]["median_ms"]
        res["torch_over_settling"] = t / res["calls"]["settling"]["median_ms"]
        # the two agree (a sanity check of the comparison, not a test)
        s, _, gk = ops.image_loss2d_grad(render, targets, 0.8, 0.2, 1.0 / n, dense=True)
        lt, gt = torch_composition(render, targets, 0.8, 0.2, 1.0 / n)
        res["agreement"] = dict(loss_kernel=float(s[2]), loss_torch=float(lt), grad_max_abs_diff=float((gk - gt).abs().max()), grad_max=float(gt.abs().max()))
        print("ratios", json.dumps({k: res[k] for k in ("torch_over_dense", "torch_over_settling", "agreement")}), flush=True)
        del gk, gt
        torch.cuda.empty_cache()
    if not a.no_step:
        steps = {"rows": HipViewCompute(scene, targets, ct, loss="l1+ssim"), "spatial": HipViewCompute(scene, targets, ct, loss="l1+ssim", ssim="spatial")}
        for key in ("rows", "spatial", "rows_again", "spatial_again"):
            hc = steps[key.replace("_again", "")]
            res["step"][key] = timed(lambda: hc(ids, 1.0 / V), 20 if not a.quick else 3)
            print("step %s" % key, json.dumps(res["step"][key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

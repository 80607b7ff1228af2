#!/usr/bin/env python3
"""Time the validation kernels on the GPU against the same metrics composed from torch ops.

    python tools/measure_eval.py [--out FILE.json] [--quick]

One process, HIP events, every shape warmed, median of 5 samples (each sample a batch of repeats), 8 views at 1920x1080:
  (i)   ops.eval_views + ops.eval_triptych       (mgr_eval_views: k_eval_views + k_eval_fold; mgr_eval_triptych)
  (ii)  the torch composition of the same results on the device: masked multiplies, squared-error sums, the SSIM of
        loss_utils.py:57-97 as the reference writes it (F.conv2d with groups = H on the HWC images), clamp / byte
        conversion and the float64 difference panel of base.py:116-127, one view after the other like validation_step
  (i) again, so that the two are alternated in one process.
Also printed: the bytes the kernels must move (inputs read once, outputs written once) against their time.  The
composition is the comparison: the commit before this tool had no validation pass at all.  The agreement of the two is
printed too; the composition's DIFFERENCE panel is not a reference (it differs from numpy's in a few per cent of the bytes -- most
likely torch's device division by a Python scalar, to whose last bit the panel's truncating cast is sensitive): the kernel's bytes are pinned against
numpy by tests/test_gpu_validation.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


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


def torch_window(H, dev):
    g = torch.tensor([torch.exp(torch.tensor(-((x - 5) ** 2) / float(2 * 1.5 ** 2))) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(H, 1, 11, 11).contiguous().to(dev)


def torch_ssim(img1, img2, window, H):
    mu1, mu2 = F.conv2d(img1, window, padding=5, groups=H), F.conv2d(img2, window, padding=5, groups=H)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img1 * img1, window, padding=5, groups=H) - mu1_sq
    s2 = F.conv2d(img2 * img2, window, padding=5, groups=H) - mu2_sq
    s12 = F.conv2d(img1 * img2, window, padding=5, groups=H) - mu1_mu2
    return (((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))).mean()


def torch_validation(pred_hwc, gt_hwc, mask_hw1, window):
    """validation_step's arithmetic per view, on the device."""
    out = []
    H = pred_hwc.shape[1]
    for v in range(pred_hwc.shape[0]):
        p, t, m = pred_hwc[v], gt_hwc[v], mask_hw1[v]
        img = (torch.clamp(p, 0, 1) * 255).to(torch.uint8)
        gt_img = (t * 255 if t.max() <= 1.0 else t).to(torch.uint8)         # (one host read per view, like dump_image)
        diff = (gt_img.double() / 255.0 - img.double() / 255.0) * 255.0
        trip = torch.cat([img, gt_img, diff.to(torch.int64).to(torch.uint8)], dim=0)
        r, g = p * m, t * m
        psnr = -10 * torch.log10(torch.mean((r - g) ** 2))
        out.append((psnr, torch_ssim(r, g, window, H), trip))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_eval.py needs a GPU"
    from manus_amd import ops
    dev = "cuda:0"
    V, H, W = (8, 1080, 1920) if not a.quick else (2, 64, 96)
    g = torch.Generator(device=dev).manual_seed(3)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    tgt = (0.5 + 0.45 * torch.sin(5 * xx + 3 * yy + torch.arange(V * 3, device=dev).float().reshape(V, 3, 1, 1))).contiguous()
    pred = (tgt + 0.05 * torch.randn((V, 3, H, W), device=dev, generator=g)).clamp(-0.1, 1.1).contiguous()
    mask = (0.5 + 0.7 * torch.sin(3 * xx + 2 * yy))[None].expand(V, H, W).clamp(0, 1).contiguous()
    pred_hwc, gt_hwc, mask_hw1 = pred.permute(0, 2, 3, 1).contiguous(), tgt.permute(0, 2, 3, 1).contiguous(), mask[..., None].contiguous()
    window = torch_window(H, dev)

    def hip():
        sq, ss, gmax = ops.eval_views(pred, tgt, mask)
        return sq, ss, ops.eval_triptych(pred, tgt, gmax)

    def hip_metrics():
        return ops.eval_views(pred, tgt, mask)

    sq, ss, trip = hip()
    ref = torch_validation(pred_hwc, gt_hwc, mask_hw1, window)
    n = float(3 * H * W)
    res = {"device": torch.cuda.get_device_name(0), "V": V, "H": H, "W": W,
           "max_psnr_diff_db": max(abs(float(-10 * torch.log10(sq[v] / n)) - float(ref[v][0])) for v in range(V)),
           "max_ssim_diff": max(abs(float(ss[v]) / n - float(ref[v][1])) for v in range(V)),
           "triptych_bytes_differing_from_torch_composition": int(sum((trip[v] != ref[v][2]).sum() for v in range(V)))}
    reps = 20 if not a.quick else 3
    res["hip_eval_views_plus_triptych"] = timed(hip, reps)
    res["torch_composition"] = timed(lambda: torch_validation(pred_hwc, gt_hwc, mask_hw1, window), 2)
    res["hip_eval_views_plus_triptych_again"] = timed(hip, reps)
    res["hip_eval_views_alone"] = timed(hip_metrics, reps)
    # bytes: pred + target (fp32, 3 channels) and the mask read by the metrics; pred + target read again and 9 bytes per
    # pixel written by the triptych
    px = V * H * W
    res["bytes_eval_views"] = px * (24 + 4)
    res["bytes_triptych"] = px * (24 + 9)
    ms_all, ms_m = res["hip_eval_views_plus_triptych_again"]["median_ms"], res["hip_eval_views_alone"]["median_ms"]
    res["eval_views_GBps"] = res["bytes_eval_views"] / (ms_m * 1e-3) / 1e9
    res["triptych_GBps"] = res["bytes_triptych"] / (max(ms_all - ms_m, 1e-6) * 1e-3) / 1e9
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

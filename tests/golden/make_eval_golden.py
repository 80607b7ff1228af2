#!/usr/bin/env python3
"""Generate tests/golden/validation.npz by IMPORTING the reference (authoring container only):

    python tests/golden/make_eval_golden.py

Same rules as make_golden.py, whose stub approach it reuses: the reference's Python is imported with stub modules for
the packages this image lacks, and only arrays are written.  Nothing is restated here: every case is one call of the
reference's own
  * src/modules/base.py:112-154   BaseTrainingModule.validation_step
on a fake `self` whose `render` returns the case's image (batch_idx = 1: no dump_gaussians), which in turn calls
  * src/utils/loss_utils.py:57-108            ssim, psnr
  * src/utils/extra.py:110-115, 153-160       concat_img_array, dump_image
`lpips_loss` is stubbed (its network weights are not in this image; the value is not recorded).  After the cases,
  * src/modules/base.py:156-188   on_validation_epoch_end
is run twice in a temporary directory and the text of the CSV it wrote and the names of its PNGs are recorded.

Contents, per case k:  pred<k> (H,W,3) f32, gt<k> (1,H,W,3) f32, mask<k> (1,H,W,1) f32, has_mask<k> (0: the product is
called WITHOUT a mask, the reference with ones), psnr<k>, ssim<k> f32, image<k> (3H,W,3) u8;  names (K,);  csv_text,
png_names and csv_psnr_vals / csv_ssim_vals (the two views' metrics the epoch end averaged).
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                      # noqa: E402  (stubs + reference import)

H, W = 48, 64


def smooth(g, lo=0.0, hi=1.0, noise=0.01):
    """A smooth (H,W,3) image in [lo, hi]: a few low-frequency waves per channel and a little noise."""
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy, ph = g.uniform(0.5, 4.0), g.uniform(0.5, 4.0), g.uniform(0, 2 * np.pi)
            out[..., c] += g.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
    out = (out - out.min()) / (out.max() - out.min())
    out = np.clip(out + noise * g.normal(size=out.shape), 0, 1)
    return (lo + (hi - lo) * out).astype(np.float32)


def soft_mask(g, binary):
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    r = np.sqrt((xx - g.uniform(-0.2, 0.2)) ** 2 + (1.4 * (yy - g.uniform(-0.2, 0.2))) ** 2)
    m = np.clip((0.8 - r) / 0.25, 0, 1)
    if binary:
        m = (m > 0.5).astype(np.float64)
    return m.astype(np.float32)[None, :, :, None]


def cases():
    g = np.random.default_rng(2024)
    ones = np.ones((1, H, W, 1), np.float32)
    out = []
    gt = smooth(g)
    out.append(("fractional_mask", np.clip(gt + 0.08 * (smooth(g) - 0.5) + 0.03 * g.normal(size=gt.shape), 0, 1), gt, soft_mask(g, False), 1))
    gt = smooth(g)
    out.append(("binary_mask", np.clip(gt + 0.05 * (smooth(g) - 0.5) + 0.05 * g.normal(size=gt.shape), 0, 1), gt, soft_mask(g, True), 1))
    gt = smooth(g)
    out.append(("no_mask", np.clip(gt + 0.1 * (smooth(g) - 0.5) + 0.02 * g.normal(size=gt.shape), 0, 1), gt, ones, 0))
    gt = smooth(g)
    out.append(("render_out_of_range", gt + 0.6 * (smooth(g) - 0.5), gt, soft_mask(g, False), 1))      # about [-0.3, 1.3]
    gt = smooth(g, 3.0, 251.5)
    out.append(("gt_0_255", np.clip(gt / 255.0 + 0.05 * (smooth(g) - 0.5), 0, 1), gt, soft_mask(g, True), 1))
    gt = smooth(g)
    out.append(("equal", gt, gt, soft_mask(g, False), 1))
    # values on a grid of 2^-12 (2^-4 for the 0..255 image, 2^-8 for the masks): exact in fp32, and the file compresses to half
    def grid(a, step):
        return np.ascontiguousarray(np.round(np.asarray(a, np.float64) / step) * step, np.float32)
    return [(n, grid(p, 2.0 ** -12), grid(t, 2.0 ** -4 if t.max() > 1 else 2.0 ** -12)[None], grid(m, 2.0 ** -8), hm)
            for n, p, t, m, hm in out]


def main():
    mods = mg._import_reference()
    base_mod = sys.modules["src.modules.base"]
    base = mods["hand_dynamic"].TrainingModule.__mro__[1]          # BaseTrainingModule
    base_mod.lpips_loss = lambda pred, ref: torch.zeros(())         # (weights absent; not recorded)
    fake = types.SimpleNamespace(val_images=[], psnr_vals=[], ssim_vals=[], lpips_vals=[], render_time=[],
                                 exp_name="golden_exp", global_step=700, batch_size=1, log=lambda *a, **k: None)
    out, names = {}, []
    with np.errstate(all="ignore"):
        for k, (name, pred, gt, mask, has_mask) in enumerate(cases()):
            fake.render = lambda batch, _p=pred: {"render": torch.from_numpy(_p.copy())}
            batch = {"rgb": torch.from_numpy(gt.copy()), "mask": torch.from_numpy(mask.copy())}
            base.validation_step(fake, batch, 1)
            names.append(name)
            out["pred%d" % k], out["gt%d" % k], out["mask%d" % k] = pred, gt, mask
            out["has_mask%d" % k] = np.int32(has_mask)
            out["psnr%d" % k] = np.float32(fake.psnr_vals[-1])
            out["ssim%d" % k] = np.float32(fake.ssim_vals[-1])
            out["image%d" % k] = np.asarray(fake.val_images[-1], np.uint8)
            print(k, name, "psnr", out["psnr%d" % k], "ssim", out["ssim%d" % k], "gt max", gt.max(), "render range", pred.min(), pred.max())
    out["names"] = np.asarray(names)
    # the epoch end: CSV text and PNG names as the reference writes them (finite metrics only: np.mean of the cases above holds an inf)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        fake.val_results_dir = os.path.join(tmp, "val_results")
        os.makedirs(fake.val_results_dir)
        keep = [i for i, v in enumerate(fake.psnr_vals) if np.isfinite(v)][:2]
        for lst in ("psnr_vals", "ssim_vals", "lpips_vals", "render_time", "val_images"):
            setattr(fake, lst, [getattr(fake, lst)[i] for i in keep])
        fake.render_time = [0.25, 0.75]
        out["csv_psnr_vals"], out["csv_ssim_vals"] = np.asarray(fake.psnr_vals, np.float32), np.asarray(fake.ssim_vals, np.float32)
        base.on_validation_epoch_end(fake)
        fake.global_step = 800
        base.on_validation_epoch_end(fake)
        out["csv_text"] = np.asarray(open(os.path.join(fake.val_results_dir, "val_results.csv")).read())
        out["png_names"] = np.asarray(sorted(os.listdir(os.path.join(fake.val_results_dir, "images"))))
    os.chdir(cwd)
    path = os.path.join(HERE, "validation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    print(str(out["csv_text"]))
    print(out["png_names"])


if __name__ == "__main__":
    main()

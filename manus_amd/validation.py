"""The validation pass of brown-ivl/manus over the HIP kernels of csrc/eval.hip.

Mirrors `BaseTrainingModule.validation_step` / `on_validation_epoch_start` / `on_validation_epoch_end`
(src/modules/base.py:103-188) with `psnr` / `write_csv` of src/utils/loss_utils.py:100-136:

    validation_step(render_hwc, batch)   masked PSNR and SSIM of one held-out view and its uint8
                                         render | ground truth | difference triptych (3H,W,3)
    Validator(result_dir, exp_name)      start() / add(...) / end(global_step): the epoch's means appended to
                                         <result_dir>/val_results/val_results.csv and the triptychs saved as
                                         <result_dir>/val_results/images/{step}_{idx}.png

`engine.Trainer.validate` is the batched form (V views per launch chain, straight from the rasterizer's layout).

LPIPS (loss_utils.py:19, 111-117; base.py:149): its network weights are not part of this package.  With a user-supplied
`manus_amd.lpips.LPIPS` (`Trainer.validate(..., lpips=...)`, `Validator.add(..., lpips=...)`) the `lpips` column of the CSV
holds the mean of the per-view values on the masked images; without one it is written as an EMPTY field so that the file
keeps the reference's six columns.  Not reproduced: the `.ply` dump of `dump_gaussians` for the first validation batch.

NaN pixels: numpy's float -> uint8 cast of NaN is undefined; here a NaN render or ground-truth pixel is written as
byte 0 in its panel.  That is this package's definition, not the reference's.
"""
import csv
import os

import numpy as np
import torch

from . import ops
from ._lib import ManusHipError

CSV_HEADER = ["name", "step", "psnr", "ssim", "lpips", "rendering_time"]     # loss_utils.write_csv

_DIFF = None


def diff_table():
    """(256,256) uint8, [gt_byte, render_byte] -> the difference panel's byte.  validation_step computes
    `diff = gt_img / 255.0 - img / 255.0; diff = diff * 255.0` on the two uint8 images (float64) and concat_img_array
    casts it with astype(np.uint8) (base.py:124-127, extra.py:110-115): the cast truncates (products such as 1.9999999
    become 1) and wraps negatives, and the result depends on the two bytes only.  The table is built with exactly that
    numpy expression on all byte pairs; the kernel gathers from it."""
    global _DIFF
    if _DIFF is None:
        gt_img = np.arange(256, dtype=np.uint8)[:, None]
        img = np.arange(256, dtype=np.uint8)[None, :]
        diff = gt_img / 255.0 - img / 255.0
        diff = diff * 255.0
        with np.errstate(invalid="ignore"):
            _DIFF = np.ascontiguousarray(diff.astype(np.int64).astype(np.uint8))
    return _DIFF


def psnr_from_sums(sq_sum, n_elements):
    """-10 log10(sq_sum / n): psnr of loss_utils.py:100-108 from the kernel's sums (+inf for sq_sum == 0)."""
    return -10 * torch.log10(sq_sum / float(n_elements))


SSIM_KINDS = ("rows", "spatial")


def check_ssim_kind(ssim):
    """"rows": the reference's ssim() on its HWC images (the window over the (W,3) plane of every image row; csrc/eval.hip);
    "spatial": the standard 2-D SSIM (csrc/ssim2d.hip), comparable with the SSIM of a paper.  Anything else: ValueError."""
    if ssim not in SSIM_KINDS:
        raise ValueError("ssim must be 'rows' or 'spatial' (got %r)" % (ssim,))
    return ssim


def spatial_ssim(pred, tgt, mask):
    """(V,) mean spatial SSIM of the masked images render * mask, target * mask (base.py:144-147): `view_sums` of a
    forward-only `ops.image_loss2d_grad`."""
    _, view_sums, _ = ops.image_loss2d_grad(pred, tgt, 0.0, 1.0, mask=mask, need_grad=False)
    return view_sums[:, 1] / float(pred[0].numel())


def validation_step(render_hwc, batch, ssim="rows"):
    """One held-out view, shaped like the reference's: render (H,W,3); batch["rgb"] (H,W,3) and batch["mask"] (H,W,1)
    (or (H,W)), each optionally with a leading batch dimension of 1; a missing / None mask means ones.  GPU tensors.
    ssim: "rows" (the reference's statistic) or "spatial" (`check_ssim_kind`) -- which SSIM fills the "ssim" value; PSNR and
    the triptych are the same either way.
    Returns {"psnr", "ssim": 0-dim device tensors, "image": (3H,W,3) uint8 device tensor, "ssim_kind": ssim}."""
    check_ssim_kind(ssim)
    gt, mask = batch["rgb"], batch.get("mask")
    if not (torch.is_tensor(render_hwc) and render_hwc.is_cuda and torch.is_tensor(gt) and gt.is_cuda):
        raise ManusHipError("validation_step needs GPU tensors; there is no CPU fallback")
    if render_hwc.dim() == 4 and render_hwc.shape[0] == 1:
        render_hwc = render_hwc[0]
    if gt.dim() == 4:
        if gt.shape[0] != 1:
            raise ManusHipError("validation_step: a batched image must have batch size 1 (as in the reference)")
        gt = gt[0]
        if mask is not None:
            mask = mask[0]
    if render_hwc.dim() != 3 or render_hwc.shape[-1] != 3 or gt.shape != render_hwc.shape:
        raise ManusHipError("validation_step: render and batch['rgb'] are (H,W,3) images of one size")
    H, W, _ = render_hwc.shape
    if mask is not None:
        if mask.numel() != H * W:
            raise ManusHipError("validation_step: batch['mask'] must be (H,W,1)")
        mask = mask.reshape(1, H, W).float().contiguous()
    pred = render_hwc.detach().float().permute(2, 0, 1).contiguous()[None]
    tgt = gt.detach().float().permute(2, 0, 1).contiguous()[None]
    sq, ss, gmax = ops.eval_views(pred, tgt, mask)
    image = ops.eval_triptych(pred, tgt, gmax)[0]
    n = 3 * H * W
    ss = spatial_ssim(pred, tgt, mask) if ssim == "spatial" else ss / float(n)
    return {"psnr": psnr_from_sums(sq, n)[0], "ssim": ss[0], "image": image, "ssim_kind": ssim}


def _scalar(x):
    return float(x.item()) if torch.is_tensor(x) else float(x)


class Validator:
    """The bookkeeping of one validation epoch (base.py:103-110, 151-188)."""

    def __init__(self, result_dir, exp_name):
        self.result_dir, self.exp_name = result_dir, exp_name
        self.val_results_dir = os.path.join(result_dir, "val_results")
        self.start()

    def start(self):
        """on_validation_epoch_start"""
        os.makedirs(self.val_results_dir, exist_ok=True)
        self.val_images, self.psnr_vals, self.ssim_vals, self.render_time = [], [], [], []
        self.lpips_vals = []

    def add(self, psnr, ssim, render_time, image=None, lpips=None):
        """One validated view: its metrics (numbers or 0-dim tensors), the wall-clock seconds of its render and its
        (3H,W,3) uint8 triptych (tensor or array; None: no image kept).  lpips: the view's LPIPS value, or None (no network)."""
        if lpips is not None:
            self.lpips_vals.append(_scalar(lpips))
        self.psnr_vals.append(_scalar(psnr))
        self.ssim_vals.append(_scalar(ssim))
        self.render_time.append(float(render_time))
        if image is not None:
            if torch.is_tensor(image):
                image = image.detach().cpu().numpy()
            self.val_images.append(np.ascontiguousarray(image, dtype=np.uint8))

    def end(self, global_step):
        """on_validation_epoch_end: append `name, step, psnr, ssim, lpips, rendering_time` (the header first when the file
        is new; `lpips` empty without values, see the module docstring) and save the triptychs.  Returns the row."""
        lp = np.mean(self.lpips_vals) if getattr(self, "lpips_vals", None) else ""
        row = [self.exp_name, int(global_step), np.mean(self.psnr_vals), np.mean(self.ssim_vals), lp, np.mean(self.render_time)]
        csv_path = os.path.join(self.val_results_dir, "val_results.csv")
        new = not os.path.exists(csv_path)
        with open(csv_path, "a") as f:
            w = csv.writer(f, delimiter=",")
            if new:
                w.writerow(CSV_HEADER)
            w.writerow(row)
        if self.val_images:
            from PIL import Image
            image_dir = os.path.join(self.val_results_dir, "images")
            os.makedirs(image_dir, exist_ok=True)
            for idx, val_image in enumerate(self.val_images):
                Image.fromarray(val_image).save(os.path.join(image_dir, "%d_%d.png" % (int(global_step), idx)))
        return row

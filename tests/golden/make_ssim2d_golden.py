"""Maker of tests/golden/ssim2d.npz: the reference's own loss_utils.ssim (src/utils/loss_utils.py:57-97) on two CHW image
pairs -- the standard 2-D SSIM that `ops.image_loss2d_grad` and tests/ssim2d_ref.py compute.

    python tests/golden/make_ssim2d_golden.py

The reference's Python is imported with the stub modules of make_golden.py (its `lpips` import is a stub: nothing is
downloaded).  Only data goes into the fixture: the two input pairs (fp32, seeded here) and the scalar each gave.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import make_golden
    import ssim2d_ref as R
    lu = make_golden._import_reference()["loss_utils"]
    out = {"n_pairs": np.int64(2)}
    for k, (H, W, seed) in enumerate(((40, 56, 101), (23, 17, 102))):
        pred, tgt = R.smooth_images(1, H, W, seed)
        a, b = pred[0].contiguous(), tgt[0].contiguous()
        with torch.no_grad():
            val = lu.ssim(a, b)      # CHW: channel = 3, the window over H x W
        out["img1_%d" % k], out["img2_%d" % k], out["ssim_%d" % k] = a.numpy(), b.numpy(), np.float32(float(val))
        print("pair %d (%dx%d): ssim %.9g" % (k, H, W, float(val)))
    np.savez_compressed(os.path.join(HERE, "ssim2d.npz"), **out)


if __name__ == "__main__":
    main()

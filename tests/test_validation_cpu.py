"""CPU: the host half of the validation pass (manus_amd.validation) -- the 256x256 difference table, the Validator's CSV
rows and PNG names against what the reference's on_validation_epoch_end wrote (tests/golden/validation.npz), and the
"GPU tensors only" rule of the two new ops."""
import csv
import os

import numpy as np
import pytest
import torch


def test_diff_table_is_the_reference_expression_on_all_byte_pairs(golden_dir):
    """base.py:124-127 on uint8 images holding every (gt, render) byte pair, cast like concat_img_array does."""
    from manus_amd.validation import diff_table
    gt_img, img = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    diff = gt_img / 255.0 - img / 255.0
    diff = diff * 255.0
    with np.errstate(invalid="ignore"):
        want = np.concatenate((img, diff), axis=0).astype(np.uint8)[256:]
    tab = diff_table()
    assert tab.shape == (256, 256) and tab.dtype == np.uint8
    assert np.array_equal(tab, want)
    # the cast truncates: 255 * (k/255 - j/255) is not always the integer k - j in float64
    assert int((tab != (gt_img.astype(np.int64) - img).astype(np.uint8)).sum()) > 0
    assert tab[0, 0] == 0 and tab[255, 0] == 255 and tab[0, 1] in (255, 0)
    # and the fixture's difference panels are this table applied to its other two panels
    d = np.load(os.path.join(golden_dir, "validation.npz"))
    for k in range(len(d["names"])):
        im = d["image%d" % k]
        H = im.shape[0] // 3
        assert np.array_equal(tab[im[H:2 * H], im[:H]], im[2 * H:]), str(d["names"][k])


def test_validator_writes_the_reference_rows_and_png_names(golden_dir, tmp_path):
    from manus_amd.validation import Validator
    d = np.load(os.path.join(golden_dir, "validation.npz"))
    ref_rows = list(csv.reader(str(d["csv_text"]).splitlines()))
    assert ref_rows[0] == ["name", "step", "psnr", "ssim", "lpips", "rendering_time"] and len(ref_rows) == 3
    v = Validator(str(tmp_path), "golden_exp")
    images = [d["image0"], d["image1"]]
    for step in (700, 800):
        v.start()
        for k, t in enumerate((0.25, 0.75)):
            v.add(torch.tensor(d["csv_psnr_vals"][k]), float(d["csv_ssim_vals"][k]), t, torch.from_numpy(images[k].copy()))
        v.end(step)
    path = os.path.join(str(tmp_path), "val_results", "val_results.csv")
    rows = list(csv.reader(open(path).read().splitlines()))
    assert rows[0] == ref_rows[0] and len(rows) == 3                 # the header once
    for got, ref in zip(rows[1:], ref_rows[1:]):
        assert got[0] == ref[0] and got[1] == ref[1]                 # name, step
        assert abs(float(got[2]) - float(ref[2])) < 1e-5 and abs(float(got[3]) - float(ref[3])) < 1e-7
        assert got[4] == ""                                          # lpips: not computed, the column stays
        assert float(got[5]) == float(ref[5])
    names = sorted(os.listdir(os.path.join(str(tmp_path), "val_results", "images")))
    assert names == [str(n) for n in d["png_names"]]
    from PIL import Image
    back = np.asarray(Image.open(os.path.join(str(tmp_path), "val_results", "images", "800_1.png")))
    assert np.array_equal(back, images[1])


def test_eval_ops_fail_loudly_without_gpu():
    from manus_amd import losses, ops, validation
    from manus_amd._lib import ManusHipError
    x = torch.zeros(1, 3, 4, 8)
    with pytest.raises(ManusHipError):
        ops.eval_views(x, x)
    with pytest.raises(ManusHipError):
        ops.eval_views(x, x, torch.ones(1, 4, 8))
    with pytest.raises(ManusHipError):
        ops.eval_triptych(x, x, torch.ones(1))
    with pytest.raises(ManusHipError):
        validation.validation_step(torch.zeros(4, 8, 3), {"rgb": torch.zeros(4, 8, 3), "mask": torch.ones(4, 8, 1)})
    with pytest.raises(ManusHipError):
        losses.psnr(torch.zeros(4, 8, 3), torch.zeros(4, 8, 3))


def test_eval_entries_validate_their_arguments():
    from manus_amd._lib import lib
    L = lib()
    assert L.mgr_eval_workspace_bytes(8, 1080, 1920) == 8 * 540 * 8 * 16
    assert L.mgr_eval_workspace_bytes(0, 4, 4) == 0
    assert L.mgr_eval_views(0, 4, 4, None, None, None, None, None, None, None, None, 0, None) == -1 and b"bad sizes" in L.mgr_last_error()
    assert L.mgr_eval_views(1, 4, 4, None, None, None, None, None, None, None, None, 0, None) == -1 and b"null" in L.mgr_last_error()
    assert L.mgr_eval_triptych(1, 4, 4, None, None, None, None, None, None) == -1 and b"null" in L.mgr_last_error()
    assert L.mgr_eval_triptych(1, 70000, 4, None, None, None, None, None, None) == -1

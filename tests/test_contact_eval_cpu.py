"""CPU: the host side of the contact evaluation (manus_amd.contact_eval) against the reference's own outputs
(tests/golden/contact_eval.npz, written by tests/golden/make_contact_eval_golden.py): the collage table, the scores from
counts, the CSV text, the averaging, the natural sort, argument checks -- and the fixture maker's OpenCV stand-ins
against scipy.ndimage, the second statement of the morphology (OpenCV itself is the unpinned leg)."""
import importlib.util
import os

import numpy as np
import pytest

from manus_amd import contact_eval as ce


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "contact_eval.npz"))


def test_palette_and_table_shapes():
    assert ce.PALETTE.shape == (16, 3) and ce.PALETTE.dtype == np.uint8
    assert len({tuple(c) for c in ce.PALETTE.tolist()}) == 16
    assert ce.CSV_HEADER == [""] + ["bone%d" % i for i in range(1, 17)] + ["combined"]
    t = ce.collage_table()
    assert t.shape == (256, 3, 2, 3) and t.dtype == np.uint8
    assert (t[:, :, 0, :] == 255).all()                      # alpha clear: white, whatever the photo and the mask
    assert (np.abs(t[:, 0, 1, 0].astype(int) - np.arange(256)) <= 1).all()   # plain panel, alpha set: uint8(b / 255 * 255), truncated
    assert np.array_equal(t[:, 1, 1, :], t[:, 2, 1, :][:, [0, 0, 0]])   # clear mask = the set mask's red / blue channels
    assert (t[:, 2, 1, 1] >= t[:, 2, 1, 0]).all()


def test_collage_table_against_combine_images(golden_dir):
    """Every byte of the reference's collage rows is the table's entry for (photo byte, panel kind, alpha, channel)."""
    d, t = _golden(golden_dir), ce.collage_table()
    for k in range(int(d["n"])):
        rgba = d["rgba%d" % k]
        al = (rgba[..., 3] > 128).astype(np.int64)
        ch = np.arange(3)[None, None, :]
        panels = [t[rgba[..., :3], 0, al[..., None], ch]]
        for m in (d["gt%d" % k], d["mano_mask%d" % k], d["harp_mask%d" % k], d["pred%d" % k]):
            panels.append(t[rgba[..., :3], 1 + (m[..., None] == 255), al[..., None], ch])
        assert np.array_equal(np.concatenate(panels, axis=1), d["row5%d" % k]), k
        assert np.array_equal(np.concatenate([panels[0], panels[1], panels[4]], axis=1), d["row%d" % k]), k


def test_scores_from_counts_match_the_reference(golden_dir):
    d = _golden(golden_dir)
    saw_nan = False
    for k in range(int(d["n"])):
        iou, f1 = ce.scores_from_counts(d["counts%d" % k])
        assert iou.shape == (3, 17) and iou.dtype == np.float64
        np.testing.assert_allclose(iou, d["iou%d" % k], rtol=0, atol=1e-9)
        np.testing.assert_allclose(f1, d["f1%d" % k], rtol=0, atol=1e-9, equal_nan=True)
        saw_nan |= bool(np.isnan(d["f1%d" % k]).any())
    assert saw_nan
    iou, f1 = ce.scores_from_counts(np.array([[0, 0, 0], [3, 4, 5], [0, 2, 0]]))
    assert iou[0] == 0.0 and np.isnan(f1[0])
    assert iou[1] == 3 / (6 + 1e-6) and f1[1] == 6 / 9
    assert f1[2] == 0.0
    with pytest.raises(ValueError):
        ce.scores_from_counts(np.zeros((17, 2)))


def test_csv_text_equals_the_reference(golden_dir, tmp_path):
    d = _golden(golden_dir)
    order = [int(i) for i in d["main_order"]]
    per = {}
    for j, m in enumerate(("ours", "mano", "harp")):
        per[m] = np.vstack([d["iou%d" % k][j] for k in order])
        per[m + "_f1"] = np.vstack([d["f1%d" % k][j] for k in order])
    p = str(tmp_path / "full.csv")
    ce.write_metric_csv(p, ["ours", "mano", "harp"], ce.metric_rows(per))
    assert open(p, newline="").read() == str(d["csv_full"])
    zeros = np.zeros((len(order), 16))
    per0 = {"ours": np.concatenate([zeros, per["ours"][:, -1:]], axis=1), "ours_f1": np.concatenate([zeros, per["ours_f1"][:, -1:]], axis=1)}
    p = str(tmp_path / "ours.csv")
    ce.write_metric_csv(p, ["ours"], ce.metric_rows(per0))
    assert open(p, newline="").read() == str(d["csv_ours"])
    assert "nan" in str(d["csv_full"])


def test_average_eval_metrics_against_pandas(golden_dir, tmp_path):
    import pandas as pd
    d = _golden(golden_dir)
    paths = []
    for i, key in enumerate(("csv_full", "csv_ours", "csv_full")):
        p = str(tmp_path / ("m%d.csv" % i))
        with open(p, "w", newline="") as f:
            f.write(str(d[key]))
        paths.append(p)
    paths.insert(1, str(tmp_path / "missing.csv"))            # skipped, like os.path.exists in the reference
    avg, last = ce.average_eval_metrics(paths)
    # get_evaluation_numbers_ours.py:6-29 with pandas
    acc, n = {}, 0
    for p in paths:
        if not os.path.exists(p):
            continue
        df = pd.read_csv(p).fillna(0).to_numpy()
        n += 1
        for row in df:
            acc[row[0]] = acc.get(row[0], 0) + row[1:].astype(np.float64)
    # (the reference divides every row by the number of files, also a row only some files have)
    assert set(avg) == set(acc)
    for k in acc:
        np.testing.assert_allclose(avg[k], acc[k] / n, rtol=0, atol=1e-12)
        assert last[k] == avg[k][-1]
    with pytest.raises(ValueError):
        ce.average_eval_metrics([str(tmp_path / "missing.csv")])


def test_natural_sort():
    assert ce.natural_sorted(["cam10.png", "cam2.png", "cam1.png"]) == ["cam1.png", "cam2.png", "cam10.png"]
    assert ce.natural_sorted(["b1", "a10", "a9", "a"]) == ["a", "a9", "a10", "b1"]
    assert ce.natural_sorted(["10", "9", "x"]) == ["9", "10", "x"]


def test_argument_checks_without_gpu():
    from manus_amd._lib import lib
    L = lib()
    assert L.mgr_ceval_workspace_bytes(1, 1080, 1080) > 1080 * 1080 * 4
    assert L.mgr_ceval_workspace_bytes(0, 8, 8) == 0 and L.mgr_ceval_workspace_bytes(1, 20000, 8) == 0
    assert L.mgr_ceval_masks(1, 0, 8, None, 0, None, None, None, None, None, None, None) != 0
    assert L.mgr_ceval_masks(1, 8, 8, None, 0, None, None, None, None, None, None, None) != 0
    assert L.mgr_ceval_labels(1, 8, 8, None, 8, None, None, None, 0, None) != 0
    assert L.mgr_ceval_fill(1, 8, 8, None, None, None, 0, None) != 0
    assert L.mgr_ceval_counts(1, 8, 8, None, None, None, None, None, 0, None) != 0
    assert L.mgr_ceval_collage(1, 8, 8, 17, None, None, None, None, None) != 0
    assert b"mgr_ceval_collage" in L.mgr_last_error()
    with pytest.raises(ValueError):
        ce.ContactEvaluator("/nonexistent").end()


def test_morphology_stand_ins_against_scipy(golden_dir):
    """The maker's erode / dilate (the OpenCV stand-ins behind the fixture's labels) against scipy.ndimage with the cross
    and border_value 1 / 0, on the fixture's own palette masks and on noise; and the fixture's unfilled labels rebuilt
    from scipy's morphology."""
    import scipy.ndimage as ndi
    spec = importlib.util.spec_from_file_location("make_contact_eval_golden_standins", os.path.join(golden_dir, "make_contact_eval_golden.py"))
    src = open(spec.origin).read()
    # only the stand-ins: the part of the file in front of the reference import machinery
    ns = {"np": np}
    start, stop = src.index("CROSS = np.array"), src.index("def make_cv2")
    exec(compile(src[start:stop], spec.origin, "exec"), ns)
    cross = ndi.generate_binary_structure(2, 1)
    assert np.array_equal(ns["CROSS"].astype(bool), cross)
    g = np.random.default_rng(5)
    masks = [((g.random((33, 47)) < p) * 255).astype(np.uint8) for p in (0.3, 0.7, 0.95)]
    d = _golden(golden_dir)
    for k in range(int(d["n"])):
        skin = d["frame%d" % k][:, :d["seg%d" % k].shape[1]]
        stack = [np.zeros(skin.shape[:2], np.uint8)]
        for c in ce.PALETTE.astype(np.float32):
            m = ns["in_range"](skin, c - 10, c + 10)
            assert np.array_equal(m == 255, (np.abs(skin.astype(np.int64) - c.astype(np.int64)) <= 10).all(axis=-1))
            masks.append(m)
            e = ndi.binary_erosion(m == 255, cross, border_value=1)
            stack.append(ndi.binary_dilation(e, cross, border_value=0).astype(np.uint8) * 255)
        labels = np.argmax(np.stack(stack, axis=-1), axis=-1) * d["hand%d" % k]
        assert np.array_equal(labels, d["labels_unfilled%d" % k]), k
    for m in masks:
        e = ns["erode"](m, ns["CROSS"])
        assert np.array_equal(e == 255, ndi.binary_erosion(m == 255, cross, border_value=1))
        assert np.array_equal(ns["dilate"](e, ns["CROSS"]) == 255, ndi.binary_dilation(e == 255, cross, border_value=0))

"""CPU: the restatement of the contact-evaluation chain (contact_eval_ref.py) against the reference's own outputs
(tests/golden/contact_eval.npz), and the conditions of the edge cases (contact_eval_cases.py) proved on that restatement
alone, so that no case of tests/test_gpu_contact_eval_edges.py passes vacuously.  Every test prints what it counted."""
import os

import numpy as np
import pytest

import contact_eval_cases as cases
import contact_eval_ref as ref
from manus_amd.contact_eval import PALETTE

_CACHE = {}


def _chain(size):
    """the chain case of a size with the restatement's outputs, computed once"""
    if size not in _CACHE:
        frame, seg, rgba = cases.chain_case(*size)
        W = size[2]
        pred, gt, hand, f8 = ref.masks_ref(frame, seg, rgba)
        skin = frame[:, :, :W]
        _CACHE[size] = dict(frame=frame, seg=seg, rgba=rgba, skin=skin, pred=pred, gt=gt, hand=hand, unfilled=ref.labels_ref(skin, hand))
    return _CACHE[size]


def _fill(name):
    if name not in _CACHE:
        frame, hand = cases.fill_case(name)
        _CACHE[name] = dict(frame=frame, hand=hand, unfilled=ref.labels_ref(frame, hand))
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------------------------------
# anchor
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_outputs(golden_dir):
    d = np.load(os.path.join(golden_dir, "contact_eval.npz"))
    for k in range(int(d["n"])):
        frame, seg, rgba = d["frame%d" % k], d["seg%d" % k], d["rgba%d" % k]
        W = seg.shape[1]
        pred, gt, hand, f8 = ref.masks_ref(frame, seg, rgba)
        assert np.array_equal(pred * 255, d["pred%d" % k]) and np.array_equal(gt * 255, d["gt%d" % k]), k
        assert np.array_equal(hand.astype(bool), d["hand%d" % k]) and f8 is frame, k
        unfilled = ref.labels_ref(frame[:, :W], hand)
        assert np.array_equal(unfilled, d["labels_unfilled%d" % k]), k
        labels = ref.fill_ref(unfilled, hand)
        assert np.array_equal(labels, d["labels%d" % k]), k
        masks = (pred, d["mano_mask%d" % k], d["harp_mask%d" % k])
        for j, m in enumerate(masks):
            c = ref.counts_ref(m, gt, labels)
            assert c.dtype == np.int64 and np.array_equal(c, d["counts%d" % k][j]), (k, j)
            iou, f1 = ref.scores_ref(c)
            np.testing.assert_allclose(iou, d["iou%d" % k][j], rtol=0, atol=1e-9)
            np.testing.assert_allclose(f1, d["f1%d" % k][j], rtol=0, atol=1e-9, equal_nan=True)
        assert np.array_equal(ref.collage_ref(rgba, [gt, pred]), d["row%d" % k]), k
        assert np.array_equal(ref.collage_ref(rgba, [gt, masks[1], masks[2], pred]), d["row5%d" % k]), k
        res = int(((hand > 0) & (unfilled == 0)).sum())
        print("camera %d %s: %d labelled, %d residual pixels" % (k, seg.shape[:2], int((unfilled > 0).sum()), res))
        assert res > 0


def test_restatement_batches_like_single_images():
    c = _chain((2, 17, 65))
    for v in range(2):
        one = ref.masks_ref(c["frame"][v], c["seg"][v], c["rgba"][v])
        for a, b in zip(one[:3], (c["pred"][v], c["gt"][v], c["hand"][v])):
            assert np.array_equal(a, b)
        assert np.array_equal(ref.labels_ref(c["skin"][v], c["hand"][v]), c["unfilled"][v])
    f = np.array([[[np.nan, -0.0, 1.7], [0.5, 128 / 255, np.inf]]], np.float32)
    assert ref.frame_bytes_ref(f).tolist() == [[[0, 0, 255], [127, int(np.float32(128 / 255) * np.float32(255)), 255]]]
    with pytest.raises(ValueError):
        ref.fill_ref(np.zeros((3, 3), np.uint8), np.ones((3, 3), np.uint8))
    assert np.array_equal(ref.fill_ref(np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint8)), np.zeros((3, 3), np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# chain cases
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_cases_hold_every_label_the_overlap_and_the_box_faces():
    seen = np.zeros(17, np.int64)
    both = two = 0
    at = {10: 0, -10: 0, 11: 0, -11: 0}
    for size in cases.CHAIN_SIZES:
        c = _chain(size)
        V, H, W = size
        assert c["frame"].shape == (V, H, 2 * W, 3) and c["seg"].shape == (V, H, W, 3) and c["rgba"].shape == (V, H, W, 4)
        seen += np.bincount(c["unfilled"].reshape(-1), minlength=17)
        for v in range(V):
            m = ref.palette_matches(c["skin"][v])
            lab = c["unfilled"][v] > 0
            both += int((m[2] & m[15] & lab).sum())
            two += int((ref.opened_masks(c["skin"][v]).sum(axis=0) >= 2).sum())
            diff = c["skin"][v].astype(np.int64)[None] - PALETTE.astype(np.int64)[:, None, None, :]      # (16,H,W,3)
            worst = np.abs(diff).max(axis=-1)
            for s in (10, 11):                              # a pixel on a box's face / one step off it, by its extreme channel
                sel = worst == s
                at[s] += int(((diff == s).any(axis=-1) & sel).sum())
                at[-s] += int(((diff == -s).any(axis=-1) & sel).sum())
            # a pixel on a face is matched, one step off is not
            assert (m[worst == 10]).all() and not (m[worst == 11]).any()
            # residual pixels never stand without a labelled one (the chain fills every case)
            if ((c["hand"][v] > 0) & ~lab).any():
                assert lab.any(), (size, v)
    print("labels 0..16 over the chain cases:", seen.tolist())
    print("labelled pixels matching entries 3 and 16 both: %d; pixels under two dilated masks: %d" % (both, two))
    print("pixels at offset +10 / -10 / +11 / -11 of a box:", at[10], at[-10], at[11], at[-11])
    assert (seen[1:] > 0).all()
    assert both > 0 and two > 0
    assert min(at.values()) > 0
    masks = [_chain(s) for s in cases.CHAIN_SIZES]
    full = sum(int(c["hand"][v].all()) for c in masks for v in range(c["hand"].shape[0]))
    empty = sum(int(not c["hand"][v].any()) for c in masks for v in range(c["hand"].shape[0]))
    print("views with a full hand: %d, with an empty hand: %d" % (full, empty))
    assert full >= 1 and empty >= 1
    for key, src in (("pred", "frame"), ("gt", "seg")):     # 127 / 128 / 129 on the deciding channel
        n = {b: 0 for b in (127, 128, 129)}
        for size, c in zip(cases.CHAIN_SIZES, masks):
            img = c["frame"][:, :, size[2]:] if key == "pred" else c["seg"]
            low = img.min(axis=-1)
            for b in n:
                n[b] += int((low == b).sum())
            assert np.array_equal(c[key], (low >= 128).astype(np.uint8))
        print("%s: pixels whose least channel is 127 / 128 / 129:" % key, n)
        assert min(n.values()) > 0
    alpha = {b: sum(int((c["rgba"][..., 3] == b).sum()) for c in masks) for b in (0, 127, 128, 129, 255)}
    print("alpha bytes:", alpha)
    assert min(alpha.values()) > 0


def test_chain_cases_reach_the_borders_and_both_sides_of_the_seams():
    rows = {"row 0": 0, "row H-1": 0, "col 0": 0, "col W-1": 0}
    for size in cases.CHAIN_SIZES:
        V, H, W = size
        u = _chain(size)["unfilled"] > 0
        rows["row 0"] += int(u[:, 0].sum())
        rows["row H-1"] += int(u[:, H - 1].sum())
        rows["col 0"] += int(u[:, :, 0].sum())
        rows["col W-1"] += int(u[:, :, W - 1].sum())
        if min(H, W) >= 3:
            assert u[:, 0].any() and u[:, H - 1].any() and u[:, :, 0].any() and u[:, :, W - 1].any(), size
        for e in range(16, W, 16):                          # every tile edge, x = 63|64 among them
            n = (int(u[:, :, e - 1].sum()), int(u[:, :, e].sum()))
            print(size, "labelled pixels in columns %d | %d:" % (e - 1, e), n)
            assert min(n) > 0, (size, e)
        for e in range(16, H, 16):
            n = (int(u[:, e - 1].sum()), int(u[:, e].sum()))
            print(size, "labelled pixels in rows %d | %d:" % (e - 1, e), n)
            assert min(n) > 0, (size, e)
    print("labelled pixels on the borders:", rows)
    assert min(rows.values()) > 0
    assert any(s[2] >= 65 for s in cases.CHAIN_SIZES) and any(s[1] >= 17 for s in cases.CHAIN_SIZES)


def test_border_values_of_the_morphology_matter():
    n_e = n_d = 0
    for size in cases.CHAIN_SIZES:
        c = _chain(size)
        e = int((ref.labels_ref(c["skin"], c["hand"], erode_border=0) != c["unfilled"]).sum())
        d = int((ref.labels_ref(c["skin"], c["hand"], dilate_border=1) != c["unfilled"]).sum())
        print(size, "labels changed by the other erosion border: %d, by the other dilation border: %d" % (e, d))
        n_e += e > 0
        n_d += d > 0
    assert n_e >= 1 and n_d >= 1


# ---------------------------------------------------------------------------------------------------------------------
# fill cases
# ---------------------------------------------------------------------------------------------------------------------
def _ring_break_pixels(unfilled, hand):
    """residual pixels whose nearest labelled pixels tie in d^2 across tiles with different labels, the winner (lower index)
    in a later ring of tiles than a loser"""
    H, W = unfilled.shape
    lab = np.argwhere(unfilled > 0).astype(np.int64)
    n = 0
    for y, x in np.argwhere((hand > 0) & (unfilled == 0)):
        d2 = (lab[:, 0] - y) ** 2 + (lab[:, 1] - x) ** 2
        near = lab[d2 == d2.min()]                          # row-major: near[0] wins
        ring = np.maximum(np.abs(near[:, 0] // 16 - y // 16), np.abs(near[:, 1] // 16 - x // 16))
        label = unfilled[near[:, 0], near[:, 1]]
        n += bool(((label != label[0]) & (ring < ring[0])).any())
    return n


def test_fill_cases_hold_ring_breaks_a_far_box_and_a_second_trip():
    n_ties = 0
    for name in ("ties-48x80", "ties-33x130"):
        c = _fill(name)
        n = _ring_break_pixels(c["unfilled"][0], c["hand"][0])
        res = int(((c["hand"][0] > 0) & (c["unfilled"][0] == 0)).sum())
        print("%s: %d labelled, %d residual pixels, %d of them ring breaks" % (name, int((c["unfilled"][0] > 0).sum()), res, n))
        n_ties += n
    assert n_ties >= 16
    c = _fill("far-box")
    u, h = c["unfilled"][0], c["hand"][0]
    ty, tx = np.nonzero(u > 0)[0] // 16, np.nonzero(u > 0)[1] // 16
    ry, rx = np.nonzero((h > 0) & (u == 0))
    first = np.maximum(np.maximum(tx.min() - rx // 16, rx // 16 - tx.max()), np.maximum(np.maximum(ty.min() - ry // 16, ry // 16 - ty.max()), 0))
    print("far-box: %d residual pixels, first ring %d .. %d" % (len(ry), first.min(), first.max()))
    assert len(ry) == 40 * 16 and first.min() >= 10
    for name, n_lab in (("corner-16", 3), ("corner-17", 3), ("corner-5x7", 3)):
        c = _fill(name)
        assert int((c["unfilled"] > 0).sum()) == n_lab, name
        assert int(((c["hand"] > 0) & (c["unfilled"] == 0)).sum()) == c["hand"].size - n_lab
    c = _fill("every-pixel")
    res = int(((c["hand"] > 0) & (c["unfilled"] == 0)).sum())
    print("every-pixel: %d labelled, %d residual pixels (the grid stride is %d)" % (int((c["unfilled"] > 0).sum()), res, 1024 * 256))
    assert res > 262144 and len(set(c["unfilled"][c["unfilled"] > 0].tolist())) == 2
    c = _fill("mixed-batch")
    u, h = c["unfilled"], c["hand"]
    assert (u[0] > 0).any() and ((h[0] > 0) & (u[0] == 0)).any()
    assert not (u[1] > 0).any() and (h[1] > 0).any()
    assert not (u[2] > 0).any() and not (h[2] > 0).any()
    ref.fill_ref(u[0], h[0])
    ref.fill_ref(u[2], h[2])
    with pytest.raises(ValueError):
        ref.fill_ref(u[1], h[1])


def test_integer_rule_equals_the_fp32_scan_below_2048_px():
    """The reference scans np.argwhere order for a strictly smaller fp32 root.  float32 sqrt over the integers is strictly
    increasing up to n = 4197200 (just above 2^22) and non-decreasing beyond, so the first least root is the first least
    d^2 whenever the winning d^2 is below that: a nearest labelled pixel closer than 2048 px."""
    n = np.arange(0, 4197300, dtype=np.float32)             # exact: below 2^24
    s = np.sqrt(n)
    assert s.dtype == np.float32
    flat = np.nonzero(s[1:] == s[:-1])[0]
    print("first n with sqrt32(n) == sqrt32(n + 1):", int(flat[0]))
    assert int(flat[0]) == 4197200 and (s[1:] >= s[:-1]).all()
    assert 2048 ** 2 - 1 < 4197200 < 2049 ** 2
    # and on a case: the scan as the reference does it, in fp32, against the integer rule
    c = _fill("ties-48x80")
    u, h = c["unfilled"][0], c["hand"][0]
    lab = np.argwhere(u > 0)
    want = ref.fill_ref(u, h)
    for y, x in np.argwhere((h > 0) & (u == 0)):
        root = np.sqrt(((lab - (y, x)) ** 2).sum(axis=1).astype(np.float32))
        first = lab[int(np.argmin(root))]                   # argmin: the first of equal minima, the strict '<' scan
        assert want[y, x] == u[first[0], first[1]]


def test_labels_entry_refuses_a_frame_off_a_dword():
    """k_ceval_labels stages rows with dword loads, so the entry refuses a frame pointer off a dword before it launches
    anything (skin_labels realigns such a frame with a copy: test_gpu_contact_eval_edges.py).  At (3,65,97) a camera's frame
    has 65 * 194 * 3 bytes, its left half 65 * 97 * 3: no multiples of 4, so frames[1:] of a stacked tensor is such a pointer."""
    from manus_amd._lib import lib
    L = lib()
    assert (65 * 194 * 3) % 4 == 2 and (65 * 97 * 3) % 4 == 3
    for off in (1, 2, 3):                                   # (no memory behind these addresses: refused before any use)
        assert L.mgr_ceval_labels(1, 8, 8, 4096 + off, 8, None, 8192, 16384, 1 << 20, None) != 0
        assert b"mgr_ceval_labels: frame not 4-byte aligned" in L.mgr_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# counts, collage, fp32 frame
# ---------------------------------------------------------------------------------------------------------------------
def test_count_cases_need_a_second_fold_trip_and_hold_labels_0_and_16():
    for size in cases.COUNT_SIZES:
        V, H, W = size
        pred, gt, labels = cases.count_case(*size)
        records = -(-H * W // 4096)
        on = (pred | gt) > 0
        print(size, "records per view: %d, pixels under pred | gt with label 0: %d, with label 16: %d, values" % (
            records, int((on & (labels == 0)).sum()), int((on & (labels == 16)).sum())), sorted(set(pred.ravel().tolist()) | set(gt.ravel().tolist())))
        if H * W > 4096 * 16:
            assert records > 16 and (on & (labels == 0)).any() and (on & (labels == 16)).any()
        c = ref.counts_ref(pred, gt, labels)
        assert c.shape == (V, 17, 3) and (c[:, 16, 0] <= c[:, 16, 1]).all()
        if V == 3:
            assert not c[1].any() and c[0].any() and c[2].any()
    big = [s for s in cases.COUNT_SIZES if s[1] * s[2] > 4096 * 16]
    assert len(big) == 2 and (big[0][1] * big[0][2]) % 4 == 0 and (big[1][1] * big[1][2]) % 2 == 1


def test_collage_and_fp32_cases_cover_their_thresholds():
    rgba, masks = cases.collage_case(1, 16, 64, 16)
    al = rgba[0, ..., 3] > 128
    for c in range(3):
        assert len(set(rgba[0, ..., c][al].tolist())) == 256 and len(set(rgba[0, ..., c][~al].tolist())) == 256
    assert set(rgba[..., 3].ravel().tolist()) == {127, 128, 129, 255} and set(masks.ravel().tolist()) == {0, 1, 255}
    small = cases.collage_case(2, 3, 5, 1)[0]
    assert set(small[..., 3].ravel().tolist()) <= {0, 127, 128, 129, 255}
    for V, H, W in cases.COLLAGE_SIZES:
        for M in cases.COLLAGE_M:
            rgba, masks = cases.collage_case(V, H, W, M)
            assert ref.collage_ref(rgba, masks).shape == (V, H, (1 + M) * W, 3)
    frame, seg, rgba, vals = cases.f32_frame_case()
    assert frame.dtype == np.float32 and frame.shape == (1, 8, 256, 3)
    for half in (frame[:, :, :128], frame[:, :, 128:]):
        flat = half.reshape(-1)
        assert np.isnan(flat).any() and np.isinf(flat).any()
        have = set(flat[~np.isnan(flat)].view(np.uint32).tolist())
        assert set(vals[~np.isnan(vals)].view(np.uint32).tolist()) <= have
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    at, below, above = (ref.frame_bytes_ref(x) for x in (k, np.nextafter(k, np.float32(-2)), np.nextafter(k, np.float32(2))))
    print("k / 255 -> byte k - 1: %d values of k; the fp32 below drops a byte: %d; the fp32 above gains one: %d"
          % (int((at.astype(int) == np.arange(256) - 1).sum()), int((below < at).sum()), int((above > at).sum())))
    assert int((below < at).sum()) > 0                      # the conversion's truncation is decided one ulp apart
    assert np.abs(at.astype(int) - np.arange(256)).max() <= 1

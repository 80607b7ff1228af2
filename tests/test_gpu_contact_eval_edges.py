"""GPU: the contact-evaluation kernels (csrc/contact_eval.hip) at seams, borders, ties and ragged sizes against the plain
restatement of the chain (contact_eval_ref.py, anchored on the reference's outputs by test_contact_eval_cases_cpu.py) on
the cases of contact_eval_cases.py, whose conditions that CPU test proves.

Bounds: everything is an integer and must be EQUAL.  Scores within 1e-9 absolute of the same expression on the
restatement's counts, NaN where that has NaN (float64 on both sides)."""
import os

import numpy as np
import pytest
import torch

import contact_eval_cases as cases
import contact_eval_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _ids(xs):
    return ["x".join(str(i) for i in x) if isinstance(x, tuple) else str(x) for x in xs]


def _offset(t, k):
    """the bytes of a uint8 device tensor, k bytes into a larger buffer"""
    buf = torch.empty(t.numel() + 8, dtype=torch.uint8, device=t.device)
    assert buf.data_ptr() % 4 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == k % 4 and v.is_contiguous()
    return v


def _c_labels(frame, row_px, hand, V, H, W, labels=None, poison=False, fill=True):
    """mgr_ceval_labels (+ mgr_ceval_fill) through lib(): (unfilled, filled, flags) on the host."""
    from manus_amd._lib import check, lib, stream
    L = lib()
    n = int(L.mgr_ceval_workspace_bytes(V, H, W))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    if poison:
        ws.fill_(0xFF)
    if labels is None:
        labels = torch.empty((V, H, W), dtype=torch.uint8, device=DEV)
    assert frame.numel() == V * H * row_px * 3 and frame.is_contiguous() and labels.is_contiguous()
    assert hand is None or (hand.is_contiguous() and tuple(hand.shape) == (V, H, W))
    check(L.mgr_ceval_labels(V, H, W, frame.data_ptr(), row_px, None if hand is None else hand.data_ptr(), labels.data_ptr(),
                             ws.data_ptr(), n, stream()), "mgr_ceval_labels")
    unfilled = host(labels).copy()
    if not fill:
        return unfilled, None, None
    flags = torch.full((V,), 7, dtype=torch.int32, device=DEV)
    check(L.mgr_ceval_fill(V, H, W, labels.data_ptr(), flags.data_ptr(), ws.data_ptr(), n, stream()), "mgr_ceval_fill")
    return unfilled, host(labels), host(flags)


def _c_counts(pred, gt, labels, poison=False):
    from manus_amd._lib import check, lib, stream
    L = lib()
    V, H, W = pred.shape
    n = int(L.mgr_ceval_workspace_bytes(V, H, W))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    if poison:
        ws.fill_(0xFF)
    counts = torch.empty((V, 17, 3), dtype=torch.int64, device=DEV)
    check(L.mgr_ceval_counts(V, H, W, pred.data_ptr(), gt.data_ptr(), labels.data_ptr(), counts.data_ptr(), ws.data_ptr(), n, stream()),
          "mgr_ceval_counts")
    return host(counts)


def _assert_scores(ce, counts, want_counts):
    iou, f1 = ce.scores_from_counts(counts)
    ref_iou, ref_f1 = ref.scores_ref(want_counts)
    np.testing.assert_allclose(iou, ref_iou, rtol=0, atol=1e-9)
    np.testing.assert_allclose(f1, ref_f1, rtol=0, atol=1e-9, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# the chain per case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.CHAIN_SIZES, ids=_ids(cases.CHAIN_SIZES))
def test_chain_equals_the_restatement(size):
    from manus_amd import contact_eval as ce
    V, H, W = size
    frame, seg, rgba = cases.chain_case(V, H, W)
    w_pred, w_gt, w_hand, _ = ref.masks_ref(frame, seg, rgba)
    w_unfilled = ref.labels_ref(frame[:, :, :W], w_hand)
    w_labels = ref.fill_ref(w_unfilled, w_hand)
    w_counts = ref.counts_ref(w_pred, w_gt, w_labels)
    w_row = ref.collage_ref(rgba, [w_gt, w_pred])
    first = None
    for run in range(2):
        pred, gt, hand, f8 = ce.contact_masks(frame, seg, rgba)
        np.testing.assert_array_equal(host(pred), w_pred)
        np.testing.assert_array_equal(host(gt), w_gt)
        np.testing.assert_array_equal(host(hand), w_hand)
        np.testing.assert_array_equal(host(f8), frame)
        outs = [pred, gt, hand]
        for fr in (f8, f8[:, :, :W].contiguous()):              # the whole frame read in place, and the left half on its own
            labels, unfilled = ce.skin_labels(fr, hand, return_unfilled=True)
            np.testing.assert_array_equal(host(unfilled), w_unfilled)
            np.testing.assert_array_equal(host(labels), w_labels)
            outs += [labels, unfilled]
        counts = ce.contact_counts(pred, gt, labels)
        assert counts.dtype == torch.int64
        np.testing.assert_array_equal(host(counts), w_counts)
        _assert_scores(ce, counts, w_counts)
        row = ce.collage_rows(rgba, [gt, pred])
        np.testing.assert_array_equal(host(row), w_row)
        outs += [counts, row]
        if first is None:
            first = outs
        else:
            for a, b in zip(first, outs):
                assert torch.equal(a, b)
    n_res = int(((w_hand > 0) & (w_unfilled == 0)).sum())
    print(size, "%d labelled, %d residual pixels, %d labels" % (int((w_unfilled > 0).sum()), n_res, len(set(w_labels.ravel().tolist()))))


def test_fp32_frame_bytes_next_to_k_over_255():
    from manus_amd import contact_eval as ce
    frame, seg, rgba, _ = cases.f32_frame_case()
    w_pred, w_gt, w_hand, w_f8 = ref.masks_ref(frame, seg, rgba)
    for run in range(2):
        pred, gt, hand, f8 = ce.contact_masks(dev(frame), seg, rgba)
        assert f8.dtype == torch.uint8
        bad = np.argwhere(host(f8) != w_f8)
        assert len(bad) == 0, (len(bad), [(frame[tuple(b)], int(host(f8)[tuple(b)]), int(w_f8[tuple(b)])) for b in bad[:8]])
        np.testing.assert_array_equal(host(pred), w_pred)
        np.testing.assert_array_equal(host(gt), w_gt)
        np.testing.assert_array_equal(host(hand), w_hand)


# ---------------------------------------------------------------------------------------------------------------------
# the fill
# ---------------------------------------------------------------------------------------------------------------------
_PLAIN_FILL = [n for n in cases.FILL_CASES if n != "mixed-batch"]


@pytest.mark.parametrize("name", _PLAIN_FILL)
def test_fill_equals_brute_force(name):
    from manus_amd import contact_eval as ce
    frame, hand = cases.fill_case(name)
    w_unfilled = ref.labels_ref(frame, hand)
    w_labels = ref.fill_ref(w_unfilled, hand)
    f, h = dev(frame), dev(hand)
    labels, unfilled = ce.skin_labels(f, h, return_unfilled=True)
    np.testing.assert_array_equal(host(unfilled), w_unfilled)
    got = host(labels)
    bad = np.argwhere(got != w_labels)
    assert len(bad) == 0, (name, len(bad), [(tuple(b), int(got[tuple(b)]), int(w_labels[tuple(b)])) for b in bad[:8]])
    assert torch.equal(ce.skin_labels(f, h), labels)
    assert (got[hand > 0] > 0).all() and (got[hand == 0] == 0).all()


def test_mixed_batch_flags_the_view_without_labels_only():
    from manus_amd import contact_eval as ce
    frame, hand = cases.fill_case("mixed-batch")
    V, H, W = hand.shape
    w_unfilled = ref.labels_ref(frame, hand)
    with pytest.raises(ValueError, match=r"view\(s\) 1 have"):
        ce.skin_labels(frame, hand)
    np.testing.assert_array_equal(host(ce.skin_labels(frame, hand, fill=False)), w_unfilled)
    for poison in (False, True):
        unfilled, labels, flags = _c_labels(dev(frame), W, dev(hand), V, H, W, poison=poison)
        np.testing.assert_array_equal(unfilled, w_unfilled)
        assert flags.tolist() == [0, 1, 0]
        np.testing.assert_array_equal(labels[0], ref.fill_ref(w_unfilled[0], hand[0]))
        np.testing.assert_array_equal(labels[1], unfilled[1])           # left as the labels kernel wrote it
        np.testing.assert_array_equal(labels[2], ref.fill_ref(w_unfilled[2], hand[2]))
        assert not labels[1].any() and not labels[2].any()


# ---------------------------------------------------------------------------------------------------------------------
# counts and collage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.COUNT_SIZES, ids=_ids(cases.COUNT_SIZES))
def test_counts_equal_the_restatement(size):
    from manus_amd import contact_eval as ce
    pred, gt, labels = cases.count_case(*size)
    want = ref.counts_ref(pred, gt, labels)
    p, g, l = dev(pred), dev(gt), dev(labels)
    counts = ce.contact_counts(p, g, l)
    np.testing.assert_array_equal(host(counts), want)
    _assert_scores(ce, counts, want)
    assert torch.equal(ce.contact_counts(p, g, l), counts)
    np.testing.assert_array_equal(_c_counts(p, g, l, poison=True), want)
    for k in (1, 2, 3):                                          # the byte route, from every alignment
        np.testing.assert_array_equal(host(ce.contact_counts(_offset(p, k), _offset(g, (k + 1) % 4), _offset(l, (k + 2) % 4))), want)


_COLLAGE = [(s, M) for s in cases.COLLAGE_SIZES for M in cases.COLLAGE_M]


@pytest.mark.parametrize("size,M", _COLLAGE, ids=["%s-M%d" % ("x".join(map(str, s)), M) for s, M in _COLLAGE])
def test_collage_equals_the_restatement(size, M):
    from manus_amd import contact_eval as ce
    rgba, masks = cases.collage_case(*size, M)
    want = ref.collage_ref(rgba, masks)
    assert want.shape == (size[0], size[1], (1 + M) * size[2], 3)
    as_list = ce.collage_rows(rgba, [dev(m) for m in masks])
    np.testing.assert_array_equal(host(as_list), want)
    if M:
        assert torch.equal(ce.collage_rows(dev(rgba), dev(masks)), as_list)
    assert torch.equal(ce.collage_rows(rgba, [dev(m) for m in masks]), as_list)


# ---------------------------------------------------------------------------------------------------------------------
# C entries the wrappers never reach
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(2, 17, 65), (1, 16, 64)], ids=_ids([(2, 17, 65), (1, 16, 64)]))
def test_labels_entry_with_other_row_strides_and_without_a_hand(size):
    V, H, W = size
    frame, seg, rgba = cases.chain_case(V, H, W)
    skin = frame[:, :, :W]
    hand = ref.masks_ref(frame, seg, rgba)[2]
    ones = np.ones_like(hand)
    w_unfilled, w_open = ref.labels_ref(skin, hand), ref.labels_ref(skin, ones)
    w_labels, w_flags = ref.fill_ref(w_unfilled, hand), [0] * V
    w_open_filled = ref.fill_ref(w_open, ones)
    assert (w_open != w_unfilled).any()
    g = np.random.default_rng(9)
    for row_px in (W, W + 1, W + 3, 2 * W):
        buf = g.integers(0, 256, (V, H, row_px, 3)).astype(np.uint8)    # whatever stands right of the first W pixels is not read
        buf[:, :, :W] = skin
        f = dev(buf)
        unfilled, labels, flags = _c_labels(f, row_px, dev(hand), V, H, W)
        np.testing.assert_array_equal(unfilled, w_unfilled, err_msg="row_px %d" % row_px)
        np.testing.assert_array_equal(labels, w_labels, err_msg="row_px %d" % row_px)
        assert flags.tolist() == w_flags
        unfilled, labels, flags = _c_labels(f, row_px, None, V, H, W, poison=True)      # hand = NULL: every pixel inside
        np.testing.assert_array_equal(unfilled, w_open, err_msg="row_px %d, no hand" % row_px)
        np.testing.assert_array_equal(labels, w_open_filled, err_msg="row_px %d, no hand" % row_px)
        assert flags.tolist() == [0] * V
        same = _c_labels(f, row_px, dev(ones), V, H, W)
        np.testing.assert_array_equal(same[0], unfilled)
        np.testing.assert_array_equal(same[1], labels)


@pytest.mark.parametrize("size", [(2, 16, 64), (2, 17, 68)], ids=_ids([(2, 16, 64), (2, 17, 68)]))
def test_unaligned_hand_and_labels_give_the_aligned_bytes(size):
    """W % 4 == 0: the dword route when hand and labels are aligned, the byte route when either is not."""
    from manus_amd import contact_eval as ce
    V, H, W = size
    g = np.random.default_rng(V * 1000 + H * 100 + W)
    frame = np.stack([cases._skin(g, H, W, 3 + v) for v in range(V)])
    hand = (~cases._blob(g, H, W, 0.05, 0.18)).astype(np.uint8)[None].repeat(V, axis=0)
    w_unfilled = ref.labels_ref(frame, hand)
    w_labels = ref.fill_ref(w_unfilled, hand)
    assert ((hand > 0) & (w_unfilled == 0)).any() and (hand == 0).any()
    f, h = dev(frame), dev(hand)
    unfilled, labels, flags = _c_labels(f, W, h, V, H, W)
    np.testing.assert_array_equal(unfilled, w_unfilled)
    np.testing.assert_array_equal(labels, w_labels)
    for k in (1, 2, 3):
        out = _offset(torch.zeros((V, H, W), dtype=torch.uint8, device=DEV), k)
        for hh, ll in ((_offset(h, k), None), (h, out), (_offset(h, 4 - k), out)):
            u2, l2, f2 = _c_labels(f, W, hh, V, H, W, labels=ll)
            np.testing.assert_array_equal(u2, unfilled)
            np.testing.assert_array_equal(l2, labels)
            assert f2.tolist() == flags.tolist()
        np.testing.assert_array_equal(host(ce.skin_labels(f, _offset(h, k))), w_labels)
    pred, gt = dev(g.choice(np.array([0, 1, 255], np.uint8), (V, H, W))), dev(g.choice(np.array([0, 1, 255], np.uint8), (V, H, W)))
    lab = dev(labels)
    want = ref.counts_ref(host(pred), host(gt), labels)
    np.testing.assert_array_equal(host(ce.contact_counts(pred, gt, lab)), want)
    for k in (1, 2, 3):
        for a, b, c in ((_offset(pred, k), gt, lab), (pred, _offset(gt, k), lab), (pred, gt, _offset(lab, k))):
            np.testing.assert_array_equal(host(ce.contact_counts(a, b, c)), want)


# ---------------------------------------------------------------------------------------------------------------------
# the wrapper on slices of a stacked tensor
# ---------------------------------------------------------------------------------------------------------------------
def test_views_of_a_stacked_frame_tensor_score_like_the_batch(golden_dir, tmp_path):
    """(3,65,97): 65 * 194 * 3 and 65 * 97 * 3 are no multiples of 4, so frames[k:] of a stacked uint8 tensor starts off a dword
    for some k.  mgr_ceval_labels refuses such a pointer (it stages rows with dword loads); skin_labels realigns with a copy."""
    from manus_amd import contact_eval as ce
    from manus_amd._lib import lib
    d = np.load(os.path.join(golden_dir, "contact_eval.npz"))
    ks = list(range(int(d["n_main"])))
    frame = dev(np.stack([d["frame%d" % k] for k in ks]))
    seg = dev(np.stack([d["seg%d" % k] for k in ks]))
    rgba = dev(np.stack([d["rgba%d" % k] for k in ks]))
    V, H, W = seg.shape[:3]
    assert (V, H, W) == (3, 65, 97)
    pred, gt, hand, f8 = ce.contact_masks(frame, seg, rgba)
    assert f8.data_ptr() == frame.data_ptr()
    off = 0
    for fr in (f8, f8[:, :, :W].contiguous()):
        batch = ce.skin_labels(fr, hand)
        np.testing.assert_array_equal(host(batch), np.stack([d["labels%d" % k] for k in ks]))
        for k in ks:
            one = fr[k:k + 1]
            off += one.data_ptr() % 4 != 0
            if one.data_ptr() % 4:                                  # the C refusal stays
                n = int(lib().mgr_ceval_workspace_bytes(1, H, W))
                ws, out = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty((1, H, W), dtype=torch.uint8, device=DEV)
                assert lib().mgr_ceval_labels(1, H, W, one.data_ptr(), int(one.shape[2]), None, out.data_ptr(), ws.data_ptr(), n, None) != 0
                assert b"4-byte aligned" in lib().mgr_last_error()
            assert torch.equal(ce.skin_labels(one, hand[k:k + 1]), batch[k:k + 1]), k
    assert off >= 2
    names = ["cam%d" % k for k in ks]
    whole = ce.ContactEvaluator(str(tmp_path / "batch"))
    whole.add(names, frame, seg, rgba)
    single = ce.ContactEvaluator(str(tmp_path / "single"))
    for k in ks:
        single.add(names[k], frame[k], seg[k], rgba[k])
    a, b = whole.end(), single.end()
    assert a["names"] == b["names"]
    np.testing.assert_array_equal(a["iou"]["ours"], b["iou"]["ours"])
    np.testing.assert_array_equal(a["f1"]["ours"], b["f1"]["ours"])
    np.testing.assert_array_equal(a["collage"], b["collage"])
    np.testing.assert_allclose(a["iou"]["ours"], np.stack([d["iou%d" % k][0] for k in ks]), rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# workspace
# ---------------------------------------------------------------------------------------------------------------------
def test_a_workspace_full_of_ones_changes_nothing():
    """mgr_ceval_labels initialises all the fill reads: every case through the entries on a workspace of 0xFF bytes."""
    from manus_amd import contact_eval as ce
    todo = [(s, cases.chain_case(*s)) for s in cases.CHAIN_SIZES] + [(n, cases.fill_case(n)) for n in _PLAIN_FILL]
    for key, c in todo:
        if len(c) == 3:
            frame, seg, rgba = c
            pred, gt, hand, f8 = ce.contact_masks(frame, seg, rgba)
        else:
            f8, hand = dev(c[0]), dev(c[1])
            pred = gt = None
        V, H, W = hand.shape
        labels, unfilled = ce.skin_labels(f8, hand, return_unfilled=True)
        for run in range(2):
            u2, l2, flags = _c_labels(f8, int(f8.shape[2]), hand, V, H, W, poison=True)
            np.testing.assert_array_equal(u2, host(unfilled), err_msg=str(key))
            np.testing.assert_array_equal(l2, host(labels), err_msg=str(key))
            assert flags.tolist() == [0] * V
        if pred is not None:
            np.testing.assert_array_equal(_c_counts(pred, gt, labels, poison=True), host(ce.contact_counts(pred, gt, labels)), err_msg=str(key))

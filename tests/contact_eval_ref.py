"""A plain restatement of the whole contact-evaluation chain (csrc/contact_eval.hip, manus_amd/contact_eval.py) in numpy /
scipy: int64 and float64, no torch, nothing of the code under test but the PALETTE (data).  Every function takes one
image or a batch with V in front.  tests/test_contact_eval_cases_cpu.py anchors it on the reference's own outputs
(tests/golden/contact_eval.npz); tests/test_gpu_contact_eval_edges.py holds the kernels to it.

    masks_ref(frame, seg, rgba)      (pred, gt, hand, frame_u8)      get_iou_ours.py:313-322, base.py:245-246
    labels_ref(skin, hand)           unfilled labels                 get_skin_mask before its fill
    fill_ref(unfilled, hand)         filled labels, brute force      get_contact_dist + the strict '<' scan
    counts_ref(pred, gt, labels)     (17,3) int64 [I, A, B]          cal_iou / f1_score inputs
    collage_ref(rgba, masks)         uint8 rows                      combine_images / blend_masks
    scores_ref(counts)               IoU, F1 in float64
"""
import numpy as np
import scipy.ndimage as ndi

from manus_amd.contact_eval import PALETTE

CROSS = ndi.generate_binary_structure(2, 1)          # MORPH_ELLIPSE (3,3) = the 4-neighbour cross


def _batched(fn, n_image_dims, first, *rest):
    """fn on one image, or on every image of a batch (one more dimension in front than n_image_dims)."""
    first = np.asarray(first)
    if first.ndim == n_image_dims:
        return fn(first, *[np.asarray(r) for r in rest])
    return np.stack([fn(first[v], *[np.asarray(r)[v] for r in rest]) for v in range(first.shape[0])])


def frame_bytes_ref(frame):
    """A uint8 frame as it is; a float32 frame as (np.clip(f32, 0, 1) * 255).astype(np.uint8) with the product in float32;
    NaN gives byte 0."""
    frame = np.asarray(frame)
    if frame.dtype == np.uint8:
        return frame
    assert frame.dtype == np.float32
    x = np.clip(np.where(np.isnan(frame), np.float32(0), frame), np.float32(0), np.float32(1)) * np.float32(255)
    assert x.dtype == np.float32
    return x.astype(np.int64).astype(np.uint8)       # truncation; the values lie in [0, 255]


def masks_ref(frame, seg, rgba):
    """(pred, gt, hand, frame_u8): uint8 0/1 masks.  pred / gt: every channel of the frame's right half / of seg >= 128;
    hand: alpha > 128."""
    f8 = frame_bytes_ref(frame)
    W = f8.shape[-2] // 2
    assert f8.shape[-2] == 2 * W
    pred = (f8[..., W:, :].astype(np.int64) >= 128).all(axis=-1)
    gt = (np.asarray(seg).astype(np.int64) >= 128).all(axis=-1)
    hand = np.asarray(rgba)[..., 3].astype(np.int64) > 128
    return pred.astype(np.uint8), gt.astype(np.uint8), hand.astype(np.uint8), f8


def palette_matches(skin):
    """(16, ...) bool: |c - p| <= 10 on all channels, per palette entry."""
    c = np.asarray(skin).astype(np.int64)
    return np.stack([(np.abs(c - p.astype(np.int64)) <= 10).all(axis=-1) for p in PALETTE])


def opened_masks(skin, erode_border=1, dilate_border=0):
    """(16,H,W) bool of one image: every palette entry's match, eroded and dilated with the cross."""
    out = []
    for m in palette_matches(skin):
        e = ndi.binary_erosion(m, CROSS, border_value=erode_border)
        out.append(ndi.binary_dilation(e, CROSS, border_value=dilate_border))
    return np.stack(out)


def _labels_one(skin, hand, erode_border=1, dilate_border=0):
    op = opened_masks(skin, erode_border, dilate_border)
    stack = np.concatenate([np.zeros((1,) + op.shape[1:], np.int64), op.astype(np.int64) * 255])
    return (np.argmax(stack, axis=0) * (hand > 0)).astype(np.uint8)       # argmax: the first of equal maxima


def labels_ref(skin, hand, erode_border=1, dilate_border=0):
    """Unfilled labels 0..16 of skin (H,W,3) / (V,H,W,3) uint8 and hand (H,W) / (V,H,W)."""
    return _batched(lambda s, h: _labels_one(s, h, erode_border, dilate_border), 3, skin, hand)


def nearest_labelled(unfilled, ys, xs):
    """For the pixels (ys, xs): (index row * W + col of the labelled pixel with the least (d^2, index), that d^2), int64."""
    H, W = unfilled.shape
    lab = np.argwhere(unfilled > 0).astype(np.int64)                        # row-major order
    if len(ys) and not len(lab):
        raise ValueError("residual pixels and nothing labelled")
    lidx = lab[:, 0] * W + lab[:, 1]
    win, d2min = np.zeros(len(ys), np.int64), np.zeros(len(ys), np.int64)
    chunk = max(1, (1 << 24) // max(1, len(lab)))
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    for s in range(0, len(ys), chunk):
        d2 = (ys[s:s + chunk, None] - lab[None, :, 0]) ** 2 + (xs[s:s + chunk, None] - lab[None, :, 1]) ** 2
        key = d2 * (1 << 32) + lidx[None]
        k = key.min(axis=1)
        win[s:s + chunk], d2min[s:s + chunk] = k % (1 << 32), k >> 32
    return win, d2min


def _fill_one(unfilled, hand):
    out = unfilled.copy()
    res = np.argwhere((hand > 0) & (unfilled == 0))
    if len(res) == 0:
        return out
    win, _ = nearest_labelled(unfilled, res[:, 0], res[:, 1])
    out[res[:, 0], res[:, 1]] = unfilled.reshape(-1)[win]
    return out


def fill_ref(unfilled, hand):
    """Every residual pixel (inside the hand, no label) takes the label of the labelled pixel with the least
    (d^2, row * W + col); raises ValueError when there are residual pixels and nothing is labelled."""
    return _batched(_fill_one, 2, unfilled, hand)


def _counts_one(pred, gt, labels):
    p, g = pred != 0, gt != 0
    out = np.zeros((17, 3), np.int64)
    for i in range(17):
        sel = (labels == i) if i < 16 else np.ones(p.shape, bool)
        out[i] = [(g & p & sel).sum(), (g & sel).sum(), (p & sel).sum()]
    return out


def counts_ref(pred, gt, labels):
    """(17,3) / (V,17,3) int64 [I, A, B] = [|gt & pred|, |gt|, |pred|]; rows 0..15 within labels == i, row 16 everything."""
    return _batched(_counts_one, 2, pred, gt, labels)


def scores_ref(counts):
    """IoU = I / (A + B - I + 1e-6); F1 = 2 I / (A + B), NaN when A + B = 0."""
    c = np.asarray(counts).astype(np.int64)
    I, A, B = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return I / (A + B - I + 1e-6), np.where(A + B == 0, np.nan, (2 * I) / (A + B).astype(np.float64))


def collage_ref(rgba, masks):
    """uint8 (..., H, (1 + M) W, 3): the photo on white, then the photo blended with each mask.  The float64 numpy
    expressions of combine_images / blend_masks on whole images.  A mask pixel is set when it is not zero (the product's
    masks are 0/1 where the reference's are 0/255)."""
    rgba = np.asarray(rgba)
    alpha = rgba[..., -1:] > 128
    rgb = rgba[..., :3] / 255
    weight = 0.5
    color = np.asarray([0, 128, 0]) / 255
    panels = [rgb * alpha + (1 - alpha) * np.array([1, 1, 1])]
    for mask in masks:
        mask = ((np.asarray(mask) != 0) * 255).astype(np.uint8) / 255
        mask = mask[..., None].repeat(3, axis=-1)
        mask = mask * color
        final = rgb * weight + (1 - weight) * mask
        panels.append(final * alpha + (1 - alpha) * np.array([1, 1, 1]))
    row = np.concatenate(panels, axis=-2)
    row = row * 255
    return row.astype(np.uint8)

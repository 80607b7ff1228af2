"""Contact evaluation of brown-ivl/manus over the HIP kernels of csrc/contact_eval.hip: how accurate are the contacts.

Mirrors the last two lines of scripts/train/eval.sh -- scripts/process/get_iou_ours.py and get_iou.py -- and
get_evaluation_numbers*.py:

    contact_masks(frame, gt_seg, gt_rgba)     pred / gt / hand masks of V cameras           get_iou_ours.py:313-322
    skin_labels(frame, hand)                  per-pixel bone labels, residual pixels filled  get_skin_mask, :74-151
    contact_counts(pred, gt, labels)          (V,17,3) integer [I, A, B]                     cal_iou / f1_score inputs
    scores_from_counts(counts)                IoU, F1 in float64 on the host                 evaluate_metric, :162-232
    collage_rows(gt_rgba, masks)              the uint8 collage rows                         combine_images, :269-291
    ContactEvaluator(exp_dir)                 add(...) per camera, end(): eval_metric.csv + eval_collage.png, :334-344
    evaluate_directory(exp_dir, gt_dir)       the file route of the two scripts (their directory layout, PNG files)
    average_eval_metrics(csv_paths)           get_evaluation_numbers_ours.py:6-35

The `frame` is the product's 'acc_gt_eval' render (`modules.CompositeRenderer`), (H, 2W, 3): skin-weight colours on the
left, the grey accumulated-contact map on the right; uint8, or the fp32 render itself (converted on the device like
test_step does).  The reference hard-codes the split at column 1080; here it is half the frame width.  Images are RGB(A)
as rendered / as Pillow reads them: the reference works on OpenCV's BGR and flips the skin half to RGB (:318); every
other step treats the three channels alike, so the scores and the written collage are the same.

Quirk kept from the reference: the per-bone rows score `label == i` for i = 0..15, where label 0 is "no label" (the
whole background) and label 16 (the last palette colour) is never scored -- calculate_per_bone_iou loops range(16) over
labels that run 0..16.  "bone1" of the CSV is therefore the unlabelled class.

A view with residual pixels (inside the hand, no label) and no labelled pixel at all makes the reference crash with an
IndexError; here it is a ValueError that names the view.

There is no CPU fallback: every image-sized step is a kernel and needs GPU tensors (arrays are uploaded).
"""
import csv
import os
import re

import numpy as np
import torch

from ._lib import ManusHipError, check, lib, stream

# get_skin_mask's colours (get_iou_ours.py:94-111), RGB; label i + 1 <-> PALETTE[i]
PALETTE = np.array([[43, 159, 43], [31, 119, 178], [173, 198, 231], [254, 186, 119], [151, 222, 137], [213, 38, 39],
                    [254, 151, 149], [196, 175, 212], [139, 85, 74], [195, 155, 147], [246, 181, 209], [126, 126, 126],
                    [198, 199, 198], [218, 218, 140], [25, 190, 206], [156, 217, 228]], dtype=np.uint8)
N_CLASSES = 16          # scored classes, labels 0..15
CSV_HEADER = [""] + ["bone%d" % i for i in range(1, 17)] + ["combined"]      # get_iou_ours.py:339-341

_TABLE = None
_TABLES_DEV = {}


def collage_table():
    """(256,3,2,3) uint8, [photo byte, kind, alpha bit, channel] -> the collage's byte; kind 0 is the plain panel, 1 / 2 the
    panel blended with a clear / set mask pixel.  combine_images / blend_masks (get_iou_ours.py:269-291) compute, in
    float64, `rgb / 255`, `mask / 255`, `rgb * 0.5 + (1 - 0.5) * (mask * colour)` with colour = (0,128,0) / 255,
    `x * alpha + (1 - alpha) * 1`, `* 255`, and main() casts with astype(np.uint8): the result depends on these four
    indices only.  The table is built with exactly those numpy expressions; the kernel gathers from it."""
    global _TABLE
    if _TABLE is None:
        byte = np.arange(256, dtype=np.uint8).reshape(256, 1, 1)
        alpha = np.array([False, True]).reshape(1, 2, 1)
        weight = 0.5
        color = np.asarray([0, 128, 0]) / 255
        rgb = (byte / 255) * np.ones((1, 1, 3))                                  # (256,1,3)
        white = np.array([1, 1, 1])
        panels = [rgb * alpha + (1 - alpha) * white]
        for mask_byte in (0, 255):
            mask = np.full((256, 1), mask_byte, np.uint8) / 255
            mask = mask[..., None].repeat(3, axis=-1) * color
            final = rgb * weight + (1 - weight) * mask
            panels.append(final * alpha + (1 - alpha) * white)
        tab = np.stack(panels, axis=1) * 255                                      # (256,3,2,3) float64
        _TABLE = np.ascontiguousarray(tab.astype(np.uint8))
    return _TABLE


def natural_sorted(names):
    """natsorted for file names: digit runs compare as numbers, the rest as text ('cam2' < 'cam10')."""
    def key(s):
        return [(0, int(t), "") if t.isdigit() else (1, 0, t) for t in re.split(r"(\d+)", str(s)) if t != ""]
    return sorted(names, key=key)


# ---------------------------------------------------------------------------------------------------------------------
# device steps
# ---------------------------------------------------------------------------------------------------------------------
def _dev_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise ManusHipError("contact evaluation needs a GPU; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _u8(x, dev, channels, name, batch_dims=4):
    """uint8 contiguous device tensor (V,H,W,channels) (or (V,H,W) for channels None) from a tensor / array, a single image
    gaining V = 1."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype != torch.uint8:
        raise ValueError("%s must be uint8 (got %s)" % (name, t.dtype))
    want = batch_dims if channels is not None else batch_dims - 1
    if t.dim() == want - 1:
        t = t[None]
    if t.dim() != want or (channels is not None and t.shape[-1] != channels):
        raise ValueError("%s must be (V,H,W%s) or one such image, got %s" % (name, "" if channels is None else ",%d" % channels, tuple(t.shape)))
    return t.to(dev).contiguous()


def _workspace(V, H, W, dev):
    n = int(lib().mgr_ceval_workspace_bytes(V, H, W))
    if n == 0:
        raise ValueError("contact evaluation: sizes out of range (V=%d, H=%d, W=%d)" % (V, H, W))
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def contact_masks(frame, gt_seg, gt_rgba):
    """(pred, gt, hand, frame_u8): uint8 0/1 device tensors (V,H,W) and the frame as uint8 (V,H,2W,3).
    frame (V,H,2W,3) uint8 or the fp32 render (converted as uint8(clamp(x,0,1) * 255), base.py:245-246); gt_seg (V,H,W,3),
    gt_rgba (V,H,W,4) uint8; single images without V are accepted.  pred / gt: every channel of the frame's right half / of
    gt_seg in [128,255]; hand: alpha > 128 (get_iou_ours.py:313-322)."""
    dev = _dev_of(frame, gt_seg, gt_rgba)
    f = frame if torch.is_tensor(frame) else torch.from_numpy(np.ascontiguousarray(frame))
    if f.dim() == 3:
        f = f[None]
    if f.dim() != 4 or f.shape[-1] != 3 or f.shape[2] % 2 != 0:
        raise ValueError("frame must be (V,H,2W,3), got %s" % (tuple(f.shape),))
    is_f32 = f.dtype == torch.float32
    if not is_f32 and f.dtype != torch.uint8:
        raise ValueError("frame must be uint8 or float32 (got %s)" % f.dtype)
    f = f.detach().to(dev).contiguous()
    V, H, W2, _ = f.shape
    W = W2 // 2
    seg, rgba = _u8(gt_seg, dev, 3, "gt_seg"), _u8(gt_rgba, dev, 4, "gt_rgba")
    if tuple(seg.shape) != (V, H, W, 3) or tuple(rgba.shape) != (V, H, W, 4):
        raise ValueError("gt_seg (V,H,W,3) and gt_rgba (V,H,W,4) must match the frame's (V,H,2W,3): got %s, %s, %s"
                         % (tuple(seg.shape), tuple(rgba.shape), tuple(f.shape)))
    out = torch.empty((3, V, H, W), dtype=torch.uint8, device=dev)
    f8 = torch.empty((V, H, W2, 3), dtype=torch.uint8, device=dev) if is_f32 else f
    check(lib().mgr_ceval_masks(V, H, W, f.data_ptr(), 1 if is_f32 else 0, seg.data_ptr(), rgba.data_ptr(),
                                f8.data_ptr() if is_f32 else None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                stream()), "mgr_ceval_masks")
    return out[0], out[1], out[2], f8


def skin_labels(frame, hand, fill=True, return_unfilled=False):
    """Bone labels (V,H,W) uint8 in 0..16 of the skin-weight render (get_skin_mask).  frame: uint8 RGB, either the left half
    (V,H,W,3) or the whole (V,H,2W,3) frame (its left half is read in place); hand (V,H,W) 0/1.  fill=False stops before the
    nearest-labelled fill; return_unfilled=True returns (filled, unfilled).  Raises ValueError for a view that has residual
    pixels and no labelled pixel."""
    dev = _dev_of(frame, hand)
    hd = _u8(hand, dev, None, "hand")
    V, H, W = hd.shape
    fr = _u8(frame, dev, 3, "frame")
    if fr.shape[0] != V or fr.shape[1] != H or fr.shape[2] not in (W, 2 * W):
        raise ValueError("frame must be (V,H,W,3) or (V,H,2W,3) for hand (V,H,W): got %s, %s" % (tuple(fr.shape), tuple(hd.shape)))
    if fr.data_ptr() % 4 != 0:      # a contiguous slice of a larger tensor (frames[k:]): the kernel stages rows with dword loads
        fr = fr.clone()
    ws, n = _workspace(V, H, W, dev)
    labels = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    check(lib().mgr_ceval_labels(V, H, W, fr.data_ptr(), int(fr.shape[2]), hd.data_ptr(), labels.data_ptr(), ws.data_ptr(), n,
                                 stream()), "mgr_ceval_labels")
    if not fill:
        return labels
    unfilled = labels.clone() if return_unfilled else None
    flags = torch.empty(V, dtype=torch.int32, device=dev)
    check(lib().mgr_ceval_fill(V, H, W, labels.data_ptr(), flags.data_ptr(), ws.data_ptr(), n, stream()), "mgr_ceval_fill")
    bad = torch.nonzero(flags).reshape(-1).tolist()
    if bad:
        raise ValueError("skin_labels: view(s) %s have residual pixels inside the hand and no labelled pixel to take a label from"
                         % ", ".join(str(b) for b in bad))
    return (labels, unfilled) if return_unfilled else labels


def contact_counts(pred, gt, labels):
    """(V,17,3) int64 device tensor of [I, A, B] = [|gt & pred|, |gt|, |pred|]: rows 0..15 restricted to labels == i, row 16
    over the whole image (`mgr_ceval_counts`)."""
    dev = _dev_of(pred, gt, labels)
    p, g, l = _u8(pred, dev, None, "pred"), _u8(gt, dev, None, "gt"), _u8(labels, dev, None, "labels")
    if p.shape != g.shape or p.shape != l.shape:
        raise ValueError("pred, gt and labels must have one shape (V,H,W): got %s, %s, %s" % (tuple(p.shape), tuple(g.shape), tuple(l.shape)))
    V, H, W = p.shape
    ws, n = _workspace(V, H, W, dev)
    counts = torch.empty((V, 17, 3), dtype=torch.int64, device=dev)
    check(lib().mgr_ceval_counts(V, H, W, p.data_ptr(), g.data_ptr(), l.data_ptr(), counts.data_ptr(), ws.data_ptr(), n, stream()),
          "mgr_ceval_counts")
    return counts


def scores_from_counts(counts):
    """(iou, f1), float64 arrays shaped like counts[..., 0].  IoU = I / (A + B - I + 1e-6) (cal_iou); F1 = 2 I / (A + B), NaN
    when A + B = 0 (sklearn's f1_score with zero_division=np.nan on the reference's 0/1 labels)."""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if c.shape[-1] != 3:
        raise ValueError("counts must end in [I, A, B], got shape %s" % (c.shape,))
    c = c.astype(np.int64)
    I, A, B = c[..., 0], c[..., 1], c[..., 2]
    iou = I / (A + B - I + 1e-6)
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = np.where(A + B == 0, np.nan, (2 * I) / (A + B).astype(np.float64))
    return iou, f1


def collage_rows(gt_rgba, masks):
    """(V,H,(1+M)W,3) uint8 device tensor: [photo on white | photo blended with masks[0] | ... ] (combine_images).  masks: a list
    of (V,H,W) 0/non-zero masks, or one (M,V,H,W) tensor."""
    dev = _dev_of(gt_rgba, *(masks if isinstance(masks, (list, tuple)) else [masks]))
    rgba = _u8(gt_rgba, dev, 4, "gt_rgba")
    V, H, W, _ = rgba.shape
    if isinstance(masks, (list, tuple)):
        ms = [_u8(m, dev, None, "mask") for m in masks]
        m = torch.stack(ms) if ms else torch.empty((0, V, H, W), dtype=torch.uint8, device=dev)
    else:
        m = _u8(masks, dev, None, "masks", batch_dims=5)
    if tuple(m.shape[1:]) != (V, H, W) or m.shape[0] > 16:
        raise ValueError("masks must be at most 16 masks of shape (V,H,W) = %s, got %s" % ((V, H, W), tuple(m.shape)))
    m = m.contiguous()
    tab = _TABLES_DEV.get(dev)
    if tab is None:
        tab = _TABLES_DEV[dev] = torch.from_numpy(collage_table()).to(dev).contiguous()
    M = int(m.shape[0])
    out = torch.empty((V, H, (1 + M) * W, 3), dtype=torch.uint8, device=dev)
    check(lib().mgr_ceval_collage(V, H, W, M, rgba.data_ptr(), m.data_ptr() if M else None, tab.data_ptr(), out.data_ptr(), stream()),
          "mgr_ceval_collage")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the scripts
# ---------------------------------------------------------------------------------------------------------------------
def metric_rows(per_camera):
    """The CSV's values from per-camera score rows {name: (n_cameras, 17)}: np.around(mean over cameras, 3) per name
    (get_iou_ours.py:334-335); NaN propagates through the mean."""
    return {k: np.around(np.vstack(v).mean(axis=0), decimals=3) for k, v in per_camera.items()}


def write_metric_csv(path, methods, rows):
    """eval_metric.csv as get_iou.py:366-377 writes it: the header, one IoU row per method, then one `<method>_f1` row each."""
    with open(path, "w") as csvfile:
        writer = csv.writer(csvfile)
        writer.writerow(CSV_HEADER)
        for m in methods:
            writer.writerow([m] + rows[m].tolist())
        for m in methods:
            writer.writerow([m + "_f1"] + rows[m + "_f1"].tolist())


class ContactEvaluator:
    """get_iou_ours.py / get_iou.py for one experiment: `add` scores cameras, `end` writes
    <exp_dir>/results/eval_results/eval_metric.csv and eval_collage.png and returns the per-camera table.

    per_bone=True is get_iou.py (calculate_per_bone_iou live); per_bone=False writes the sixteen zeros get_iou_ours.py
    puts in the bone columns.  `baselines` of `add`: {name: mask image (H,W,3) uint8}, thresholded like the prediction
    (every channel in [128,255]) and scored against the same labels -- the `mano` / `harp` rows of get_iou.py; their
    panels stand between the ground truth's and ours in the collage, and their CSV rows between `ours` and `ours_f1`
    in the order get_iou.py writes them (methods: mano, harp, ours when both are given)."""

    def __init__(self, exp_dir, per_bone=True):
        self.exp_dir, self.per_bone = exp_dir, bool(per_bone)
        self.out_dir = os.path.join(exp_dir, "results", "eval_results")
        self.names, self.counts, self.collage, self.methods = [], {}, [], None

    def add(self, camera_name, frame, gt_seg, gt_rgba, baselines=None):
        """One camera (images without V) or V cameras at once (camera_name a list); device tensors or arrays."""
        names = [camera_name] if isinstance(camera_name, str) else list(camera_name)
        baselines = dict(baselines or {})
        methods = list(baselines) + ["ours"]
        if self.methods is None:
            self.methods = methods
        elif methods != self.methods:
            raise ValueError("every camera needs the same baselines: %s, got %s" % (self.methods[:-1], methods[:-1]))
        pred, gt, hand, frame_u8 = contact_masks(frame, gt_seg, gt_rgba)
        V, H, W = pred.shape
        if len(names) != V:
            raise ValueError("%d camera names for %d views" % (len(names), V))
        labels = skin_labels(frame_u8, hand)
        masks = {"ours": pred}
        for k, img in baselines.items():
            b = _u8(img, pred.device, 3, "baseline %r" % k)
            if tuple(b.shape) != (V, H, W, 3):
                raise ValueError("baseline %r must be (V,H,W,3) = %s, got %s" % (k, (V, H, W, 3), tuple(b.shape)))
            masks[k] = (b >= 128).all(dim=-1).to(torch.uint8)
        for k in methods:
            self.counts.setdefault(k, []).append(contact_counts(masks[k], gt, labels))
        self.collage.append(collage_rows(gt_rgba, [gt] + [masks[k] for k in methods]))
        self.names += names

    def end(self):
        """Write the CSV and the collage; returns {"names", "iou": {method: (n,17)}, "f1": {...}, "rows": the CSV's values}."""
        if not self.names:
            raise ValueError("ContactEvaluator.end: no camera was added")
        os.makedirs(self.out_dir, exist_ok=True)
        iou, f1, per_camera = {}, {}, {}
        for k in self.methods:
            i, f = scores_from_counts(torch.cat(self.counts[k]))
            iou[k], f1[k] = i, f
            if self.per_bone:
                per_camera[k], per_camera[k + "_f1"] = i, f
            else:       # get_iou_ours.py:229-231
                zeros = np.zeros((i.shape[0], N_CLASSES))
                per_camera[k] = np.concatenate([zeros, i[:, -1:]], axis=1)
                per_camera[k + "_f1"] = np.concatenate([zeros, f[:, -1:]], axis=1)
        rows = metric_rows(per_camera)
        # get_iou.py writes ours first, then the baselines
        order = ["ours"] + [k for k in self.methods if k != "ours"]
        write_metric_csv(os.path.join(self.out_dir, "eval_metric.csv"), order, rows)
        from PIL import Image
        widths = {int(c.shape[2]) for c in self.collage}
        if len(widths) != 1:
            raise ValueError("the cameras' collage rows have different widths %s: np.vstack of the reference fails too" % sorted(widths))
        collage = torch.cat([c.reshape(-1, c.shape[2], 3) for c in self.collage]).cpu().numpy()
        Image.fromarray(collage).save(os.path.join(self.out_dir, "eval_collage.png"))
        return {"names": list(self.names), "iou": iou, "f1": f1, "rows": rows, "collage": collage}


def _read(path, mode):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert(mode)))


def evaluate_directory(exp_dir, gt_contact_dir, per_bone=True, baselines=("mano", "harp")):
    """The file route of get_iou.py (per_bone=False, baselines=(): get_iou_ours.py), on the reference's layout:
        <gt_contact_dir>/*.png                                        ground-truth segmentation ("…/gt_contacts_seg")
        <gt_contact_dir with gt_contacts_seg -> gt_contacts>/*.png    ground-truth RGBA photos
        <exp_dir>/results/eval_results/ours/acc_gt_eval/*.png         the frames
        <exp_dir>/results/eval_results/<baseline>/acc_eval_rendered/*.png   for every baseline whose directory exists
    each list in natural order and paired by position.  Cameras of one size go through one launch chain."""
    def pngs(d):
        return [os.path.join(d, n) for n in natural_sorted(n for n in os.listdir(d) if n.endswith(".png"))] if os.path.isdir(d) else []
    seg_paths = pngs(gt_contact_dir)
    rgba_paths = pngs(gt_contact_dir.replace("gt_contacts_seg", "gt_contacts"))
    res = os.path.join(exp_dir, "results", "eval_results")
    frame_paths = pngs(os.path.join(res, "ours", "acc_gt_eval"))
    base_paths = {b: pngs(os.path.join(res, b, "acc_eval_rendered")) for b in baselines}
    base_paths = {b: p for b, p in base_paths.items() if p}
    n = len(seg_paths)
    if n == 0:
        raise ValueError("no ground-truth segmentation under %s" % gt_contact_dir)
    for what, p in [("photos", rgba_paths), ("frames", frame_paths)] + [(b, p) for b, p in base_paths.items()]:
        if len(p) < n:
            raise ValueError("%d %s for %d ground-truth masks" % (len(p), what, n))
    ev = ContactEvaluator(exp_dir, per_bone=per_bone)
    items = []
    for i in range(n):
        items.append((os.path.splitext(os.path.basename(seg_paths[i]))[0], _read(frame_paths[i], "RGB"), _read(seg_paths[i], "RGB"),
                      _read(rgba_paths[i], "RGBA"), {b: _read(p[i], "RGB") for b, p in base_paths.items()}))
    i = 0
    while i < n:        # runs of one size -> one call
        j = i
        while j < n and items[j][1].shape == items[i][1].shape and items[j][2].shape == items[i][2].shape:
            j += 1
        run = items[i:j]
        ev.add([r[0] for r in run], np.stack([r[1] for r in run]), np.stack([r[2] for r in run]), np.stack([r[3] for r in run]),
               {b: np.stack([r[4][b] for r in run]) for b in base_paths})
        i = j
    return ev.end()


def average_eval_metrics(csv_paths):
    """get_evaluation_numbers_ours.py:6-35: read the eval_metric.csv files that exist, NaN -> 0, average every row over the
    files; returns ({row name: (17,) averages}, {row name: the last column}) -- the reference prints the latter."""
    tables = []
    for path in csv_paths:
        if not os.path.exists(path):
            continue
        with open(path, newline="") as f:
            rd = list(csv.reader(f))
        d = {}
        for row in rd[1:]:
            if not row:
                continue
            vals = np.array([float(x) if x != "" else np.nan for x in row[1:]], dtype=np.float64)
            d[row[0]] = np.where(np.isnan(vals), 0.0, vals)
        tables.append(d)
    if not tables:
        raise ValueError("average_eval_metrics: none of the files exists")
    avg = {}
    for d in tables:
        for k, v in d.items():
            avg[k] = avg[k] + v if k in avg else v.copy()
    avg = {k: v / len(tables) for k, v in avg.items()}
    return avg, {k: float(v[-1]) for k, v in avg.items()}

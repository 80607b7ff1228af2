#!/usr/bin/env python3
"""Generate tests/golden/contact_eval.npz by IMPORTING the reference's evaluation scripts (authoring container only; the
location of the reference checkout is make_golden.REF):

    python tests/golden/make_contact_eval_golden.py

Same rules as make_golden.py: the reference's Python is imported, only arrays and the CSV text are written, nothing of
the reference is restated as an expected value.  Every expected value is the output of the reference's own
  * scripts/process/get_iou.py / get_iou_ours.py:  get_skin_mask, cal_iou, evaluate_metric (both files'),
    calculate_per_bone_iou, blend_masks, combine_images, and main() -- the CSV / collage block -- run against a
    temporary directory in the reference's layout,
with the real scikit-learn doing the F1.

Stand-ins of this file's own writing, for the two packages this image lacks (DESIGN section 3 lists the leg as unpinned;
tests/test_contact_eval_cpu.py cross-checks the morphology against scipy.ndimage):
  * cv2:    inRange, getStructuringElement(MORPH_ELLIPSE, (3,3)) = the 4-neighbour cross, erode / dilate with OpenCV's
            default borders (outside the image: set for the erosion, unset for the dilation), imread / imwrite through
            Pillow in BGR(A) order;
  * taichi: ndarrays over numpy float32 and a `kernel` decorator that runs the reference's kernel body as plain Python,
            `ti.sqrt` rounding to fp32 like the device kernel does;
  * natsort.natsorted: digit runs as numbers.
main() hard-codes the frame's split at column 1080; it is executed from its own source with that literal replaced by
the fixture's width (the only edit; nothing of it is kept).

Contents: n_main cameras of one odd size that go through main(), one extra camera of an even size that only goes
through the functions.  Per camera k: frame<k> (H,2W,3) RGB, seg<k> (H,W,3), rgba<k> (H,W,4), mano<k>, harp<k> (H,W,3)
inputs; pred<k>, gt<k>, mano_mask<k>, harp_mask<k> (0/255), hand<k> (bool), labels<k> / labels_unfilled<k> (the
reference's final_mask and what it was before the fill), iou<k> / f1<k> (3,17) for ours, mano, harp (per bone then
combined), counts<k> (3,17,3) [I, A, B] counted with numpy from the reference's masks, row<k> / row5<k> the collage rows
of get_iou_ours.py / get_iou.py as uint8.  csv_ours / csv_full: the two eval_metric.csv texts; collage_ours /
collage_full: the written PNGs decoded to RGB.
"""
import importlib.util
import os
import re
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                      # noqa: E402  (stub machinery, REF)

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from manus_amd.contact_eval import PALETTE    # noqa: E402  (data: the inputs are painted with it)


# ---------------------------------------------------------------------------------------------------------------------
# stand-ins
# ---------------------------------------------------------------------------------------------------------------------
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)


def in_range(img, lower, upper):
    img = np.asarray(img).astype(np.int64)
    lo, hi = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    ok = np.all((img >= lo) & (img <= hi), axis=-1)
    return (ok * 255).astype(np.uint8)


def _morph(mask, kernel, border, op):
    assert np.array_equal(kernel, CROSS)
    p = np.pad(mask, 1, constant_values=border)
    H, W = mask.shape
    stack = [p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))]
    return op(np.stack(stack), axis=0)


def erode(mask, kernel, iterations=1):
    assert iterations == 1
    return _morph(mask, kernel, 255, np.min)


def dilate(mask, kernel, iterations=1):
    assert iterations == 1
    return _morph(mask, kernel, 0, np.max)


def make_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.MORPH_ELLIPSE, cv2.IMREAD_UNCHANGED = 2, -1

    def get_structuring_element(shape, ksize):
        assert shape == cv2.MORPH_ELLIPSE and tuple(ksize) == (3, 3)
        return CROSS.copy()

    def imread(path, flags=1):
        im = Image.open(path)
        if flags == cv2.IMREAD_UNCHANGED and im.mode == "RGBA":
            return np.ascontiguousarray(np.asarray(im)[..., [2, 1, 0, 3]])
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])

    def imwrite(path, img):
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(path)
        return True

    cv2.getStructuringElement, cv2.inRange, cv2.erode, cv2.dilate = get_structuring_element, in_range, erode, dilate
    cv2.imread, cv2.imwrite = imread, imwrite
    return cv2


class _TiArray:
    def __init__(self, shape, dtype):
        self.a = np.zeros(shape, np.float32)

    def from_numpy(self, x):
        self.a[...] = x

    def to_numpy(self):
        return self.a.copy()

    def __getitem__(self, i):
        return self.a[i]

    def __setitem__(self, i, v):
        self.a[i] = v


def make_taichi():
    ti = types.ModuleType("taichi")
    ti.cuda, ti.f32 = "cuda", np.float32
    ti.init = lambda **k: None
    ti.ndarray = lambda shape, dtype: _TiArray(shape, dtype)
    ti.kernel = lambda f: f
    ti.types = types.SimpleNamespace(ndarray=lambda **k: object)
    ti.sqrt = lambda x: np.float32(np.sqrt(np.float32(x)))
    return ti


def natsorted(xs):
    return sorted(xs, key=lambda s: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)])


def import_scripts():
    sys.modules["cv2"], sys.modules["taichi"] = make_cv2(), make_taichi()
    ns = types.ModuleType("natsort")
    ns.natsorted = natsorted
    sys.modules["natsort"] = ns
    mods = {}
    for name in ("get_iou", "get_iou_ours"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(mg.REF, "scripts", "process", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods[name] = m
    return mods


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def blob(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def make_camera(g, H, W, k):
    """One camera's five images, built so that every rule of the evaluation has pixels that exercise it."""
    yy, xx = np.mgrid[0:H, 0:W]
    # palette regions: a grid of cells, each of one palette colour (a few colours never used: classes without pixels)
    used = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 15] if k % 2 == 0 else [0, 1, 2, 4, 5, 7, 8, 9, 10, 12, 13, 15]
    cell = ((yy // 11) * 7 + (xx // 13) + k) % len(used)
    skin = PALETTE[np.asarray(used)[cell]].astype(np.float64)
    # blurred seams (3x3 box, twice): mixed colours fall out of every +-10 box -> residual pixels
    for _ in range(2):
        p = np.pad(skin, ((1, 1), (1, 1), (0, 0)), mode="edge")
        skin = sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    skin = np.round(skin).astype(np.int64)
    skin += g.integers(-2, 3, size=skin.shape) * (g.random((H, W, 1)) < 0.15)          # a little noise inside the boxes
    # a sharp unlabelled band of odd height between two different colours: its middle row is equidistant from both
    skin[20:23, 30:50] = (90, 20, 200)
    skin[16:20, 30:50] = PALETTE[5]
    skin[23:27, 30:50] = PALETTE[8]
    # patches at exactly +-10 (labelled) and +-11 (not) from palette entry 1 / 4
    skin[40:45, 15:20] = PALETTE[1].astype(np.int64) + (10, -10, 10)
    skin[40:45, 22:27] = PALETTE[1].astype(np.int64) + (11, 0, 0)
    skin[47:52, 15:20] = PALETTE[4].astype(np.int64) + (0, 0, -11)
    skin[47:52, 22:27] = PALETTE[4].astype(np.int64) + (-10, 10, -10)
    # the boxes of entries 2 and 15 overlap: this colour lies in both, the first one (label 3) wins
    skin[54:60, 40:48] = (165, 208, 230)
    skin[54:60, 50:58] = PALETTE[15]                                                    # label 16
    # one-pixel-wide lines of a palette colour on a colour of no box: the opening removes them
    skin[30:38, 60:75] = (60, 60, 60)
    skin[33, 60:75] = PALETTE[6]
    skin[30:38, 67] = PALETTE[6]
    # labelled pixels on the border
    skin[0:6, 0:9] = PALETTE[9]
    skin[H - 5:H, W - 8:W] = PALETTE[10]
    skin = np.clip(skin, 0, 255).astype(np.uint8)
    # the grey contact map (right half): a blob, with edge values 127 / 128 and one channel below
    grey = np.full((H, W, 3), 30, np.uint8)
    b = blob(H, W, 24 + 3 * k, 40 + 4 * k, 13, 21)
    grey[b] = 200
    grey[blob(H, W, 24 + 3 * k, 40 + 4 * k, 15, 23) & ~b] = 128
    grey[blob(H, W, 24 + 3 * k, 40 + 4 * k, 17, 25) & ~blob(H, W, 24 + 3 * k, 40 + 4 * k, 15, 23)] = 127
    grey[50:54, 60:70] = (255, 255, 127)
    grey[56:60, 60:70] = (255, 255, 255)
    frame = np.concatenate([skin, grey], axis=1)
    # ground truth segmentation
    seg = np.zeros((H, W, 3), np.uint8)
    seg[blob(H, W, 27 + 2 * k, 44 + 3 * k, 14, 19)] = 255
    seg[blob(H, W, 52, 22, 6, 9)] = (128, 200, 255)
    seg[2:5, 70:80] = (127, 255, 255)
    # the photo: smooth colours; alpha: the hand (129 / 255 inside, 128 / 0 outside)
    rgb = np.stack([127 + 120 * np.sin(0.07 * xx + 0.05 * yy + c + k) for c in range(3)], axis=-1)
    inside = blob(H, W, H / 2 - 1, W / 2, H / 2 - 2, W / 2 - 6) | (yy < 8) & (xx < 12) | (yy >= H - 5) & (xx >= W - 8)
    alpha = np.where(inside, 255, 0)
    alpha[inside & (blob(H, W, H / 2 - 1, W / 2, H / 2 - 4, W / 2 - 9) == 0)] = 129
    alpha[~inside & blob(H, W, H / 2 - 1, W / 2, H / 2, W / 2 - 3)] = 128
    rgba = np.concatenate([np.clip(rgb, 0, 255), alpha[..., None]], axis=-1).astype(np.uint8)
    # baselines
    mano = np.zeros((H, W, 3), np.uint8)
    mano[blob(H, W, 30, 50 + 2 * k, 10, 24)] = 255
    harp = np.zeros((H, W, 3), np.uint8)
    harp[blob(H, W, 22 + k, 36, 16, 14)] = 180
    return frame, seg, rgba, mano, harp


def counts_of(gt_mask, pred_mask, labels):
    out = np.zeros((17, 3), np.int64)
    g, p = gt_mask == 255, pred_mask == 255
    for i in range(17):
        sel = (labels == i) if i < 16 else np.ones_like(g)
        out[i] = [(g & p & sel).sum(), (g & sel).sum(), (p & sel).sum()]
    return out


def main():
    mods = import_scripts()
    full, ours = mods["get_iou"], mods["get_iou_ours"]
    cv2 = sys.modules["cv2"]
    g = np.random.default_rng(77)
    H, W, n_main = 65, 97, 3
    cams = [make_camera(g, H, W, k) for k in range(n_main)] + [make_camera(g, 64, 96, 3)]
    out = {"n_main": np.int32(n_main), "n": np.int32(len(cams))}
    seen = dict(tie=False, label16=False, nan=False, border=False, pm10=False, pm11=False, overlap=False, line=False, residual=False)
    for k, (frame, seg, rgba, mano, harp) in enumerate(cams):
        h, w = seg.shape[:2]
        # what main() does per camera, on what imread would return (BGR / BGRA)
        gt_rgb = np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])
        gt_mask = cv2.inRange(seg[..., ::-1], (128, 128, 128), (255, 255, 255))
        our = frame[..., ::-1]
        skin_img = our[:, :w, :][..., ::-1]
        our_mask = cv2.inRange(our[:, w:, :], (128, 128, 128), (255, 255, 255))
        mano_mask = cv2.inRange(mano[..., ::-1], (128, 128, 128), (255, 255, 255))
        harp_mask = cv2.inRange(harp[..., ::-1], (128, 128, 128), (255, 255, 255))
        hand = gt_rgb[..., -1] > 128
        # get_skin_mask, with the fill's two coordinate lists caught on the way
        caught = {}
        orig = full.get_contact_dist

        def spy(pt1, pt2, _o=orig, _c=caught):
            _c["res"], _c["skin"] = pt1.copy(), pt2.copy()
            return _o(pt1, pt2)

        full.get_contact_dist = spy
        labels = full.get_skin_mask(skin_img, hand)
        full.get_contact_dist = orig
        labels_ours = labels if k else ours.get_skin_mask(skin_img, hand)          # (the two files' copies agree; checked once)
        assert np.array_equal(labels, labels_ours)
        unfilled = labels.copy()
        unfilled[caught["res"][:, 0], caught["res"][:, 1]] = 0
        iou, f1 = np.zeros((3, 17)), np.zeros((3, 17))
        for j, m in enumerate((our_mask, mano_mask, harp_mask)):
            il, fl, ia, fa = full.evaluate_metric(labels, gt_mask, m)
            iou[j], f1[j] = [*il, ia], [*fl, fa]
            assert ia == full.cal_iou(gt_mask, m)
        il0, fl0, ia0, fa0 = ours.evaluate_metric(labels, gt_mask, our_mask)
        assert not np.any(il0) and not np.any(fl0) and ia0 == iou[0, 16] and (fa0 == f1[0, 16] or (np.isnan(fa0) and np.isnan(f1[0, 16])))
        row = ours.combine_images(gt_rgb, gt_mask, our_mask).astype(np.uint8)[..., ::-1]
        row5 = full.combine_images(gt_rgb, gt_mask, our_mask, mano_mask, harp_mask).astype(np.uint8)[..., ::-1]
        # the rules the inputs were built for, asserted on the reference's output
        lab_yx = np.argwhere(unfilled > 0)
        for (y, x) in caught["res"]:
            d2 = ((lab_yx - (y, x)) ** 2).sum(axis=1)
            near = lab_yx[d2 == d2.min()]
            if len({int(unfilled[a, b]) for a, b in near}) > 1:
                seen["tie"] = True
                assert labels[y, x] == unfilled[near[0, 0], near[0, 1]]              # first in row-major order
        seen["residual"] |= len(caught["res"]) > 0
        seen["label16"] |= bool((labels == 16).any())
        seen["nan"] |= bool(np.isnan(f1).any())
        seen["border"] |= bool(unfilled[0, 0] > 0 and unfilled[h - 1, w - 1] > 0)
        seen["pm10"] |= bool(unfilled[42, 17] == 2 and unfilled[49, 24] == 5)
        seen["pm11"] |= bool(unfilled[42, 24] == 0 and unfilled[49, 17] == 0)
        seen["overlap"] |= bool(unfilled[57, 44] == 3)
        seen["line"] |= bool(unfilled[33, 62] == 0 and unfilled[31, 67] == 0)
        assert hand[42, 17] and hand[49, 24] and hand[42, 24] and hand[49, 17] and hand[57, 44] and hand[57, 54] and hand[33, 62]
        print(k, (h, w), "residual", len(caught["res"]), "labelled", len(caught["skin"]), "labels", sorted(set(labels.ravel().tolist())),
              "iou", iou[:, 16], "f1", f1[:, 16])
        out.update({"frame%d" % k: frame, "seg%d" % k: seg, "rgba%d" % k: rgba, "mano%d" % k: mano, "harp%d" % k: harp,
                    "pred%d" % k: our_mask, "gt%d" % k: gt_mask, "mano_mask%d" % k: mano_mask, "harp_mask%d" % k: harp_mask,
                    "hand%d" % k: hand, "labels%d" % k: labels.astype(np.uint8), "labels_unfilled%d" % k: unfilled.astype(np.uint8),
                    "iou%d" % k: iou, "f1%d" % k: f1, "row%d" % k: row, "row5%d" % k: row5,
                    "counts%d" % k: np.stack([counts_of(gt_mask, m, labels) for m in (our_mask, mano_mask, harp_mask)])})
    assert all(seen.values()), seen

    # main() of both scripts in the reference's layout
    with tempfile.TemporaryDirectory() as tmp:
        exp_dir = os.path.join(tmp, "outputs", "exp") + "/"
        root = os.path.join(tmp, "data")
        grasp_path = os.path.join(root, "a", "b", "c")
        seg_dir = os.path.join(root, "evals", "obj_action", "gt_contacts_seg")
        dirs = {"seg": seg_dir, "rgba": seg_dir.replace("gt_contacts_seg", "gt_contacts"),
                "frame": os.path.join(exp_dir, "results/eval_results/ours/acc_gt_eval"),
                "mano": os.path.join(exp_dir, "results/eval_results/mano/acc_eval_rendered"),
                "harp": os.path.join(exp_dir, "results/eval_results/harp/acc_eval_rendered")}
        for d in dirs.values():
            os.makedirs(d)
        names = ["cam2", "cam10", "cam1"]              # natural order: cam1, cam2, cam10 -> cameras 2, 0, 1
        order = [names.index(n) for n in natsorted(names)]
        for k in range(n_main):
            frame, seg, rgba, mano, harp = cams[k]
            for key, img in (("frame", frame), ("seg", seg), ("rgba", rgba), ("mano", mano), ("harp", harp)):
                Image.fromarray(img).save(os.path.join(dirs[key], names[k] + ".png"))
        argv = sys.argv
        sys.argv = ["x", "--exp_dir", exp_dir, "--object_exp_name", "obj", "--grasp_path", grasp_path]
        import inspect
        for key, mod in (("ours", ours), ("full", full)):
            src = inspect.getsource(mod.main)
            assert src.count("1080") == 2
            exec(compile(src.replace("1080", str(W)), "main_of_" + key, "exec"), mod.__dict__)
            mod.main()
            out["csv_" + key] = np.asarray(open(os.path.join(exp_dir, "results/eval_results/eval_metric.csv"), newline="").read())
            out["collage_" + key] = np.asarray(Image.open(os.path.join(exp_dir, "results/eval_results/eval_collage.png")).convert("RGB"))
        sys.argv = argv
    out["main_names"], out["main_order"] = np.asarray(names), np.asarray(order, np.int32)
    # no averaged value on a rounding boundary of the third decimal
    for j in range(3):
        for arr in ("iou", "f1"):
            m = np.vstack([out["%s%d" % (arr, k)][j] for k in range(n_main)]).mean(axis=0)
            frac = np.abs((m * 1000) % 1.0 - 0.5)
            assert not np.any(frac[~np.isnan(m)] < 1e-3), (arr, j, m)
    assert np.array_equal(out["collage_ours"], np.vstack([out["row%d" % k] for k in order]))
    path = os.path.join(HERE, "contact_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    print(str(out["csv_ours"]))
    print(str(out["csv_full"]))


if __name__ == "__main__":
    main()

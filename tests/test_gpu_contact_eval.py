"""GPU: the contact evaluation (csrc/contact_eval.hip: mgr_ceval_masks / labels / fill / counts / collage,
manus_amd.contact_eval) against the reference's own scripts/process/get_iou.py and get_iou_ours.py
(tests/golden/contact_eval.npz, written by tests/golden/make_contact_eval_golden.py), a brute-force statement of the
fill's integer rule at 1080p, and the properties the kernels promise.

Bounds: masks, labels before and after the fill, counts and collage bytes are integers and must be EQUAL.  Scores
within 1e-9 absolute, NaN where the reference has NaN: float64 on both sides, the margin covers scikit-learn's order
of operations only."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "contact_eval.npz"))


def _stack(d, key, ks):
    return np.stack([d["%s%d" % (key, k)] for k in ks])


def _groups(d):
    """camera groups of one size: the cameras main() saw (odd H and W: byte paths) and the extra one (even: dword paths)"""
    n_main, n = int(d["n_main"]), int(d["n"])
    return [list(range(n_main)), list(range(n_main, n))]


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# against the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_masks_labels_counts_collage_equal_the_reference(golden_dir):
    from manus_amd import contact_eval as ce
    d = _golden(golden_dir)
    for ks in _groups(d):
        frame, seg, rgba = _stack(d, "frame", ks), _stack(d, "seg", ks), _stack(d, "rgba", ks)
        pred, gt, hand, f8 = ce.contact_masks(frame, seg, rgba)
        np.testing.assert_array_equal(host(pred) * 255, _stack(d, "pred", ks))
        np.testing.assert_array_equal(host(gt) * 255, _stack(d, "gt", ks))
        np.testing.assert_array_equal(host(hand).astype(bool), _stack(d, "hand", ks))
        assert np.array_equal(host(f8), frame)                  # a uint8 frame comes back as it is
        W = seg.shape[2]
        for fr in (f8, f8[:, :, :W].contiguous()):              # the whole frame read in place, and the left half on its own
            labels, unfilled = ce.skin_labels(fr, hand, return_unfilled=True)
            np.testing.assert_array_equal(host(unfilled), _stack(d, "labels_unfilled", ks))
            np.testing.assert_array_equal(host(labels), _stack(d, "labels", ks))
        assert np.array_equal(host(ce.skin_labels(f8, hand, fill=False)), host(unfilled))
        want = _stack(d, "counts", ks)                          # (V, 3 methods, 17, 3)
        masks = {"ours": pred, "mano": torch.tensor(_stack(d, "mano_mask", ks) // 255, device=DEV),
                 "harp": torch.tensor(_stack(d, "harp_mask", ks) // 255, device=DEV)}
        for j, m in enumerate(("ours", "mano", "harp")):
            counts = ce.contact_counts(masks[m], gt, labels)
            assert counts.dtype == torch.int64 and tuple(counts.shape) == (len(ks), 17, 3)
            np.testing.assert_array_equal(host(counts), want[:, j])
            iou, f1 = ce.scores_from_counts(counts)
            ref_iou, ref_f1 = _stack(d, "iou", ks)[:, j], _stack(d, "f1", ks)[:, j]
            print(m, "max |iou - ref|", np.nanmax(np.abs(iou - ref_iou)), "max |f1 - ref|", np.nanmax(np.abs(f1 - ref_f1)))
            np.testing.assert_allclose(iou, ref_iou, rtol=0, atol=1e-9)
            np.testing.assert_allclose(f1, ref_f1, rtol=0, atol=1e-9, equal_nan=True)
        np.testing.assert_array_equal(host(ce.collage_rows(rgba, [gt, pred])), _stack(d, "row", ks))
        np.testing.assert_array_equal(host(ce.collage_rows(rgba, torch.stack([gt, masks["mano"], masks["harp"], pred]))), _stack(d, "row5", ks))
    lab = _stack(d, "labels", range(int(d["n"]))[:1])
    assert (lab == 16).any() and np.isnan(d["f10"]).any()


def test_evaluator_and_file_route_write_the_reference_files(golden_dir, tmp_path):
    """ContactEvaluator with baselines = get_iou.py, without and per_bone=False = get_iou_ours.py: CSV text string-equal,
    collage PNG pixel-equal; evaluate_directory on the reference's directory layout with naturally sorted names."""
    from PIL import Image
    from manus_amd import contact_eval as ce
    d = _golden(golden_dir)
    order = [int(i) for i in d["main_order"]]
    names = [str(n) for n in d["main_names"]]
    full = ce.ContactEvaluator(str(tmp_path / "a"), per_bone=True)
    ours = ce.ContactEvaluator(str(tmp_path / "b"), per_bone=False)
    for k in order:
        args = (names[k], torch.tensor(d["frame%d" % k], device=DEV), d["seg%d" % k], torch.tensor(d["rgba%d" % k], device=DEV))
        full.add(*args, baselines={"mano": d["mano%d" % k], "harp": d["harp%d" % k]})
        ours.add(*args)
    with pytest.raises(ValueError):
        full.add(*args)                                           # other baselines than the cameras before
    for ev, key in ((full, "full"), (ours, "ours")):
        res = ev.end()
        assert res["names"] == [names[k] for k in order]
        assert open(os.path.join(ev.out_dir, "eval_metric.csv"), newline="").read() == str(d["csv_" + key])
        png = np.asarray(Image.open(os.path.join(ev.out_dir, "eval_collage.png")).convert("RGB"))
        np.testing.assert_array_equal(png, d["collage_" + key])
        np.testing.assert_array_equal(res["collage"], d["collage_" + key])
    np.testing.assert_allclose(res["iou"]["ours"], _stack(d, "iou", order)[:, 0], rtol=0, atol=1e-9)
    # the file route
    exp, root = str(tmp_path / "exp"), tmp_path / "data" / "evals" / "obj_action"
    dirs = {"seg": str(root / "gt_contacts_seg"), "rgba": str(root / "gt_contacts"),
            "frame": os.path.join(exp, "results", "eval_results", "ours", "acc_gt_eval"),
            "mano": os.path.join(exp, "results", "eval_results", "mano", "acc_eval_rendered"),
            "harp": os.path.join(exp, "results", "eval_results", "harp", "acc_eval_rendered")}
    for p in dirs.values():
        os.makedirs(p)
    for k in range(len(names)):
        for key, p in dirs.items():
            Image.fromarray(d["%s%d" % (key, k)]).save(os.path.join(p, names[k] + ".png"))
    res = ce.evaluate_directory(exp, dirs["seg"])
    assert res["names"] == ce.natural_sorted(names)
    assert open(os.path.join(exp, "results", "eval_results", "eval_metric.csv"), newline="").read() == str(d["csv_full"])
    res = ce.evaluate_directory(exp, dirs["seg"], per_bone=False, baselines=())
    assert open(os.path.join(exp, "results", "eval_results", "eval_metric.csv"), newline="").read() == str(d["csv_ours"])
    png = np.asarray(Image.open(os.path.join(exp, "results", "eval_results", "eval_collage.png")).convert("RGB"))
    np.testing.assert_array_equal(png, d["collage_ours"])
    avg, last = ce.average_eval_metrics([os.path.join(exp, "results", "eval_results", "eval_metric.csv")])
    assert last["ours"] == float(str(d["csv_ours"]).splitlines()[1].split(",")[-1])


# ---------------------------------------------------------------------------------------------------------------------
# the fill against brute force
# ---------------------------------------------------------------------------------------------------------------------
def _brute_fill(unfilled, hand):
    """The integer rule on the device with torch: every residual pixel takes the label of the labelled pixel with the least
    (d^2, row * W + col); int64 coordinates, residual pixels in chunks."""
    H, W = unfilled.shape
    out = unfilled.clone()
    lab = torch.nonzero(unfilled > 0)                              # row-major order
    res = torch.nonzero((hand > 0) & (unfilled == 0))
    if res.shape[0] == 0:
        return out
    assert lab.shape[0] > 0
    ly, lx = lab[:, 0].long(), lab[:, 1].long()
    lidx = ly * W + lx
    chunk = max(1, (1 << 26) // max(1, lab.shape[0]))
    for s in range(0, res.shape[0], chunk):
        r = res[s:s + chunk].long()
        d2 = (r[:, 0:1] - ly[None]) ** 2 + (r[:, 1:2] - lx[None]) ** 2
        key = d2 * (1 << 32) + lidx[None]
        win = lidx[key.argmin(dim=1)]
        assert torch.equal(key.min(dim=1).values % (1 << 32), win)
        out[r[:, 0], r[:, 1]] = unfilled.reshape(-1)[win]
    return out


def _stamped_frame(g, H, W, n_blocks, box, n_res, one_pixel=False):
    """(frame_left (H,W,3) uint8, hand (H,W) uint8): 3x3 blocks of random palette colours with their top-left corners in
    `box` = (y0, y1, x0, x1) on black -- the opening keeps the cross of each -- and a hand of every pixel the opening keeps
    plus n_res random pixels (one_pixel: of the centre of the single block only)."""
    from manus_amd.contact_eval import PALETTE
    frame = np.zeros((H, W, 3), np.uint8)
    ys, xs = g.integers(box[0], box[1] - 3, n_blocks), g.integers(box[2], box[3] - 3, n_blocks)
    cols = PALETTE[g.integers(0, 16, n_blocks)]
    for dy in range(3):
        for dx in range(3):
            frame[ys + dy, xs + dx] = cols
    # the pixels the opening keeps, stated with scipy (the frame holds exact palette colours and black only)
    import scipy.ndimage as ndi
    cross = ndi.generate_binary_structure(2, 1)
    hand = np.zeros((H, W), bool)
    for c in PALETTE:
        m = (frame == c).all(axis=-1)
        if m.any():
            hand |= ndi.binary_dilation(ndi.binary_erosion(m, cross, border_value=1), cross, border_value=0)
    hand = hand.astype(np.uint8)
    if one_pixel:
        hand[:] = 0
        hand[ys[0] + 1, xs[0] + 1] = 1
    if n_res:
        hand.reshape(-1)[g.choice(H * W, n_res, replace=False)] = 1
    return frame, hand


def test_fill_equals_brute_force_at_1080p():
    from manus_amd import contact_eval as ce
    H = W = 1080
    g = np.random.default_rng(11)
    cases = [("random", _stamped_frame(g, H, W, 24000, (0, H, 0, W), 10000)),
             ("corner", _stamped_frame(g, H, W, 1500, (0, 160, 0, 200), 10000)),
             ("single pixel", _stamped_frame(g, H, W, 1, (700, 800, 900, 1000), 10000, one_pixel=True)),
             ("no residual", _stamped_frame(g, H, W, 5000, (0, H, 0, W), 0))]
    frame = torch.tensor(np.stack([c[1][0] for c in cases]), device=DEV)
    hand = torch.tensor(np.stack([c[1][1] for c in cases]), device=DEV)
    labels, unfilled = ce.skin_labels(frame, hand, return_unfilled=True)
    for v, (name, _) in enumerate(cases):
        n_lab, n_res = int((unfilled[v] > 0).sum()), int(((hand[v] > 0) & (unfilled[v] == 0)).sum())
        print("%s: %d labelled, %d residual pixels" % (name, n_lab, n_res))
        want = _brute_fill(unfilled[v], hand[v])
        assert torch.equal(labels[v], want), name
        assert bool((labels[v][hand[v] > 0] > 0).all()) and bool((labels[v][hand[v] == 0] == 0).all())
    counts = [(int((unfilled[v] > 0).sum()), int(((hand[v] > 0) & (unfilled[v] == 0)).sum())) for v in range(4)]
    assert counts[0][0] > 80000 and counts[0][1] > 8000           # about 1e5 labelled, 1e4 residual
    assert counts[2][0] == 1 and counts[3][1] == 0
    assert int(unfilled[1][200:, :].sum()) == 0 and int(unfilled[1][:, 240:].sum()) == 0
    again = ce.skin_labels(frame, hand)
    assert torch.equal(again, labels)


# ---------------------------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------------------------
def test_fp32_frame_gives_the_masks_of_the_uint8_conversion(golden_dir):
    from manus_amd import contact_eval as ce
    d = _golden(golden_dir)
    g = np.random.default_rng(3)
    for ks in _groups(d):
        seg, rgba = _stack(d, "seg", ks), _stack(d, "rgba", ks)
        f8 = _stack(d, "frame", ks)
        f32 = (f8.astype(np.float32) + g.uniform(0.02, 0.98, f8.shape).astype(np.float32)) / np.float32(255)
        f32[0, :4, :6] = (-0.3, 1.7, 127.999 / 255)             # clamped both ways
        img = (np.clip(f32, 0, 1) * 255).astype(np.uint8)       # base.py:245-246 (float32 * int stays float32)
        a = ce.contact_masks(torch.tensor(f32, device=DEV), seg, rgba)
        b = ce.contact_masks(img, seg, rgba)
        assert a[3].dtype == torch.uint8 and np.array_equal(host(a[3]), img)
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y)
        assert torch.equal(ce.skin_labels(a[3], a[2]), ce.skin_labels(img, b[2]))
    with pytest.raises(ValueError):
        ce.contact_masks(torch.zeros((1, 8, 16, 3), dtype=torch.float64, device=DEV), np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 8, 8, 4), np.uint8))
    with pytest.raises(ValueError):
        ce.contact_masks(np.zeros((1, 8, 16, 3), np.uint8), np.zeros((1, 8, 9, 3), np.uint8), np.zeros((1, 8, 8, 4), np.uint8))


def _chain(ce, frame, seg, rgba):
    pred, gt, hand, f8 = ce.contact_masks(frame, seg, rgba)
    labels = ce.skin_labels(f8, hand)
    return [pred, gt, hand, labels, ce.contact_counts(pred, gt, labels), ce.collage_rows(rgba, [gt, pred])]


def test_views_are_independent_and_repeats_bit_equal(golden_dir):
    from manus_amd import contact_eval as ce
    d = _golden(golden_dir)
    ks = _groups(d)[0]
    frame, seg, rgba = _stack(d, "frame", ks), _stack(d, "seg", ks), _stack(d, "rgba", ks)
    base = _chain(ce, frame, seg, rgba)
    for a, b in zip(base, _chain(ce, frame, seg, rgba)):
        assert torch.equal(a, b)
    k = 1
    f2, s2, r2 = frame.copy(), seg.copy(), rgba.copy()
    f2[k] = np.roll(frame[k], 7, axis=0)
    s2[k] = np.roll(seg[k], 5, axis=1)
    r2[k] = np.roll(rgba[k], 3, axis=0)
    other = _chain(ce, f2, s2, r2)
    for a, b in zip(base, other):
        for v in range(len(ks)):
            assert torch.equal(a[v], b[v]) == (v != k), v
    # one view on its own = its row of the batch
    for a, b in zip(base, _chain(ce, frame[2:3], seg[2:3], rgba[2:3])):
        assert torch.equal(a[2:3], b)


def test_residual_pixels_without_any_label_raise(golden_dir):
    from manus_amd import contact_eval as ce
    d = _golden(golden_dir)
    ks = _groups(d)[0]
    frame = _stack(d, "frame", ks)
    hand = torch.tensor(_stack(d, "hand", ks).astype(np.uint8), device=DEV)
    W = hand.shape[2]
    frame[1, :, :W] = 3                                           # no palette colour anywhere in view 1
    with pytest.raises(ValueError, match=r"view\(s\) 1 "):
        ce.skin_labels(frame, hand)
    unfilled = ce.skin_labels(frame, hand, fill=False)
    assert int(unfilled[1].sum()) == 0 and int(unfilled[0].sum()) > 0
    hand[1] = 0                                                   # no residual pixel either: nothing to fill, no error
    labels = ce.skin_labels(frame, hand)
    assert int(labels[1].sum()) == 0
    np.testing.assert_array_equal(host(labels[0]), d["labels0"])


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _composite_scene(n=20000, frames=3, W=160, H=120):
    from manus_amd.structures import Bones
    from manus_amd.synthetic import make_scene
    sc = make_scene(n_gaussians=n, kind="composite", seed=4, grid_res=24, n_cameras=2, width=W, height=H, cam_radius=0.5,
                    sigma_range=(1e-3, 3e-3), device="cpu", n_poses=frames)
    n_h = sc["n_hand"]
    P = {k: v.to(DEV) for k, v in sc["params"].items()}

    def model(sl, hand):
        m = SimpleNamespace(_xyz=P["_xyz"][sl].contiguous(), _scaling=P["_scaling"][sl].contiguous(), _rotation=P["_rotation"][sl].contiguous(),
                            get_features=torch.cat([P["_features_dc"][sl], P["_features_rest"][sl]], 1).contiguous(),
                            get_opacity=torch.sigmoid(P["_opacity"][sl]).contiguous())
        if hand:
            m.grid_center, m.grid_scale, m.grid_weights = sc["grid_center"], sc["grid_scale"], sc["grid"]
        return m

    def camera(c):
        return SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                               world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32),
                               full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32),
                               camera_center=torch.tensor(c["camera_center"], dtype=torch.float32)[None])

    batches = [dict(bones_posed=Bones(None, None, None, sc["posed"][f]), bones_rest=Bones(None, None, None, sc["rest"]),
                    camera=camera(sc["cameras"][0]), cano_camera=camera(sc["cameras"][1]), bg_color=torch.zeros(3))
               for f in range(frames)]
    return sc, model(slice(0, n_h), True), model(slice(n_h, None), False), batches


def test_end_to_end_from_the_renderer(tmp_path):
    """'gt_eval' over a grasp -> save_accumulated / load_accumulated -> 'acc_gt_eval' -> ContactEvaluator on the fp32 frame.
    Ground truth painted from the product's own frame: the identical mask scores IoU = I / (I + 1e-6) and F1 = 1; a mask
    shifted by five columns scores what numpy counts on the two masks."""
    from manus_amd import contact_eval as ce
    from manus_amd.modules import CompositeRenderer, hand_forward
    sc, hand, obj, batches = _composite_scene()
    H, W = 120, 160
    skin_w = hand_forward(hand, batches[0]).skin_wts
    skin = torch.tensor(ce.PALETTE.astype(np.float32) / 255, device=DEV)[skin_w.argmax(dim=1) % 16]
    first = CompositeRenderer(hand, obj, "gt_eval", c_thresh=0.02)
    with pytest.raises(ValueError):
        first.save_accumulated(str(tmp_path / "acc_contacts.npy"))
    for b in batches:
        assert tuple(first.render(b).render.shape) == (H, 2 * W, 3)
    path = str(tmp_path / "acc_contacts.npy")
    first.save_accumulated(path)
    np.testing.assert_array_equal(np.load(path), host(first.acc))
    second = CompositeRenderer(hand, obj, "acc_gt_eval", skin_colors=skin, c_thresh=0.02)
    assert torch.equal(second.load_accumulated(path), first.acc) and second.acc_contacts.is_cuda
    frame = second.render(batches[-1]).render                       # (H, 2W, 3) fp32 on the device
    assert tuple(frame.shape) == (H, 2 * W, 3) and frame.dtype == torch.float32
    img = (np.clip(host(frame), 0, 1) * 255).astype(np.uint8)
    pred_np = (img[:, W:] >= 128).all(axis=-1)
    assert pred_np.sum() > 20, "the synthetic grasp shows no contact in this camera"
    rgba = np.concatenate([img[:, :W], np.where(img[:, :W].any(axis=-1) | pred_np, 255, 0).astype(np.uint8)[..., None]], axis=-1)
    seg_same = img[:, W:].copy()
    seg_shift = np.zeros_like(seg_same)
    seg_shift[:, 5:] = seg_same[:, :-5]
    ev = ce.ContactEvaluator(str(tmp_path / "exp"))
    ev.add("same", frame, seg_same, rgba)
    ev.add("shifted", frame, seg_shift, rgba)
    res = ev.end()
    iou, f1 = res["iou"]["ours"], res["f1"]["ours"]
    n = int(pred_np.sum())
    assert iou[0, 16] == n / (n + 1e-6) and f1[0, 16] == 1.0
    gt_np = (seg_shift >= 128).all(axis=-1)
    I, A, B = int((gt_np & pred_np).sum()), int(gt_np.sum()), int(pred_np.sum())
    assert 0 < I < B
    assert iou[1, 16] == I / (A + B - I + 1e-6) and f1[1, 16] == 2 * I / (A + B)
    # per bone: the classes partition the combined counts but for label 16, and every hand pixel got a label
    pred, gt, hand_m, f8 = ce.contact_masks(frame, seg_shift, rgba)
    labels = ce.skin_labels(f8, hand_m)
    assert bool((labels[hand_m > 0] > 0).all())
    counts = host(ce.contact_counts(pred, gt, labels))[0]
    l16 = host(labels[0]) == 16
    np.testing.assert_array_equal(counts[:16].sum(axis=0) + [int((gt_np & pred_np & l16).sum()), int((gt_np & l16).sum()), int((pred_np & l16).sum())],
                                  counts[16])
    assert os.path.exists(os.path.join(str(tmp_path / "exp"), "results", "eval_results", "eval_metric.csv"))
    assert res["collage"].shape == (2 * H, 3 * W, 3)

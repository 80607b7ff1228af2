#!/usr/bin/env python3
"""Time the contact-evaluation kernels on the GPU against two other ways of computing the same thing.

    python tools/measure_contact_eval.py [--out FILE.json] [--quick] [--hip-only]

One process, HIP events, every shape warmed, median of 5 samples, 8 cameras of 1080x1080 (the reference's frame is
1080 + 1080 wide) with a hand over about a quarter of the image, painted in the 16 palette colours with blurred seams:
  (i)   the chain contact_masks -> skin_labels -> contact_counts -> collage_rows, and each kernel on its own through the
        library's event profiler (manus_amd._lib.profile_enable);
  (ii)  a plain torch composition of the same results on the same device: comparisons, max-pooling morphology, argmax,
        and the fill as the chunked all-pairs minimum over (d^2, index) keys in int64;
  (iii) the fill in the brute-force form the reference uses (one N_res x N_skin scan per camera; here the in-house
        mgr_contact_dist kernel on (row, col, 0) points, which has the taichi kernel's strict '<' rule);
  (i) again, so that the ways are alternated in one process.
The three fills are compared element for element and the number of differing pixels is printed.  Also printed: the
fill's residual pixels per second and the pair tests per second the brute-force scan would need to match it.
Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, repeats, samples=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / repeats)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), repeats=repeats)


def make_inputs(V, H, W, dev, palette):
    g = torch.Generator(device=dev).manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev).float(), torch.arange(W, device=dev).float(), indexing="ij")
    frames, segs, rgbas = [], [], []
    pal = torch.tensor(palette, device=dev).float()
    for v in range(V):
        cy, cx = H * (0.5 + 0.03 * v / V), W * (0.5 - 0.02 * v / V)
        hand = ((yy - cy) / (0.33 * H)) ** 2 + ((xx - cx) / (0.24 * W)) ** 2 <= 1.0
        seeds = torch.stack([cy + 0.3 * H * (torch.rand(16, device=dev, generator=g) * 2 - 1), cx + 0.22 * W * (torch.rand(16, device=dev, generator=g) * 2 - 1)], 1)
        cell = ((yy[..., None] - seeds[:, 0]) ** 2 + (xx[..., None] - seeds[:, 1]) ** 2).argmin(dim=-1)
        skin = pal[cell] * hand[..., None]
        skin = F.avg_pool2d(skin.permute(2, 0, 1)[None], 5, 1, 2)[0].permute(1, 2, 0).round()      # blurred seams and rim
        blob = ((yy - cy - 0.05 * H) / (0.12 * H)) ** 2 + ((xx - cx) / (0.1 * W)) ** 2 <= 1.0
        grey = (blob * 220.0)[..., None].expand(H, W, 3)
        frames.append(torch.cat([skin, grey], dim=1).to(torch.uint8))
        gtb = ((yy - cy - 0.03 * H) / (0.13 * H)) ** 2 + ((xx - cx - 0.02 * W) / (0.09 * W)) ** 2 <= 1.0
        segs.append((gtb * 255.0)[..., None].expand(H, W, 3).to(torch.uint8))
        photo = (127 + 100 * torch.sin(0.01 * xx + 0.013 * yy + v)).clamp(0, 255)
        rgbas.append(torch.stack([photo, photo * 0.8, photo * 0.6, hand * 255.0], dim=-1).to(torch.uint8))
    return torch.stack(frames).contiguous(), torch.stack(segs).contiguous(), torch.stack(rgbas).contiguous()


def torch_fill(unfilled, hand):
    """The all-pairs minimum over (d^2 << 32 | row * W + col), residual pixels in chunks."""
    H, W = unfilled.shape
    out = unfilled.clone()
    lab, res = torch.nonzero(unfilled > 0), torch.nonzero((hand > 0) & (unfilled == 0))
    if res.shape[0] == 0 or lab.shape[0] == 0:
        return out
    ly, lx = lab[:, 0], lab[:, 1]
    lidx = ly * W + lx
    chunk = max(1, (1 << 27) // lab.shape[0])
    for s in range(0, res.shape[0], chunk):
        r = res[s:s + chunk]
        key = ((r[:, 0:1] - ly[None]) ** 2 + (r[:, 1:2] - lx[None]) ** 2) * (1 << 32) + lidx[None]
        out[r[:, 0], r[:, 1]] = unfilled.reshape(-1)[lidx[key.argmin(dim=1)]]
    return out


def torch_chain(frame, seg, rgba, pal, fill=True):
    V, H, W2, _ = frame.shape
    W = W2 // 2
    pred = (frame[:, :, W:] >= 128).all(dim=-1)
    gt = (seg >= 128).all(dim=-1)
    hand = rgba[..., 3] > 128
    skin = frame[:, :, :W].to(torch.int16)
    labels = []
    for v in range(V):
        m = ((skin[v][:, :, None, :] - pal[None, None]).abs() <= 10).all(dim=-1).permute(2, 0, 1).float()[None]      # (1,16,H,W)
        # (a 3x3 pooling would be the square element: the cross is the centre and its four shifts)
        p = F.pad(m, (1, 1, 1, 1), value=1.0)
        e = torch.minimum(torch.minimum(p[..., 1:-1, 1:-1], p[..., :-2, 1:-1]), torch.minimum(torch.minimum(p[..., 2:, 1:-1], p[..., 1:-1, :-2]), p[..., 1:-1, 2:]))
        q = F.pad(e, (1, 1, 1, 1), value=0.0)
        dl = torch.maximum(torch.maximum(q[..., 1:-1, 1:-1], q[..., :-2, 1:-1]), torch.maximum(torch.maximum(q[..., 2:, 1:-1], q[..., 1:-1, :-2]), q[..., 1:-1, 2:]))[0]
        first = torch.cat([torch.zeros((1, H, W), device=dl.device), dl], 0).argmax(dim=0)
        lab = (first * hand[v]).to(torch.uint8)
        labels.append(torch_fill(lab, hand[v]) if fill else lab)
    labels = torch.stack(labels)
    counts = torch.zeros((V, 17, 3), dtype=torch.int64, device=frame.device)
    for i in range(17):
        sel = (labels == i) if i < 16 else torch.ones_like(gt)
        counts[:, i, 0] = (gt & pred & sel).sum(dim=(1, 2))
        counts[:, i, 1] = (gt & sel).sum(dim=(1, 2))
        counts[:, i, 2] = (pred & sel).sum(dim=(1, 2))
    return pred, gt, hand, labels, counts


def brute_fill(unfilled, hand):
    """One N_res x N_skin scan per camera, the form of the reference's taichi kernel (mgr_contact_dist)."""
    from manus_amd import contact
    out = unfilled.clone()
    for v in range(unfilled.shape[0]):
        lab, res = torch.nonzero(unfilled[v] > 0), torch.nonzero((hand[v] > 0) & (unfilled[v] == 0))
        if res.shape[0] == 0 or lab.shape[0] == 0:
            continue
        z = lambda p: torch.cat([p.float(), torch.zeros((p.shape[0], 1), device=p.device)], 1).contiguous()
        _, idx = contact._nearest(z(res), z(lab), True)
        win = lab[idx.long()]
        out[v][res[:, 0], res[:, 1]] = unfilled[v][win[:, 0], win[:, 1]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--hip-only", action="store_true", help="only the kernel chain, 10 times (for a rocprofv3 --kernel-trace --stats run)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_contact_eval.py needs a GPU"
    from manus_amd import _lib
    from manus_amd import contact_eval as ce
    dev = "cuda:0"
    V, H, W = (8, 1080, 1080) if not a.quick else (2, 96, 128)
    frame, seg, rgba = make_inputs(V, H, W, dev, ce.PALETTE)
    pal = torch.tensor(ce.PALETTE, device=dev).to(torch.int16)

    def hip():
        pred, gt, hand, f8 = ce.contact_masks(frame, seg, rgba)
        labels = ce.skin_labels(f8, hand)
        return pred, gt, hand, labels, ce.contact_counts(pred, gt, labels), ce.collage_rows(rgba, [gt, pred])

    if a.hip_only:
        for _ in range(10):
            hip()
        torch.cuda.synchronize()
        return
    pred, gt, hand, labels, counts, _ = hip()
    unfilled = ce.skin_labels(frame, hand, fill=False)
    n_lab = (unfilled > 0).sum(dim=(1, 2)).tolist()
    n_res = ((hand > 0) & (unfilled == 0)).sum(dim=(1, 2)).tolist()
    ref = torch_chain(frame, seg, rgba, pal)
    brute = brute_fill(unfilled, hand)
    res = {"device": torch.cuda.get_device_name(0), "V": V, "H": H, "W": W, "labelled_pixels": n_lab, "residual_pixels": n_res,
           "hand_share": float((hand > 0).float().mean()),
           "labels_differing_from_torch_composition": int((labels != ref[3]).sum()),
           "labels_differing_from_brute_force_scan": int((labels != brute).sum()),
           "counts_differing_from_torch_composition": int((counts != ref[4]).sum()),
           "iou_combined": ce.scores_from_counts(counts)[0][:, 16].tolist()}
    reps = 10 if not a.quick else 2
    res["hip_chain"] = timed(hip, reps)
    res["torch_composition"] = timed(lambda: torch_chain(frame, seg, rgba, pal), 1, samples=3)
    res["torch_composition_without_fill"] = timed(lambda: torch_chain(frame, seg, rgba, pal, fill=False), 1, samples=3)
    res["brute_force_scan_fill"] = timed(lambda: brute_fill(unfilled, hand), 1, samples=3)
    res["hip_chain_again"] = timed(hip, reps)
    # per kernel, by the library's events
    _lib.profile_enable(True)
    _lib.profile_report()
    for _ in range(reps):
        hip()
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    res["kernel_ms"] = {k: ms / cnt for k, (cnt, ms) in rep.items() if k.startswith("k_ceval")}
    fill_ms = res["kernel_ms"].get("k_ceval_fill", float("nan"))
    pairs = float(sum(r * l for r, l in zip(n_res, n_lab)))
    res["fill_residual_pixels_per_s"] = sum(n_res) / (fill_ms * 1e-3)
    res["pair_tests_of_the_scan"] = pairs
    res["pair_tests_per_s_the_scan_would_need"] = pairs / (fill_ms * 1e-3)
    res["brute_force_scan_pair_tests_per_s"] = pairs / (res["brute_force_scan_fill"]["median_ms"] * 1e-3)
    # bytes the chain must move per pixel: frame 6 + seg 3 + rgba 4 read, masks 3 written (masks); left half 3 + hand 1 read,
    # label 1 written (labels); 3 read (counts); rgba 4 + masks 2 read, 9 written (collage)
    px = V * H * W
    res["bytes_min"] = {"k_ceval_masks": px * 16, "k_ceval_labels": px * 5, "k_ceval_counts": px * 3, "k_ceval_collage": px * 15}
    res["GBps"] = {k: b / (res["kernel_ms"][k] * 1e-3) / 1e9 for k, b in res["bytes_min"].items() if k in res["kernel_ms"]}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

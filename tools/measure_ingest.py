#!/usr/bin/env python3
"""Time the way from dataset items to the targets of a step: `SequenceDataset.view_batch` on the host against the device frame
store (`frames.FrameStore`, mgr_frames_decode).

    python tools/measure_ingest.py [--out FILE.json] [--quick]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats), 8 views of
1920x1080 with 480x480 crops (a synthetic capture in the dataset's schema, two frames of 8 cameras, the crops of the second frame
somewhere else in the image):
  * `view_batch` of 8 items on the host, including its copy to the device;
  * `store.decode` of 8 views, whole images and dirty rectangles (alternating between the two frames), at k = 1 and at k = 2
    (960x540 out of the same source frames);
  * one fused HipViewCompute step (300k Gaussians on the capture's skeleton, l1+ssim) with unchanged views against a step right
    after `load_step` (alternating between the two frames): the gap is the decode, the small table copies and the rebuild of the
    loss's target map and the other per-view constants.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from measure_feature_render import timed  # noqa: E402


def write_capture(path, width, height, crop, n_cams, focal):
    """Two frames of `n_cams` cameras, every crop `crop` x `crop` with a round alpha mask, at a random place per (frame, camera)."""
    from manus_amd import dataset as D
    arr = D.synthetic_sequence(3, n_frames=2, n_cams=n_cams, width=width, height=height)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:crop, 0:crop]
    disc = ((xx - crop / 2) ** 2 + (yy - crop / 2) ** 2 <= (crop / 2) ** 2)
    for key in [k for k in arr if "/images/" in k]:
        c = rng.integers(0, 256, (crop, crop, 4), dtype=np.uint8)
        c[..., 3] = np.where(disc, 255, 0)
        x0, y0 = 2 * int(rng.integers(0, (width - crop) // 2)), 2 * int(rng.integers(0, (height - crop) // 2))
        arr[key] = c
        arr[key.replace("/images/", "/bbox/")] = np.array([x0, y0, x0 + crop, y0 + crop], np.int64)
    for key in [k for k in arr if k.startswith("K/")]:
        arr[key] = np.array([[focal, 0, width / 2 - 0.5], [0, focal, height / 2 - 0.5], [0, 0, 1]], np.float64)
    D.write_tree(os.path.join(path, "grasp_1.npz"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_ingest.py needs a GPU"
    from manus_amd import dataset as D
    from manus_amd.engine import HipViewCompute
    from manus_amd.frames import FrameStore
    from manus_amd.synthetic import camera_table
    dev = "cuda:0"
    V, N, W, H, crop = (8, 300000, 1920, 1080, 480) if not a.quick else (3, 3000, 96, 64, 24)
    opts = dict(bg_color="white", subject="s1", rand_views_per_timestep=-1, n_bones=20, num_time_steps=-1, split_ratio=1.0,
                sequences="all", split_by_action=False, width=W, height=H)
    first, second = list(range(V)), list(range(V, 2 * V))
    res = {"device": torch.cuda.get_device_name(0), "sizes": dict(V=V, N=N, W=W, H=H, crop=crop), "host": {}, "decode": {}, "step": {}}
    with tempfile.TemporaryDirectory() as tmp:
        write_capture(tmp, W, H, crop, V, 1800.0 if not a.quick else 90.0)
        ds = D.SequenceDataset(tmp, dict(opts, resize_factor=1.0), "train")
        res["host"]["view_batch"] = timed(lambda: ds.view_batch(first, dev), 1)
        print("host view_batch", json.dumps(res["host"]["view_batch"]), flush=True)
        rep = 20 if not a.quick else 3
        for k in (1, 2):
            dsk = ds if k == 1 else D.SequenceDataset(tmp, dict(opts, resize_factor=0.5), "train")
            st = FrameStore.from_dataset(dsk, device=dev)
            tg = torch.empty((V, 3, H // k, W // k), device=dev)
            mk = torch.empty((V, H // k, W // k), device=dev)
            white = np.ones(3, np.float32)
            turn = [0]

            def decode(dirty, masks):
                turn[0] ^= 1
                st.decode(second if turn[0] else first, white, tg, mk if masks else None, dirty=dirty)

            r = res["decode"]["k%d" % k] = {"pool_bytes": st.nbytes, "out": [H // k, W // k]}
            for key, dirty, masks in (("full", False, True), ("dirty", True, True), ("full_no_masks", False, False), ("full_again", False, True),
                                      ("dirty_again", True, True)):
                r[key] = timed(lambda: decode(dirty, masks), rep)
                print("decode k=%d %s" % (k, key), json.dumps(r[key]), flush=True)
            if k == 1:
                store = st
        # the step: unchanged views against freshly loaded ones
        batch = ds.view_batch(first)
        scene, targets = D.hand_scene_from_batch(batch, ds[0]["bones_rest"], N, seed=1, device=dev)
        hc = HipViewCompute(scene, targets, camera_table(scene["cameras"], dev), loss="l1+ssim",
                            mask_targets=scene["masks"].float().contiguous().clone())
        ids = list(range(V))
        turn = [0]

        def loaded_step():
            turn[0] ^= 1
            store.load_step(hc, second if turn[0] else first)
            hc(ids, 1.0 / V)

        def load_only():
            turn[0] ^= 1
            store.load_step(hc, second if turn[0] else first)

        for key, fn in (("unchanged", lambda: hc(ids, 1.0 / V)), ("after_load_step", loaded_step), ("unchanged_again", lambda: hc(ids, 1.0 / V)),
                        ("after_load_step_again", loaded_step), ("load_step_alone", load_only)):
            res["step"][key] = timed(fn, rep)
            print("step %s" % key, json.dumps(res["step"][key]), flush=True)
        D.close_sequences()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

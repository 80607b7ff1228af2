#!/usr/bin/env python3
"""Time the feature render (rasterizer.blend_features) against a second full forward, and one 'results' frame of
CompositeRenderer with share_binning off and on.

    python tools/measure_feature_render.py [--out FILE.json] [--quick]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats):
  (i)  on the bench scene (300k hand Gaussians, one 1920x1080 view of the posed hand, evaluation forward):
       blend_features at C = 3 and C = 9, depth + alpha alone, and a second mgr_raster_forward of the same geometry
       (rasterize_views under no_grad: projection, instance sort, binning, blend, and the blocking read of the pair count)
  (ii) one 'results' frame of modules.CompositeRenderer at 1920x1080 on the composite scene of tools/measure_contact.py
       (300k hand + 200k object), share_binning off, on, off.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, repeats, samples=5):
    fn()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_feature_render.py needs a GPU"
    from types import SimpleNamespace
    from manus_amd import rasterizer as rz
    from manus_amd.modules import CompositeRenderer, hand_forward
    from manus_amd.render import calculate_colors_from_sh
    from manus_amd.structures import Bones
    from manus_amd.synthetic import camera_table, make_scene
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "blend_features": {}, "frames": {}}

    def model(P, sl, sc=None):
        m = SimpleNamespace(_xyz=P["_xyz"][sl].contiguous(), _scaling=P["_scaling"][sl].contiguous(), _rotation=P["_rotation"][sl].contiguous(),
                            get_features=torch.cat([P["_features_dc"][sl], P["_features_rest"][sl]], 1).contiguous(),
                            get_opacity=torch.sigmoid(P["_opacity"][sl]).contiguous())
        if sc is not None:
            m.grid_center, m.grid_scale, m.grid_weights = sc["grid_center"], sc["grid_scale"], sc["grid"]
        return m

    def camera(c):
        return SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                               world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32, device=dev),
                               full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32, device=dev),
                               camera_center=torch.tensor(c["camera_center"], dtype=torch.float32, device=dev)[None])

    # (i) the bench scene, one view
    n = 300000 if not a.quick else 5000
    sc = make_scene(n_gaussians=n, kind="hand", seed=0, grid_res=128 if not a.quick else 24, n_cameras=1, device="cpu", cam_radius=1.2)
    P = {k: v.to(dev) for k, v in sc["params"].items()}
    batch = dict(bones_posed=Bones(None, None, None, sc["posed"][0]), bones_rest=Bones(None, None, None, sc["rest"]))
    W, H = sc["cameras"][0]["width"], sc["cameras"][0]["height"]
    with torch.no_grad():
        pred = hand_forward(model(P, slice(None), sc), batch)
        col = calculate_colors_from_sh(pred.posed_xyz, pred.cano_features, pred.cano_xyz, camera(sc["cameras"][0]), 3, pred.tf)
        ct = camera_table(sc["cameras"][:1], dev)
        bg = torch.ones(3, device=dev)
        m2d = torch.zeros((1, n, 3), device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        f9 = torch.rand((n, 9), device=dev, generator=g)
        f3, bg9 = f9[:, :3].contiguous(), torch.rand(9, device=dev, generator=g)
        full = lambda: rz.rasterize_views(ct, pred.posed_xyz, m2d, col, pred.cano_opacity, pred.posed_cov, bg, W, H)
        for _ in range(3):
            img, _ = full()
        same = rz.blend_features(col, bg=bg)["features"]
        res["blend_features"]["max_abs_diff_of_the_forward_colours_as_features"] = float((same - img).abs().max())
        # alternate the calls in one process; every blend_features works on the lists of the forward warmed above
        for key, fn, rep in (("C=3", lambda: rz.blend_features(f3, bg=bg9[:3]), 10),
                             ("second_full_forward", full, 10),
                             ("C=9", lambda: rz.blend_features(f9, bg=bg9), 10),
                             ("depth+alpha", lambda: rz.blend_features(depth=True, alpha=True), 10),
                             ("C=3_again", lambda: rz.blend_features(f3, bg=bg9[:3]), 10),
                             ("second_full_forward_again", full, 10)):
            res["blend_features"][key] = timed(fn, rep)
            print("%dx%d, %d Gaussians, %s" % (W, H, n, key), json.dumps(res["blend_features"][key]), flush=True)

    # (ii) one 'results' frame on the composite scene
    n = 500000 if not a.quick else 5000
    sc = make_scene(n_gaussians=n, kind="composite", seed=0, grid_res=128 if not a.quick else 24, n_cameras=2, device="cpu", n_poses=1)
    n_h = sc["n_hand"]
    P = {k: v.to(dev) for k, v in sc["params"].items()}
    batch = dict(bones_posed=Bones(None, None, None, sc["posed"][0]), bones_rest=Bones(None, None, None, sc["rest"]),
                 camera=camera(sc["cameras"][0]), cano_camera=camera(sc["cameras"][1]), bg_color=torch.ones(3, device=dev))
    hm, om = model(P, slice(0, n_h), sc), model(P, slice(n_h, None))
    for share in (False, True, False):
        R = CompositeRenderer(hm, om, "results", share_binning=share)
        with torch.no_grad():
            r = timed(lambda: R.render(batch), 2)
        res["frames"].setdefault("share_binning=%s" % share, []).append(r)
        print("results frame 1920x1080, %d + %d Gaussians, share_binning=%s" % (n_h, n - n_h, share), json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

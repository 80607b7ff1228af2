#!/usr/bin/env python3
"""Time the feature render's backward (mgr_raster_blend_features_backward) against the colour backward (mgr_raster_backward) of
the same forward.

    python tools/measure_feature_grad.py [--out FILE.json] [--quick]

One process, HIP events, every shape warmed, median of 5 samples with min - max (each sample a batch of repeats), on the bench
scene of tools/measure_feature_render.py (300k hand Gaussians, one 1920x1080 view of the posed hand): the feature backward for
alpha only, depth + alpha, 8 channels + depth + alpha and 32 channels + depth + alpha, through the C ABI (each call includes its
blocking read of the workspace header and the clearing of its scratch tags), alternated with mgr_raster_backward on the same
workspace.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from measure_feature_render import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_feature_grad.py needs a GPU"
    from types import SimpleNamespace
    from manus_amd import rasterizer as rz
    from manus_amd._lib import check, lib, ptr, stream
    from manus_amd.modules import hand_forward
    from manus_amd.render import calculate_colors_from_sh
    from manus_amd.structures import Bones
    from manus_amd.synthetic import camera_table, make_scene
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "backward": {}}
    n = 300000 if not a.quick else 5000
    sc = make_scene(n_gaussians=n, kind="hand", seed=0, grid_res=128 if not a.quick else 24, n_cameras=1, device="cpu", cam_radius=1.2)
    P = {k: v.to(dev) for k, v in sc["params"].items()}
    m = SimpleNamespace(_xyz=P["_xyz"], _scaling=P["_scaling"], _rotation=P["_rotation"],
                        get_features=torch.cat([P["_features_dc"], P["_features_rest"]], 1).contiguous(),
                        get_opacity=torch.sigmoid(P["_opacity"]).contiguous(), grid_center=sc["grid_center"], grid_scale=sc["grid_scale"],
                        grid_weights=sc["grid"])
    c0 = sc["cameras"][0]
    cam = SimpleNamespace(fovx=c0["fovx"], fovy=c0["fovy"], height=c0["height"], width=c0["width"],
                          world_view_transform=torch.tensor(c0["world_view_transform"], dtype=torch.float32, device=dev),
                          full_proj_transform=torch.tensor(c0["full_proj_transform"], dtype=torch.float32, device=dev),
                          camera_center=torch.tensor(c0["camera_center"], dtype=torch.float32, device=dev)[None])
    batch = dict(bones_posed=Bones(None, None, None, sc["posed"][0]), bones_rest=Bones(None, None, None, sc["rest"]))
    W, H = c0["width"], c0["height"]
    with torch.no_grad():
        pred = hand_forward(m, batch)
        col = calculate_colors_from_sh(pred.posed_xyz, pred.cano_features, pred.cano_xyz, cam, 3, pred.tf).contiguous()
        ct = camera_table(sc["cameras"][:1], dev)
        bg = torch.ones(3, device=dev)
        means, cov, op = pred.posed_xyz.contiguous(), pred.posed_cov.contiguous(), pred.cano_opacity.reshape(-1).contiguous()
        for _ in range(3):
            img, _ = rz.rasterize_views(ct, means, torch.zeros((1, n, 3), device=dev), col, op, cov, bg, W, H)
        ws = rz.context().last_ws
        g = torch.Generator(device=dev).manual_seed(1)
        f32 = torch.rand((n, 32), device=dev, generator=g)
        gmaps = torch.randn((1, 34, H, W), device=dev, generator=g)
        d3, d2, dop, dcov = (torch.empty((1, n, k), device=dev) for k in (3, 3, 1, 6))
        dcol, df = torch.empty((1, n, 3), device=dev), torch.empty((1, n, 32), device=dev)

        def colour_backward():
            check(lib().mgr_raster_backward(1, n, W, H, ptr(ct), ptr(bg), ptr(means), 0, ptr(cov), 0, ptr(col), 0, ptr(op), 0, ptr(img),
                                            ptr(gmaps[:, :3].contiguous()), ptr(d3), ptr(d2), ptr(dcol), ptr(dop), ptr(dcov), ptr(ws.buf),
                                            ws.nbytes, ws.cap, 0, stream()), "mgr_raster_backward")

        def feature_backward(C, depth, alpha):
            feat = f32[:, :C].contiguous() if C else None
            maps = rz.blend_features(feat, depth=depth, alpha=alpha)
            n_out = C + int(depth)
            out = torch.cat([x for x in (maps["features"], maps["depth"][:, None] if depth else None) if x is not None], 1).contiguous() if n_out else None
            g_out = gmaps[:, :n_out].contiguous() if n_out else None
            g_a = gmaps[:, 33].contiguous() if alpha else None
            need = int(lib().mgr_raster_feat_backward_workspace_bytes(1, n, C, W, H, ws.cap))
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)

            def call():
                check(lib().mgr_raster_blend_features_backward(1, n, C, W, H, ptr(ct), ptr(means), 0, ptr(cov), 0, ptr(feat), 0, None, int(depth),
                                                               ptr(out), ptr(maps["alpha"]), ptr(g_out), ptr(g_a), ptr(d3), ptr(d2), ptr(dop),
                                                               ptr(dcov), ptr(df[:, :, :C].contiguous()) if C else None, ptr(ws.buf), ws.nbytes,
                                                               ws.cap, ptr(scratch), need, 0, stream()), "mgr_raster_blend_features_backward")
            return call

        res["backward"]["scratch_bytes"] = int(lib().mgr_raster_feat_backward_workspace_bytes(1, n, 32, W, H, ws.cap))
        res["backward"]["workspace_bytes"] = int(ws.nbytes)
        for key, fn in (("colour_backward", colour_backward), ("alpha", feature_backward(0, False, True)),
                        ("depth+alpha", feature_backward(0, True, True)), ("C=8+depth+alpha", feature_backward(8, True, True)),
                        ("colour_backward_again", colour_backward), ("C=32+depth+alpha", feature_backward(32, True, True)),
                        ("alpha_again", feature_backward(0, False, True))):
            res["backward"][key] = timed(fn, 5)
            print("%dx%d, %d Gaussians, %s" % (W, H, n, key), json.dumps(res["backward"][key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

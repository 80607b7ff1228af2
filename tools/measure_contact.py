#!/usr/bin/env python3
"""Time the contact-map searches and one 'results' frame of CompositeRenderer on the GPU.

    python tools/measure_contact.py [--out FILE.json] [--quick]

One process, HIP events, every shape warmed, median of 5 samples (each sample a batch of repeats for the short calls):
  (i)   contact.get_cmap_values   brute-force search (mgr_contact_dist) + torch value formula
  (ii)  contact.get_cmap_near     grid search (mgr_contact_near) + colour lookup
  (iii) one 'results' frame of modules.CompositeRenderer at 1920x1080 with each search
at 300k x 200k and 300k x 20k points, both directions.  Needs a GPU; there is no fallback."""
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
    assert torch.cuda.is_available(), "measure_contact.py needs a GPU"
    from types import SimpleNamespace
    from manus_amd import contact
    from manus_amd.modules import CompositeRenderer
    from manus_amd.structures import Bones
    from manus_amd.synthetic import make_scene
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "searches": {}, "frames": {}}
    g = torch.Generator(device=dev).manual_seed(3)
    n_big, n_mid, n_small = (300000, 200000, 20000) if not a.quick else (3000, 2000, 200)
    hand = torch.randn((n_big, 3), device=dev, generator=g) * 0.05
    for n2 in (n_mid, n_small):
        obj = torch.randn((n2, 3), device=dev, generator=g) * 0.05 + torch.tensor([0.04, 0.0, 0.0], device=dev)
        for name, p1, p2 in (("hand->object", hand, obj), ("object->hand", obj, hand)):
            key = "%dx%d %s" % (n_big, n2, name)
            v_old = contact.get_cmap_values(p1, p2)[0]
            v_new = contact.get_cmap_near(p1, p2)[0]
            r = {"in_contact": float((v_new > 0).float().mean()), "values_differing_from_get_cmap_values": int((v_old != v_new).sum())}
            # alternate the two in one process
            r["get_cmap_values"] = timed(lambda: contact.get_cmap_values(p1, p2), 3)
            r["get_cmap_near"] = timed(lambda: contact.get_cmap_near(p1, p2), 20)
            r["get_cmap_values_again"] = timed(lambda: contact.get_cmap_values(p1, p2), 3)
            res["searches"][key] = r
            print(key, json.dumps(r), flush=True)
    # one 'results' frame at 1920x1080 on the synthetic composite scene (BASELINE cfg4 sizes: 300k hand + 200k object)
    n = 500000 if not a.quick else 5000
    sc = make_scene(n_gaussians=n, kind="composite", seed=0, grid_res=128 if not a.quick else 24, n_cameras=2, device="cpu", n_poses=1)
    n_h = sc["n_hand"]
    P = {k: v.to(dev) for k, v in sc["params"].items()}

    def model(sl, is_hand):
        m = SimpleNamespace(_xyz=P["_xyz"][sl].contiguous(), _scaling=P["_scaling"][sl].contiguous(), _rotation=P["_rotation"][sl].contiguous(),
                            get_features=torch.cat([P["_features_dc"][sl], P["_features_rest"][sl]], 1).contiguous(),
                            get_opacity=torch.sigmoid(P["_opacity"][sl]).contiguous())
        if is_hand:
            m.grid_center, m.grid_scale, m.grid_weights = sc["grid_center"], sc["grid_scale"], sc["grid"]
        return m

    def camera(c):
        return SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                               world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32, device=dev),
                               full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32, device=dev),
                               camera_center=torch.tensor(c["camera_center"], dtype=torch.float32, device=dev)[None])

    batch = dict(bones_posed=Bones(None, None, None, sc["posed"][0]), bones_rest=Bones(None, None, None, sc["rest"]),
                 camera=camera(sc["cameras"][0]), cano_camera=camera(sc["cameras"][1]), bg_color=torch.ones(3, device=dev))
    hm, om = model(slice(0, n_h), True), model(slice(n_h, None), False)
    for search in ("brute", "near", "brute"):
        R = CompositeRenderer(hm, om, "results", search=search)
        with torch.no_grad():
            r = timed(lambda: R.render(batch), 2)
        res["frames"].setdefault(search, []).append(r)
        print("results frame 1920x1080, %d + %d Gaussians, search=%s" % (n_h, n - n_h, search), json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

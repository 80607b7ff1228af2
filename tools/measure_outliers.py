#!/usr/bin/env python3
"""Time the exact k-nearest search and the LoOP scores (mgr_knn_self / mgr_outlier_scores, csrc/knn_k.hip) on the centres of
the bench hand (300 k Gaussians) and of a 500 k composite, at k = 128 and k = 512:

    knn_self                 the search alone, sigma and count out (no (N,k) output)
    knn_self_idx_d2          the search with the (N,k) indices and distances written
    outlier_scores           search + second pass over the stored indices + scores, mask and stats
    torch_cdist_topk         the comparison: chunked torch.cdist(chunk, all).topk(k, largest=False) on the same device (its
                             squared distances come from a matrix product, so it is a cost yardstick, not a bit reference)
    densify_off / densify_on `GaussianOptimizer.densify_and_prune` on the 300 k hand with remove_outliers off and on (a
                             fresh optimizer per sample, its construction outside the timed region; every third row carries
                             a gradient above the threshold)

    python tools/measure_outliers.py [--out FILE.json] [--quick] [--search-only]

One process, HIP events, every shape warmed, median of 5 samples with min and max (`measure_pose_refine.timed`).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from measure_pose_refine import timed  # noqa: E402

DEV = "cuda:0"


def cdist_topk(x, k, chunk=4096):
    out = []
    for s in range(0, x.shape[0], chunk):
        out.append(torch.cdist(x[s:s + chunk], x).topk(k, dim=1, largest=False).indices)
    return out


def timed_fresh(make, run, samples=5):
    """`run(make())` with only `run` inside the events: for calls that consume their input."""
    out = []
    for it in range(samples + 1):
        obj = make()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(obj)
        b.record()
        b.synchronize()
        if it:
            out.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), repeats=1)


def measure_points(name, xyz, ks, res, quick, search_only=False):
    from manus_amd.outliers import knn_self, outlier_scores
    N = xyz.shape[0]
    for k in ks:
        key = "%s_N%d_k%d" % (name, N, k)
        out = res.setdefault(key, {"shape": dict(N=N, k=k)})
        rows = (("knn_self", lambda: knn_self(xyz, k), 3), ("knn_self_idx_d2", lambda: knn_self(xyz, k, want_d2=True, want_idx=True), 3),
                ("outlier_scores", lambda: outlier_scores(xyz, k=k, prob=0.8), 3), ("torch_cdist_topk", lambda: cdist_topk(xyz, k), 1))
        for row, fn, reps in rows[:1] if search_only else rows:
            out[row] = timed(fn, 1 if quick else reps)
            print("%-28s %-18s %s" % (key, row, json.dumps(out[row])), flush=True)
        s = outlier_scores(xyz, k=k, prob=0.8)
        out["stats_nplof_valid_flagged"] = s.stats.cpu().tolist()
        print("%-28s stats %s" % (key, out["stats_nplof_valid_flagged"]), flush=True)


def measure_densify(scene, res):
    from manus_amd.optim import GaussianOptimizer
    params = {k: v.to(DEV) for k, v in scene["params"].items()}
    N = params["_xyz"].shape[0]
    noise = torch.randn((2 * N, 3), device=DEV)

    def make():
        go = GaussianOptimizer(params, opts=dict(percent_dense=0.01))
        go.xyz_gradient_accum[::3] = 0.001
        go.denom.fill_(1.0)
        return go

    out = res.setdefault("densify_N%d" % N, {})
    for row, flag in (("densify_off", False), ("densify_on", True)):
        out[row] = timed_fresh(make, lambda go: go.densify_and_prune(0.0002, 0.005, 1.0, None, remove_outliers=flag, noise=noise, noise_is_pool=True))
        print("%-28s %-18s %s" % ("densify_N%d" % N, row, json.dumps(out[row])), flush=True)
    go = make()
    out["info_on"] = go.densify_and_prune(0.0002, 0.005, 1.0, None, remove_outliers=True, noise=noise, noise_is_pool=True)
    print("densify_on info %s" % json.dumps(out["info_on"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--search-only", action="store_true", help="the knn_self rows only (e.g. on a library built with another MGR_KNN_CELL_K_DIV: "
                    "MGR_VARIANT=div4 MGR_EXTRA_FLAGS=-DMGR_KNN_CELL_K_DIV=4.0f python -m manus_amd.build, then MANUS_HIP_VARIANT=div4)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_outliers.py needs a GPU"
    from manus_amd.synthetic import make_scene
    res = {"device": torch.cuda.get_device_name(0)}
    n_hand, n_comp = (300000, 500000) if not a.quick else (20000, 30000)
    hand = make_scene(n_gaussians=n_hand, kind="hand", grid_res=16, n_cameras=1, width=64, height=64)
    measure_points("hand", hand["params"]["_xyz"].to(DEV).contiguous(), (128, 512), res, a.quick, a.search_only)
    comp = make_scene(n_gaussians=n_comp, kind="composite", grid_res=16, n_cameras=1, width=64, height=64)
    measure_points("composite", comp["params"]["_xyz"].to(DEV).contiguous(), (128, 512), res, a.quick, a.search_only)
    if not a.search_only:
        measure_densify(hand, res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

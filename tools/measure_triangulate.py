#!/usr/bin/env python3
"""Time the robust multi-view triangulation (mgr_triangulate, csrc/triangulate.hip) at F = 512 frames of the hand's K = 21 keypoints
with C = 53 cameras (the BRICS rig) and with C = 8, on the fixtures of tests/triangulate_ref.py (a ring of cameras, 0.5 px of noise,
a fifth of the detections outliers at C = 53 and one per problem at C = 8):

    triangulate              the entry with its defaults (seed over all pairs, two refits, two Gauss-Newton steps), all five outputs
    triangulate_no_polish    the same with gn_iters = 0
    triangulate_lean         the defaults with inliers and dist NULL
    torch_plain_solve        the plain NON-robust weighted solve -- planes, N = sum s (n n^T), X = N^-1 b over every confident
                             detection, no consensus -- as a composition of torch operators on the device: what the consensus
                             stage costs on top of a fit
    numpy_restatement        tests/triangulate_ref.triangulate (fp64) on the host, on the first 4 frames only (84 problems; one
                             sample, wall clock), reported per problem and scaled to the call

    python tools/measure_triangulate.py [--out FILE.json] [--quick]

One process, HIP events around a batch of calls, every shape warmed, median of 5 samples with min and max (`measure_pose_refine.timed`).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from measure_pose_refine import timed  # noqa: E402


def plain_solve(P, t, s, min_conf=0.1):
    """X (F,K,3): the weighted least-squares point of EVERY detection above min_conf on the normalised planes, device torch."""
    w = torch.where((s > min_conf) & torch.isfinite(t).all(-1), s, torch.zeros_like(s))      # (F,C,K)
    t = torch.nan_to_num(t)
    au = t[..., 0:1] * P[None, :, None, 2] - P[None, :, None, 0]                               # (F,C,K,4)
    av = t[..., 1:2] * P[None, :, None, 2] - P[None, :, None, 1]
    au = au / au[..., :3].norm(dim=-1, keepdim=True)
    av = av / av[..., :3].norm(dim=-1, keepdim=True)
    N = torch.einsum("fck,fcki,fckj->fkij", w, au[..., :3], au[..., :3]) + torch.einsum("fck,fcki,fckj->fkij", w, av[..., :3], av[..., :3])
    b = -(torch.einsum("fck,fck,fcki->fki", w, au[..., 3], au[..., :3]) + torch.einsum("fck,fck,fcki->fki", w, av[..., 3], av[..., :3]))
    return torch.linalg.solve(N, b)


def measure(C, F, K, a, res):
    import numpy as np
    import triangulate_ref as Q
    from manus_amd._lib import check, lib, ptr, stream
    dev = "cuda:0"
    fx = Q.fixture(C, F, K)
    P, t, s = (torch.tensor(fx[k]).to(dev).contiguous() for k in ("proj", "targets", "weights"))
    xyz, conf = torch.empty((F, K, 3), device=dev), torch.empty((F, K), device=dev)
    n_in = torch.empty((F, K), dtype=torch.int32, device=dev)
    inl, dist = torch.empty((F, C, K), dtype=torch.uint8, device=dev), torch.empty((F, C, K), device=dev)
    L = lib()

    def entry(gn=2, lean=False):
        check(L.mgr_triangulate(F, C, K, ptr(P), ptr(t), ptr(s), 25.0, 0.1, 3, 1e-2, 1e-6, 2, gn, ptr(xyz), ptr(conf), ptr(n_in),
                                None if lean else ptr(inl), None if lean else ptr(dist), stream()), "mgr_triangulate")

    key = "C%d_F%d" % (C, F)
    out = res.setdefault(key, {"shape": dict(F=F, C=C, K=K, problems=F * K, pairs=C * (C - 1) // 2)})
    reps = 20 if C > 16 else 100
    for name, fn, n in (("triangulate", entry, reps), ("triangulate_no_polish", lambda: entry(0), reps), ("triangulate_lean", lambda: entry(2, True), reps),
                        ("torch_plain_solve", lambda: plain_solve(P, t, s), 20), ("triangulate_again", entry, reps)):
        out[name] = timed(fn, n)
        print("%-10s %-24s %s" % (key, name, json.dumps(out[name])), flush=True)
    entry()
    torch.cuda.synchronize()
    valid = ~torch.isnan(xyz[..., 0])
    pts = torch.tensor(fx["points"], device=dev)
    plain = plain_solve(P, t, s).double()
    out["valid_problems"] = int(valid.sum())
    out["mean_error_mm"] = dict(triangulate=float((xyz.double() - pts).norm(dim=-1)[valid].mean()) * 1e3,
                                torch_plain_solve=float((plain - pts).norm(dim=-1)[valid].mean()) * 1e3)
    print("%-10s %d of %d problems valid; mean distance to the planted point, mm: %s" % (key, out["valid_problems"], F * K, json.dumps(out["mean_error_mm"])),
          flush=True)
    f_host = min(F, 4 if not a.quick else 1)
    t0 = time.perf_counter()
    Q.triangulate(fx["proj"], fx["targets"][:f_host], fx["weights"][:f_host], np.float64)
    wall = time.perf_counter() - t0
    out["numpy_restatement"] = dict(problems=f_host * K, wall_s=wall, ms_per_problem=1e3 * wall / (f_host * K), scaled_to_the_call_ms=1e3 * wall * F / f_host)
    print("%-10s %-24s %s" % (key, "numpy_restatement", json.dumps(out["numpy_restatement"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_triangulate.py needs a GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    for C, F in (((53, 512), (8, 512)) if not a.quick else ((8, 4),)):
        measure(C, F, 21, a, res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

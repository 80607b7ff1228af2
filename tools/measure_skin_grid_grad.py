#!/usr/bin/env python3
"""Time the bench step (300 k Gaussians, 8 views, 1920x1080, hand scene, l1+ssim) with the skin-grid gradient off and on, and
the modular call (`ops.skin_grid_grad`) alone on the bench step's active list.

    python tools/measure_skin_grid_grad.py [--out FILE.json] [--quick]

One process, HIP events around a batch of steps, every shape warmed, median of 5 samples with min and max; the two settings
alternate (off, on, off again) so that a drift of the clocks shows.  Also prints the per-kernel HIP-event times of the chain
behind mgr_skin_grid_bwd next to k_skin_bwd24 (which does the same gathers), the length of the active list, the number of
listed voxels and of (Gaussian, corner) slots, and the row Adam on that list.  Needs a GPU; there is no fallback."""
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
    assert torch.cuda.is_available(), "measure_skin_grid_grad.py needs a GPU"
    from manus_amd import _lib, ops, rasterizer
    from manus_amd.engine import HipViewCompute
    from manus_amd.optim import SkinGridAdam
    from manus_amd.synthetic import camera_table, make_scene
    dev = "cuda:0"
    N, V, W, H = (300000, 8, 1920, 1080) if not a.quick else (3000, 8, 96, 64)
    scene = make_scene(n_gaussians=N, kind="hand", seed=0, n_cameras=V, width=W, height=H, device=dev, cam_radius=1.2,
                       **({} if not a.quick else dict(grid_res=24, cam_radius=0.5, sigma_range=(2e-3, 8e-3))))
    ct = camera_table(scene["cameras"], dev)
    g = torch.Generator(device="cpu").manual_seed(123)      # targets as in bench.py: the scene perturbed by 1 %
    pert = dict(scene)
    pert["params"] = {k: (v + 0.01 * v.abs().mean() * torch.randn(v.shape, generator=g).to(dev)) for k, v in scene["params"].items()}
    ids = list(range(V))
    with torch.no_grad():
        targets = HipViewCompute(pert, torch.zeros((V, 3, H, W), device=dev), ct).forward_views_fused(ids)[0].contiguous()
    rasterizer.context(dev).clear()
    off = HipViewCompute(scene, targets, ct, loss="l1+ssim")
    on = HipViewCompute(scene, targets, ct, loss="l1+ssim", skin_grid_grad=True)
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(N=N, V=V, W=W, H=H, grid=list(scene["grid"].shape))}
    reps = 20
    for name, hc in (("off", off), ("on", on), ("off_again", off), ("on_again", on)):
        res[name] = timed(lambda: hc(ids, 1.0 / V), reps)
        print("step, skin_grid_grad %-9s %s" % (name, json.dumps(res[name])), flush=True)
    # the modular call alone on the step's active list (the list and dL/dw of the last step stay valid until the next forward)
    out = on(ids, 1.0 / V)
    lst, cnt = on.last_active
    d_w, xyz, s = on.last_skin_w_grad, on.params["_xyz"].detach(), scene
    res["modular_call"] = timed(lambda: ops._skin_grid_grad(on.n_art, xyz, on.grid, s["grid_center"], s["grid_scale"], d_w, lst, cnt, N), reps)
    print("ops._skin_grid_grad on the active list:", json.dumps(res["modular_call"]), flush=True)
    d = ops._skin_grid_grad(on.n_art, xyz, on.grid, s["grid_center"], s["grid_scale"], d_w, lst, cnt, N)
    rows = int(d.count[0])
    res["sizes"] = dict(listed_voxels=rows, voxels=int(on.grid.D * on.grid.H * on.grid.W),
                        workspace_bytes=int(_lib.lib().mgr_skin_grid_bwd_workspace_bytes(on.grid.D, on.grid.H, on.grid.W, N)))
    print("sizes:", json.dumps(res["sizes"]), flush=True)
    opt = SkinGridAdam(ops.SkinGrid(on.grid.dense(), dev), lr=1e-4)
    res["row_adam"] = timed(lambda: opt.step(d), reps)
    print("SkinGridAdam.step on that list:", json.dumps(res["row_adam"]), flush=True)
    # the kernels behind the figure
    _lib.profile_enable(True)
    for _ in range(10):
        on(ids, 1.0 / V)
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    names = ("k_skin_bwd24", "k_sg_prep24", "k_sg_scan_a", "k_sg_scan_b", "k_sg_scan_c", "k_sg_scatter", "k_sg_rank", "k_sg_reduce")
    res["kernels_ms"] = {k: rep[k][1] / rep[k][0] for k in names if k in rep}
    print("kernels (ms per launch):", json.dumps(res["kernels_ms"]), flush=True)
    # every other output does not depend on the setting
    o_off, o_on = off(ids, 1.0 / V), on(ids, 1.0 / V)
    res["leaf_grads_bit_equal"] = all(torch.equal(o_off["grads"][k], o_on["grads"][k]) for k in o_off["grads"])
    print("leaf gradients bit-equal off / on:", res["leaf_grads_bit_equal"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

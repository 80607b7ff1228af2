#!/usr/bin/env python3
"""Time the skin-grid refinement step on the bench step (300 k Gaussians, 8 views, 1920x1080, hand scene, l1+ssim):

    fused        `SkinGridRefiner.step` (mgr_skin_grid_refine: prior, row Adam, clamp, projection, value in one pass) on the
                 list of one bench step, with the prior on and with it off
    adam         `SkinGridAdam.step` alone on the same list
    composition  what the fused call replaces: a torch prior-add on the gathered rows, `SkinGridAdam.step`, a torch
                 normalise-scatter of the stepped rows, the prior's value
    trainer      `Trainer.train_step` with the refiner off (skin_grid_grad on, the gradient formed and ignored) and on

    python tools/measure_skin_refine.py [--out FILE.json] [--quick]

One process, HIP events around a batch of calls, every shape warmed, median of 5 samples with min and max; the trainer variants
alternate so that a drift of the clocks shows.  Needs a GPU; there is no fallback."""
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
    assert torch.cuda.is_available(), "measure_skin_refine.py needs a GPU"
    from manus_amd import ops, rasterizer
    from manus_amd.engine import HipViewCompute, Trainer
    from manus_amd.optim import SkinGridAdam, SkinGridRefiner
    from manus_amd.synthetic import camera_table, make_scene
    dev = "cuda:0"
    N, V, W, H = (300000, 8, 1920, 1080) if not a.quick else (3000, 8, 96, 64)

    def scene_of():
        return make_scene(n_gaussians=N, kind="hand", seed=0, n_cameras=V, width=W, height=H, device=dev, cam_radius=1.2,
                          **({} if not a.quick else dict(grid_res=24, cam_radius=0.5, sigma_range=(2e-3, 8e-3))))
    scene = scene_of()
    ct = camera_table(scene["cameras"], dev)
    g = torch.Generator(device="cpu").manual_seed(123)      # targets as in bench.py: the scene perturbed by 1 %
    pert = dict(scene)
    pert["params"] = {k: (v + 0.01 * v.abs().mean() * torch.randn(v.shape, generator=g).to(dev)) for k, v in scene["params"].items()}
    ids = list(range(V))
    with torch.no_grad():
        targets = HipViewCompute(pert, torch.zeros((V, 3, H, W), device=dev), ct).forward_views_fused(ids)[0].contiguous()
    rasterizer.context(dev).clear()
    hc = HipViewCompute(scene, targets, ct, loss="l1+ssim", skin_grid_grad=True)
    d = hc(ids, 1.0 / V)["d_skin_grid"]
    # the list of one bench step, kept: the compute object's buffers are overwritten by its next step
    d = ops.SkinGridGrad(d.voxel.clone(), d.grad.clone(), d.count.clone(), d.shape)
    n = int(d.count[0])
    sg0 = hc.grid
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(N=N, V=V, W=W, H=H, B=sg0.B, grid=(sg0.D, sg0.H, sg0.W)),
           "list": dict(rows=n, capacity=int(d.voxel.numel()))}
    print(json.dumps(res), flush=True)
    w, min_sum = 0.5, 1e-12

    def grid_copy():
        return ops.SkinGrid(sg0.dense(), dev)

    sg_f, sg_p, sg_a, sg_c = grid_copy(), grid_copy(), grid_copy(), grid_copy()
    fused = SkinGridRefiner(sg_f, lr=1e-4, prior_weight=w, project=True)
    fused_plain = SkinGridRefiner(sg_p, lr=1e-4, prior_weight=0.0, project=True)
    adam = SkinGridAdam(sg_a, lr=1e-4)
    adam_c = SkinGridAdam(sg_c, lr=1e-4)
    prior = sg_c.data.clone()
    flat, flat0 = sg_c.data.reshape(-1, sg_c.stride), prior.reshape(-1, sg_c.stride)
    w2 = float(torch.tensor(2.0 * w, dtype=torch.float32))

    def composition():
        v, rows = d.rows()                                   # (reads the count: the host-side composition has to)
        v = v.long()
        diff = flat[v] - flat0[v]
        value = w * (diff.double() ** 2).sum()
        adam_c.step(ops.SkinGridGrad(d.voxel, torch.cat([rows + w2 * diff, d.grad[rows.shape[0]:]]), d.count, d.shape))
        x = flat[v]
        S = x.sum(1, keepdim=True)
        flat[v] = torch.where(S > min_sum, x / S, x)
        return value

    for name, fn, reps in (("fused_prior_on", lambda: fused.step(d), 200), ("fused_prior_off", lambda: fused_plain.step(d), 200),
                           ("adam_alone", lambda: adam.step(d), 200), ("composition", composition, 50),
                           ("fused_prior_on_again", lambda: fused.step(d), 200)):
        res[name] = timed(fn, reps)
        print("%-26s %s" % (name, json.dumps(res[name])), flush=True)

    # Trainer.train_step, the refiner off and on (densification and pruning off: the step itself)
    opts = dict(densify_from_step=10 ** 9, densify_until_step=0, opacity_reset_interval=10 ** 9, remove_seg_end=0)
    trainers = {}
    for name in ("trainer_refiner_off", "trainer_refiner_on"):
        c = HipViewCompute(scene_of(), targets, ct, loss="l1+ssim", skin_grid_grad=True)
        r = SkinGridRefiner(c.grid, lr=1e-4, prior_weight=w, project=True) if name.endswith("on") else None
        trainers[name] = Trainer(c, V, extent=0.3, opts=opts, spatial_lr_scale=0.05, skin_grid=r)
    for name in ("trainer_refiner_off", "trainer_refiner_on", "trainer_refiner_off_again", "trainer_refiner_on_again"):
        res[name] = timed(trainers[name.replace("_again", "")].train_step, 20)
        print("%-26s %s" % (name, json.dumps(res[name])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

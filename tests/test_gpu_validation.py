"""GPU: the validation pass (csrc/eval.hip: mgr_eval_views / mgr_eval_triptych, manus_amd.validation, Trainer.validate)
against the reference's own validation_step (tests/golden/validation.npz, written by tests/golden/make_eval_golden.py),
a numpy / CPU restatement at other sizes, and the properties the kernels promise: per-view independence, bit-equal
repeats, exact zero for equal images.

Bounds: PSNR within 1e-4 dB of the reference (torch's fp32 mean and the kernel's fp32 partial sums each carry a few 1e-6
relative; 10 / ln 10 * 2e-5 = 8.7e-5 dB); sq_sum within 1e-5 relative of the same fp32 element operations summed in
float64; SSIM within 5e-6 absolute (the bar of test_gpu_image_loss.py for this statistic); triptychs byte for byte."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "validation.npz"))
    return d, [str(n) for n in d["names"]]


def _chw(hwc):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(hwc, (2, 0, 1))))


def _sq_oracle(pred, tgt, mask):
    """(V,) float64: the element operations in fp32 (two products, a difference, a square), the sum in float64."""
    p, t = pred.numpy(), tgt.numpy()
    m = np.ones((p.shape[0], 1) + p.shape[2:], np.float32) if mask is None else mask.numpy()[:, None]
    d = (p * m).astype(np.float32) - (t * m).astype(np.float32)
    return (d * d).astype(np.float32).astype(np.float64).sum(axis=(1, 2, 3))


def _triptych_numpy(pred_hwc, gt_hwc):
    """base.py:116-127 + extra.py:110-115,153-160 on numpy arrays."""
    img = (np.clip(pred_hwc, 0, 1) * 255).astype(np.uint8)
    gt_img = gt_hwc
    if gt_img.max() <= 1.0:
        gt_img = gt_img * 255
    gt_img = gt_img.astype(np.uint8)
    diff = gt_img / 255.0 - img / 255.0
    diff = diff * 255.0
    final = np.concatenate((img, gt_img), axis=0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        return np.concatenate((final, diff), axis=0).astype(np.uint8)


def _smooth(V, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    f = torch.rand((V, 3, 3), generator=g) * 6
    gt = 0.5 + 0.45 * torch.sin(f[:, :, 0, None, None] * xx + f[:, :, 1, None, None] * yy + f[:, :, 2, None, None])
    pred = (gt + 0.05 * torch.randn((V, 3, H, W), generator=g)).clamp(-0.1, 1.1)
    mask = (0.5 + 0.7 * torch.sin(3 * xx + 2 * yy + torch.arange(V)[:, None, None].float())).clamp(0, 1)
    return pred.contiguous(), gt.contiguous(), mask.contiguous()


def _eval(pred, tgt, mask=None, **kw):
    from manus_amd import ops
    return ops.eval_views(pred.to(DEV), tgt.to(DEV), None if mask is None else mask.to(DEV), **kw)


def test_validation_step_matches_the_reference(golden_dir):
    """validation.validation_step on the reference-shaped inputs of every fixture case: PSNR, SSIM, triptych."""
    from manus_amd.validation import validation_step
    d, names = _golden(golden_dir)
    assert {"fractional_mask", "binary_mask", "no_mask", "render_out_of_range", "gt_0_255", "equal"} <= set(names)
    for k, name in enumerate(names):
        batch = {"rgb": torch.tensor(d["gt%d" % k], device=DEV)}
        if int(d["has_mask%d" % k]):
            batch["mask"] = torch.tensor(d["mask%d" % k], device=DEV)
        out = validation_step(torch.tensor(d["pred%d" % k], device=DEV), batch)
        psnr, ssim, ref_psnr, ref_ssim = float(out["psnr"]), float(out["ssim"]), float(d["psnr%d" % k]), float(d["ssim%d" % k])
        print(name, "psnr", psnr, "ref", ref_psnr, "diff", psnr - ref_psnr, "ssim", ssim, "ref", ref_ssim, "diff", ssim - ref_ssim)
        if np.isinf(ref_psnr):
            assert psnr == ref_psnr, name
        else:
            assert abs(psnr - ref_psnr) < 1e-4, (name, psnr, ref_psnr)
        assert abs(ssim - ref_ssim) < 5e-6, (name, ssim, ref_ssim)
        img = out["image"].cpu().numpy()
        assert img.dtype == np.uint8 and img.shape == d["image%d" % k].shape
        assert np.array_equal(img, d["image%d" % k]), (name, int((img != d["image%d" % k]).sum()))
        assert np.array_equal(img, _triptych_numpy(d["pred%d" % k], d["gt%d" % k][0])), name


def test_batched_ops_match_the_reference_and_the_fp64_sum(golden_dir):
    """All fixture cases as ONE batch of views through ops.eval_views / ops.eval_triptych."""
    from manus_amd import ops
    d, names = _golden(golden_dir)
    K = len(names)
    pred = torch.stack([_chw(d["pred%d" % k]) for k in range(K)])
    tgt = torch.stack([_chw(d["gt%d" % k][0]) for k in range(K)])
    mask = torch.stack([torch.from_numpy(d["mask%d" % k][0, :, :, 0].copy()) for k in range(K)])
    sq, ss, gmax = _eval(pred, tgt, mask)
    n = float(pred[0].numel())
    want_sq = _sq_oracle(pred, tgt, mask)
    for k, name in enumerate(names):
        s = float(sq[k])
        print(name, "sq_sum", s, "fp64", want_sq[k], "rel", abs(s - want_sq[k]) / max(want_sq[k], 1e-300))
        assert abs(s - want_sq[k]) <= 1e-5 * want_sq[k], name
        ref_psnr = float(d["psnr%d" % k])
        psnr = float(-10 * torch.log10(sq[k] / n))
        assert psnr == ref_psnr if np.isinf(ref_psnr) else abs(psnr - ref_psnr) < 1e-4, (name, psnr, ref_psnr)
        assert abs(float(ss[k]) / n - float(d["ssim%d" % k])) < 5e-6, name
        assert float(gmax[k]) == float(d["gt%d" % k].max()), name
    trip = ops.eval_triptych(pred.to(DEV), tgt.to(DEV), gmax).cpu().numpy()
    for k, name in enumerate(names):
        assert np.array_equal(trip[k], d["image%d" % k]), name


def test_reference_shaped_psnr(golden_dir):
    """losses.psnr with the reference's signature: no mask, a boolean selection, reduction='none'."""
    from manus_amd import losses
    d, names = _golden(golden_dir)
    k = names.index("binary_mask")
    pred, gt, mask = torch.tensor(d["pred%d" % k]), torch.tensor(d["gt%d" % k]), torch.tensor(d["mask%d" % k])
    sel = mask[0] > 0.5                                         # (H,W,1) bool
    value = (pred - gt[0]) ** 2
    got = float(losses.psnr(pred.to(DEV), gt[0].to(DEV)))
    assert abs(got - float(-10 * torch.log10(value.mean()))) < 1e-4
    got = float(losses.psnr(pred.to(DEV), gt[0].to(DEV), valid_mask=sel.to(DEV)))
    want = float(-10 * torch.log10(value[sel[..., 0]].double().mean()))      # the reference's value[valid_mask] then mean
    assert abs(got - want) < 1e-4, (got, want)
    two_p, two_g = torch.stack([pred, torch.tensor(d["pred0"])]), torch.stack([gt[0], torch.tensor(d["gt0"][0])])
    got = losses.psnr(two_p.to(DEV), two_g.to(DEV), reduction="none").cpu()
    want = -10 * torch.log10(((two_p - two_g) ** 2).mean(dim=(1, 2, 3)))
    assert got.shape == (2,) and float((got - want).abs().max()) < 1e-4


def test_views_are_independent_and_repeatable():
    V, H, W = 5, 37, 300
    pred, tgt, mask = _smooth(V, H, W, 3)
    pred[2, 1, 20, 150] = float("nan")                          # one bad pixel in view 2
    tgt[4, 0, 5, 7] = float("inf")                              # and an Inf in the target of view 4
    a = [t.cpu() for t in _eval(pred, tgt, mask, flags=True)]
    b = [t.cpu() for t in _eval(pred, tgt, mask, flags=True)]
    for x, y in zip(a, b):                                      # two calls: the same bits
        assert np.array_equal(x.numpy().view(np.int32), y.numpy().view(np.int32))
    sq, ss, gmax, fl = a
    assert fl.tolist() == [0, 0, 1, 0, 1]
    for v in range(V):
        one = [t.cpu() for t in _eval(pred[v:v + 1], tgt[v:v + 1], mask[v:v + 1])]
        for x, y in zip((sq, ss, gmax), one):                   # a view alone: the same bits as in the batch
            assert x[v:v + 1].numpy().view(np.int32).tolist() == y.numpy().view(np.int32).tolist(), v
        if v in (2, 4):
            assert torch.isnan(sq[v]) and torch.isnan(ss[v])
        else:
            assert torch.isfinite(sq[v]) and torch.isfinite(ss[v]) and float(sq[v]) > 0
    assert float(gmax[4]) == float("inf") and float(gmax[0]) == float(tgt[0].max())
    # the NaN pixel is written as byte 0 (this package's definition), every other render byte follows the expression
    from manus_amd import ops
    trip = ops.eval_triptych(pred.to(DEV), tgt.to(DEV), gmax.to(DEV)).cpu().numpy()
    assert trip[2, 20, 150, 1] == 0
    want = (np.clip(np.nan_to_num(pred[2].numpy(), nan=0.0), 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(trip[2, :H], want)


def test_equal_images_give_exact_zero_and_infinite_psnr():
    from manus_amd import losses
    pred, tgt, mask = _smooth(2, 21, 130, 9)
    tgt[0] = pred[0]
    sq, ss, _ = _eval(pred, tgt, mask)
    assert float(sq[0]) == 0.0 and float(sq[1]) > 0.0
    assert float(-10 * torch.log10(sq[0] / pred[0].numel())) == float("inf")
    assert abs(float(ss[0]) / pred[0].numel() - 1.0) < 5e-6
    hwc = pred[0].permute(1, 2, 0).contiguous().to(DEV)
    assert float(losses.psnr(hwc, hwc.clone())) == float("inf")


@pytest.mark.parametrize("V,H,W,masked", [(2, 1080, 1920, True), (2, 33, 258, True), (1, 7, 1, False), (3, 5, 513, False)])
def test_sizes_against_the_cpu_restatement(V, H, W, masked):
    """The bench resolution, a width that is not a multiple of 4, odd heights, workgroup seams at 256."""
    from manus_amd import ops
    pred, tgt, mask = _smooth(V, H, W, 100 + W)
    if not masked:
        mask = None
    if V == 3:
        tgt[1] = tgt[1] * 200.0                                  # one view whose ground truth is already 0..255
    sq, ss, gmax = _eval(pred, tgt, mask)
    want_sq = _sq_oracle(pred, tgt, mask)
    n = float(3 * H * W)
    for v in range(V):
        m = 1.0 if mask is None else mask[v][..., None]
        p_hwc, t_hwc = pred[v].permute(1, 2, 0) * m, tgt[v].permute(1, 2, 0) * m
        want_ss = float(tr.ssim_hwc(p_hwc, t_hwc))
        print((V, H, W), v, "sq rel", abs(float(sq[v]) - want_sq[v]) / want_sq[v], "ssim", float(ss[v]) / n, "cpu", want_ss)
        assert abs(float(sq[v]) - want_sq[v]) <= 1e-5 * want_sq[v]
        assert abs(float(ss[v]) / n - want_ss) < 5e-6
        assert float(gmax[v]) == float(tgt[v].max())
    trip = ops.eval_triptych(pred.to(DEV), tgt.to(DEV), gmax).cpu().numpy()
    assert trip.shape == (V, 3 * H, W, 3)
    for v in range(V):
        want = _triptych_numpy(pred[v].permute(1, 2, 0).numpy(), tgt[v].permute(1, 2, 0).numpy())
        assert np.array_equal(trip[v], want), (v, int((trip[v] != want).sum()))


def _trainer(V, W, H):
    from manus_amd.engine import HipViewCompute, Trainer
    from manus_amd.synthetic import camera_table, make_scene
    torch.manual_seed(0)
    sc = make_scene(n_gaussians=4000, kind="hand", seed=4, grid_res=32, n_cameras=V, width=W, height=H, cam_radius=0.5,
                    sigma_range=(2e-3, 6e-3), device=DEV)
    ct = camera_table(sc["cameras"], DEV)
    g = torch.Generator(device="cpu").manual_seed(5)
    tgt_scene = dict(sc)
    tgt_scene["params"] = {k: (v + (1.5 * torch.randn(v.shape, generator=g).to(DEV) if k == "_features_dc" else 0))
                           for k, v in sc["params"].items()}
    with torch.no_grad():
        hp = HipViewCompute(tgt_scene, torch.zeros((V, 3, H, W), device=DEV), ct)
        targets = torch.cat([hp.forward_views([v])[0] for v in range(V)]).contiguous()
    compute = HipViewCompute(sc, targets, ct, loss="l1+ssim")
    opts = dict(densify_from_step=1000, densification_interval=1000, densify_until_step=2000, opacity_reset_interval=100000)
    return Trainer(compute, V, extent=0.3, opts=opts, spatial_lr_scale=0.05, bg_white=False)


def test_trainer_validate_leaves_training_untouched(tmp_path):
    from manus_amd import ops, rasterizer
    from manus_amd.validation import Validator
    V, W, H = 3, 128, 96
    grads = {}
    for validated in (False, True):
        rasterizer.context(DEV).clear()
        t = _trainer(V, W, H)
        t.train_step()
        t.train_step()
        if validated:
            masks = _smooth(V, H, W, 1)[2].to(DEV)
            val = Validator(str(tmp_path), "exp")
            policy, step = rasterizer.context(DEV).sync_every_forward, t.global_step
            res = t.validate([2, 0, 1], masks=masks, validator=val, group=2)       # two groups, another view order
            val.end(t.global_step)
            assert rasterizer.context(DEV).sync_every_forward == policy and t.global_step == step
            # the metrics are eval_views on forward_views' images (rendered here in validate's groups; the compute object's
            # cache of per-view constants is put back, as validate itself does)
            saved = t.compute._cache, t.compute._const_stamp
            with torch.no_grad():
                img = torch.cat([t.compute.forward_views([2, 0])[0], t.compute.forward_views([1])[0]])
            t.compute._cache, t.compute._const_stamp = saved
            sq, ss, gmax = ops.eval_views(img, t.compute.targets[[2, 0, 1]].contiguous(), masks)
            n = float(img[0].numel())
            assert res["psnr"] == (-10 * torch.log10(sq / n)).cpu().tolist()
            assert res["ssim"] == (ss / n).cpu().tolist()
            assert res["psnr_mean"] == float(np.mean(res["psnr"])) and res["render_time"] > 0
            assert torch.equal(res["images"], ops.eval_triptych(img, t.compute.targets[[2, 0, 1]].contiguous(), gmax))
            assert sorted(os.listdir(os.path.join(str(tmp_path), "val_results", "images"))) == ["2_0.png", "2_1.png", "2_2.png"]
            assert all(np.isfinite(res["psnr"])) and all(0 < s <= 1 for s in res["ssim"])
        out = t.train_step()
        grads[validated] = {k: v.detach().cpu().clone() for k, v in out["grads"].items()}
        grads[validated]["loss"] = out["loss"].detach().cpu().clone()
    for k in grads[False]:
        assert torch.equal(grads[False][k], grads[True][k]), k

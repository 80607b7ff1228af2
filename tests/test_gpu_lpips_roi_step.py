"""GPU: the windowed LPIPS term on the training step (HipViewCompute(lpips_rects=, lpips_norm=, lpips_cache_targets=), both
routes) and `FrameStore.load_step(lpips_rects=True)`.  The set-up of test_gpu_lpips_step.py: 64x48, 2000 Gaussians, 3 views,
stand-in weights.
"""
import functools

import numpy as np
import pytest
import torch

import lpips_ref as R
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, W, H, N = 3, 64, 48, 2000
BAR = 1e-4          # the repository's fused-against-modular bar on leaf gradients (max-rel-err)
IDS = list(range(V))
FULL = [(0, 0, W, H)] * V
RECTS = [(8, 6, 40, 30), (0, 0, 32, 24), (20, 16, 44, 32)]
KW = dict(loss="l1+ssim", persistent_grads=False)


@functools.lru_cache(maxsize=None)
def net():
    from manus_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(*R.state_dicts("vgg", R.make_weights("vgg", 0)), net="vgg")


@functools.lru_cache(maxsize=None)
def scene():
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=N, kind="hand", seed=6, grid_res=24, n_cameras=V, width=W, height=H, cam_radius=0.5,
                    sigma_range=(2e-3, 8e-3), device=DEV)
    g = torch.Generator().manual_seed(11)
    return sc, camera_table(sc["cameras"], DEV), torch.rand((V, 3, H, W), generator=g).to(DEV), torch.rand((V, 3, H, W), generator=g).to(DEV)


def clone_out(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def compute(fused, targets=None, **kw):
    from manus_amd.engine import HipViewCompute
    sc, ct, tg, _ = scene()
    return HipViewCompute(sc, tg if targets is None else targets, ct, fused=fused, lpips=net(), w_lpips=0.1, **KW, **kw)


def step(hc):
    return clone_out(hc(IDS, 1.0 / V))


def same(a, b, what):
    for k in ("loss", "loss_lpips", "grad2d", "vis", "radii"):
        assert torch.equal(a[k], b[k]), (what, k)
    for k, g in b["grads"].items():
        assert torch.equal(a["grads"][k], g), (what, k)


@functools.lru_cache(maxsize=None)
def plain(fused):
    return step(compute(fused))


@pytest.mark.parametrize("fused", [True, False])
def test_no_rects_and_full_frame_rects_are_the_plain_step(fused):
    same(step(compute(fused, lpips_rects=None)), plain(fused), "lpips_rects=None")
    same(step(compute(fused, lpips_rects=FULL, lpips_norm="window")), plain(fused), "full-frame rects, window norm")
    # (w h) / (W H) = 1 exactly: the frame norm is the same step here
    same(step(compute(fused, lpips_rects=FULL, lpips_norm="frame")), plain(fused), "full-frame rects, frame norm")
    with pytest.raises(ValueError, match="lpips_norm"):
        compute(fused, lpips_norm="area")
    hc = compute(fused, lpips_rects=FULL[:2])
    with pytest.raises(ValueError, match="lpips_rects"):
        hc(IDS, 1.0 / V)


@pytest.mark.parametrize("norm", ["frame", "window"])
def test_real_rects_fused_against_modular(norm):
    from manus_amd.engine import HipViewCompute
    sc, ct, tg, _ = scene()
    outs = {fused: step(compute(fused, lpips_rects=RECTS, lpips_norm=norm)) for fused in (True, False)}
    of, om = outs[True], outs[False]
    # the term's value: scale * sum_v factor_v d_v of the direct windowed call on the step's image
    hc = HipViewCompute(sc, tg, ct, fused=True, **KW)
    hc(IDS, 1.0 / V)
    d = net().values_grad(hc.last_image, tg, need_grad=False, rects=RECTS)[0].double().cpu()
    fac = torch.tensor([r[2] * r[3] / float(W * H) if norm == "frame" else 1.0 for r in RECTS], dtype=torch.float64)
    direct = float((d * fac).sum()) / V
    assert direct > 0 and abs(float(of["loss_lpips"]) - direct) <= 1e-6 * direct
    assert float(of["loss_lpips"]) != float(plain(True)["loss_lpips"])
    off = {fused: clone_out(HipViewCompute(sc, tg, ct, fused=fused, **KW)(IDS, 1.0 / V)) for fused in (True, False)}
    for fused in (True, False):
        o = outs[fused]
        assert abs(float(o["loss"]) - (float(off[fused]["loss"]) + 0.1 * float(o["loss_lpips"]))) <= 1e-6 * abs(float(o["loss"]))
    assert abs(float(of["loss"]) - float(om["loss"])) <= BAR * abs(float(om["loss"]))
    worst = 0.0
    for k, g in om["grads"].items():
        e = max_rel_err(of["grads"][k].cpu().numpy(), g.cpu().numpy())
        share = max_rel_err(g.cpu().numpy(), off[False]["grads"][k].cpu().numpy())
        print("%-16s fused against modular %.3g; the term changes it by %.3g of its maximum" % (k, e, share))
        assert share > 0, k          # the term reaches the leaf
        worst = max(worst, e)
    e2d = max_rel_err(of["grad2d"].cpu().numpy(), om["grad2d"].cpu().numpy())
    print("grad2d fused against modular %.3g" % e2d)
    assert worst < BAR, worst
    assert e2d < BAR, e2d
    assert torch.equal(of["vis"], om["vis"])
    for fused in (True, False):
        assert not torch.equal(outs[fused]["grad2d"], off[fused]["grad2d"])


@pytest.mark.parametrize("fused", [True, False])
def test_cached_targets(fused):
    sc, ct, tg, other = scene()
    rects = [RECTS[0], (0, 0, 0, 0), RECTS[2]]          # (one view's term is off)
    ref = compute(fused, lpips_rects=rects)
    r1 = step(ref)
    hc = compute(fused, targets=tg.clone(), lpips_rects=rects, lpips_cache_targets=True)
    same(step(hc), r1, "first step")
    taps = hc._cache[tuple(IDS)]["lpips"]["taps"]
    assert taps is not None and taps.bufs[1] is None and taps.nbytes > 0
    same(step(hc), step(ref), "second step")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is taps          # (kept, not rebuilt)
    # new targets through torch (the version counter moves): no stale taps
    hc.targets.copy_(other)
    fresh = step(compute(fused, targets=other, lpips_rects=rects))
    assert float(fresh["loss_lpips"]) != float(r1["loss_lpips"])
    same(step(hc), fresh, "after targets.copy_")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is not taps
    # a raw write that torch does not see, then view_constants_changed()
    _raw_copy(hc.targets, tg)
    hc.view_constants_changed()
    same(step(hc), r1, "after a raw write and view_constants_changed()")
    # new rects rebuild the cache, replaced or written in place
    taps = hc._cache[tuple(IDS)]["lpips"]["taps"]
    hc.lpips_rects = RECTS
    same(step(hc), step(compute(fused, lpips_rects=RECTS)), "new rects")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is not taps and hc._cache[tuple(IDS)]["lpips"]["taps"].bufs[1] is not None
    table = np.asarray(RECTS, np.int32)
    hc.lpips_rects = table
    step(hc)
    table[0] = (4, 2, 50, 40)
    same(step(hc), step(compute(fused, lpips_rects=[(4, 2, 50, 40)] + RECTS[1:])), "rects written in place")
    # switching the cache off again gives the same step
    hc.lpips_cache_targets = False
    same(step(hc), step(compute(fused, lpips_rects=[(4, 2, 50, 40)] + RECTS[1:])), "cache off")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is None


def _raw_copy(dst, src):
    """dst <- src without moving dst's version counter (what a kernel given the raw pointer does)."""
    v = dst._version
    dst.data.copy_(src)
    torch.cuda.synchronize()
    assert dst._version == v


def test_load_step_writes_the_rects(tmp_path_factory):
    from test_gpu_frames import CASES, Capture
    from manus_amd import dataset as D
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table
    cap = Capture(str(tmp_path_factory.mktemp("roi")), *CASES["64x48k1"])
    ds, st = cap.ds, cap.store
    scene_, targets = D.hand_scene_from_batch(ds.view_batch([9, 10, 11]), ds[0]["bones_rest"], 2000, grid_res=24, seed=1, device=DEV)
    hc = HipViewCompute(scene_, targets, camera_table(scene_["cameras"], DEV), fused=True, lpips=net(), w_lpips=0.1, **KW)
    assert hc.lpips_rects is None
    st.load_step(hc, [0, 1, 2])
    assert hc.lpips_rects is None                       # (not asked: nothing written)
    items = [0, 1]                                      # a large box on the left, a small box on the right
    st.load_step(hc, items, slots=[2, 0], lpips_rects=True)
    want = st.lpips_rects(items)
    table = np.asarray(hc.lpips_rects)
    assert table.shape == (3, 4) and (table[[2, 0]] == want).all() and tuple(table[1]) == (0, 0, 64, 48)
    assert tuple(want[1]) != (0, 0, 64, 48) and want[1][2] >= 16 and want[1][3] >= 16
    out = step_of(hc)
    direct = net().values_grad(hc.last_image, hc.targets, need_grad=False, rects=table)[0].double().cpu()
    fac = torch.tensor([float(r[2] * r[3]) / (64 * 48) for r in table.tolist()], dtype=torch.float64)
    want_l = float((direct * fac).sum()) / 3
    assert want_l > 0 and abs(float(out["loss_lpips"]) - want_l) <= 1e-6 * want_l
    # a second load into an existing table keeps the other rows
    st.load_step(hc, [4, 3], slots=[1, 2], lpips_rects=True)         # an empty bbox, a one-pixel bbox
    t2 = np.asarray(hc.lpips_rects)
    assert (t2[[1, 2]] == st.lpips_rects([4, 3])).all() and (t2[0] == table[0]).all()
    assert tuple(t2[1]) == (0, 0, 0, 0) and t2[2][2] >= 16 and t2[2][3] >= 16
    assert float(step_of(hc)["loss_lpips"]) > 0


def step_of(hc):
    return clone_out(hc([0, 1, 2], 1.0 / 3))

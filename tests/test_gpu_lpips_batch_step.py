"""GPU: the batched windowed LPIPS term on the training step (HipViewCompute(lpips_batch=), both routes) and
`FrameStore.load_step(lpips_rects=True)` with the store's `lpips_fit`.  The batched call is the sequential one bit for bit, so
every check is `torch.equal` against lpips_batch = 0.  The set-up of test_gpu_lpips_roi_step.py: 64x48, 2000 Gaussians, 3
views, stand-in weights; two views share a window size and one differs.
"""
import functools

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, W, H, N = 3, 64, 48, 2000
IDS = list(range(V))
RECTS = [(8, 6, 40, 30), (0, 0, 32, 24), (23, 17, 40, 30)]
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
def sequential(fused):
    return step(compute(fused, lpips_rects=RECTS))


@pytest.mark.parametrize("fused", [True, False])
def test_batched_step_is_the_sequential_step(fused):
    ref = sequential(fused)
    assert float(ref["loss_lpips"]) > 0
    hc = compute(fused, lpips_rects=RECTS, lpips_batch=8)
    assert hc.lpips_batch == 8
    same(step(hc), ref, "lpips_batch=8")
    # a plain attribute: switched per step
    hc.lpips_batch = 2
    same(step(hc), ref, "lpips_batch=2")
    # 0 is the step built without the argument
    assert compute(fused, lpips_rects=RECTS).lpips_batch == 0
    same(step(compute(fused, lpips_rects=RECTS, lpips_batch=0)), ref, "lpips_batch=0")


@pytest.mark.parametrize("fused", [True, False])
def test_batched_step_with_cached_targets(fused):
    sc, ct, tg, other = scene()
    ref = sequential(fused)
    hc = compute(fused, targets=tg.clone(), lpips_rects=RECTS, lpips_cache_targets=True, lpips_batch=8)
    same(step(hc), ref, "first step")
    taps = hc._cache[tuple(IDS)]["lpips"]["taps"]
    assert taps is not None and taps.nbytes > 0
    same(step(hc), ref, "second step")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is taps          # (kept, not rebuilt)
    # the batch is no part of the key: the taps are the same bits
    hc.lpips_batch = 0
    same(step(hc), ref, "batch switched off on kept taps")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is taps
    hc.lpips_batch = 8
    # new targets: a raw write that torch does not see, then view_constants_changed()
    v = hc.targets._version
    hc.targets.data.copy_(other)
    torch.cuda.synchronize()
    assert hc.targets._version == v
    hc.view_constants_changed()
    fresh = step(compute(fused, targets=other, lpips_rects=RECTS))
    assert float(fresh["loss_lpips"]) != float(ref["loss_lpips"])
    same(step(hc), fresh, "after targets.copy_ and view_constants_changed()")
    assert hc._cache[tuple(IDS)]["lpips"]["taps"] is not taps


def test_load_step_with_the_store_s_fit(tmp_path_factory):
    from test_gpu_frames import CASES, Capture
    from manus_amd import dataset as D
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table
    cap = Capture(str(tmp_path_factory.mktemp("batch")), *CASES["64x48k1"])
    ds, st = cap.ds, cap.store
    scene_, targets = D.hand_scene_from_batch(ds.view_batch([9, 10, 11]), ds[0]["bones_rest"], 2000, grid_res=24, seed=1, device=DEV)
    hc = HipViewCompute(scene_, targets, camera_table(scene_["cameras"], DEV), fused=True, lpips=net(), w_lpips=0.1, **KW)
    items = [0, 1, 3]          # a large box on the left, a small box on the right, a one-pixel bbox
    # the default is today's rows
    st.load_step(hc, items, lpips_rects=True)
    assert (np.asarray(hc.lpips_rects) == st.lpips_rects(items)).all()
    st.lpips_fit = dict(margin=4, quantum=16, common=True)
    st.load_step(hc, items, lpips_rects=True)
    table = np.asarray(hc.lpips_rects)
    want = st.lpips_rects(items, margin=4, quantum=16, common=True)
    assert (table == want).all()
    assert len({(int(r[2]), int(r[3])) for r in table}) == 1 and table[0][2] % 16 == 0 and (table[0][3] % 16 == 0 or table[0][3] == 48)
    assert not (want == st.lpips_rects(items)).all()
    ref = clone_out(hc([0, 1, 2], 1.0 / 3))
    assert float(ref["loss_lpips"]) > 0
    hc.lpips_batch = 8
    same(clone_out(hc([0, 1, 2], 1.0 / 3)), ref, "lpips_batch=8 on the store's rects")

"""No GPU: the fp64 restatement of the map loss against central differences, the ABI of the new entries (header, binding,
built library), and the refusals of HipViewCompute that need no device."""
import ctypes
import os
import re

import pytest
import torch

from map_loss_ref import map_loss_grads_fp32, map_loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mgr_map_loss_workspace_bytes", "mgr_map_loss", "mgr_views_maps_backward_workspace_bytes", "mgr_views_maps_backward")


def _maps(seed=0, V=2, H=5, W=7):
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand((V, H, W), generator=g, dtype=torch.float64)
    mask = (torch.rand((V, H, W), generator=g, dtype=torch.float64) * 3 - 1).clamp(0, 1)     # zeros, ones and fractions
    depth = torch.rand((V, H, W), generator=g, dtype=torch.float64) * 2
    dtgt = torch.rand((V, H, W), generator=g, dtype=torch.float64) * 2
    return alpha, mask, depth, dtgt


def test_restatement_against_central_differences():
    alpha, mask, depth, dtgt = _maps()
    # away from the kinks: no difference within the step of the kink
    h = 1e-6
    alpha = torch.where((alpha - mask).abs() < 1e-3, alpha + 0.01, alpha)
    depth = torch.where((depth - dtgt).abs() < 1e-3, depth + 0.01, depth)
    w_mask, w_depth, k = 0.7, 0.3, 1.9
    ref = map_loss_ref(alpha, mask, depth, dtgt, w_mask, w_depth, k)
    total = lambda a, d: float(map_loss_ref(a, mask, d, dtgt, w_mask, w_depth)["total"]) * k
    for name, x, g in (("alpha", alpha, ref["g_alpha"]), ("depth", depth, ref["g_depth"])):
        for idx in [(0, 0, 0), (1, 4, 6), (0, 2, 3), (1, 1, 5)]:
            p, m = x.clone(), x.clone()
            p[idx] += h
            m[idx] -= h
            fd = (total(p, depth) - total(m, depth)) / (2 * h) if name == "alpha" else (total(alpha, p) - total(alpha, m)) / (2 * h)
            assert abs(fd - float(g[idx])) <= 1e-8 + 1e-6 * abs(float(g[idx])), (name, idx, fd, float(g[idx]))
    # the weighted sum and the terms
    n = alpha.numel()
    assert abs(float(ref["L_mask"]) - float((alpha - mask).abs().sum()) / n) < 1e-15
    assert abs(float(ref["total"]) - (w_mask * float(ref["L_mask"]) + w_depth * float(ref["L_depth"]))) < 1e-15


def test_gradient_is_exactly_zero_at_the_kinks():
    alpha, mask, depth, dtgt = _maps(1)
    ref = map_loss_ref(mask.clone(), mask, dtgt.clone(), dtgt, 1.0, 1.0, 3.0)
    assert float(ref["L_mask"]) == 0.0 and float(ref["L_depth"]) == 0.0
    assert bool((ref["g_alpha"] == 0).all()) and bool((ref["g_depth"] == 0).all())
    g_a, g_d = map_loss_grads_fp32(mask.float(), mask.float(), dtgt.float(), dtgt.float(), 1.0, 1.0, 3.0)
    assert bool((g_a == 0).all()) and bool((g_d == 0).all())
    # without the depth term: no depth gradient, the depth weight does not count
    ref = map_loss_ref(alpha, mask, None, None, 0.5, 9.0)
    assert ref["g_depth"] is None and abs(float(ref["total"]) - 0.5 * float(ref["L_mask"])) < 1e-15


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib
    header = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        n_decl = _declared_args(header, name)
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_decl, (name, len(args), n_decl)
        assert res is (ctypes.c_size_t if name.endswith("_workspace_bytes") else ctypes.c_int), name
        assert hasattr(so, name), "%s is not exported by the built library" % name
    assert _declared_args(header, "mgr_views_maps_backward") == 30 and _declared_args(header, "mgr_map_loss") == 16
    from manus_amd import build
    assert "map_loss.hip" in build.SOURCES


def _cpu_object_scene():
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=50, kind="object", seed=1, grid_res=8, n_cameras=2, width=24, height=16, device="cpu")
    return sc, camera_table(sc["cameras"], "cpu")


def test_refusals_that_need_no_device():
    from manus_amd.engine import HipViewCompute
    sc, ct = _cpu_object_scene()
    tg = torch.zeros((2, 3, 16, 24))
    good = torch.zeros((2, 16, 24))
    hc = HipViewCompute(sc, tg, ct, mask_targets=good, w_mask=1.0, depth_targets=good, w_depth=0.5)
    assert hc._map_terms() == (True, True)
    assert HipViewCompute(sc, tg, ct, mask_targets=good)._map_terms() == (False, False)        # weights zero: off
    assert HipViewCompute(sc, tg, ct, w_mask=1.0)._map_terms() == (False, False)               # no targets: off
    assert HipViewCompute(sc, tg, ct, mask_targets=good, depth_targets=good, w_depth=1.0)._map_terms() == (False, True)
    for bad in (torch.zeros((2, 24, 16)), torch.zeros((3, 16, 24)), torch.zeros((2, 1, 16, 24)), torch.zeros((2, 16, 24), dtype=torch.int32),
                torch.zeros((2, 16, 24), device="meta")):
        with pytest.raises(ValueError):
            HipViewCompute(sc, tg, ct, mask_targets=bad, w_mask=1.0)
        with pytest.raises(ValueError):
            HipViewCompute(sc, tg, ct, mask_targets=good, w_mask=1.0, depth_targets=bad, w_depth=1.0)
        with pytest.raises(ValueError):
            hc.mask_targets = bad
    with pytest.raises(ValueError, match="depth_cut"):
        HipViewCompute(sc, tg, ct, mask_targets=good, w_mask=1.0, depth_cut=True)
    # a term switched on after construction is refused by the step's own check
    cut = HipViewCompute(sc, tg, ct, mask_targets=good, depth_cut=True)
    if cut.depth_cut:       # (MANUS_DEPTH_CUT=0 in the environment forces the cut off)
        cut.w_mask = 1.0
        with pytest.raises(ValueError, match="depth_cut"):
            cut._map_terms()
    # pose_grad / skin_grid_grad need articulated Gaussians, which need a device: the same check, asked directly
    for name in ("pose_grad", "skin_grid_grad"):
        setattr(hc, name, True)
        with pytest.raises(ValueError, match=name):
            hc._map_terms()
        setattr(hc, name, False)
    assert hc._map_terms() == (True, True)

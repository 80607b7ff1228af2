"""CPU: the feature render's backward, as far as it can be checked without a device -- the ABI declares the new symbols, the
operator refuses CPU tensors, and the REFERENCE CONSTRUCTION of tests/test_gpu_feature_grad.py (alpha and expected depth as the
oracle run with colours (z, 1, 0) on a zero background, plus dL/dz times the z row of the view matrix on the means) is itself
checked against central differences of the fp64 oracle."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import RasterOracle

from util import cam_args, make_camera, max_rel_err, random_gaussians

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mgr_raster_blend_features_backward": 30, "mgr_raster_feat_backward_workspace_bytes": 6}


def test_header_and_binding_declare_the_new_symbols():
    from manus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    for name, arity in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, "include/manus_hip.h does not declare " + name
        assert len(m.group(1).split(",")) == arity, (name, m.group(1))
        assert name in _lib.SIGNATURES, "python binding missing for " + name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    assert _lib.SIGNATURES["mgr_raster_feat_backward_workspace_bytes"][0] is _lib.c_sz
    assert re.search(r"#define\s+MGR_VERSION\s+100\b", text)


def test_rasterize_views_features_refuses_cpu_tensors_and_bad_requests():
    from manus_amd._lib import ManusHipError
    from manus_amd.rasterizer import rasterize_views_features
    n = 4
    z = lambda *s: torch.zeros(s)
    args = (z(1, 40), z(n, 3), z(1, n, 3), z(n, 3), z(n), z(n, 6), z(3), 16, 16)
    with pytest.raises(ManusHipError):
        rasterize_views_features(*args, alpha=True)
    with pytest.raises(ManusHipError):
        rasterize_views_features(*args, features=z(n, 2), depth=True)
    with pytest.raises(ManusHipError):          # nothing asked for
        rasterize_views_features(*args)
    with pytest.raises(ManusHipError):          # 33 channels
        rasterize_views_features(*args, features=z(n, 33))


# ---------------------------------------------------------------------------------------------------------------------
# the reference construction against central differences (fp64)
# ---------------------------------------------------------------------------------------------------------------------
W = H = 32
N = 40
SEED = 1
STEP = 1e-6


def _scene():
    cam = make_camera(W, H)
    m, c, _, op = random_gaussians(N, seed=SEED, spread=0.15, sigma=(0.02, 0.05), opacity=(0.1, 0.6))
    return cam, m.astype(np.float64), c.astype(np.float64), op.astype(np.float64)


def _maps(cam, m, c, op):
    """(oracle of the (z, 1, 0) run, depth map, alpha map = 1 - final_T) in fp64."""
    a = cam_args(cam)
    args = (a["W"], a["H"], a["tanfovx"], a["tanfovy"], a["view"], a["proj"])
    pre = RasterOracle(*args, m, c, np.zeros((N, 3)), op, np.zeros(3), dtype=np.float64, blend=False)
    zc = np.zeros((N, 3))
    zc[:, 0] = np.where(pre.radii > 0, pre.geom()["depth"], 0.0)
    zc[:, 1] = 1.0
    o = RasterOracle(*args, m, c, zc, op, np.zeros(3), dtype=np.float64)
    return o, np.array(o.color[0]), 1.0 - o.image_state()[0]


def test_reference_construction_matches_central_differences():
    cam, m, c, op = _scene()
    g = np.random.default_rng(11)
    g_depth, g_alpha = g.normal(size=(H, W)), g.normal(size=(H, W))
    o, depth, alpha = _maps(cam, m, c, op)
    assert np.abs(alpha - o.color[1]).max() < 1e-12           # channel 1 of the run IS 1 - final_T
    ft = o.image_state()[0]
    assert ft.min() > 1e-3 and alpha.max() > 0.3                # no walk near the stop rule T < 1e-4; not an empty image
    assert op.max() < 0.99 - 1e-3                               # ... nor an alpha near the 0.99 clamp
    _, amb, _ = o.ambiguous_pairs(eps=1e-3)                     # Gaussians with a pair within 1e-3 of the 1/255 keep rule
    use = np.setdiff1d(np.nonzero(o.radii > 0)[0], np.unique(amb))
    assert (o.radii > 0).sum() >= 30 and len(use) >= 0.9 * N, (int((o.radii > 0).sum()), len(use))

    b = o.backward(np.stack([g_depth, g_alpha, np.zeros((H, W))]))
    view = np.asarray(cam_args(cam)["view"], np.float64)
    d_m = b["means3D"] + b["colors"][:, :1] * view.reshape(4, 4)[:3, 2][None]
    d_op = b["opacity"]

    def loss(m_, op_):
        _, d, a_ = _maps(cam, m_, c, op_)
        return float((g_alpha * a_).sum() + (g_depth * d).sum())

    fd_op, fd_m = np.zeros(N), np.zeros((N, 3))
    for i in use:
        e = np.zeros(N)
        e[i] = STEP
        fd_op[i] = (loss(m, op + e) - loss(m, op - e)) / (2 * STEP)
        for k in range(3):
            dm = np.zeros((N, 3))
            dm[i, k] = STEP
            fd_m[i, k] = (loss(m + dm, op) - loss(m - dm, op)) / (2 * STEP)
    e_op, e_m = max_rel_err(d_op[use], fd_op[use]), max_rel_err(d_m[use], fd_m[use])
    print("reference construction vs central differences: opacity %.3e, means3D %.3e (%d of %d Gaussians)" % (e_op, e_m, len(use), N))
    assert np.abs(fd_m[use]).max() > 0 and np.abs(fd_op[use]).max() > 0
    assert e_op < 1e-5 and e_m < 1e-5, (e_op, e_m)

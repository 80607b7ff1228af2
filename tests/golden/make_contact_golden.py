#!/usr/bin/env python3
"""Generate tests/golden/contact_cmap.npz by IMPORTING the reference (authoring container only):

    python tests/golden/make_contact_golden.py

Same rules as make_golden.py, whose stub approach it reuses: the reference's Python is imported with stub modules
for the packages this image lacks, and only arrays are written.  Reference functions exercised:
  * src/utils/vis_util.py:22-25          get_colors_from_cmap  (matplotlib's lookup, the real matplotlib)
  * src/utils/gaussian_utils.py:431-449  calculate_colors_from_sh
`get_cmap` / `get_contact_dist` (gaussian_utils.py:521-577) cannot be imported and run: they are a taichi kernel and
taichi is not in this image.  The distances and indices recorded here come from the loop oracle
(oracle.torch_ref.contact_dist, pinned against the reference's torch.cdist by contact.npz), the value formula of
get_cmap lines 573-574 is applied in float32 torch on the CPU exactly as written there, and the one-line colour
choices of Composite.render_contacts (src/modules/composite.py:143-214) are restated below in this file's own words.

Contents:
  lut_<name> (256,3) f32            the 256 entries of magma / gray / viridis
  values (K,) f32, colors_<name>    edge-case values and what get_colors_from_cmap returns for them (as float32)
  s<k>_*                            two small composite scenes: inputs, recorded dist / indices, and colors_<render_type>
"""
import os
import sys

sys.dont_write_bytecode = True
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg                      # noqa: E402  (stubs + reference import)
from oracle import torch_ref as tr            # noqa: E402

CMAPS = ("magma", "gray", "viridis")
C_THRESH = 0.004
ALPHA = 0.3


def edge_values():
    g = np.random.default_rng(5)
    one = np.float32(1)
    v = [0.0, 1.0, 1.5, 7.0, -0.1, np.nan, np.inf, np.nextafter(one, np.float32(0)), -0.0, -np.inf, 1e-8, 0.5]
    v += [k / 256.0 for k in range(257)]
    v += [np.nextafter(np.float32(k / 256.0), np.float32(0)) for k in range(1, 257)]
    v += list(g.uniform(-0.05, 1.05, size=3000))
    return np.asarray(v, np.float32)


def value_formula(dist):
    """get_cmap lines 573-574 on a float32 CPU tensor."""
    d = torch.from_numpy(np.asarray(dist, np.float32))
    d = torch.clamp(d.clone(), 0, C_THRESH) / C_THRESH
    return (1 - d).numpy()


def spd6(g, n, lo, hi):
    s = g.uniform(lo, hi, size=(n, 3))
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)
    L = R * s[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1).astype(np.float32)


def make_scene(gu, colors_of, seed, n_h, n_o):
    g = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    cano = f32(g.normal(size=(n_h, 3)) * 0.012)
    bones = mg._rand_rigid(g, 4, ang=0.5, trans=0.01)
    w = g.dirichlet(np.ones(4) * 0.4, size=n_h)
    tf = f32(np.einsum("nb,bij->nij", w, bones))
    tf[:, 3] = (0, 0, 0, 1)
    posed = f32(np.einsum("nij,nj->ni", tf[:, :3, :3], cano) + tf[:, :3, 3])
    obj = f32(g.normal(size=(n_o, 3)) * 0.012 + np.array([0.012, 0.0, 0.0]))
    obj[:7] = posed[11:18]                                   # exact contacts
    obj[20] = obj[3]                                         # a duplicated target (index tie)
    out = dict(h_cano_xyz=cano, h_tf=tf, h_posed_xyz=posed, o_xyz=obj,
               h_features=f32(np.concatenate([g.normal(size=(n_h, 1, 3)), 0.1 * g.normal(size=(n_h, 15, 3))], 1)),
               o_features=f32(np.concatenate([g.normal(size=(n_o, 1, 3)), 0.1 * g.normal(size=(n_o, 15, 3))], 1)),
               h_opacity=f32(g.uniform(0.3, 0.95, size=(n_h, 1))), o_opacity=f32(g.uniform(0.05, 0.5, size=(n_o, 1))),
               h_cano_cov=spd6(g, n_h, 8e-4, 3e-3), h_posed_cov=spd6(g, n_h, 8e-4, 3e-3), o_cov=spd6(g, n_o, 8e-4, 3e-3),
               nocs_grid=f32(g.uniform(0, 1, size=(n_h, 3))), skin_colors=f32(g.uniform(0, 1, size=(n_h, 3))),
               acc_dist=f32(g.uniform(0, 1, size=n_h) * (g.uniform(size=n_h) < 0.5) * 1.6),
               camera_center=f32([0.02, -0.03, -0.25]), cano_camera_center=f32([-0.04, 0.05, -0.22]))
    # recorded nearest-point results (loop oracle) and get_cmap's value
    hd, hi = tr.contact_dist(posed, obj)
    od, oi = tr.contact_dist(obj, posed)
    out.update(h_dist=hd, h_idx=hi.astype(np.int32), o_dist=od, o_idx=oi.astype(np.int32),
               h_value=value_formula(hd), o_value=value_formula(od))
    t = torch.from_numpy
    cam = types.SimpleNamespace(camera_center=t(out["camera_center"])[None])
    cano_cam = types.SimpleNamespace(camera_center=t(out["cano_camera_center"])[None])
    # the reference evaluates the SH colours of one body with that body's own tf: the hand's (N,4,4), None for the object
    rgb_h = gu.calculate_colors_from_sh(t(cano), t(out["h_features"]), t(cano), cano_cam, 3, t(tf)).numpy()
    rgb_o = gu.calculate_colors_from_sh(t(obj), t(out["o_features"]), t(obj), cam, 3, None).numpy()
    out.update(rgb_hand=f32(rgb_h), rgb_object=f32(rgb_o))
    a = ALPHA
    blend = lambda rgb, cm: (t(f32(rgb)) * a + (1 - a) * t(cm)).numpy()      # float32 torch, Python-float weights
    nocs = out["nocs_grid"]
    out["colors_object_only"] = blend(rgb_o, colors_of(out["o_value"], "magma"))
    out["colors_hand_only"] = blend(rgb_h, colors_of(out["h_value"], "magma"))
    out["colors_nocs_hand_only"] = np.where(out["h_value"][:, None] > 0, nocs, np.float32(0))
    out["colors_nocs_object_only"] = np.where(out["o_value"][:, None] > 0, nocs[oi], np.float32(0))
    out["colors_accumulated"] = blend(rgb_h, colors_of(out["acc_dist"], "magma"))
    out["colors_acc_gt_eval"] = colors_of(out["acc_dist"], "gray")
    out["colors_skin_wts"] = out["skin_colors"]
    return out


def main():
    mods = mg._import_reference()
    import src.utils.vis_util as vis_util
    gu = mods["gaussian_utils"]
    import matplotlib.pyplot as plt

    def colors_of(values, name):          # the reference's lookup, then to_tensor's float32
        return np.asarray(vis_util.get_colors_from_cmap(np.asarray(values, np.float32), cmap_name=name)[..., :3]).astype(np.float32)

    out = {}
    for name in CMAPS:
        out["lut_" + name] = np.asarray(plt.get_cmap(name)(np.arange(256))[:, :3]).astype(np.float32)
    out["values"] = edge_values()
    with np.errstate(all="ignore"):
        for name in CMAPS:
            out["colors_" + name] = colors_of(out["values"], name)
        for k, (seed, n_h, n_o) in enumerate(((21, 300, 200), (22, 150, 260))):
            for key, v in make_scene(gu, colors_of, seed, n_h, n_o).items():
                out["s%d_%s" % (k, key)] = v
    path = os.path.join(HERE, "contact_cmap.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    for k in range(2):
        print("scene", k, "hand in contact", float((out["s%d_h_value" % k] > 0).mean()), "object", float((out["s%d_o_value" % k] > 0).mean()))


if __name__ == "__main__":
    main()

"""GPU: contact-map rendering -- the grid search (mgr_contact_near), the colour epilogue (mgr_contact_colors), get_cmap,
render_contacts and CompositeRenderer.  Every check is against a CPU result: oracle.torch_ref.contact_dist (or the
NaN-safe restatement of the same loop in contact_oracle.py where inputs hold NaN, which the oracle's argmin does not
define), numpy restatements of the value formula / matplotlib lookup / blends (pinned to the reference's recorded colours
by test_contact_render_cpu.py), the fixture tests/golden/contact_cmap.npz, and oracle.RasterOracle."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import contact_oracle as co
from oracle import RasterOracle
from oracle import torch_ref as tr
from util import cam_args, make_camera, max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA = 0.3


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "contact_cmap.npz"))


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# mgr_contact_near
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(1, 0), (3, 1), (513, 1024), (5000, 7000), (20000, 30000)])
def test_near_search_equals_brute_force_contract(n1, n2):
    """value for all points, index and distance where value > 0, -1 / 1e9 elsewhere; duplicates, coincident pairs, a far
    outlier and NaN points planted.  The two large sizes must have at least 15 % of their points in contact."""
    from manus_amd.contact import contact_near
    pt1, pt2 = co.contact_inputs(n1, n2)
    has_nan = bool(np.isnan(pt1).any() or np.isnan(pt2).any())
    assert has_nan == (n1 > 100)
    ref_v, ref_i, ref_d = co.near_reference(pt1, pt2, nearest=co.nearest_nan_safe if has_nan else tr.contact_dist)
    if has_nan:       # where no NaN is involved the restated loop is the oracle (rows of pt1 without NaN, pt2 without its NaN row)
        ok1, ok2 = ~np.isnan(pt1).any(1), ~np.isnan(pt2).any(1)
        sub = np.flatnonzero(ok1)[:1500]
        od, oi = tr.contact_dist(pt1[sub], pt2[ok2])
        nd, ni = co.nearest_nan_safe(pt1[sub], pt2)
        np.testing.assert_array_equal(nd, od)
        np.testing.assert_array_equal(ni, np.flatnonzero(ok2)[oi])
    value, idx, dist = contact_near(dev(pt1), dev(pt2), 0.004, want_dist=True)
    assert value.dtype == torch.float32 and idx.dtype == torch.int32 and dist.dtype == torch.float32
    value, idx, dist = host(value), host(idx).astype(np.int64), host(dist)
    hit = ref_v > 0
    print("near %dx%d: %.1f %% in contact, %d distinct LUT bins" % (n1, n2, 100 * hit.mean() if n1 else 0.0,
                                                                    len(np.unique(co.lut_index(ref_v)))))
    np.testing.assert_array_equal(value, ref_v)
    np.testing.assert_array_equal(idx[hit], ref_i[hit])
    np.testing.assert_array_equal(dist[hit], ref_d[hit])
    assert (idx[~hit] == -1).all() and (dist[~hit] == np.float32(1e9)).all()
    if n1 >= 5000:
        assert hit.mean() >= 0.15
    if has_nan:
        assert value[55] == 0 and idx[55] == -1                    # the NaN query
        assert not (idx == 91).any()                               # the NaN target is nobody's neighbour
        assert (value[:20] == 1).all() and (idx[:20] == np.arange(20)).all()   # coincident: distance 0, lowest duplicate


def test_near_search_empty_query_set_and_bad_threshold():
    from manus_amd._lib import ManusHipError
    from manus_amd.contact import contact_near
    v, i, d = contact_near(torch.zeros((0, 3), device=DEV), torch.zeros((5, 3), device=DEV), want_dist=True)
    assert v.shape == (0,) and i.shape == (0,) and d.shape == (0,)
    with pytest.raises(ManusHipError):
        contact_near(torch.zeros((4, 3), device=DEV), torch.zeros((5, 3), device=DEV), c_thresh=0.0)


def test_near_search_composite_scene_size():
    """300k hand x 200k object points (the inputs of test_composite_scene_size_properties): every 997th point against the
    CPU, planted contacts, run-to-run identical bits."""
    from manus_amd.contact import contact_near
    g = torch.Generator(device=DEV).manual_seed(3)
    pt1 = torch.randn((300000, 3), device=DEV, generator=g) * 0.05
    pt2 = torch.randn((200000, 3), device=DEV, generator=g) * 0.05 + torch.tensor([0.04, 0.0, 0.0], device=DEV)
    pt2[1000:1100] = pt1[5000:5100]
    value, idx, dist = contact_near(pt1, pt2, want_dist=True)
    v2, i2, d2 = contact_near(pt1, pt2, want_dist=True)
    assert torch.equal(value, v2) and torch.equal(idx, i2) and torch.equal(dist, d2)
    assert (value[5000:5100] == 1).all() and torch.equal(idx[5000:5100].long(), torch.arange(1000, 1100, device=DEV))
    sub = torch.arange(0, 300000, 997, device=DEV)
    ref_v, ref_i, ref_d = co.near_reference(host(pt1[sub]), host(pt2))
    hit = ref_v > 0
    print("composite size: %.1f %% of the sampled points in contact" % (100 * hit.mean()))
    assert hit.mean() >= 0.15
    np.testing.assert_array_equal(host(value[sub]), ref_v)
    np.testing.assert_array_equal(host(idx[sub]).astype(np.int64)[hit], ref_i[hit])
    np.testing.assert_array_equal(host(dist[sub])[hit], ref_d[hit])
    assert (host(idx[sub])[~hit] == -1).all()
    # get_cmap_values (the existing entry) leaves the division to torch: report, do not assert, how many values differ
    from manus_amd.contact import get_cmap_values
    old = get_cmap_values(pt1, pt2)[0]
    print("get_cmap_values (torch division on the device) differs from the IEEE division in %d of %d values, max %.3g"
          % (int((old != value).sum()), value.numel(), float((old - value).abs().max())))


# ---------------------------------------------------------------------------------------------------------------------
# mgr_contact_colors, get_cmap
# ---------------------------------------------------------------------------------------------------------------------
def test_colour_lookup_equals_reference_colours(fx):
    from manus_amd.contact import contact_colors, get_colors_from_cmap
    v = dev(fx["values"])
    for name in ("magma", "gray", "viridis"):
        np.testing.assert_array_equal(host(contact_colors(v, dev(fx["lut_" + name]))), fx["colors_" + name])
        np.testing.assert_array_equal(host(contact_colors(v, name)), fx["colors_" + name])
    out = get_colors_from_cmap(v.reshape(-1, 1)[:600].reshape(20, 30), "viridis")
    assert tuple(out.shape) == (20, 30, 3)
    np.testing.assert_array_equal(host(out).reshape(-1, 3), fx["colors_viridis"][:600])


def test_colour_blend_and_table_modes_bit_exact(fx):
    """base * alpha + (1 - alpha) * lut[k] equals the numpy expression in fp32 in the same order, bit for bit (the kernel
    is compiled without contraction for that line); the NOCS mode equals np.where."""
    from manus_amd.contact import contact_colors, contact_table_colors
    v = fx["values"]
    g = np.random.default_rng(0)
    base = g.uniform(0, 1.3, size=(v.shape[0], 3)).astype(np.float32)
    for alpha in (0.3, 0.0, 0.77):
        want = co.blend(base, co.lut_colors(v, fx["lut_magma"]), alpha)
        np.testing.assert_array_equal(host(contact_colors(dev(v), dev(fx["lut_magma"]), dev(base), alpha)), want)
    table = g.uniform(0, 1, size=(50, 3)).astype(np.float32)
    idx = g.integers(-1, 50, size=v.shape[0]).astype(np.int32)
    with np.errstate(all="ignore"):
        on = (v > 0) & (idx >= 0)
    want = np.where(on[:, None], table[np.maximum(idx, 0)], np.float32(0))
    np.testing.assert_array_equal(host(contact_table_colors(dev(v), dev(table), dev(idx, torch.int32))), want)
    own = g.uniform(0, 1, size=(v.shape[0], 3)).astype(np.float32)
    with np.errstate(all="ignore"):
        want = np.where((v > 0)[:, None], own, np.float32(0))
    np.testing.assert_array_equal(host(contact_table_colors(dev(v), dev(own))), want)


@pytest.mark.parametrize("k", [0, 1])
def test_get_cmap_returns_the_reference_triple(fx, k):
    from manus_amd.contact import get_cmap, get_cmap_near
    s = lambda name: fx["s%d_%s" % (k, name)]
    for a, b, pre in ((s("h_posed_xyz"), s("o_xyz"), "h"), (s("o_xyz"), s("h_posed_xyz"), "o")):
        for cmap in ("gray", "magma"):
            value, idx, colors = get_cmap(dev(a), dev(b), cmap_type=cmap)
            assert value.dtype == idx.dtype == colors.dtype == torch.float32
            assert tuple(value.shape) == tuple(idx.shape) == (a.shape[0],) and tuple(colors.shape) == (a.shape[0], 3)
            np.testing.assert_array_equal(host(value), s(pre + "_value"))
            np.testing.assert_array_equal(host(idx), s(pre + "_idx").astype(np.float32))
            np.testing.assert_array_equal(host(colors), co.lut_colors(s(pre + "_value"), fx["lut_" + cmap]))
            nv, ni, nc = get_cmap_near(dev(a), dev(b), cmap_type=cmap)
            assert ni.dtype == torch.float32
            hit = s(pre + "_value") > 0
            np.testing.assert_array_equal(host(nv), s(pre + "_value"))
            np.testing.assert_array_equal(host(ni), np.where(hit, s(pre + "_idx"), -1).astype(np.float32))
            np.testing.assert_array_equal(host(nc), host(colors))
    # the default map is the reference's: gray
    np.testing.assert_array_equal(host(get_cmap(dev(s("h_posed_xyz")), dev(s("o_xyz")))[2]),
                                  co.lut_colors(s("h_value"), fx["lut_gray"]))


# ---------------------------------------------------------------------------------------------------------------------
# render_contacts on the fixture scenes
# ---------------------------------------------------------------------------------------------------------------------
W, H = 96, 64


def camera_at(center):
    c = make_camera(W, H, pos=tuple(float(x) for x in center), target=(0.004, 0.0, 0.0))
    return c, SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=H, width=W,
                              world_view_transform=torch.tensor(np.asarray(c["world_view_transform"]), dtype=torch.float32),
                              full_proj_transform=torch.tensor(np.asarray(c["full_proj_transform"]), dtype=torch.float32),
                              camera_center=torch.tensor(center, dtype=torch.float32)[None])   # the fixture's, to the bit


def fixture_pred(fx, k):
    from manus_amd.modules import Pred, _composite
    s = lambda name: dev(fx["s%d_%s" % (k, name)])
    h = Pred(posed_xyz=s("h_posed_xyz"), posed_cov=s("h_posed_cov"), cano_xyz=s("h_cano_xyz"), cano_features=s("h_features"),
             cano_opacity=s("h_opacity"), tf=s("h_tf"))
    o = Pred(posed_xyz=s("o_xyz"), posed_cov=s("o_cov"), cano_xyz=s("o_xyz"), cano_features=s("o_features"),
             cano_opacity=s("o_opacity"), tf=None)
    pred = _composite(h, Pred(o, tf=None))
    pred["h_out"], pred["o_out"] = h, o
    kw = dict(hand_model=SimpleNamespace(get_covariance=lambda: s("h_cano_cov")), obj_model=SimpleNamespace(get_covariance=lambda: s("o_cov")),
              nocs_grid=s("nocs_grid"), skin_colors=s("skin_colors"))
    return pred, kw


CASES = [  # render type, body, camera, cmap, alpha, SH colours involved
    ("object_only", "o", "camera", "magma", ALPHA, True), ("hand_only", "h", "cano_camera", "magma", ALPHA, True),
    ("nocs_hand_only", "h", "cano_camera", "magma", ALPHA, False), ("nocs_object_only", "o", "camera", "magma", ALPHA, False),
    ("accumulated", "h", "cano_camera", "magma", ALPHA, True), ("acc_gt_eval", "h", "camera", "gray", 0, False),
    ("skin_wts", "h", "camera", "gray", 0, False)]


@pytest.mark.parametrize("search", ["near", "brute"])
@pytest.mark.parametrize("k", [0, 1])
def test_render_contacts_every_type(fx, k, search):
    """colors_precomp of each render type against the fixture and the image against render_gaussians on CPU-made colours.

    Types without spherical harmonics (NOCS, acc_gt_eval, skin_wts): colours equal the fixture bit for bit and the image
    equals render_gaussians(..., colors_precomp=<fixture colours>) bit for bit.  The three blended types contain
    calculate_colors_from_sh, which this project's SH kernel matches to the reference at max-rel-err 2e-5
    (test_gpu_lbs_sh.py), not to the bit; so for them: (a) the SH colours meet that bound against the fixture's, (b) the
    blended colours meet the same bound against the fixture (the blend scales the error by alpha < 1), (c) they equal, bit
    for bit, the numpy blend of those SH colours with the fixture's colour-map colours, and (d) the image equals
    render_gaussians on the colours of (c) bit for bit."""
    from manus_amd.modules import contact_render_inputs, render_contacts
    from manus_amd.render import calculate_colors_from_sh, render_gaussians
    s = lambda name: fx["s%d_%s" % (k, name)]
    pred, kw = fixture_pred(fx, k)
    batch = dict(bg_color=torch.ones(3))
    cams = {"camera": camera_at(s("camera_center")), "cano_camera": camera_at(s("cano_camera_center"))}
    n_h = s("h_posed_xyz").shape[0]
    for rtype, body, cam_name, cmap, alpha, has_sh in CASES:
        cam = cams[cam_name][1]
        acc = dev(s("acc_dist")) if rtype in ("accumulated", "acc_gt_eval") else None
        r = contact_render_inputs(pred, cam, rtype, cmap, alpha, acc, search=search, **kw)
        want = s("colors_" + rtype)
        if has_sh:
            b = pred.h_out if body == "h" else pred.o_out
            rgb = host(calculate_colors_from_sh(b.cano_xyz, b.cano_features, b.cano_xyz, cam, 3, b.get("tf")))
            assert max_rel_err(rgb, s("rgb_hand" if body == "h" else "rgb_object")) < 2e-5, rtype
            assert max_rel_err(host(r.colors_precomp), want) < 2e-5, rtype
            value = s("acc_dist") if rtype == "accumulated" else s(body + "_value")
            want = co.blend(rgb, co.lut_colors(value, fx["lut_" + cmap]), alpha)
        np.testing.assert_array_equal(host(r.colors_precomp), want, err_msg=rtype)
        if rtype == "skin_wts":
            assert r.dist is None
        else:
            np.testing.assert_array_equal(host(r.dist), s("acc_dist") if acc is not None else s(body + "_value"), err_msg=rtype)
        xyz = {"object_only": "o_xyz", "nocs_object_only": "o_xyz", "acc_gt_eval": "h_posed_xyz", "skin_wts": "h_posed_xyz"}.get(rtype, "h_cano_xyz")
        cov = {"object_only": "o_cov", "nocs_object_only": "o_cov", "acc_gt_eval": "h_posed_cov", "skin_wts": "h_posed_cov"}.get(rtype, "h_cano_cov")
        np.testing.assert_array_equal(host(r.posed_xyz), s(xyz), err_msg=rtype)
        np.testing.assert_array_equal(host(r.posed_cov), s(cov), err_msg=rtype)
        np.testing.assert_array_equal(host(r.opacity), s("o_opacity") if body == "o" else s("h_opacity"), err_msg=rtype)
        dist, img = render_contacts(pred, batch, cam, rtype, cmap, alpha, acc, search=search, **kw)
        assert tuple(img.shape) == (H, W, 3)
        ref = render_gaussians(dev(s(xyz)), dev(s(cov)), pred.cano_xyz, pred.cano_features,
                               dev(s("o_opacity") if body == "o" else s("h_opacity")), cam, batch["bg_color"], dev(want))["render"]
        assert torch.equal(img, ref), rtype
        assert float((img - 1).abs().max()) > 0.05, rtype            # something was drawn on the white background


def test_object_only_opacity_rows(fx):
    """Each body is rendered with its own opacities; reference_opacity_rows=True takes the composite's first n rows, which
    for the object are the hand's (the reference's behaviour, composite.py:208-213)."""
    from manus_amd.modules import contact_render_inputs, render_contacts
    s = lambda name: fx["s0_" + name]
    pred, kw = fixture_pred(fx, 0)
    cam = camera_at(s("camera_center"))[1]
    n_o = s("o_xyz").shape[0]
    own = contact_render_inputs(pred, cam, "object_only", **kw)
    ref = contact_render_inputs(pred, cam, "object_only", reference_opacity_rows=True, **kw)
    np.testing.assert_array_equal(host(own.opacity), s("o_opacity"))
    np.testing.assert_array_equal(host(ref.opacity), np.concatenate([s("h_opacity"), s("o_opacity")])[:n_o])
    assert tuple(ref.opacity.shape) == (n_o, 1)
    np.testing.assert_array_equal(host(own.colors_precomp), host(ref.colors_precomp))
    batch = dict(bg_color=torch.ones(3))
    a = render_contacts(pred, batch, cam, "object_only", **kw)[1]
    b = render_contacts(pred, batch, cam, "object_only", reference_opacity_rows=True, **kw)[1]
    assert not torch.equal(a, b)
    hand = contact_render_inputs(pred, cam, "hand_only", reference_opacity_rows=True, **kw)
    np.testing.assert_array_equal(host(hand.opacity), s("h_opacity"))      # the hand's rows come first: the same either way


def test_hand_only_against_raster_oracle(fx):
    """hand_only on the 96x64 fixture scene: the CPU rasterizer on the fixture's (reference-made) colours, at the image
    tolerance of test_gpu_raster.py (max 5e-3: isolated threshold flips only, mean 2e-6)."""
    from manus_amd.modules import render_contacts
    s = lambda name: fx["s0_" + name]
    pred, kw = fixture_pred(fx, 0)
    c, cam = camera_at(s("cano_camera_center"))
    dist, img = render_contacts(pred, dict(bg_color=torch.ones(3)), cam, "hand_only", **kw)
    a = cam_args(c)
    ro = RasterOracle(a["W"], a["H"], a["tanfovx"], a["tanfovy"], a["view"], a["proj"], s("h_cano_xyz"), s("h_cano_cov"),
                      s("colors_hand_only"), s("h_opacity")[:, 0], np.ones(3, np.float32))
    ref = np.transpose(ro.color, (1, 2, 0))
    assert (ro.radii > 0).sum() > 100
    d = np.abs(host(img) - ref)
    print("hand_only vs RasterOracle: max %.3g mean %.3g" % (d.max(), d.mean()))
    assert d.max() < 5e-3 and d.mean() < 2e-6
    np.testing.assert_array_equal(host(dist), s("h_value"))


# ---------------------------------------------------------------------------------------------------------------------
# CompositeRenderer
# ---------------------------------------------------------------------------------------------------------------------
def synthetic_composite(n=20000, frames=3):
    from manus_amd.structures import Bones
    from manus_amd.synthetic import make_scene
    sc = make_scene(n_gaussians=n, kind="composite", seed=4, grid_res=24, n_cameras=2, width=W, height=H, cam_radius=0.5,
                    sigma_range=(1e-3, 3e-3), device="cpu", n_poses=frames)
    n_h = sc["n_hand"]
    P = {k: v.to(DEV) for k, v in sc["params"].items()}

    def model(sl, hand):
        m = SimpleNamespace(_xyz=P["_xyz"][sl].contiguous(), _scaling=P["_scaling"][sl].contiguous(),
                            _rotation=P["_rotation"][sl].contiguous(),
                            get_features=torch.cat([P["_features_dc"][sl], P["_features_rest"][sl]], 1).contiguous(),
                            get_opacity=torch.sigmoid(P["_opacity"][sl]).contiguous())
        if hand:
            m.grid_center, m.grid_scale, m.grid_weights = sc["grid_center"], sc["grid_scale"], sc["grid"]
        return m

    def camera(c):
        return SimpleNamespace(fovx=c["fovx"], fovy=c["fovy"], height=c["height"], width=c["width"],
                               world_view_transform=torch.tensor(c["world_view_transform"], dtype=torch.float32),
                               full_proj_transform=torch.tensor(c["full_proj_transform"], dtype=torch.float32),
                               camera_center=torch.tensor(c["camera_center"], dtype=torch.float32)[None])

    batches = [dict(bones_posed=Bones(None, None, None, sc["posed"][f]), bones_rest=Bones(None, None, None, sc["rest"]),
                    camera=camera(sc["cameras"][0]), cano_camera=camera(sc["cameras"][1]), bg_color=torch.ones(3))
               for f in range(frames)]
    return sc, model(slice(0, n_h), True), model(slice(n_h, None), False), batches


def test_composite_renderer_results_over_three_frames(fx):
    """'results' over 3 frames: (H, 4W, 3) = rgb | hand | object | accumulated.  The accumulated panel is coloured from the
    RUNNING SUM of the hand's contact values, kept on the device and updated in frame order: acc = h0; acc += h1;
    acc += h2 (fp32).  The CPU restatement does the same sequential float32 additions on values it computed itself, so the
    colours are compared with assert_array_equal.  The reference sums torch.stack(list) instead, whose order of additions
    is not pinned: the number of points whose colour entry differs from a float64 sum is printed, not asserted."""
    from manus_amd.modules import CompositeRenderer, contact_render_inputs
    from manus_amd.render import calculate_colors_from_sh, render_gaussians
    sc, hand, obj, batches = synthetic_composite()
    R = CompositeRenderer(hand, obj, "results")
    magma = fx["lut_magma"]
    acc = None
    acc64 = 0.0
    for f, batch in enumerate(batches):
        pred = R.render(batch)
        assert tuple(pred.render.shape) == (H, 4 * W, 3)
        assert pred.h_out.posed_xyz.shape[0] == sc["n_hand"] and pred.o_out.tf is None
        h_value, _, _ = co.near_reference(host(pred.h_out.posed_xyz), host(pred.o_out.posed_xyz))
        acc = h_value.copy() if acc is None else (acc + h_value).astype(np.float32)
        acc64 = acc64 + h_value.astype(np.float64)
        np.testing.assert_array_equal(host(R.acc), acc)
        rgb = host(calculate_colors_from_sh(pred.h_out.cano_xyz, pred.h_out.cano_features, pred.h_out.cano_xyz,
                                            batch["cano_camera"], 3, pred.h_out.tf))
        want = co.blend(rgb, co.lut_colors(acc, magma), ALPHA)
        got = contact_render_inputs(pred, batch["cano_camera"], "accumulated", acc_dist=R.acc, hand_model=hand, obj_model=obj)
        np.testing.assert_array_equal(host(got.colors_precomp), want)
        panel = render_gaussians(pred.h_out.cano_xyz, got.posed_cov, pred.cano_xyz, pred.cano_features, pred.h_out.cano_opacity,
                                 batch["cano_camera"], batch["bg_color"], dev(want))["render"]
        assert torch.equal(pred.render[:, 3 * W:], panel)
        full = render_gaussians(pred.posed_xyz, pred.posed_cov, pred.cano_xyz, pred.cano_features, pred.cano_opacity,
                                batch["camera"], batch["bg_color"], None, sh_degree=3, tf=pred.tf)["render"]
        assert torch.equal(pred.render[:, :W], full)
        hand_panel = render_gaussians(pred.h_out.cano_xyz, got.posed_cov, pred.cano_xyz, pred.cano_features, pred.h_out.cano_opacity,
                                      batch["cano_camera"], batch["bg_color"],
                                      dev(co.blend(rgb, co.lut_colors(h_value, magma), ALPHA)))["render"]
        assert torch.equal(pred.render[:, W:2 * W], hand_panel)
        print("frame %d: %.1f %% of the hand in contact, %d points above 1 in the sum" % (f, 100 * (h_value > 0).mean(), int((acc > 1).sum())))
    assert (acc > 0).mean() > 0.01 and R.n_frames == 3
    differ = int((co.lut_index(acc) != co.lut_index(acc64.astype(np.float32))).sum())
    print("colour entries that differ between the fp32 running sum and a float64 sum: %d of %d" % (differ, acc.shape[0]))
    R.reset()
    assert R.acc is None and R.n_frames == 0
    first = R.render(batches[0])
    h0, _, _ = co.near_reference(host(first.h_out.posed_xyz), host(first.o_out.posed_xyz))
    np.testing.assert_array_equal(host(R.acc), h0)


def test_composite_renderer_other_layouts():
    from manus_amd.modules import CompositeRenderer
    sc, hand, obj, batches = synthetic_composite(n=6000, frames=1)
    n_h = sc["n_hand"]
    g = torch.Generator().manual_seed(0)
    nocs, skin, accc = torch.rand((n_h, 3), generator=g).to(DEV), torch.rand((n_h, 3), generator=g).to(DEV), torch.rand((n_h,), generator=g).to(DEV)
    R = CompositeRenderer(hand, obj, "nocs", nocs_grid=nocs, skin_colors=skin, acc_contacts=accc)
    assert tuple(R.render(batches[0]).render.shape) == (H, 3 * W, 3)
    assert tuple(R.render(batches[0], "gt_eval").render.shape) == (H, 2 * W, 3)
    assert tuple(R.render(batches[0], "acc_gt_eval").render.shape) == (H, 2 * W, 3)
    brute = CompositeRenderer(hand, obj, "results", search="brute").render(batches[0]).render
    near = CompositeRenderer(hand, obj, "results").render(batches[0]).render
    assert torch.equal(brute, near)
    with pytest.raises(ValueError):
        R.render(batches[0], "video")

"""Shared by the GPU parity tests (the helpers bench.py also needs live in tools/parity.py): the fused path (mgr_views_forward / mgr_views_backward) against the
ORACLE on identical blend inputs, with the alpha-threshold flips accounted for.

The fused kernels never materialise the rasterizer's inputs, so the comparison is closed around the blend: the
kernels' own per-(view, Gaussian) records (pixel centre, conic, opacity, colour, depth, radius -- read back from the
workspace) are blended by the scalar oracle, forward and backward; the oracle's per-Gaussian blend sums are then pushed
through the torch restatement of the rest of the chain (projection -> LBS / covariance / SH / sigmoid, pinned to the
reference by the golden fixtures) down to the six leaves.

Threshold flips.  On bit-identical inputs the kernels and the oracle still evaluate exp differently (v_exp_f32 in the
log2 domain vs expf), so a (pixel, Gaussian) pair whose alpha lies within rounding of 1/255 can pass the
alpha >= 1/255 test on one side only -- an isolated 1/255-sized difference that says nothing about the arithmetic
being compared.  Instead of choosing seeds without such pairs, they are accounted for: the oracle lists every pair it
evaluated with |255 alpha - 1| <= FLIP_EPS, the device is asked for ITS decision on exactly those pairs
(mgr_debug_pair_alpha runs the device function both blend kernels call), and the oracle composites again with the
pairs on which the two disagree forced to the kernels' outcome.  What is then compared is arithmetic only, at the
north_star bars (PSNR delta < 0.01 dB, gradient max-rel-err < 1e-4) for any seed."""
import ctypes
import math

import numpy as np
import torch

from regimes import oracle_rows_zero, regime_facts, view_depth
from util import max_rel_err, psnr

from tools.parity import (DEV, FLIP_EPS, align_threshold_decisions, device_alpha_decisions, fused_records,  # noqa: F401
                          kernel_last_gaussian, layout, read_records)


def _contributors_at(bo, rec, pix, W):
    """Gaussians that can contribute at the given pixels (a superset: the early stop is ignored): the entries of the
    pixel's tile list whose alpha there reaches 1/255 (within 0.1 %)."""
    pl, rg = bo.binning()
    gx = (W + 15) // 16
    out = set()
    for p in np.unique(np.asarray(pix)):
        px, py = int(p) % W, int(p) // W
        t = (py // 16) * gx + px // 16
        g = pl[rg[t, 0]:rg[t, 1]]
        r = rec[g].astype(np.float64)
        dx, dy = r[:, 0] - px, r[:, 1] - py
        power = -0.5 * (r[:, 2] * dx * dx + r[:, 4] * dy * dy) - r[:, 3] * dx * dy
        alpha = np.minimum(0.99, r[:, 5] * np.exp(np.minimum(power, 0.0)))
        out.update(int(x) for x in g[(power <= 1e-6) & (alpha >= (1.0 - 1e-3) / 255.0)])
    return out


def _ulps(a, b):
    """Distance in units of the last place between two float32 arrays of equal sign."""
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def run_fused_vs_oracle(kind, views, n, W, H, seed, grid_res=24, cam_radius=0.5, sigma_range=(2e-3, 8e-3), account_flips=True,
                        device=DEV, n_cameras=None, g_scale=1.0, own_projection=False, mutate=None, cameras=None):
    """One fused forward + backward of `views` views against the oracle on identical blend inputs.  Returns a dict of
    measured deviations; asserts nothing except exact integer state (visibility counts, radii).

    own_projection=True also runs the ORACLE'S OWN per-Gaussian preprocess (RasterOracle(blend=False) on the torch chain's
    posed means / covariances: an fp32 chain independent of the kernels') and reports, per view, how its integer state
    compares with the kernels': the Gaussians whose radius or tile rectangle differs (listed, with both values), the pair
    counts of both sides, and the depth keys' distance in units of the last place.

    mutate(params) changes the scene's CPU leaves in place before anything reads them (tests/regimes.py): the upload and
    the torch restatement both see the mutated leaves.  res["regime"] holds, per view, regimes.regime_facts of the
    oracle's blend (and whether the oracle's own gradient rows of the Gaussians below 1/255 are exactly zero).

    cameras(scene) replaces or appends entries of the CPU scene's camera list in place, before anything reads it (tests/fused_shapes.py:
    a camera turned away from the scene; one that appends also appends the pose rows of its view).  A view that sees nothing
    adds nothing to the projection figures."""
    from manus_amd import rasterizer as rz
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table, make_scene
    from oracle import BlendOracle
    from oracle import torch_ref as tr
    sc = make_scene(n_gaussians=n, kind=kind, seed=seed, grid_res=grid_res, n_cameras=n_cameras or views, width=W, height=H,
                    cam_radius=cam_radius, sigma_range=sigma_range, device="cpu")
    if mutate is not None:
        mutate(sc["params"])
    if cameras is not None:
        cameras(sc)
    scd = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in sc.items() if k != "params"}
    scd["params"] = {k: v.to(device) for k, v in sc["params"].items()}
    ct = camera_table(sc["cameras"], device)
    hc = HipViewCompute(scd, torch.zeros((len(sc["cameras"]), 3, H, W), device=device), ct)
    rng = np.random.default_rng(7)
    g_img = (g_scale * rng.normal(size=(views, 3, H, W))).astype(np.float32)
    ids = list(range(views))
    rz.set_sync_policy(True)
    out = hc._step_direct(ids, 1.0, g_img=torch.tensor(g_img, device=device))
    torch.cuda.synchronize()
    ws = rz.context().last_ws
    grec, depth, iacc, kernel_last = fused_records(ws, views, n, W, H)
    radii = hc.last_radii.cpu().numpy()
    img = hc.last_image.cpu().numpy()
    bg = np.ones(3, np.float32)
    P = {k: v.clone().requires_grad_(True) for k, v in sc["params"].items()}
    chain, g2, vis_cnt = 0.0, np.zeros(n), np.zeros(n)
    wts = torch.tensor(tr.CONIC_GRAD_WEIGHTS)
    res = dict(ambiguous=0, flips=0, stop_flips=0, stop_violations=0, img_max=0.0, img_mean=0.0, img_frac_2e6=0.0, dpsnr=0.0, sums9=0.0, proj_pix=0.0, proj_conic=0.0,
               proj_col=0.0)
    bos, bws = [], []
    touched = set()      # Gaussians that contribute at a pixel where a threshold decision was (or could be) flipped
    for v in ids:
        bo = BlendOracle(W, H, grec[v][:, 0:2], depth[v], grec[v][:, 2:5], grec[v][:, 5], radii[v], grec[v][:, 6:9], bg)
        # The pixels where the kernels decide a threshold differently from the oracle (alpha >= 1/255 on a pair within rounding
        # of it; the end of a pixel's walk), found on the un-forced oracle whether or not the decisions are then aligned:
        # a flipped decision changes the gradient of everything composited at its pixel, and nothing else.
        klast = kernel_last_gaussian(v, views, n, W, H, kernel_last[v])
        apix, agid, aal = bo.ambiguous_pairs(FLIP_EPS)
        fpix = np.zeros(0, np.int64)
        if len(apix):
            _, dvalid = device_alpha_decisions(grec[v][agid][:, :6], apix % W, apix // W, device)
            fpix = apix[dvalid != (aal >= np.float32(1.0) / np.float32(255.0)).astype(np.int32)].astype(np.int64)
        _, onc = bo.image_state()
        pl, rg = bo.binning()
        gx_ = (W + 15) // 16
        ys_, xs_ = np.mgrid[0:H, 0:W]
        tl = (ys_ // 16) * gx_ + xs_ // 16
        olast = np.where(onc > 0, pl[np.clip(rg[tl, 0].astype(np.int64) + onc - 1, 0, max(len(pl) - 1, 0))] if len(pl) else -1, -1)
        spix = np.nonzero((olast != klast).reshape(-1))[0]
        touched |= _contributors_at(bo, grec[v], np.concatenate([fpix, spix]), W)
        res["decision_pixels"] = res.get("decision_pixels", 0) + int(len(np.unique(np.concatenate([fpix, spix]))))
        if account_flips:
            a, f, sf, sv = align_threshold_decisions(bo, grec[v], grec[v][:, 6:9], bg, W, klast, device)
            res["ambiguous"] += a
            res["flips"] += f
            res["stop_flips"] += sf
            res["stop_violations"] += sv
        bos.append(bo)
        bws.append(bo.backward(g_img[v]))
    nine = lambda b: np.concatenate([b["means2D"][:, :2], b["conic"], b["opacity"][:, None], b["colors"]], 1)
    # the kernel keeps the sums of a Gaussian's lane group (8 views) when any of the group's views is active
    grp_active = np.zeros(n, bool)
    for v in ids:
        grp_active |= np.abs(nine(bws[v])).max(1) > 0
    for v in ids:
        r, bo, b = grec[v], bos[v], bws[v]
        d = np.abs(img[v] - bo.color)
        res["img_max"], res["img_mean"] = max(res["img_max"], float(d.max())), max(res["img_mean"], float(d.mean()))
        res["img_frac_2e6"] = max(res["img_frac_2e6"], float(np.mean(d > 2e-6)))
        tgt = np.clip(bo.color + 0.05 * rng.normal(size=bo.color.shape), 0, 1)
        res["dpsnr"] = max(res["dpsnr"], abs(psnr(img[v], tgt) - psnr(bo.color, tgt)))
        if views <= 8:   # (with more than 8 views the buffer holds the last view group only)
            want9, got9 = nine(b), iacc[:, v % iacc.shape[1], :9]
            for c in range(9):
                res["sums9"] = max(res["sums9"], max_rel_err(got9[grp_active, c], want9[grp_active, c]))
        cc = torch.tensor(np.asarray(sc["cameras"][v]["camera_center"], np.float32))
        if kind == "hand":
            o = tr.hand_forward(P, sc["grid"], sc["grid_center"], sc["grid_scale"], sc["posed"][v], sc["rest"], cc)
        elif kind == "object":
            o = tr.object_forward(P, cc)
        else:
            o = tr.composite_forward(P, sc["n_hand"], sc["grid"], sc["grid_center"], sc["grid_scale"], sc["posed"][v],
                                     sc["rest"], cc)
        c = sc["cameras"][v]
        ndc, conic = tr.project_ewa(o["posed_xyz"], o["posed_cov"], W, H, math.tan(c["fovx"] / 2), math.tan(c["fovy"] / 2),
                                    torch.tensor(np.asarray(c["world_view_transform"], np.float32)),
                                    torch.tensor(np.asarray(c["full_proj_transform"], np.float32)))
        visible = radii[v] > 0
        facts = regime_facts(bos[v], r[:, 5], c, view_depth(o["posed_xyz"].detach().numpy(), c))
        below = visible & (r[:, 5] < np.float32(1.0) / np.float32(255.0))
        facts["oracle_faint_rows_zero"] = oracle_rows_zero(b, below)
        res.setdefault("regime", []).append(facts)
        if own_projection:
            from oracle import RasterOracle
            ro = RasterOracle(W, H, math.tan(c["fovx"] / 2), math.tan(c["fovy"] / 2),
                              np.asarray(c["world_view_transform"], np.float32).reshape(-1),
                              np.asarray(c["full_proj_transform"], np.float32).reshape(-1),
                              o["posed_xyz"].detach().numpy(), o["posed_cov"].detach().numpy(), o["colors"].detach().numpy(),
                              o["opacity"].detach().numpy()[:, 0], bg, blend=False)
            geo = ro.geom()
            kgeo = bos[v].geom()     # the kernels' state through the oracle's rectangle rule (what the identical-inputs blend used)
            dr = np.nonzero(ro.radii != radii[v])[0]
            drect = np.nonzero((geo["rect"] != kgeo["rect"]).any(1) & (ro.radii == radii[v]))[0]
            both = (ro.radii > 0) & visible
            own = res.setdefault("own", [])
            own.append(dict(view=v, radius_differs=[(int(i), int(radii[v][i]), int(ro.radii[i])) for i in dr[:64]], n_radius_differs=int(len(dr)),
                            max_radius_delta=int(np.abs(ro.radii[dr] - radii[v][dr]).max()) if len(dr) else 0,
                            n_rect_differs=int(len(drect)), pairs_kernels=int(bos[v].num_rendered), pairs_oracle=int(ro.num_rendered),
                            pairs_delta_explained=int((geo["tiles_touched"].astype(np.int64) - kgeo["tiles_touched"].astype(np.int64))[np.union1d(dr, drect)].sum()),
                            depth_max_ulps=int(_ulps(geo["depth"][both], depth[v][both]).max()) if both.any() else 0,
                            depth_bit_equal=float(np.mean(geo["depth"][both].view(np.int32) == depth[v][both].view(np.int32))) if both.any() else 1.0,
                            xy_max=float(np.abs(geo["xy"][both] - r[both, 0:2]).max()) if both.any() else 0.0))
            ro.close()
        pix = ((ndc.detach().numpy() + 1.0) * np.array([W, H]) - 1.0) * 0.5
        if visible.any():
            res["proj_pix"] = max(res["proj_pix"], float(np.abs(pix[visible] - r[visible, 0:2]).max()))
            res["proj_conic"] = max(res["proj_conic"], max_rel_err(conic.detach().numpy()[visible], r[visible, 2:5]))
            res["proj_col"] = max(res["proj_col"], float(np.abs(o["colors"].detach().numpy()[visible] - r[visible, 6:9]).max()))
        tv = torch.tensor(visible[:, None].astype(np.float32))
        chain = chain + ((ndc * torch.tensor(b["means2D"][:, :2])).mul(tv).sum()
                         + (conic * wts * torch.tensor(b["conic"])).mul(tv).sum()
                         + (o["colors"] * torch.tensor(b["colors"])).mul(tv).sum()
                         + (o["opacity"][:, 0] * torch.tensor(b["opacity"])).mul(tv[:, 0]).sum())
        g2 += np.linalg.norm(b["means2D"][:, :2], axis=1) * visible
        vis_cnt += visible
    chain.backward()
    res["grads"], res["rows_over_2e5"] = {}, {}
    dev_rows = set()
    for k in P:
        a, b = out["grads"][k].cpu().numpy().reshape(P[k].shape).astype(np.float64), P[k].grad.numpy().astype(np.float64)
        res["grads"][k] = max_rel_err(a, b)
        over = np.abs(a - b).reshape(a.shape[0], -1).max(1) > 2e-5 * np.abs(b).max()
        res["rows_over_2e5"][k] = float(np.mean(over))
        dev_rows.update(int(i) for i in np.nonzero(over)[0])
    # every leaf row that deviates belongs to a Gaussian that contributes at a pixel holding a pair within rounding of the
    # alpha threshold (a flipped pair changes the gradient of everything composited at its pixel)
    res["dev_rows"] = len(dev_rows)
    res["dev_rows_unexplained"] = sorted(dev_rows - touched)[:32]
    res["n_touched"] = len(touched)
    res["grad2d"] = max_rel_err(out["grad2d"].cpu().numpy(), g2)
    np.testing.assert_array_equal(out["vis"].cpu().numpy(), vis_cnt)
    np.testing.assert_array_equal(out["radii"].cpu().numpy(), radii.max(0))
    res["num_rendered"] = [int(bo.num_rendered) for bo in bos]
    res["width"] = W
    for bo in bos:
        bo.close()
    return res


def assert_north_star(res, tag=""):
    """PSNR delta < 0.01 dB, gradient max-rel-err < 1e-4 (BASELINE.json north_star), and the image agrees to fp32 rounding."""
    assert res["stop_violations"] == 0, (tag, res)   # a walk that ends elsewhere than the oracle's does so within rounding of T = 1e-4
    assert res["dpsnr"] < 0.01, (tag, res)
    assert res["img_mean"] < 2e-7 and res["img_max"] < 2e-4 and res["img_frac_2e6"] < 1e-3, (tag, res)
    assert res["sums9"] < 1e-4, (tag, res)
    for k, e in res["grads"].items():
        assert e < 1e-4, (tag, k, res)
    assert res["grad2d"] < 1e-4, (tag, res)
    # pixel centres of two independent fp32 chains: 2e-4 px measured at 1920 x 1080 (coordinates up to 2e3: 1-2 units of the last place)
    assert res["proj_pix"] < 1.1e-6 * res["width"] and res["proj_conic"] < 1e-4 and res["proj_col"] < 2e-5, (tag, res)

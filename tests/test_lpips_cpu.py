"""No GPU: the LPIPS restatement (tests/lpips_ref.py) against central differences and a hand-computed head, the ABI of the new
entries, every refusal that is decided on the host, the workspace layout, the state-dict errors, and the seed conditions of
the GPU gradient tests."""
import ctypes
import os
import re

import pytest
import torch

import lpips_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mgr_lpips_net_bytes", "mgr_lpips_net_pack", "mgr_lpips_workspace_bytes", "mgr_lpips_layout", "mgr_lpips",
               "mgr_lpips_conv_scratch_bytes", "mgr_lpips_conv")


def test_restatement_against_central_differences():
    """fp64, 18x17 VGG input, decisions frozen at the base point: the frozen function is smooth, its gradient exact."""
    W, H = 18, 17
    wts = R.make_weights("vgg", 0)
    pred, target, mask = R.images(0, 1, H, W)
    x0, x1, mk = pred[0].double(), target[0].double(), mask[0].double()
    for normalize, m in ((False, None), (True, mk)):
        _, fa, fb = R.forward("vgg", wts, x0, x1, m, normalize)
        dec = R.decisions_of("vgg", fa["act"])
        val, fz, fzb = R.forward("vgg", wts, x0, x1, m, normalize, decisions=dec)
        assert abs(float(val) - float(R.forward("vgg", wts, x0, x1, m, normalize)[0])) <= 1e-14 * abs(float(val))
        g = R.backward("vgg", wts, fz, fzb, dec, (H, W), m, normalize)
        f = lambda x: float(R.forward("vgg", wts, x, x1, m, normalize, decisions=dec)[0])
        gen = torch.Generator().manual_seed(1)
        h = 1e-5
        dirs = [torch.randn((3, H, W), generator=gen, dtype=torch.float64) for _ in range(6)]
        for idx in [(0, 0, 0), (1, 16, 17), (2, 8, 9), (0, 16, 0), (2, 3, 17)]:
            e = torch.zeros((3, H, W), dtype=torch.float64)
            e[idx[0], idx[1], idx[2]] = 1.0
            dirs.append(e)
        scale = float(g.abs().max())
        for d in dirs:
            fd = (f(x0 + h * d) - f(x0 - h * d)) / (2 * h)
            an = float((g * d).sum())
            assert abs(fd - an) <= 1e-6 * scale * float(d.abs().sum()) ** 0.5 + 1e-6 * abs(an), (fd, an)


def test_head_by_hand():
    """One tap, two channels, two pixels: f0 = (3, 4) and (0, 2), f1 = (0, 5) and (1, 0), lin = (2, 0.5).
    Pixel 0: fh0 = (0.6, 0.8), fh1 = (0, 1): 2 * 0.36 + 0.5 * 0.04 = 0.74.  Pixel 1: fh0 = (0, 1), fh1 = (1, 0): 2 + 0.5 = 2.5.
    Mean 1.62."""
    f0 = torch.tensor([[[3.0, 0.0]], [[4.0, 2.0]]], dtype=torch.float64)
    f1 = torch.tensor([[[0.0, 1.0]], [[5.0, 0.0]]], dtype=torch.float64)
    lin = torch.tensor([2.0, 0.5])
    assert abs(float(R.head(f0, f1, lin, torch.float64)) - 1.62) < 1e-9
    # its gradient against autograd, and the zero-norm rule
    x = f0.clone().requires_grad_(True)
    R.head(x, f1, lin, torch.float64).backward()
    assert float((x.grad - R.head_grad(f0, f1, lin, torch.float64)).abs().max()) < 1e-12
    fz = f0.clone()
    fz[:, 0, 1] = 0.0
    g = R.head_grad(fz, f1, lin, torch.float64)
    assert bool((g[:, 0, 1] == 0).all()) and bool(torch.isfinite(g).all()) and bool((g[:, 0, 0] != 0).any())


def test_pool_winner_is_the_first_maximum():
    a = torch.tensor([[[1.0, 1.0, 0.0], [1.0, 1.0, 5.0], [9.0, 9.0, 9.0]]])
    assert R.winners2(a).tolist() == [[[0]]]
    a = torch.tensor([[[0.0, 2.0], [2.0, 1.0]]])
    assert R.winners2(a).tolist() == [[[1]]]


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        n_decl = _declared_args(header, name)
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_decl, (name, len(args), n_decl)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int), name
        assert hasattr(so, name), "%s is not exported by the built library" % name
    assert _declared_args(header, "mgr_lpips") == 17 and _declared_args(header, "mgr_lpips_net_pack") == 7
    assert "lpips.hip" in build.SOURCES
    for cite in ("loss_utils.py:111-117", "base.py:333-341"):
        assert cite in header


def _err():
    from manus_amd import _lib
    return _lib.lib().mgr_last_error().decode()


def test_refusals_are_decided_on_the_host():
    """Every refusal returns before any launch: with made-up non-null pointers and no device."""
    from manus_amd import _lib
    L = _lib.lib()
    P = 0x1000          # never dereferenced
    nb, H, W = {n: L.mgr_lpips_net_bytes(n) for n in (0, 1)}, 24, 40
    wsb = {0: L.mgr_lpips_workspace_bytes(0, H, W, 1), 1: L.mgr_lpips_workspace_bytes(1, 35, 67, 0)}
    assert nb[0] > 0 and nb[1] > 0 and wsb[0] > 0 and wsb[1] > 0

    def call(net=0, V=1, H=H, W=W, pred=P, target=P, mask=None, blob=P, blob_bytes=None, values=P, grad=P, ws=P, ws_bytes=None):
        return L.mgr_lpips(net, V, H, W, pred, target, mask, blob, nb.get(net, 1) if blob_bytes is None else blob_bytes, 0, 1.0, values,
                           grad, 0, ws, wsb.get(net, 1) if ws_bytes is None else ws_bytes, None)

    for kw, word in ((dict(net=2), "net"), (dict(net=-1), "net"), (dict(V=0), "sizes"), (dict(H=15), "too small"), (dict(W=15), "too small"),
                     (dict(net=1, H=24, W=40, grad=None), "too small"), (dict(pred=None), "null"), (dict(target=None), "null"),
                     (dict(blob=None), "null"), (dict(values=None), "null"), (dict(ws=None), "null"),
                     (dict(blob_bytes=nb[0] - 4), "blob_bytes"), (dict(net=1, H=35, W=67), "forward only")):
        assert call(**kw) == _lib.MGR_EINVAL, kw
        assert word in _err(), (kw, _err())
    assert call(ws_bytes=wsb[0] - 1) == _lib.MGR_ENOMEM and "workspace" in _err()
    # sizes: 0 where there is nothing to size
    assert L.mgr_lpips_net_bytes(2) == 0 and L.mgr_lpips_workspace_bytes(0, 15, 40, 1) == 0 and L.mgr_lpips_workspace_bytes(3, 64, 64, 1) == 0
    assert L.mgr_lpips_workspace_bytes(1, 24, 40, 0) == 0          # AlexNet's last pool has no pixel at 40x24
    # pack
    arr13, arr5 = (ctypes.c_void_p * 13)(*[P] * 13), (ctypes.c_void_p * 5)(*[P] * 5)
    assert L.mgr_lpips_net_pack(2, arr13, arr13, arr5, P, nb[0], None) == _lib.MGR_EINVAL and "net" in _err()
    assert L.mgr_lpips_net_pack(0, arr13, arr13, arr5, P, nb[0] + 1, None) == _lib.MGR_EINVAL and "blob_bytes" in _err()
    assert L.mgr_lpips_net_pack(0, arr13, arr13, arr5, None, nb[0], None) == _lib.MGR_EINVAL and "null" in _err()
    hole = (ctypes.c_void_p * 13)(*([P] * 12 + [None]))
    assert L.mgr_lpips_net_pack(0, hole, arr13, arr5, P, nb[0], None) == _lib.MGR_EINVAL and "null" in _err()
    # layout
    buf = (ctypes.c_size_t * 22)()
    assert L.mgr_lpips_layout(0, H, W, 1, buf, 21) == _lib.MGR_EINVAL and L.mgr_lpips_layout(2, H, W, 1, buf, 22) == _lib.MGR_EINVAL
    assert L.mgr_lpips_layout(0, 8, 8, 1, buf, 22) == _lib.MGR_EINVAL
    # the single convolution
    assert L.mgr_lpips_conv(0, 4, 8, 8, 3, 3, 1, 1, P, None, P, None, 1, 0, P, P, 1 << 20, None) == _lib.MGR_EINVAL
    assert L.mgr_lpips_conv(4, 4, 8, 8, 3, 3, 2, 1, P, None, P, None, 0, 1, P, P, 1 << 20, None) == _lib.MGR_EINVAL
    assert L.mgr_lpips_conv(4, 4, 8, 8, 3, 3, 1, 1, P, None, P, None, 1, 0, P, P, 16, None) == _lib.MGR_ENOMEM


def test_layout_is_consistent_and_monotone():
    from manus_amd.lpips import TAP_CHANNELS, layout
    from manus_amd import _lib
    L = _lib.lib()
    for net, nid, sizes in (("vgg", 0, [(16, 16), (17, 33), (24, 40), (25, 40), (24, 41), (48, 64), (1080, 1920)]),
                            ("alex", 1, [(35, 67), (36, 67), (35, 68), (48, 64), (1080, 1920)])):
        last = None
        for H, W in sizes:
            for need in (0, 1):
                lay = layout(net, H, W, need)
                total = L.mgr_lpips_workspace_bytes(nid, H, W, need)
                assert lay["total"] == total > 0
                # ascending, 256-byte aligned, and every block as large as what it stores
                offs = lay["act"] + lay["tap"] + list(lay["scratch"]) + [lay["part"], lay["total"]]
                assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and all(a < b for a, b in zip(offs, offs[1:]))
                feats = R.features(net, R.make_weights(net, 0), torch.zeros((3, H, W)), torch.float32) if H * W < 10000 else None
                if feats is not None:
                    for i, a in enumerate(feats["act"]):
                        assert offs[i + 1] - offs[i] >= 4 * a.numel(), (net, H, W, i)
                    for k in range(5):
                        j = len(feats["act"]) + k
                        assert offs[j + 1] - offs[j] >= 4 * feats["tap"][k].numel() and feats["tap"][k].shape[0] == TAP_CHANNELS[net][k]
                    assert lay["scratch"][1] - lay["scratch"][0] >= 4 * 3 * H * W
            assert L.mgr_lpips_workspace_bytes(nid, H, W, 1) >= L.mgr_lpips_workspace_bytes(nid, H, W, 0)
        # monotone in H and in W
        for H in (35, 36, 47, 48, 100):
            row = [L.mgr_lpips_workspace_bytes(nid, H, W, 1) for W in (67, 68, 95, 96, 97, 200)]
            assert all(a <= b for a, b in zip(row, row[1:])), (net, H, row)
            col = [L.mgr_lpips_workspace_bytes(nid, Hh, 67 + H, 1) for Hh in (35, 36, 47, 48, 49, 200)]
            assert all(a <= b for a, b in zip(col, col[1:])), (net, H, col)
    # the sizes the issue derives at 1920x1080, per pixel of the input: 270 floats of pred's activations, 122 of the target's taps
    lay = layout("vgg", 1080, 1920, 1)
    px = 1080 * 1920
    assert abs((lay["tap"][0] - lay["act"][0]) / (4 * px) - 270) < 0.5 and abs((lay["scratch"][0] - lay["tap"][0]) / (4 * px) - 122) < 0.5
    assert abs((lay["part"] - lay["scratch"][0]) / (4 * px) - 128) < 0.5


def test_state_dict_errors():
    from manus_amd._lib import ManusHipError
    from manus_amd.lpips import LPIPS
    with pytest.raises(ManusHipError, match="net must be"):
        LPIPS("squeeze")
    for net in ("vgg", "alex"):
        sd, lin = R.state_dicts(net, R.make_weights(net, 0))
        first = "features.%d.weight" % R.CONV_INDEX[net][1]
        bad = dict(sd)
        del bad[first]
        with pytest.raises(ManusHipError, match=re.escape(first)):
            LPIPS.from_state_dicts(bad, lin, net=net, device="cpu")
        bad = dict(sd)
        bad[first] = sd[first][:, :-1]
        with pytest.raises(ManusHipError, match="shape"):
            LPIPS.from_state_dicts(bad, lin, net=net, device="cpu")
        bad = dict(sd)
        bad["features.0.bias"] = sd["features.0.bias"][None]
        with pytest.raises(ManusHipError, match="shape"):
            LPIPS.from_state_dicts(bad, lin, net=net, device="cpu")
        bl = dict(lin)
        del bl["lin3.model.1.weight"]
        with pytest.raises(ManusHipError, match="lin3"):
            LPIPS.from_state_dicts(sd, bl, net=net, device="cpu")
        bl = dict(lin)
        bl["lin0.model.1.weight"] = lin["lin0.model.1.weight"].reshape(-1)
        with pytest.raises(ManusHipError, match="shape"):
            LPIPS.from_state_dicts(sd, bl, net=net, device="cpu")
    with pytest.raises(ManusHipError, match="no weights"):
        LPIPS("vgg").values_grad(torch.zeros((1, 3, 24, 40)), torch.zeros((1, 3, 24, 40)))


@pytest.mark.parametrize("W,H,seed", R.GRAD_CASES)
def test_seed_conditions_of_the_gpu_gradient_tests(W, H, seed):
    """The caps of tests/test_gpu_lpips.py are conditions on the committed seeds, not measurements: for the fp32 restatement
    against fp64 no decision differs away from a threshold, at most 0.1 % of a layer's decisions differ, and no pixel has
    all-zero tap features."""
    wts = R.make_weights("vgg", 0)
    pred, target, mask = R.images(seed, 1, H, W)
    for normalize, m in ((False, None), (True, mask[0])):
        _, fa, _ = R.forward("vgg", wts, pred[0], target[0], m, normalize)
        _, fa32, _ = R.forward("vgg", wts, pred[0], target[0], m, normalize, dtype=torch.float32)
        for kind, i, n, differing, off_threshold in R.compare_decisions("vgg", R.decisions_of("vgg", fa32["act"]), fa, fa32):
            assert off_threshold == 0 and differing <= 1e-3 * n, (kind, i, n, differing, off_threshold)
        for f in (fa, fa32):
            for k in range(5):
                assert bool(((f["tap"][k] ** 2).sum(0) > 0).all())

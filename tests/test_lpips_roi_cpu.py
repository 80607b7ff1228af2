"""No GPU: the ABI of the windowed LPIPS entries, `fit_rects` against a brute-force restatement, `FrameStore.lpips_rects` on
hand-written bboxes, the sizes, and every refusal of the windowed calls that is decided before the device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_lpips_roi_workspace_bytes": 4, "mgr_lpips_taps_bytes": 3, "mgr_lpips_roi_taps_op": 14, "mgr_lpips_roi_op": 20,
               "mgr_lpips_roi": 19}
MIN = {"vgg": 16, "alex": 31}          # by the layer tables (the library is asked, this restates it)


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return len(m.group(1).strip().split(","))


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib
    header = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_ENTRIES.items():
        assert _declared_args(header, name) == n_args, name
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_args, (name, len(args))
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int), name
        assert hasattr(so, name), "%s is not exported by the built library" % name
    assert "NOT the full-frame value restricted to a region" in header


def test_min_size_is_the_library_s():
    from manus_amd.lpips import min_size
    assert {n: min_size(n) for n in MIN} == MIN


# ---------------------------------------------------------------------------
# fit_rects
# ---------------------------------------------------------------------------
def _brute_span(a, n, margin, m, F):
    """The pixels of [a - margin, a + n + margin) inside [0, F) as a set; then pixels added one at a time, alternately on the
    left (first) and on the right, skipping a side at its border, until there are m."""
    px = [p for p in range(a - margin, a + n + margin) if 0 <= p < F]
    if not px:
        return None
    lo, hi = px[0], px[-1] + 1
    need = max(m - (hi - lo), 0)
    left = need // 2
    lo2 = lo - left
    hi2 = hi + (need - left)
    while lo2 < 0:
        lo2 += 1
        hi2 += 1
    while hi2 > F:
        lo2 -= 1
        hi2 -= 1
    return lo2, hi2 - lo2


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_fit_rects_against_brute_force(net):
    from manus_amd.lpips import fit_rects
    rng = np.random.default_rng(7 if net == "vgg" else 8)
    m = MIN[net]
    seen_grown = seen_shifted = seen_clamped = seen_gone = 0
    for _ in range(300):
        H, W = int(rng.integers(m, 4 * m)), int(rng.integers(m, 5 * m))
        margin = int(rng.choice([0, 0, 1, 3, 16]))
        V = 4
        rects = np.stack([rng.integers(-m, W + m, V), rng.integers(-m, H + m, V), rng.integers(0, 2 * m, V), rng.integers(0, 2 * m, V)], 1)
        out = fit_rects(rects, H, W, net, margin)
        assert out.shape == (V, 4) and out.dtype == np.int32
        for (x0, y0, w, h), (fx, fy, fw, fh) in zip(rects.tolist(), out.tolist()):
            bx = _brute_span(x0, w, margin, m, W) if w and h else None
            by = _brute_span(y0, h, margin, m, H) if w and h else None
            if bx is None or by is None:
                assert (fx, fy, fw, fh) == (0, 0, 0, 0)           # empty stays empty; nothing of it in the frame: empty
                seen_gone += 1
                continue
            assert (fx, fw) == bx and (fy, fh) == by, ((x0, y0, w, h), margin, (H, W))
            # inside the frame, at least the minimum
            assert 0 <= fx and fx + fw <= W and 0 <= fy and fy + fh <= H and fw >= m and fh >= m
            # contains the input with its margin where the frame allows: all of it that lies inside the frame
            cx0, cx1 = max(x0 - margin, 0), min(x0 + w + margin, W)
            cy0, cy1 = max(y0 - margin, 0), min(y0 + h + margin, H)
            assert fx <= cx0 and cx1 <= fx + fw and fy <= cy0 and cy1 <= fy + fh
            seen_clamped += (x0 - margin < 0 or x0 + w + margin > W)
            seen_grown += cx1 - cx0 < m
            seen_shifted += (cx1 - cx0 < m and (fx == 0 or fx + fw == W))
    assert min(seen_grown, seen_shifted, seen_clamped, seen_gone) > 20


def test_fit_rects_by_hand():
    from manus_amd.lpips import fit_rects
    H, W = 40, 56
    got = fit_rects([(5, 3, 33, 17), (5, 3, 33, 17), (20, 10, 4, 6), (54, 38, 2, 2), (0, 0, 0, 7), (7, 9, 0, 0), (0, 0, 56, 40)], H, W, "vgg",
                    margin=0).tolist()
    assert got == [[5, 3, 33, 17], [5, 3, 33, 17], [14, 5, 16, 16], [40, 24, 16, 16], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 56, 40]]
    # a margin is applied, then clamped
    assert fit_rects([(5, 3, 33, 17)], H, W, "vgg", margin=4).tolist() == [[1, 0, 41, 24]]
    assert fit_rects([(5, 3, 33, 17)], H, W, "vgg", margin=100).tolist() == [[0, 0, 56, 40]]
    # a frame smaller than the minimum, negative sizes
    for hw in ((15, 56), (40, 15)):
        with pytest.raises(ValueError, match="smaller"):
            fit_rects([(0, 0, 4, 4)], hw[0], hw[1], "vgg")
    with pytest.raises(ValueError, match="smaller"):
        fit_rects([(0, 0, 4, 4)], 30, 56, "alex")
    assert fit_rects([(0, 0, 4, 4)], 31, 56, "alex").tolist() == [[0, 0, 31, 31]]
    with pytest.raises(ValueError, match="negative"):
        fit_rects([(0, 0, -4, 4)], H, W, "vgg")
    assert fit_rects(np.zeros((0, 4), np.int64), H, W, "vgg").shape == (0, 4)


def test_frame_store_lpips_rects():
    from manus_amd.frames import FrameStore
    # source frame 128 x 96, k = 2: the output frame is 64 x 48
    bboxes = [(2, 6, 61, 85), (101, 38, 115, 52), (0, 0, 128, 96), (9, 9, 9, 9), (11, 15, 12, 16), (100, 70, 128, 96)]
    st = FrameStore(torch.zeros(16 * len(bboxes), dtype=torch.uint8), [16 * i for i in range(len(bboxes))], bboxes, 48, 64, k=2)
    got = st.lpips_rects(range(len(bboxes)), margin=0).tolist()
    # out_rect rounds outwards: (1,3)-(31,43); (50,19)-(58,26) is 8 x 7 -> grown to 16 x 16 around it; the frame; empty; one
    # pixel (5,7) -> 16 x 16 clamped at the left / top; the corner box (50,35)-(64,48) is 14 x 13 -> shifted inside
    assert got == [[1, 3, 30, 40], [46, 15, 16, 16], [0, 0, 64, 48], [0, 0, 0, 0], [0, 0, 16, 16], [48, 32, 16, 16]]
    got = st.lpips_rects([1, 3, 0]).tolist()            # margin 16 by default
    assert got == [[34, 3, 30, 39], [0, 0, 0, 0], [0, 0, 47, 48]]
    assert st.lpips_rects([1], margin=0, net="alex").tolist() == [[33, 7, 31, 31]]
    with pytest.raises(KeyError):
        st.lpips_rects([99])


# ---------------------------------------------------------------------------
# sizes and refusals
# ---------------------------------------------------------------------------
def _rects(rows):
    a = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 4))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _err():
    from manus_amd import _lib
    return _lib.lib().mgr_last_error().decode()


def test_sizes():
    from manus_amd import _lib
    from manus_amd.lpips import layout
    L = _lib.lib()
    keep, r = _rects([(5, 3, 33, 17), (0, 0, 0, 0), (1, 1, 40, 24), (9, 9, 0, 5)])
    for need in (0, 1):
        assert L.mgr_lpips_roi_workspace_bytes(0, 4, r, need) == max(L.mgr_lpips_workspace_bytes(0, 17, 33, need),
                                                                     L.mgr_lpips_workspace_bytes(0, 24, 40, need))
    keep, r = _rects([(0, 0, 0, 0)])
    assert L.mgr_lpips_roi_workspace_bytes(0, 1, r, 1) == 0
    for bad in ((5, 3, 15, 16), (5, 3, -16, 16), (5, 3, 16, -1)):
        keep, r = _rects([(5, 3, 33, 17), bad])
        assert L.mgr_lpips_roi_workspace_bytes(0, 2, r, 1) == 0, bad
    assert L.mgr_lpips_roi_workspace_bytes(2, 1, r, 1) == 0 and L.mgr_lpips_roi_workspace_bytes(0, 1, None, 1) == 0
    # the taps: the tap region of the workspace, 122 floats per pixel at a large window
    for net, nid, (h, w) in (("vgg", 0, (17, 33)), ("vgg", 0, (512, 512)), ("alex", 1, (35, 67))):
        lay = layout(net, h, w, 0)
        assert L.mgr_lpips_taps_bytes(nid, h, w) == lay["scratch"][0] - lay["tap"][0] > 0
    assert abs(L.mgr_lpips_taps_bytes(0, 512, 512) / (4.0 * 512 * 512) - 122) < 0.5
    assert L.mgr_lpips_taps_bytes(0, 15, 40) == 0 and L.mgr_lpips_taps_bytes(1, 24, 40) == 0 and L.mgr_lpips_taps_bytes(2, 64, 64) == 0


def test_refusals_are_decided_on_the_host():
    """Every refusal returns before any launch: with made-up non-null pointers and no device."""
    from manus_amd import _lib
    L = _lib.lib()
    P = 0x1000          # never dereferenced
    nb = {n: L.mgr_lpips_net_bytes(n) for n in (0, 1)}
    H, W = 40, 56
    good = (5, 3, 33, 17)
    scales = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    BIG = 1 << 40

    def call(net=0, V=3, H=H, W=W, rects=(good, good, good), pred=P, target=P, mask=None, blob=P, blob_bytes=None, gs=scales, values=P,
             grad=P, taps=None, ws=P, ws_bytes=BIG, operands=0):
        keep, r = _rects(rects) if rects is not None else (None, None)
        return L.mgr_lpips_roi_op(net, V, H, W, r, pred, target, mask, blob, nb.get(net, 1) if blob_bytes is None else blob_bytes, 0, gs,
                                  values, grad, 0, taps, ws, ws_bytes, None, operands)

    three = lambda r: (good, good, r)
    no_taps = (ctypes.c_void_p * 3)(P, P, None)
    for kw, word in ((dict(net=2), "net"), (dict(operands=2), "operands"), (dict(V=0), "sizes"), (dict(H=0), "sizes"),
                     (dict(rects=three((30, 20, 40, 16))), "not inside"), (dict(rects=three((5, 30, 33, 17))), "not inside"),
                     (dict(rects=three((-1, 3, 33, 17))), "not inside"), (dict(rects=three((5, -1, 33, 17))), "not inside"),
                     (dict(rects=three((2 ** 31 - 8, 3, 33, 17))), "not inside"),
                     (dict(rects=three((5, 3, -16, 16))), "negative"), (dict(rects=three((5, 3, 16, -16))), "negative"),
                     (dict(rects=three((5, 3, 15, 16))), "too small"), (dict(rects=three((5, 3, 16, 15))), "too small"),
                     (dict(net=1, grad=None, gs=None, rects=three((5, 3, 40, 30))), "too small"),
                     (dict(rects=None), "null"), (dict(pred=None), "null"), (dict(target=None), "null"), (dict(blob=None), "null"),
                     (dict(values=None), "null"), (dict(ws=None), "null"), (dict(gs=None), "null"),
                     (dict(target=None, taps=no_taps), "neither a target nor cached taps"),
                     (dict(blob_bytes=nb[0] - 4), "blob_bytes"), (dict(blob_bytes=L.mgr_lpips_net_bytes_op(0, 1)), "blob_bytes"),
                     (dict(net=1, H=48, W=80, rects=three((9, 5, 67, 35))), "forward only")):
        assert call(**kw) == _lib.MGR_EINVAL, kw
        assert word in _err(), (kw, _err())
    keep, r = _rects([good] * 3)
    need = L.mgr_lpips_roi_workspace_bytes(0, 3, r, 1)
    assert call(ws_bytes=need - 1) == _lib.MGR_ENOMEM and "workspace" in _err()
    # the plain fp32 wrapper refuses alike
    assert L.mgr_lpips_roi(0, 3, H, W, _rects(three((5, 3, 15, 16)))[1], P, P, None, P, nb[0], 0, scales, P, P, 0, None, P, BIG,
                           None) == _lib.MGR_EINVAL and "too small" in _err()

    # the taps entry
    def taps_call(net=0, H=H, W=W, rect=good, target=P, blob=P, blob_bytes=None, out=P, ws=P, ws_bytes=BIG, operands=0):
        keep, r = _rects([rect]) if rect is not None else (None, None)
        return L.mgr_lpips_roi_taps_op(net, H, W, r, target, None, blob, nb.get(net, 1) if blob_bytes is None else blob_bytes, 0, out, ws,
                                       ws_bytes, None, operands)

    for kw, word in ((dict(net=2), "net"), (dict(operands=3), "operands"), (dict(W=0), "sizes"), (dict(rect=(30, 20, 40, 16)), "not inside"),
                     (dict(rect=(5, 3, -16, 16)), "negative"), (dict(rect=(5, 3, 15, 16)), "too small"), (dict(rect=(0, 0, 0, 0)), "empty"),
                     (dict(rect=None), "null"), (dict(target=None), "null"), (dict(blob=None), "null"), (dict(out=None), "null"),
                     (dict(ws=None), "null"), (dict(blob_bytes=nb[0] + 4), "blob_bytes")):
        assert taps_call(**kw) == _lib.MGR_EINVAL, kw
        assert word in _err(), (kw, _err())
    assert taps_call(ws_bytes=L.mgr_lpips_workspace_bytes(0, 17, 33, 0) - 1) == _lib.MGR_ENOMEM and "workspace" in _err()


def test_python_refusals_before_the_device():
    from manus_amd._lib import ManusHipError
    from manus_amd.lpips import LPIPS, TargetTaps
    z = torch.zeros((2, 3, 40, 56))
    with pytest.raises(ManusHipError, match="no weights"):
        LPIPS("vgg").values_grad(z, z, rects=[(0, 0, 56, 40)] * 2)
    with pytest.raises(ManusHipError, match="no weights"):
        LPIPS("vgg").target_taps(z, [(0, 0, 56, 40)] * 2)
    m = LPIPS("vgg")
    m.blob = torch.zeros(4, dtype=torch.uint8)           # (a stand-in: every refusal below comes before it is read)
    with pytest.raises(ManusHipError, match=r"\(2,4\)"):
        m.values_grad(z, z, rects=[(0, 0, 56, 40)])
    with pytest.raises(ManusHipError, match="one float per view"):
        m.values_grad(z, z, rects=[(0, 0, 56, 40)] * 2, grad_scales=[1.0])
    with pytest.raises(ManusHipError, match="target or target_taps"):
        m.values_grad(z, None, rects=[(0, 0, 56, 40)] * 2)
    with pytest.raises(ManusHipError, match="windowed call"):
        m.values_grad(z, z, grad_scales=[1.0, 1.0])
    rects = np.asarray([(0, 0, 56, 40)] * 2, np.int32)
    taps = TargetTaps([None, None], rects, (40, 56), "vgg", "fp32", False, False)
    assert taps.matches(rects, (40, 56), "vgg", "fp32", False, False) and taps.nbytes == 0
    for other in ((rects + 1, (40, 56), "vgg", "fp32", False, False), (rects, (41, 56), "vgg", "fp32", False, False),
                  (rects, (40, 56), "alex", "fp32", False, False), (rects, (40, 56), "vgg", "bf16", False, False),
                  (rects, (40, 56), "vgg", "fp32", True, False), (rects, (40, 56), "vgg", "fp32", False, True),
                  (rects[:1], (40, 56), "vgg", "fp32", False, False)):
        assert not taps.matches(*other)
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(z, z, rects=rects + 1, target_taps=taps)
    with pytest.raises(ManusHipError, match="target_taps"):
        m.values_grad(z, z, rects=rects, target_taps=[None, None])

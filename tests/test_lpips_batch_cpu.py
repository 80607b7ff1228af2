"""No GPU: the ABI of the batched LPIPS entries (mgr_lpips_roi_batch*, mgr_lpips_roi_taps_batch_op), the batched workspace
sizes, `fit_rects(quantum=, common=)` against a brute-force restatement, `FrameStore.lpips_rects(quantum=, common=)` on
hand-written bboxes, and every refusal of the batched calls that is decided before the device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_lpips_roi_batch_workspace_bytes": 5, "mgr_lpips_roi_taps_batch_op": 16, "mgr_lpips_roi_batch_op": 21,
               "mgr_lpips_roi_batch": 20}
MIN = {"vgg": 16, "alex": 31}


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return len(m.group(1).strip().split(","))


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib, lpips
    header = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_ENTRIES.items():
        assert _declared_args(header, name) == n_args, name
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_args, (name, len(args))
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int), name
        assert hasattr(so, name), "%s is not exported by the built library" % name
    # the batched call is the sequential one and a trailing max_batch
    assert _declared_args(header, "mgr_lpips_roi_batch_op") == _declared_args(header, "mgr_lpips_roi_op") + 1
    m = re.search(r"^#define\s+LP_MAX_BATCH\s+(\d+)", header, re.M)
    assert m and int(m.group(1)) == _lib.LP_MAX_BATCH == lpips.LP_MAX_BATCH == 16


# ---------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------
def _rects(rows):
    a = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 4))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _err():
    from manus_amd import _lib
    return _lib.lib().mgr_last_error().decode()


def test_batched_sizes():
    from manus_amd import _lib
    from manus_amd.lpips import layout
    L = _lib.lib()
    mixed = [(5, 3, 33, 17), (0, 0, 0, 0), (1, 1, 40, 24), (9, 9, 0, 5), (7, 2, 33, 17)]
    keep, r = _rects(mixed)
    for need in (0, 1):
        assert L.mgr_lpips_roi_batch_workspace_bytes(0, 5, r, need, 1) == L.mgr_lpips_roi_workspace_bytes(0, 5, r, need) > 0
    # one size: monotone in max_batch up to the group's size, constant beyond it (and beyond LP_MAX_BATCH)
    for n_views, top in ((5, 5), (20, _lib.LP_MAX_BATCH)):
        keep, r = _rects([(i % 7, i % 5, 24, 16) for i in range(n_views)])
        for need in (0, 1):
            sizes = [L.mgr_lpips_roi_batch_workspace_bytes(0, n_views, r, need, b) for b in range(1, n_views + 4)]
            assert sizes[0] == L.mgr_lpips_workspace_bytes(0, 16, 24, need)
            assert all(a < b for a, b in zip(sizes[:top - 1], sizes[1:top])), sizes
            assert all(s == sizes[top - 1] for s in sizes[top - 1:]), sizes
            # every region G times as long: between G and G + 1 one-view sizes less the alignment slack
            lay = layout("vgg", 16, 24, need)
            n_regions = len(lay["act"]) + len(lay["tap"]) + 3
            for g, s in enumerate(sizes[:top], 1):
                assert g * sizes[0] - 256 * n_regions * g <= s <= g * sizes[0], (g, s, sizes[0])
    # the largest chunk counts, not the largest view: three small views of one size outgrow one larger view
    keep, r = _rects([(0, 0, 24, 16), (1, 1, 24, 16), (2, 2, 33, 17), (3, 3, 24, 16)])
    one = L.mgr_lpips_workspace_bytes(0, 17, 33, 1)
    assert L.mgr_lpips_roi_batch_workspace_bytes(0, 4, r, 1, 1) == one
    assert L.mgr_lpips_roi_batch_workspace_bytes(0, 4, r, 1, 8) > one
    # refused: 0
    assert L.mgr_lpips_roi_batch_workspace_bytes(0, 4, r, 1, 0) == 0 and L.mgr_lpips_roi_batch_workspace_bytes(0, 4, r, 1, -3) == 0
    assert L.mgr_lpips_roi_batch_workspace_bytes(2, 4, r, 1, 4) == 0 and L.mgr_lpips_roi_batch_workspace_bytes(0, 4, None, 1, 4) == 0
    for bad in ((5, 3, 15, 16), (5, 3, -16, 16), (5, 3, 16, -1)):
        keep, r = _rects([(5, 3, 33, 17), bad])
        assert L.mgr_lpips_roi_batch_workspace_bytes(0, 2, r, 1, 4) == 0, bad
    keep, r = _rects([(0, 0, 0, 0)])
    assert L.mgr_lpips_roi_batch_workspace_bytes(0, 1, r, 1, 4) == 0


# ---------------------------------------------------------------------------
# fit_rects(quantum=, common=)
# ---------------------------------------------------------------------------
def _brute_widen(lo, n, to, F):
    """[lo, lo + n) of a side F widened to min(to, F) pixels one at a time: on the right while there is room, else on the left."""
    px = set(range(lo, lo + n))
    while len(px) < min(to, F):
        px.add(max(px) + 1 if max(px) + 1 < F else min(px) - 1)
    return min(px), len(px)


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_fit_rects_quantum_common_against_brute_force(net):
    from manus_amd.lpips import fit_rects
    rng = np.random.default_rng(17 if net == "vgg" else 18)
    m = MIN[net]
    seen_capped = seen_shifted = seen_rounded = seen_empty = seen_common_grew = 0
    for _ in range(300):
        H, W = int(rng.integers(m, 4 * m)), int(rng.integers(m, 5 * m))
        margin = int(rng.choice([0, 0, 1, 3, 16]))
        q = int(rng.choice([0, 1, 2, 8, 16, 32]))
        common = bool(rng.integers(0, 2))
        V = 4
        rects = np.stack([rng.integers(-m, W + m, V), rng.integers(-m, H + m, V), rng.integers(0, 2 * m, V), rng.integers(0, 2 * m, V)], 1)
        base = fit_rects(rects, H, W, net, margin)
        # both off is today's output exactly
        assert np.array_equal(fit_rects(rects, H, W, net, margin, quantum=0, common=False), base)
        out = fit_rects(rects, H, W, net, margin, quantum=q, common=common)
        assert out.shape == (V, 4) and out.dtype == np.int32
        # the restatement: quantum per view, then the set's largest sides
        want = []
        for fx, fy, fw, fh in base.tolist():
            if fw == 0:
                want.append((0, 0, 0, 0))
                continue
            if q > 0:
                fx, fw = _brute_widen(fx, fw, -(-fw // q) * q, W)
                fy, fh = _brute_widen(fy, fh, -(-fh // q) * q, H)
            want.append((fx, fy, fw, fh))
        if common and any(w[2] for w in want):
            cw, ch = max(w[2] for w in want), max(w[3] for w in want)
            want = [w if w[2] == 0 else _brute_widen(w[0], w[2], cw, W)[:1] + _brute_widen(w[1], w[3], ch, H)[:1] + (cw, ch) for w in want]
        assert out.tolist() == [list(w) for w in want], (rects.tolist(), (H, W), margin, q, common)
        live = [(b, o) for b, o in zip(base.tolist(), out.tolist()) if b[2]]
        for b, o in zip(base.tolist(), out.tolist()):
            if b[2] == 0:
                assert o == [0, 0, 0, 0]          # empty rectangles stay empty
                seen_empty += 1
                continue
            fx, fy, fw, fh = o
            assert 0 <= fx and fx + fw <= W and 0 <= fy and fy + fh <= H                             # inside the frame
            assert fx <= b[0] and b[0] + b[2] <= fx + fw and fy <= b[1] and b[1] + b[3] <= fy + fh      # contains today's
            if q > 0 and not common:
                assert (fw % q == 0 or fw == W) and (fh % q == 0 or fh == H)
                assert fw - b[2] < q and fh - b[3] < q
                seen_capped += (fw % q != 0) or (fh % q != 0)
                seen_rounded += fw > b[2]
            seen_shifted += fx < b[0] or fy < b[1]
        if common and live:
            assert len({(o[2], o[3]) for _, o in live}) == 1
            bw, bh = max(o[2] for _, o in live), max(o[3] for _, o in live)
            if q > 0:
                assert (bw % q == 0 or bw == W) and (bh % q == 0 or bh == H)
            seen_common_grew += any(o[2] > b[2] for b, o in live)
    assert min(seen_capped, seen_shifted, seen_rounded, seen_empty, seen_common_grew) > 20


def test_fit_rects_quantum_common_by_hand():
    from manus_amd.lpips import fit_rects
    H, W = 40, 56
    rects = [(5, 3, 33, 17), (20, 10, 4, 6), (0, 0, 0, 7), (50, 30, 6, 10)]
    assert fit_rects(rects, H, W, "vgg").tolist() == [[5, 3, 33, 17], [14, 5, 16, 16], [0, 0, 0, 0], [40, 24, 16, 16]]
    # 33 x 17 -> 48 x 32, shifted up by nothing (3 + 32 <= 40) and left by nothing (5 + 48 <= 56); 16 x 16 stays
    assert fit_rects(rects, H, W, "vgg", quantum=16).tolist() == [[5, 3, 48, 32], [14, 5, 16, 16], [0, 0, 0, 0], [40, 24, 16, 16]]
    # 33 -> 64 is capped at the frame's 56; 17 -> 32 fits
    assert fit_rects(rects, H, W, "vgg", quantum=32).tolist() == [[0, 3, 56, 32], [14, 5, 32, 32], [0, 0, 0, 0], [24, 8, 32, 32]]
    assert fit_rects(rects, H, W, "vgg", common=True).tolist() == [[5, 3, 33, 17], [14, 5, 33, 17], [0, 0, 0, 0], [23, 23, 33, 17]]
    assert fit_rects(rects, H, W, "vgg", quantum=16, common=True).tolist() == [[5, 3, 48, 32], [8, 5, 48, 32], [0, 0, 0, 0], [8, 8, 48, 32]]
    assert fit_rects([(0, 0, 0, 0)], H, W, "vgg", quantum=8, common=True).tolist() == [[0, 0, 0, 0]]
    with pytest.raises(ValueError, match="negative"):
        fit_rects(rects, H, W, "vgg", quantum=-1)


def test_frame_store_lpips_rects_quantum_common():
    from manus_amd.frames import FrameStore
    # source frame 128 x 96, k = 2: the output frame is 64 x 48 (the bboxes of test_lpips_roi_cpu.py)
    bboxes = [(2, 6, 61, 85), (101, 38, 115, 52), (0, 0, 128, 96), (9, 9, 9, 9), (11, 15, 12, 16), (100, 70, 128, 96)]
    st = FrameStore(torch.zeros(16 * len(bboxes), dtype=torch.uint8), [16 * i for i in range(len(bboxes))], bboxes, 48, 64, k=2)
    assert st.lpips_fit is None
    tight = [[1, 3, 30, 40], [46, 15, 16, 16], [0, 0, 64, 48], [0, 0, 0, 0], [0, 0, 16, 16], [48, 32, 16, 16]]
    assert st.lpips_rects(range(6), margin=0).tolist() == tight
    assert st.lpips_rects(range(6), margin=0, quantum=0, common=False).tolist() == tight
    # 30 x 40 -> 32 x 48 (the frame's height), shifted to the top; the others are multiples already
    assert st.lpips_rects(range(6), margin=0, quantum=16).tolist() == [[1, 0, 32, 48], [46, 15, 16, 16], [0, 0, 64, 48], [0, 0, 0, 0],
                                                                      [0, 0, 16, 16], [48, 32, 16, 16]]
    # without the frame-sized item: one 32 x 48 window for every non-empty view
    assert st.lpips_rects([0, 1, 3, 5], margin=0, quantum=16, common=True).tolist() == [[1, 0, 32, 48], [32, 0, 32, 48], [0, 0, 0, 0],
                                                                                        [32, 0, 32, 48]]
    assert st.lpips_rects([1, 4, 5], margin=0, common=True).tolist() == [[46, 15, 16, 16], [0, 0, 16, 16], [48, 32, 16, 16]]


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
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
             grad=P, taps=None, ws=P, ws_bytes=BIG, operands=0, max_batch=4):
        keep, r = _rects(rects) if rects is not None else (None, None)
        return L.mgr_lpips_roi_batch_op(net, V, H, W, r, pred, target, mask, blob, nb.get(net, 1) if blob_bytes is None else blob_bytes, 0,
                                        gs, values, grad, 0, taps, ws, ws_bytes, None, operands, max_batch)

    three = lambda r: (good, good, r)
    no_taps = (ctypes.c_void_p * 3)(P, P, None)
    for kw, word in ((dict(max_batch=0), "max_batch"), (dict(max_batch=-2), "max_batch"),
                     (dict(net=2), "net"), (dict(operands=2), "operands"), (dict(V=0), "sizes"), (dict(H=0), "sizes"),
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
    # a workspace below the batched size: the sequential size is not enough for a chunk of three
    keep, r = _rects([good] * 3)
    need = L.mgr_lpips_roi_batch_workspace_bytes(0, 3, r, 1, 4)
    assert need > L.mgr_lpips_roi_workspace_bytes(0, 3, r, 1)
    assert call(ws_bytes=need - 1) == _lib.MGR_ENOMEM and "workspace" in _err()
    assert call(ws_bytes=L.mgr_lpips_roi_workspace_bytes(0, 3, r, 1)) == _lib.MGR_ENOMEM
    assert call(ws_bytes=L.mgr_lpips_roi_workspace_bytes(0, 3, r, 1) - 1, max_batch=1) == _lib.MGR_ENOMEM
    # the plain fp32 wrapper refuses alike
    assert L.mgr_lpips_roi_batch(0, 3, H, W, _rects(three((5, 3, 15, 16)))[1], P, P, None, P, nb[0], 0, scales, P, P, 0, None, P, BIG,
                                 None, 4) == _lib.MGR_EINVAL and "too small" in _err()
    assert L.mgr_lpips_roi_batch(0, 3, H, W, _rects([good] * 3)[1], P, P, None, P, nb[0], 0, scales, P, P, 0, None, P, BIG,
                                 None, 0) == _lib.MGR_EINVAL and "max_batch" in _err()

    # the batched taps entry
    outs = (ctypes.c_void_p * 3)(P, P, P)
    def taps_call(net=0, V=3, H=H, W=W, rects=(good, good, good), target=P, blob=P, blob_bytes=None, out=outs, max_batch=4, ws=P,
                  ws_bytes=BIG, operands=0):
        keep, r = _rects(rects) if rects is not None else (None, None)
        return L.mgr_lpips_roi_taps_batch_op(net, V, H, W, r, target, None, blob, nb.get(net, 1) if blob_bytes is None else blob_bytes, 0,
                                             out, max_batch, ws, ws_bytes, None, operands)

    for kw, word in ((dict(max_batch=0), "max_batch"), (dict(net=2), "net"), (dict(operands=3), "operands"), (dict(W=0), "sizes"),
                     (dict(V=0), "sizes"), (dict(rects=three((30, 20, 40, 16))), "not inside"),
                     (dict(rects=three((5, 3, -16, 16))), "negative"), (dict(rects=three((5, 3, 15, 16))), "too small"),
                     (dict(rects=None), "null"), (dict(target=None), "null"), (dict(blob=None), "null"), (dict(out=None), "null"),
                     (dict(out=no_taps), "no tap buffer"), (dict(ws=None), "null"), (dict(blob_bytes=nb[0] + 4), "blob_bytes")):
        assert taps_call(**kw) == _lib.MGR_EINVAL, kw
        assert word in _err(), (kw, _err())
    need = L.mgr_lpips_roi_batch_workspace_bytes(0, 3, r, 0, 4)
    assert need > L.mgr_lpips_workspace_bytes(0, 17, 33, 0)
    assert taps_call(ws_bytes=need - 1) == _lib.MGR_ENOMEM and "workspace" in _err()


def test_python_refusals_before_the_device():
    from manus_amd._lib import ManusHipError
    from manus_amd.lpips import LPIPS
    z = torch.zeros((2, 3, 40, 56))
    m = LPIPS("vgg")
    m.blob = torch.zeros(4, dtype=torch.uint8)           # (a stand-in: every refusal below comes before it is read)
    with pytest.raises(ManusHipError, match="batch belongs to the windowed call"):
        m.values_grad(z, z, batch=4)
    with pytest.raises(ManusHipError, match="batch must be"):
        m.values_grad(z, z, rects=[(0, 0, 56, 40)] * 2, batch=-1)
    with pytest.raises(ManusHipError, match="batch must be"):
        m.target_taps(z, [(0, 0, 56, 40)] * 2, batch=-1)
    # batch = 0 without rects is the plain call's keyword default: not refused for the batch
    with pytest.raises(ManusHipError, match="windowed call"):
        m.values_grad(z, z, grad_scales=[1.0, 1.0], batch=0)

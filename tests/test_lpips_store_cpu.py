"""No GPU: the bf16 storage mode of LPIPS -- the emulation (tests/lpips_store_ref.py) against the operand mode's, the ABI of the
*_st entries, their sizes, the refusals decided on the host, and the blocked packing of the Python layer."""
import ctypes
import os
import re

import pytest
import torch

import lpips_bf16_ref as B
import lpips_ref as R
import lpips_store_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> (base entry, number of trailing storage arguments)
ST_ENTRIES = {"mgr_lpips_workspace_bytes_st": ("mgr_lpips_workspace_bytes", 1), "mgr_lpips_layout_st": ("mgr_lpips_layout", 1),
              "mgr_lpips_taps_bytes_st": ("mgr_lpips_taps_bytes", 1),
              "mgr_lpips_roi_batch_workspace_bytes_st": ("mgr_lpips_roi_batch_workspace_bytes", 1), "mgr_lpips_st": ("mgr_lpips_op", 1),
              "mgr_lpips_roi_batch_st": ("mgr_lpips_roi_batch_op", 1), "mgr_lpips_roi_taps_batch_st": ("mgr_lpips_roi_taps_batch_op", 1),
              "mgr_lpips_conv_st": ("mgr_lpips_conv_op", 2)}
SIZES = (("vgg", 16, 16), ("vgg", 33, 17), ("vgg", 40, 24), ("vgg", 1920, 1080), ("alex", 67, 35))
NET = {"vgg": 0, "alex": 1}


def align(n):
    return (n + 255) // 256 * 256


def pad8(c):
    return (c + 7) // 8 * 8


# ---------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,seed", S.CASES)
def test_stored_activations_are_the_operand_modes_rounded_once(W, H, seed):
    """Rounding at the store instead of at the load gives the next convolution the same operand, and a maximum commutes with a
    monotone rounding: every stored activation is rb(the operand mode's), every ReLU decision the same.  The distances to the
    fp64 restatement are printed beside the operand mode's: they are the units of the GPU bars."""
    c = S.case(W, H, seed)
    o = c["operand"]
    for i, (a, b) in enumerate(zip(c["emul"]["act"], o["emul"]["act"])):
        assert torch.equal(a, S.rb(b)), i
        assert torch.equal(a > 0, b > 0), i
    ties = []
    ds, do = R.decisions_of("vgg", c["emul"]["act"]), R.decisions_of("vgg", o["emul"]["act"])
    for ps, po in zip(ds["pool"], do["pool"]):
        ties.append("%d/%d" % (int((ps != po).sum()), ps.numel()))
    print("%dx%d seed %d: storage / operand mode against fp64: value %.3g / %.3g; gradient max-rel-err %.3g / %.3g; 1 - cosine %.3g / %.3g; "
          "pool winners that differ %s" % (W, H, seed, c["value_err"], o["value_err"], c["grad_err"], o["grad_err"], 1 - c["grad_cos"],
                                           1 - o["grad_cos"], " ".join(ties)))
    assert 0 < c["value_err"] < 1 and 0 < c["grad_err"] < 1 and 0 < c["grad_cos"] < 1
    assert all(0 < e < 1 for e in c["act_err"])
    for k in range(5):
        assert float((c["emul"]["tap"][k] ** 2).sum(0).min()) > 0
    # frozen to its own decisions the emulation reproduces itself
    v, fz, _ = S.forward("vgg", B.weights(), c["pred"][0], c["target"][0], decisions=ds)
    assert float(v) == c["value_emul"] and all(torch.equal(a, b) for a, b in zip(fz["act"], c["emul"]["act"]))


# ---------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------
def _declared(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return [" ".join(a.split()) for a in m.group(1).strip().split(",")]


def _types(args):
    """the declared arguments without their names"""
    return [re.sub(r"\s*\b\w+$", "", a) for a in args]


def test_st_entries_are_declared_bound_and_exported():
    from manus_amd import _lib
    header = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, (base, extra) in ST_ENTRIES.items():
        decl, dbase = _declared(header, name), _declared(header, base)
        assert len(decl) == len(dbase) + extra, name
        assert _types(decl[:len(dbase)]) == _types(dbase), name                  # exactly the base entry's arguments ...
        assert all(re.fullmatch(r"int \w*storage", a) for a in decl[len(dbase):]), (name, decl[len(dbase):])       # ... plus the trailing ones
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.SIGNATURES[base][0] and args[:-extra] == _lib.SIGNATURES[base][1], name
        assert all(a is ctypes.c_int for a in args[-extra:]), name
        assert hasattr(so, name) and hasattr(so, base), name
    assert re.search(r"MGR_LPIPS_STORE_F32\s*=\s*0\b", header) and re.search(r"MGR_LPIPS_STORE_BF16\s*=\s*1\b", header)
    assert (_lib.MGR_LPIPS_STORE_F32, _lib.MGR_LPIPS_STORE_BF16) == (0, 1)


def _layout(L, net, H, W, need_grad, storage=None):
    n_conv = 13 if net == 0 else 5
    buf = (ctypes.c_size_t * (n_conv + 9))()
    rc = L.mgr_lpips_layout(net, H, W, need_grad, buf, len(buf)) if storage is None else L.mgr_lpips_layout_st(net, H, W, need_grad, buf,
                                                                                                             len(buf), storage)
    assert rc == n_conv + 9
    return list(buf)


@pytest.mark.parametrize("net,W,H", SIZES)
def test_sizes(net, W, H):
    from manus_amd import _lib
    L = _lib.lib()
    n = NET[net]
    shapes, taps = S.conv_shapes(net, H, W)
    n_conv = len(shapes)
    grads = (0, 1) if net == "vgg" else (0,)
    rect = (ctypes.c_int * 8)(0, 0, W, H, 0, 0, W, H)
    for need_grad in grads:
        # fp32 storage: every _st size is its base
        assert L.mgr_lpips_workspace_bytes_st(n, H, W, need_grad, 0) == L.mgr_lpips_workspace_bytes(n, H, W, need_grad) > 0
        assert _layout(L, n, H, W, need_grad, 0) == _layout(L, n, H, W, need_grad)
        for mb in (1, 2):
            assert (L.mgr_lpips_roi_batch_workspace_bytes_st(n, 2, rect, need_grad, mb, 0)
                    == L.mgr_lpips_roi_batch_workspace_bytes(n, 2, rect, need_grad, mb) > 0)
        # bf16 storage
        f32, b16 = _layout(L, n, H, W, need_grad), _layout(L, n, H, W, need_grad, 1)
        assert b16[-1] == L.mgr_lpips_workspace_bytes_st(n, H, W, need_grad, 1)
        regions = shapes + [shapes[taps[k]] for k in range(5)]
        for j, (C, h, w) in enumerate(regions):
            assert b16[j + 1] - b16[j] == align(2 * pad8(C) * h * w), (j, C, h, w)
            assert b16[j] % 256 == 0
        part32, part16 = f32[-1] - f32[-2], b16[-1] - b16[-2]
        assert part16 == part32 > 0
        n_regions = n_conv + 5 + 2 + 1
        assert b16[-1] <= f32[-1] // 2 + part32 + 256 * n_regions, (b16[-1], f32[-1])
        # a chunk of two views: every act and tap region twice as long
        one = L.mgr_lpips_roi_batch_workspace_bytes_st(n, 2, rect, need_grad, 1, 1)
        two = L.mgr_lpips_roi_batch_workspace_bytes_st(n, 2, rect, need_grad, 2, 1)
        assert one == b16[-1] and b16[-1] < two <= 2 * b16[-1]
    assert L.mgr_lpips_taps_bytes_st(n, H, W, 0) == L.mgr_lpips_taps_bytes(n, H, W) > 0
    assert L.mgr_lpips_taps_bytes_st(n, H, W, 1) == sum(align(2 * pad8(C) * h * w) for C, h, w in (shapes[taps[k]] for k in range(5)))
    assert L.mgr_lpips_taps_bytes_st(n, H, W, 1) <= L.mgr_lpips_taps_bytes(n, H, W) // 2 + 256 * 5


def _err():
    from manus_amd import _lib
    return _lib.lib().mgr_last_error().decode()


def test_refusals_are_decided_on_the_host():
    """Every refusal returns before any launch: with made-up non-null pointers and no device."""
    from manus_amd import _lib
    L = _lib.lib()
    P = 0x1000          # never dereferenced
    F32, BF16, SF, SB = _lib.MGR_LPIPS_F32, _lib.MGR_LPIPS_BF16, _lib.MGR_LPIPS_STORE_F32, _lib.MGR_LPIPS_STORE_BF16
    H, W = 24, 40
    nb = {(n, o): L.mgr_lpips_net_bytes_op(n, o) for n in (0, 1) for o in (F32, BF16)}
    rect = (ctypes.c_int * 4)(0, 0, W, H)
    # the size queries
    for bad in (2, -1, 16):
        assert L.mgr_lpips_workspace_bytes_st(0, H, W, 1, bad) == 0 and L.mgr_lpips_taps_bytes_st(0, H, W, bad) == 0
        assert L.mgr_lpips_roi_batch_workspace_bytes_st(0, 1, rect, 1, 1, bad) == 0
        buf = (ctypes.c_size_t * 22)()
        assert L.mgr_lpips_layout_st(0, H, W, 1, buf, 22, bad) == _lib.MGR_EINVAL and "storage" in _err()
    for st in (SF, SB):
        assert L.mgr_lpips_workspace_bytes_st(2, H, W, 1, st) == 0 and L.mgr_lpips_workspace_bytes_st(0, 15, 15, 1, st) == 0
        assert L.mgr_lpips_taps_bytes_st(0, 15, 40, st) == 0 and L.mgr_lpips_roi_batch_workspace_bytes_st(0, 1, rect, 1, 0, st) == 0
        buf = (ctypes.c_size_t * 22)()
        assert L.mgr_lpips_layout_st(0, H, W, 1, buf, 21, st) == _lib.MGR_EINVAL and "offsets" in _err()
        assert L.mgr_lpips_layout_st(3, H, W, 1, buf, 22, st) == _lib.MGR_EINVAL and "net" in _err()

    def ws(net, h, w, grad, st):
        return L.mgr_lpips_workspace_bytes_st(net, h, w, grad, st if st in (SF, SB) else SF)

    def full(op, st, net=0, V=1, H=H, W=W, pred=P, target=P, blob=P, blob_bytes=None, values=P, grad=P, work=P, ws_bytes=None):
        return L.mgr_lpips_st(net, V, H, W, pred, target, None, blob, nb.get((net, op), 1) if blob_bytes is None else blob_bytes, 0, 1.0,
                              values, grad, 0, work, (ws(net, H, W, int(grad is not None), st) or 1) if ws_bytes is None else ws_bytes,
                              None, op, st)

    scales, taps1 = (ctypes.c_float * 1)(1.0), (ctypes.c_void_p * 1)(P)

    def roi(op, st, net=0, rect=rect, pred=P, target=P, grad=P, mb=1, work=P, ws_bytes=None, blob_bytes=None):
        need = L.mgr_lpips_roi_batch_workspace_bytes_st(net, 1, rect, int(grad is not None), max(mb, 1), st if st in (SF, SB) else SF) or 1
        return L.mgr_lpips_roi_batch_st(net, 1, H, W, rect, pred, target, None, P, nb.get((net, op), 1) if blob_bytes is None else blob_bytes,
                                        0, scales, P, grad, 0, None, work, need if ws_bytes is None else ws_bytes, None, op, mb, st)

    def tapsb(op, st, net=0, rect=rect, target=P, out=taps1, mb=1, work=P, ws_bytes=None, blob_bytes=None):
        need = L.mgr_lpips_roi_batch_workspace_bytes_st(net, 1, rect, 0, max(mb, 1), st if st in (SF, SB) else SF) or 1
        return L.mgr_lpips_roi_taps_batch_st(net, 1, H, W, rect, target, None, P, nb.get((net, op), 1) if blob_bytes is None else blob_bytes,
                                             0, out, mb, work, need if ws_bytes is None else ws_bytes, None, op, st)

    def conv(op, xs, ys, cin=4, stride=1, bias=None, transposed=0, scratch=P, nbytes=1 << 20):
        return L.mgr_lpips_conv_st(cin, 4, 8, 8, 3, 3, stride, 1, P, None, P, bias, 1 - transposed, transposed, P, scratch, nbytes, None, op,
                                   xs, ys)

    # a storage other than 0 / 1, and bf16 storage with fp32 operands
    for call in (full, roi, tapsb):
        for bad in (2, -1):
            assert call(BF16, bad) == _lib.MGR_EINVAL and "storage" in _err(), call
        assert call(F32, SB) == _lib.MGR_EINVAL and "bf16 operands" in _err(), call
        assert call(2, SF) == _lib.MGR_EINVAL and "operands" in _err(), call
    for xs, ys in ((2, 0), (0, 2), (-1, 1)):
        assert conv(BF16, xs, ys) == _lib.MGR_EINVAL and "storage" in _err()
    for xs, ys in ((1, 0), (0, 1), (1, 1)):
        assert conv(F32, xs, ys) == _lib.MGR_EINVAL and "bf16 operands" in _err()
    # everything the base entries refuse, in both storages of bf16 operands and in fp32 / fp32
    small = (ctypes.c_int * 4)(0, 0, 15, 15)
    outside = (ctypes.c_int * 4)(30, 0, 16, 16)
    negative = (ctypes.c_int * 4)(0, 0, -16, 16)
    hole = (ctypes.c_void_p * 1)(None)
    for op, st in ((F32, SF), (BF16, SF), (BF16, SB)):
        for kw, word in ((dict(net=2), "net"), (dict(V=0), "sizes"), (dict(H=15), "too small"), (dict(pred=None), "null"),
                         (dict(target=None), "null"), (dict(blob=None), "null"), (dict(values=None), "null"), (dict(work=None), "null"),
                         (dict(blob_bytes=nb[0, op] - 4), "blob_bytes"), (dict(net=1, H=35, W=67), "forward only")):
            assert full(op, st, **kw) == _lib.MGR_EINVAL, (op, st, kw)
            assert word in _err(), (op, st, kw, _err())
        assert full(op, st, ws_bytes=ws(0, H, W, 1, st) - 1) == _lib.MGR_ENOMEM and "workspace" in _err()
        for kw, word in ((dict(net=2), "net"), (dict(mb=0), "max_batch"), (dict(rect=small), "too small"), (dict(rect=outside), "inside"),
                         (dict(rect=negative), "negative"), (dict(pred=None), "null"), (dict(target=None), "null"), (dict(work=None), "null"),
                         (dict(blob_bytes=nb[0, op] - 4), "blob_bytes"), (dict(net=1), "forward only")):
            assert roi(op, st, **kw) == _lib.MGR_EINVAL, (op, st, kw)
            assert word in _err(), (op, st, kw, _err())
        need = L.mgr_lpips_roi_batch_workspace_bytes_st(0, 1, rect, 1, 1, st)
        assert roi(op, st, ws_bytes=need - 1) == _lib.MGR_ENOMEM and "workspace" in _err()
        for kw, word in ((dict(net=2), "net"), (dict(mb=0), "max_batch"), (dict(rect=small), "too small"), (dict(rect=outside), "inside"),
                         (dict(target=None), "null"), (dict(out=hole), "null"), (dict(work=None), "null"),
                         (dict(blob_bytes=nb[0, op] - 4), "blob_bytes")):
            assert tapsb(op, st, **kw) == _lib.MGR_EINVAL, (op, st, kw)
            assert word in _err(), (op, st, kw, _err())
        need = L.mgr_lpips_roi_batch_workspace_bytes_st(0, 1, rect, 0, 1, st)
        assert tapsb(op, st, ws_bytes=need - 1) == _lib.MGR_ENOMEM and "workspace" in _err()
        assert conv(op, st, st, cin=0) == _lib.MGR_EINVAL
        assert conv(op, st, st, stride=2, transposed=1) == _lib.MGR_EINVAL
        assert conv(op, st, st, bias=P, transposed=1) == _lib.MGR_EINVAL
        assert conv(op, st, st, scratch=None) == _lib.MGR_EINVAL
        assert conv(op, st, st, nbytes=16) == _lib.MGR_ENOMEM
    # the workspace of fp32 storage is too small for nothing, that of bf16 storage is too small for fp32 storage
    assert full(BF16, SF, ws_bytes=ws(0, H, W, 1, SB)) == _lib.MGR_ENOMEM


# ---------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,h,w", [(3, 5, 7), (8, 1, 1), (13, 4, 9), (64, 3, 2)])
def test_pack_blocked_round_trips_and_pads_with_zero(C, h, w):
    from manus_amd.lpips import pack_blocked, unpack_blocked
    g = torch.Generator().manual_seed(C)
    t = torch.randn((C, h, w), generator=g)
    buf = pack_blocked(t)
    nb = (C + 7) // 8
    assert buf.dtype == torch.uint8 and buf.numel() == 2 * nb * 8 * h * w
    assert torch.equal(unpack_blocked(buf, C, h, w).double(), S.rb(t))
    full = unpack_blocked(buf, C, h, w, pads=True)
    assert full.shape == (nb * 8, h, w) and bool((full[C:] == 0).all()) and bool((buf.view(torch.int16).reshape(nb, h, w, 8).permute(0, 3, 1, 2)
                                                                                  .reshape(nb * 8, h, w)[C:] == 0).all())
    # the layout: channel c of pixel (y, x) is lane c % 8 of block c / 8
    raw = buf.view(torch.bfloat16).reshape(nb, h, w, 8)
    c, y, x = C - 1, h - 1, w // 2
    assert float(raw[c // 8, y, x, c % 8]) == float(S.rb(t)[c, y, x])
    # packing what was unpacked gives the same bytes
    assert torch.equal(pack_blocked(unpack_blocked(buf, C, h, w)), buf)


def test_python_surface():
    from manus_amd._lib import ManusHipError
    from manus_amd.lpips import LPIPS, TargetTaps, conv2d, layout
    m = LPIPS("vgg", operands="bf16", storage="bf16")
    assert (m.operands, m.storage) == ("bf16", "bf16")
    assert LPIPS("vgg").storage == "fp32" and LPIPS("alex", operands="bf16").storage == "fp32"
    with pytest.raises(ManusHipError, match="operands='bf16'"):
        LPIPS("vgg", operands="fp32", storage="bf16")
    with pytest.raises(ManusHipError, match="operands='bf16'"):
        LPIPS("vgg", storage="bf16")
    with pytest.raises(ManusHipError, match="operands='bf16'"):
        LPIPS.from_state_dicts({}, {}, net="vgg", device="cpu", operands="fp32", storage="bf16")
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ManusHipError, match="storage"):
            LPIPS("vgg", operands="bf16", storage=bad)
        with pytest.raises(ManusHipError, match="storage"):
            LPIPS.from_state_dicts({}, {}, net="vgg", device="cpu", operands="bf16", storage=bad)
        with pytest.raises(ManusHipError, match="storage"):
            conv2d(torch.zeros((3, 4, 4)), torch.zeros((2, 3, 3, 3)), pad=1, operands="bf16", y_storage=bad)
        with pytest.raises(ManusHipError, match="storage"):
            layout("vgg", 24, 40, True, storage=bad)
    with pytest.raises(ManusHipError, match="operands='bf16'"):
        conv2d(torch.zeros((3, 4, 4)), torch.zeros((2, 3, 3, 3)), pad=1, x_storage="bf16")
    # the layout of the two storages
    a, b = layout("vgg", 24, 40, True), layout("vgg", 24, 40, True, storage="bf16")
    assert a == layout("vgg", 24, 40, True, storage="fp32") and b["total"] < a["total"] and b["act"][1] == 64 * 24 * 40 * 2
    # taps remember their storage
    import numpy as np
    r = np.array([[0, 0, 16, 16]], np.int32)
    t = TargetTaps([None], r, (24, 40), "vgg", "bf16", False, False, "bf16")
    assert t.matches(r, (24, 40), "vgg", "bf16", False, False, "bf16")
    assert not t.matches(r, (24, 40), "vgg", "bf16", False, False, "fp32") and not t.matches(r, (24, 40), "vgg", "bf16", False, False)
    assert TargetTaps([None], r, (24, 40), "vgg", "bf16", False, False).matches(r, (24, 40), "vgg", "bf16", False, False)

"""No GPU: the bf16 operand mode of LPIPS -- the rounding of the restatement (tests/lpips_bf16_ref.py), the ABI of the *_op
entries, the refusals decided on the host, and the conditions the committed cases of tests/test_gpu_lpips_bf16.py rest on."""
import ctypes
import os
import re

import pytest
import torch

import lpips_bf16_ref as B
import lpips_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_ENTRIES = {"mgr_lpips_net_bytes_op": "mgr_lpips_net_bytes", "mgr_lpips_net_pack_op": "mgr_lpips_net_pack", "mgr_lpips_op": "mgr_lpips",
              "mgr_lpips_conv_op": "mgr_lpips_conv", "mgr_lpips_conv_scratch_bytes_op": "mgr_lpips_conv_scratch_bytes"}


def test_rb_rounds_to_nearest_even():
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 3 * 2.0 ** -8), 3.0],
                     dtype=torch.float64)
    want = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -6), 3.0]
    assert B.rb(t).tolist() == want
    # a product of two rounded values is exact in fp32
    g = torch.Generator().manual_seed(0)
    a, b = B.rb(torch.randn(1000, generator=g)), B.rb(torch.randn(1000, generator=g))
    assert torch.equal((a * b).float().double(), a * b)


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return len(m.group(1).strip().split(","))


def test_op_entries_are_declared_bound_and_exported():
    from manus_amd import _lib
    header = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, base in OP_ENTRIES.items():
        n_decl = _declared_args(header, name)
        assert n_decl == _declared_args(header, base) + 1, name              # the trailing `operands`
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_decl and args[-1] is ctypes.c_int, (name, len(args), n_decl)
        assert args[:-1] == _lib.SIGNATURES[base][1] and res is _lib.SIGNATURES[base][0], name
        assert hasattr(so, name) and hasattr(so, base), name
    assert re.search(r"MGR_LPIPS_F32\s*=\s*0\b", header) and re.search(r"MGR_LPIPS_BF16\s*=\s*1\b", header)
    assert (_lib.MGR_LPIPS_F32, _lib.MGR_LPIPS_BF16) == (0, 1)


def _err():
    from manus_amd import _lib
    return _lib.lib().mgr_last_error().decode()


def test_sizes_of_the_two_modes():
    from manus_amd import _lib
    L = _lib.lib()
    for net in (0, 1):
        assert L.mgr_lpips_net_bytes_op(net, _lib.MGR_LPIPS_F32) == L.mgr_lpips_net_bytes(net) > 0
        b16 = L.mgr_lpips_net_bytes_op(net, _lib.MGR_LPIPS_BF16)
        assert 0 < b16 < L.mgr_lpips_net_bytes(net)
        for bad in (2, -1, 16):
            assert L.mgr_lpips_net_bytes_op(net, bad) == 0
    assert L.mgr_lpips_net_bytes_op(2, 1) == 0
    for ci, co, k in ((3, 64, 3), (5, 33, 3), (512, 512, 3), (3, 64, 11)):
        assert L.mgr_lpips_conv_scratch_bytes_op(ci, co, k, k, 0) == L.mgr_lpips_conv_scratch_bytes(ci, co, k, k) > 0
        n16 = L.mgr_lpips_conv_scratch_bytes_op(ci, co, k, k, 1)
        # both weight sets in bf16, channels padded to 8 along k and to 64 across: at least 2 bytes per weight, twice
        assert n16 >= 2 * 2 * ci * co * k * k and n16 % 256 == 0
        assert L.mgr_lpips_conv_scratch_bytes_op(ci, co, k, k, 2) == 0 and L.mgr_lpips_conv_scratch_bytes_op(0, co, k, k, 1) == 0


def test_refusals_are_decided_on_the_host():
    """Every refusal returns before any launch: with made-up non-null pointers and no device."""
    from manus_amd import _lib
    L = _lib.lib()
    P = 0x1000          # never dereferenced
    F32, BF16 = _lib.MGR_LPIPS_F32, _lib.MGR_LPIPS_BF16
    H, W = 24, 40
    nb = {(n, o): L.mgr_lpips_net_bytes_op(n, o) for n in (0, 1) for o in (F32, BF16)}
    wsb = {0: L.mgr_lpips_workspace_bytes(0, H, W, 1), 1: L.mgr_lpips_workspace_bytes(1, 35, 67, 0)}

    def call(op, net=0, V=1, H=H, W=W, pred=P, target=P, blob=P, blob_bytes=None, values=P, grad=P, ws=P, ws_bytes=None):
        return L.mgr_lpips_op(net, V, H, W, pred, target, None, blob, nb.get((net, op), 1) if blob_bytes is None else blob_bytes, 0, 1.0,
                              values, grad, 0, ws, wsb.get(net, 1) if ws_bytes is None else ws_bytes, None, op)

    for bad in (2, -1):
        assert call(bad, blob_bytes=nb[0, F32]) == _lib.MGR_EINVAL and "operands" in _err()
    for op in (F32, BF16):
        other = BF16 if op == F32 else F32
        # a blob of the other mode's size
        assert call(op, blob_bytes=nb[0, other]) == _lib.MGR_EINVAL and "blob_bytes" in _err()
        assert call(op, net=1, H=35, W=67, grad=None, blob_bytes=nb[1, other]) == _lib.MGR_EINVAL and "blob_bytes" in _err()
        # what the fp32 entries refuse
        for kw, word in ((dict(net=2), "net"), (dict(net=-1), "net"), (dict(V=0), "sizes"), (dict(H=15), "too small"), (dict(W=15), "too small"),
                         (dict(net=1, H=24, W=40, grad=None), "too small"), (dict(pred=None), "null"), (dict(target=None), "null"),
                         (dict(blob=None), "null"), (dict(values=None), "null"), (dict(ws=None), "null"),
                         (dict(blob_bytes=nb[0, op] - 4), "blob_bytes"), (dict(net=1, H=35, W=67), "forward only")):
            assert call(op, **kw) == _lib.MGR_EINVAL, (op, kw)
            assert word in _err(), (op, kw, _err())
        assert call(op, ws_bytes=wsb[0] - 1) == _lib.MGR_ENOMEM and "workspace" in _err()
    # pack
    arr13, arr5 = (ctypes.c_void_p * 13)(*[P] * 13), (ctypes.c_void_p * 5)(*[P] * 5)
    assert L.mgr_lpips_net_pack_op(0, arr13, arr13, arr5, P, nb[0, F32], None, 2) == _lib.MGR_EINVAL and "operands" in _err()
    hole = (ctypes.c_void_p * 13)(*([P] * 12 + [None]))
    for op in (F32, BF16):
        other = BF16 if op == F32 else F32
        assert L.mgr_lpips_net_pack_op(2, arr13, arr13, arr5, P, nb[0, op], None, op) == _lib.MGR_EINVAL and "net" in _err()
        assert L.mgr_lpips_net_pack_op(0, arr13, arr13, arr5, P, nb[0, other], None, op) == _lib.MGR_EINVAL and "blob_bytes" in _err()
        assert L.mgr_lpips_net_pack_op(0, arr13, arr13, arr5, None, nb[0, op], None, op) == _lib.MGR_EINVAL and "null" in _err()
        assert L.mgr_lpips_net_pack_op(0, hole, arr13, arr5, P, nb[0, op], None, op) == _lib.MGR_EINVAL and "null" in _err()
    # the single convolution
    assert L.mgr_lpips_conv_op(4, 4, 8, 8, 3, 3, 1, 1, P, None, P, None, 1, 0, P, P, 1 << 20, None, 2) == _lib.MGR_EINVAL and "operands" in _err()
    for op in (F32, BF16):
        assert L.mgr_lpips_conv_op(0, 4, 8, 8, 3, 3, 1, 1, P, None, P, None, 1, 0, P, P, 1 << 20, None, op) == _lib.MGR_EINVAL
        assert L.mgr_lpips_conv_op(4, 4, 8, 8, 3, 3, 2, 1, P, None, P, None, 0, 1, P, P, 1 << 20, None, op) == _lib.MGR_EINVAL
        assert L.mgr_lpips_conv_op(4, 4, 8, 8, 3, 3, 1, 1, P, None, P, P, 0, 1, P, P, 1 << 20, None, op) == _lib.MGR_EINVAL
        assert L.mgr_lpips_conv_op(4, 4, 8, 8, 3, 3, 1, 1, P, None, P, None, 1, 0, P, None, 1 << 20, None, op) == _lib.MGR_EINVAL
        assert L.mgr_lpips_conv_op(4, 4, 8, 8, 3, 3, 1, 1, P, None, P, None, 1, 0, P, P, 16, None, op) == _lib.MGR_ENOMEM


def test_python_surface():
    from manus_amd._lib import ManusHipError
    from manus_amd.lpips import LPIPS, conv2d
    assert LPIPS("vgg").operands == "fp32" and LPIPS("alex", operands="bf16").operands == "bf16"
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ManusHipError, match="operands"):
            LPIPS("vgg", operands=bad)
        with pytest.raises(ManusHipError, match="operands"):
            LPIPS.from_state_dicts({}, {}, net="vgg", device="cpu", operands=bad)
        with pytest.raises(ManusHipError, match="operands"):
            conv2d(torch.zeros((3, 4, 4)), torch.zeros((2, 3, 3, 3)), pad=1, operands=bad)
    # the state-dict errors come before any device work in both modes
    sd, lin = R.state_dicts("vgg", B.weights())
    bad = dict(sd)
    del bad["features.2.weight"]
    with pytest.raises(ManusHipError, match=re.escape("features.2.weight")):
        LPIPS.from_state_dicts(bad, lin, net="vgg", device="cpu", operands="bf16")


@pytest.mark.parametrize("W,H,seed", B.CASES)
def test_conditions_of_the_gpu_cases_hold_for_the_emulation(W, H, seed):
    """The GPU test judges the device by multiples of the emulation's own distance to the fp64 restatement, and judges the
    gradient for frozen decisions: no tap pixel may have all-zero features (the zero-gradient rule would hide an error there),
    every distance must be a positive finite number, and the emulation with its decisions frozen must reproduce itself."""
    c = B.case(W, H, seed)
    for f in (c["emul"], c["f64"]):
        for k in range(5):
            assert float((f["tap"][k] ** 2).sum(0).min()) > 0
    print("%dx%d seed %d: emulation against the fp64 restatement: value %.3g relative; activations %s; gradient max-rel-err %.3g, cosine %.6f; "
          "smallest sum_c f^2 %.3g" % (W, H, seed, c["value_err"], " ".join("%.2g" % e for e in c["act_err"]), c["grad_err"], c["grad_cos"],
                                       min(float((c["emul"]["tap"][k] ** 2).sum(0).min()) for k in range(5))))
    assert 0 < c["value_err"] < 1 and 0 < c["grad_err"] < 1 and 0 < c["grad_cos"] < 1
    assert all(0 < e < 1 for e in c["act_err"])
    wts = B.weights()
    dec = R.decisions_of("vgg", c["emul"]["act"])
    v, fz, _ = B.forward("vgg", wts, c["pred"][0], c["target"][0], decisions=dec)
    assert float(v) == c["value_emul"] and all(torch.equal(a, b) for a, b in zip(fz["act"], c["emul"]["act"]))

"""The exposure entries on the device (csrc/exposure.hip) against the restatement of tests/exposure_ref.py: apply, backward with
its deterministic table gradient, the row Adam against torch.optim.SparseAdam, the refusals, and the recovery of a planted
table on image tensors alone.  Bound: the project's `check_rows`."""
import functools

import pytest
import torch

import exposure_ref as R
from exposure_ref import F32, F64, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from manus_amd import _lib
    return _lib


def _block():
    return int(_lib().lib().mgr_exposure_block())


def _sizes():
    # resolved at collection without the library: the block-relative sizes are filled in by the test
    return list(R.SIZES) + [("block", -1), ("block", 0), ("block", 1), ("3block", 5)]


def _hw(size):
    if size[0] == "block":
        return 1, _block() + size[1]
    if size[0] == "3block":
        return 1, 3 * _block() + size[1]
    return size


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def apply(img, E, rows):
    from manus_amd import ops
    return ops.exposure_forward(_dev(img), _dev(E), _i32(rows))


def backward(img, E, rows, g, inplace=False):
    from manus_amd import ops
    gd = _dev(g).clone()
    g_out, dE = ops.exposure_backward(_dev(img), _dev(E), _i32(rows), gd, inplace=inplace)
    if inplace:
        assert g_out.data_ptr() == gd.data_ptr()
    return g_out, dE


def _check_all(tag, img, E, rows, g):
    out = apply(img, E, rows)
    g_out, dE = backward(img, E, rows, g)
    check_rows(tag + " apply", R.image_rows(out), R.image_rows(R.apply_ref(img, E, rows)), R.image_rows(R.apply_ref(img, E, rows, F32)))
    g64, dE64 = R.backward_ref(img, E, rows, g)
    g32, dE32 = R.backward_ref(img, E, rows, g, F32)
    check_rows(tag + " g_out", R.image_rows(g_out), R.image_rows(g64), R.image_rows(g32))
    check_rows(tag + " dE", R.view_rows(dE), R.view_rows(dE64), R.view_rows(dE32))
    # in place: the bits of the out-of-place call; two runs: equal bits
    g_in_place, dE_in_place = backward(img, E, rows, g, inplace=True)
    assert torch.equal(g_in_place, g_out) and torch.equal(dE_in_place, dE)
    again = backward(img, E, rows, g)
    assert torch.equal(again[0], g_out) and torch.equal(again[1], dE) and torch.equal(apply(img, E, rows), out)
    return out, g_out, dE


@pytest.mark.parametrize("V", R.VIEWS)
@pytest.mark.parametrize("size", _sizes(), ids=lambda s: "%sx%s" % s)
def test_apply_and_backward_against_the_restatement(size, V):
    H, W = _hw(size)
    E = R.table(V, seed=V)
    img, g = R.images(V, H, W, seed=H * W % 1000 + V)
    rows = list(reversed(range(V)))                    # C = V, every row used once, not in position order
    _check_all("%dx%d V=%d" % (H, W, V), img, E, rows, g)
    # the identity table: out' = img and g = g' bit for bit (finite inputs)
    ident = R.identity_table(V)
    assert torch.equal(apply(img, ident, rows), _dev(img))
    g_id, _ = backward(img, ident, rows, g)
    assert torch.equal(g_id, _dev(g))


@pytest.mark.parametrize("size", [(5, 7), (16, 16), ("block", 1)], ids=lambda s: "%sx%s" % s)
def test_shared_rows_and_views_without_a_row(size):
    H, W = _hw(size)
    V, rows = 6, [1, 0, 1, -1, 0, 2]                   # C = 2: rows shared between views, a -1 view, a row beyond the table
    E = R.table(2, seed=3)
    img, g = R.images(V, H, W, seed=11)
    out, g_out, dE = _check_all("%dx%d shared" % (H, W), img, E, rows, g)
    for k in (3, 5):
        assert torch.equal(out[k], _dev(img)[k]) and torch.equal(g_out[k], _dev(g)[k])
        assert bool((dE[k] == 0).all())
    # views that share a row see the same coefficients: each view alone gives the bits it has in the batch
    for k in (0, 2):
        alone = backward(img[k:k + 1], E, [rows[k]], g[k:k + 1])
        assert torch.equal(alone[0][0], g_out[k]) and torch.equal(alone[1][0], dE[k])


def test_autograd_form_gives_the_dense_table_gradient():
    """`ops.exposure_apply` under autograd: the image gradient is the raw call's, the table gradient the per-view rows summed per
    camera in ascending position; both against fp64 autograd through the restatement."""
    from manus_amd import ops
    V, H, W, rows = 5, 7, 6, [1, 0, 1, -1, 1]
    E64 = R.table(3, seed=2)                           # row 2 is used by no view: its gradient is exactly zero
    img64, g64 = R.images(V, H, W, seed=19)
    img, E = _dev(img64).requires_grad_(True), _dev(E64).requires_grad_(True)
    out = ops.exposure_apply(img, E, rows)
    assert torch.equal(out.detach(), apply(img64, E64, rows))
    out.backward(_dev(g64))
    g_raw, dE_raw = backward(img64, E64, rows, g64)
    assert torch.equal(img.grad, g_raw)
    dense = torch.zeros_like(dE_raw[:3])
    for k, r in enumerate(rows):
        if r >= 0:
            dense[r] += dE_raw[k]
    assert torch.equal(E.grad, dense) and not bool(E.grad[2].any())
    refs = []
    for dtype in (F64, F32):
        x, t = (a.detach().clone().to(dtype).requires_grad_(True) for a in (img64, E64))      # (leaves of their own)
        R.apply_views(x, *R.per_view_table(t, rows)).backward(g64.to(dtype))
        refs.append((x.grad, t.grad))
    check_rows("autograd d img", R.image_rows(img.grad), R.image_rows(refs[0][0]), R.image_rows(refs[1][0]))
    check_rows("autograd d table", R.view_rows(E.grad[:2]), R.view_rows(refs[0][1][:2]), R.view_rows(refs[1][1][:2]))
    # a list, an int32 device vector and nothing else for the rows; the table on the image's device
    with pytest.raises(Exception, match="cam_of_view"):
        ops.exposure_apply(img.detach(), E.detach(), [0, 1])
    with pytest.raises(Exception, match="GPU tensors"):
        ops.exposure_apply(img.detach(), E.detach().cpu(), rows)
    with pytest.raises(Exception, match="table"):
        ops.exposure_apply(img.detach(), E.detach()[:, :, :3].contiguous(), rows)


def test_buffers_off_the_16_byte_grid_take_the_single_float_walk():
    """H W a multiple of 4 but the buffers 4 bytes off a 16-byte boundary: the entries may not use 16-byte accesses.  The
    per-pixel results are those of the aligned call bit for bit; the table gradient adds the same terms in another order."""
    from manus_amd import ops
    V, H, W = 3, 16, 16
    rows = _i32([2, 0, 1])
    E = _dev(R.table(3, seed=8))
    img64, g64 = R.images(V, H, W, seed=17)
    img, g = _dev(img64), _dev(g64)
    n = img.numel()

    def shifted(x):
        buf = torch.empty(n + 4, device=DEV)
        view = buf[1:1 + n].view(V, 3, H, W)
        view.copy_(x)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    out = ops.exposure_forward(img, E, rows)
    g_out, dE = ops.exposure_backward(img, E, rows, g.clone())
    assert torch.equal(ops.exposure_forward(shifted(img), E, rows), out)
    gs = shifted(g)
    g_off, dE_off = ops.exposure_backward(shifted(img), E, rows, gs, inplace=True)
    assert g_off.data_ptr() == gs.data_ptr() and torch.equal(g_off, g_out)
    _, dE64 = R.backward_ref(img64, R.table(3, seed=8), [2, 0, 1], g64)
    _, dE32 = R.backward_ref(img64, R.table(3, seed=8), [2, 0, 1], g64, F32)
    check_rows("dE off the grid", R.view_rows(dE_off), R.view_rows(dE64), R.view_rows(dE32))
    check_rows("dE on the grid", R.view_rows(dE), R.view_rows(dE64), R.view_rows(dE32))


@pytest.mark.parametrize("size", [(7, 6), (56, 40), ("block", 1)], ids=lambda s: "%sx%s" % s)
def test_a_non_finite_term_stays_in_its_view(size):
    H, W = _hw(size)
    V, rows = 3, [2, 0, 1]
    E = R.table(3, seed=5)
    img, g = R.images(V, H, W, seed=13)
    g_clean, dE_clean = backward(img, E, rows, g)
    for bad in (float("nan"), float("inf")):
        g_bad = g.clone()
        g_bad[1, 2, H - 1, W - 1] = bad                # the last pixel of the last plane: the tail of the last workgroup
        g_out, dE = backward(img, E, rows, g_bad)
        assert bool(torch.isnan(dE[1]).all())
        assert torch.equal(dE[0], dE_clean[0]) and torch.equal(dE[2], dE_clean[2])
        assert torch.equal(g_out[0], g_clean[0]) and torch.equal(g_out[2], g_clean[2])


def test_refusals_leave_the_outputs_untouched():
    L, lib = _lib(), _lib().lib()
    ptr, stream = L.ptr, L.stream
    V, H, W, C = 2, 5, 7, 2
    img, g = (_dev(x) for x in R.images(V, H, W))
    E, cov = _dev(R.table(C)), _i32([0, 1])
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out, g_out, dE = nan(V, 3, H, W), nan(V, 3, H, W), nan(V, 3, 4)
    need = int(lib.mgr_exposure_workspace_bytes(V, H, W))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in (out, g_out, dE))

    assert lib.mgr_exposure_backward(V, H, W, C, ptr(cov), ptr(E), ptr(img), ptr(g), ptr(g_out), ptr(dE), ptr(ws), need - 1, stream()) == L.MGR_ENOMEM
    assert b"workspace" in lib.mgr_last_error() and untouched()
    for bad in ((0, H, W, C), (V, 0, W, C), (V, H, 0, C), (V, H, W, 0), (-1, H, W, C)):
        assert lib.mgr_exposure_apply(*bad, ptr(cov), ptr(E), ptr(img), ptr(out), stream()) == L.MGR_EINVAL
        assert lib.mgr_exposure_backward(*bad, ptr(cov), ptr(E), ptr(img), ptr(g), ptr(g_out), ptr(dE), ptr(ws), need, stream()) == L.MGR_EINVAL
    assert b"at least 1" in lib.mgr_last_error() and untouched()
    for k in range(4):
        a = [ptr(cov), ptr(E), ptr(img), ptr(out)]
        a[k] = None
        assert lib.mgr_exposure_apply(V, H, W, C, *a, stream()) == L.MGR_EINVAL
    for k in range(7):
        a = [ptr(cov), ptr(E), ptr(img), ptr(g), ptr(g_out), ptr(dE), ptr(ws)]
        a[k] = None
        assert lib.mgr_exposure_backward(V, H, W, C, *a, need, stream()) == L.MGR_EINVAL
    assert b"null" in lib.mgr_last_error() and untouched()
    assert lib.mgr_exposure_apply(V, H, W, C, ptr(cov), ptr(E), ptr(img), ptr(img), stream()) == L.MGR_EINVAL       # out aliases img
    # the row Adam: step < 1, a rate that is not finite, sizes, NULL
    tab, m, v = _dev(R.table(C)), torch.zeros((C, 3, 4), device=DEV), torch.zeros((C, 3, 4), device=DEV)
    before = tab.clone()
    d = torch.ones((V, 3, 4), device=DEV)
    head = (C, 2, ptr(cov), V, ptr(cov), ptr(d), ptr(tab), ptr(m), ptr(v))
    assert lib.mgr_exposure_adam(*head, 0.01, 0.9, 0.999, 1e-8, 0, stream()) == L.MGR_EINVAL
    for lr in (float("nan"), float("inf"), -float("inf")):
        assert lib.mgr_exposure_adam(*head, lr, 0.9, 0.999, 1e-8, 1, stream()) == L.MGR_EINVAL
    assert lib.mgr_exposure_adam(0, 2, *head[2:], 0.01, 0.9, 0.999, 1e-8, 1, stream()) == L.MGR_EINVAL
    assert lib.mgr_exposure_adam(C, 0, *head[2:], 0.01, 0.9, 0.999, 1e-8, 1, stream()) == L.MGR_EINVAL
    assert lib.mgr_exposure_adam(C, 2, None, *head[3:], 0.01, 0.9, 0.999, 1e-8, 1, stream()) == L.MGR_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(tab, before) and not bool(m.any()) and not bool(v.any())


# ---------------------------------------------------------------------------------------------------------------------------
# the row Adam
# ---------------------------------------------------------------------------------------------------------------------------
ADAM_C, ADAM_LR = 5, 0.01
# per step: the table row of every position (a shared camera, a view without one) and the rows listed (row 3 is never listed:
# "frozen"; row 4 is never seen)
ADAM_STEPS = (([0, 1, 1, 2], [0, 1, 2]), ([2, -1, 0, 2], [0, 2]), ([1, 3, 3, 1], [1]))


def _adam_inputs():
    gen = torch.Generator().manual_seed(77)
    E0 = R.table(ADAM_C, seed=9)
    grads = [R.rounded(torch.randn((4, 3, 4), generator=gen, dtype=F64) * 10.0 ** (-s)) for s in range(len(ADAM_STEPS))]
    return E0, grads


def _sparse_adam(dtype):
    """torch.optim.SparseAdam on the rows summed over the positions in ascending order, in `dtype` on the host."""
    E0, grads = _adam_inputs()
    p = E0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.SparseAdam([p], lr=ADAM_LR, betas=(0.9, 0.999), eps=1e-8)
    for (cov, listed), d in zip(ADAM_STEPS, grads):
        rows = []
        for c in listed:
            acc = torch.zeros((3, 4), dtype=dtype)
            for k, r in enumerate(cov):
                if r == c:
                    acc = acc + d[k].to(dtype)
            rows.append(acc)
        p.grad = torch.sparse_coo_tensor(torch.tensor(listed)[None], torch.stack(rows), p.shape)
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


def _device_adam(permute=False):
    L, lib = _lib(), _lib().lib()
    E0, grads = _adam_inputs()
    E = _dev(E0)
    m, v = torch.zeros_like(E), torch.zeros_like(E)
    for s, ((cov, listed), d) in enumerate(zip(ADAM_STEPS, grads)):
        lst_t, cov_t, d_t = _i32(list(reversed(listed)) if permute else listed), _i32(cov), _dev(d)      # (alive across the call)
        L.check(lib.mgr_exposure_adam(ADAM_C, len(listed), L.ptr(lst_t), len(cov), L.ptr(cov_t), L.ptr(d_t), L.ptr(E), L.ptr(m),
                                      L.ptr(v), ADAM_LR, 0.9, 0.999, 1e-8, s + 1, L.stream()), "mgr_exposure_adam")
    return E, m, v


def test_row_adam_against_sparse_adam():
    E0, _ = _adam_inputs()
    got = _device_adam()
    ref64, ref32 = _sparse_adam(F64), _sparse_adam(F32)
    for name, a, r64, r32 in zip(("table", "exp_avg", "exp_avg_sq"), got, ref64, ref32):
        check_rows("adam " + name, R.view_rows(a), R.view_rows(r64), R.view_rows(r32))
    # rows never listed -- the "frozen" row 3, which views do show, and row 4 -- keep their bits, moments included
    E, m, v = got
    for r in (3, 4):
        assert torch.equal(E[r], _dev(E0)[r]) and not bool(m[r].any()) and not bool(v[r].any())
    # the order of the list does not matter
    for a, b in zip(got, _device_adam(permute=True)):
        assert torch.equal(a, b)
    # a negative entry and one beyond the table are skipped, the rest of the list steps as without them
    L, lib = _lib(), _lib().lib()
    outs = []
    for lst in ([0, 2], [0, -1, 2, 7]):
        E = _dev(E0)
        m, v = torch.zeros_like(E), torch.zeros_like(E)
        lst_t, cov_t, d_t = _i32(lst), _i32([0, 1, 1, 2]), _dev(_adam_inputs()[1][0])
        L.check(lib.mgr_exposure_adam(ADAM_C, len(lst), L.ptr(lst_t), 4, L.ptr(cov_t), L.ptr(d_t), L.ptr(E), L.ptr(m), L.ptr(v), ADAM_LR,
                                      0.9, 0.999, 1e-8, 1, L.stream()), "mgr_exposure_adam")
        outs.append((E, m, v))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# recovery of a planted table, image tensors alone
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_recovery():
    img, planted, tgt = R.recovery_fixture()
    losses, E = R.recovery_host_loop(img, tgt)
    return img, planted, tgt, losses, E


def test_refiner_recovers_a_planted_table():
    from manus_amd import ops
    from manus_amd.exposure import ExposureRefiner
    img, planted, tgt, host_losses, _ = _host_recovery()
    V = img.shape[0]
    x, y = _dev(img), _dev(tgt)
    ids = list(range(V))
    rows = _i32(ids)
    refiner = ExposureRefiner(["cam%d" % k for k in ids], lr_init=R.RECOVERY_LR, lr_final=R.RECOVERY_LR, device=DEV)
    n = float(x.numel())

    def loss_of():
        d = (ops.exposure_forward(x, refiner.E, rows) - y).double()
        return (d * d).mean()

    first = loss_of()
    for _ in range(R.RECOVERY_STEPS):
        g = (ops.exposure_forward(x, refiner.E, rows) - y) * (2.0 / n)
        _, dE = ops.exposure_backward(x, refiner.E, rows, g, inplace=True)
        refiner.step(dE, ids, ids)
    last = loss_of()
    first, last = float(first), float(last)
    print("recovery: device %.4e -> %.4e, fp64 host loop %.4e -> %.4e" % (first, last, host_losses[0], host_losses[-1]))
    assert refiner.steps == R.RECOVERY_STEPS
    assert abs(last - host_losses[-1]) <= 0.01 * host_losses[-1]
    assert last < first / 100.0
    assert float((refiner.E.cpu().double() - planted).abs().max()) < float((R.identity_table(V) - planted).abs().max())

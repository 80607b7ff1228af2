"""GPU: the device pose chain -- mgr_pose_apply / mgr_pose_backward / mgr_pose_adam (csrc/pose.hip), `pose.PoseRefiner` on top of
them and `HipViewCompute.transforms_changed()`.

Checker: tests/pose_chain_ref.py, the existing host chain (PoseCorrection + linalg.inv + autograd) in fp64 and fp32 on the CPU.
Tolerance where one is needed: e_kernel <= 8 * max(e32, 2^-23) in `row_rel_err` (check_rows), per (view, bone) or (frame, bone)
row.  Shapes B = 1, 20, 32 and V = 1, 3, 9; frames [0,1,1,3,0,1,3,3,0] of F = 4 (frame 2 is never viewed)."""
import functools

import pytest
import torch

import pose_chain_ref as R
from pose_chain_ref import F32, F64, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.5
SHAPES = [(B, V) for B in R.BONES for V in R.VIEWS]


def _dev(x):
    return x.to(F32).to(DEV).contiguous()


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def case(B, V):
    """The inputs of one shape and their references, computed once and shared (left unchanged by the tests)."""
    inp = R.chain_inputs(B, V)
    return inp, R.host_chain(inp, F64), R.host_chain(inp, F32)


def apply(inp, rotvec, trans, frames, gathered=True, table=None):
    from manus_amd._lib import check, lib, ptr, stream
    B, V = inp["B"], inp["V"]
    table = torch.full((inp["n_all"], B + 1, 4, 4), SENTINEL, device=DEV) if table is None else table
    g = torch.full((V, B + 1, 4, 4), SENTINEL, device=DEV) if gathered else None
    args = [_i32(inp["rows"]), _i32(frames), _dev(inp["posed"]), _dev(inp["rest"]), _dev(rotvec), _dev(trans)]      # (kept alive over the call)
    check(lib().mgr_pose_apply(V, B, inp["F"], *[ptr(t) for t in args], ptr(table), ptr(g), stream()), "mgr_pose_apply")
    return table, g


def backward(inp, frames, listed, pad_rows=1):
    """-> d_rotvec, d_trans (U + pad_rows, B, 3): NaN-filled, the rows behind U are not the kernel's to write."""
    from manus_amd._lib import check, lib, ptr, stream
    B, V, U = inp["B"], inp["V"], len(listed)
    g_r = torch.full((U + pad_rows, B, 3), float("nan"), device=DEV)
    g_t = torch.full((U + pad_rows, B, 3), float("nan"), device=DEV)
    args = [_i32(listed), _i32(inp["rows"]), _i32(frames)] + [_dev(inp[k]) for k in ("posed", "rest", "rotvec", "trans", "dT")]
    check(lib().mgr_pose_backward(V, B, inp["F"], U, *[ptr(t) for t in args], ptr(g_r), ptr(g_t), stream()), "mgr_pose_backward")
    return g_r, g_t


# =================================================================================================================
# apply
# =================================================================================================================
@pytest.mark.parametrize("B,V", SHAPES)
def test_apply_without_a_correction_is_bone_transforms_bit_for_bit(B, V):
    from manus_amd.transforms import bone_transforms
    inp = case(B, V)[0]
    posed, rest = _dev(inp["posed"]), _dev(inp["rest"])
    want = torch.stack([bone_transforms(posed[v], rest) for v in inp["rows"]])         # mgr_bone_transforms on the device
    eye = torch.eye(4, device=DEV)
    others = [v for v in range(inp["n_all"]) if v not in inp["rows"]]
    zero = torch.zeros_like(inp["rotvec"])
    for what, rotvec, trans, frames in (("zero tables", zero, zero, inp["frames"]), ("f = -1", inp["rotvec"], inp["trans"], [-1] * V),
                                        ("f = F", inp["rotvec"], inp["trans"], [inp["F"]] * V)):
        table, g = apply(inp, rotvec, trans, frames)
        assert torch.equal(table[inp["rows"]], want), what
        assert torch.equal(g, want), what                                               # gathered = the table's rows
        assert all(torch.equal(table[v, B], eye) for v in inp["rows"]), what            # the background row
        assert bool((table[others] == SENTINEL).all()), what                            # views not listed are not touched
    table, g = apply(inp, zero, zero, inp["frames"], gathered=False)                    # no gathered copy asked for
    assert g is None and torch.equal(table[inp["rows"]], want)


@pytest.mark.parametrize("B,V", SHAPES)
def test_apply_accuracy(B, V):
    inp, (T64, _, _), (T32, _, _) = case(B, V)
    table, g = apply(inp, inp["rotvec"], inp["trans"], inp["frames"])
    assert torch.equal(g, table[inp["rows"]])
    assert bool((table[[v for v in range(inp["n_all"]) if v not in inp["rows"]]] == SENTINEL).all())
    assert torch.equal(g[:, B], torch.eye(4, device=DEV).expand(V, 4, 4))
    rows = lambda x: x[:, :B].reshape(V * B, 16)
    check_rows("apply T B=%d V=%d" % (B, V), rows(g), rows(T64), rows(T32))
    # a mixed list: the odd positions uncorrected
    mixed = [f if k % 2 == 0 else -1 for k, f in enumerate(inp["frames"])]
    _, gm = apply(inp, inp["rotvec"], inp["trans"], mixed)
    plain = apply(inp, inp["rotvec"], inp["trans"], [-1] * V)[1]
    for k in range(V):
        assert torch.equal(gm[k], g[k] if k % 2 == 0 else plain[k]), k


# =================================================================================================================
# backward
# =================================================================================================================
@pytest.mark.parametrize("B,V", SHAPES)
def test_backward(B, V):
    inp, (_, dr64, dt64), (_, dr32, dt32) = case(B, V)
    every = list(range(inp["F"]))
    g_r, g_t = backward(inp, inp["frames"], every)
    rows = lambda x: x.reshape(-1, 3)
    # the planted row just above the series threshold (frame 0, bone 2; pose_chain_ref.chain_inputs) is judged on its own: its
    # fp32 host-chain error is ten times every other row's and must not set their bound
    planted = torch.zeros(4 * B, dtype=torch.bool)
    if B > 2:
        planted[2] = True

    def check_split(tag, got, r64, r32):
        got, r64, r32 = rows(got[:4]).cpu(), rows(r64), rows(r32)
        check_rows(tag + ", ordinary rows", got[~planted], r64[~planted], r32[~planted])
        if bool(planted.any()):
            check_rows(tag + ", threshold row", got[planted], r64[planted], r32[planted])
    check_split("backward d_rotvec B=%d V=%d" % (B, V), g_r, dr64, dr32)
    check_split("backward d_trans  B=%d V=%d" % (B, V), g_t, dt64, dt32)
    for f in every:             # a listed frame without a view: zeros (frame 2 at every V)
        if f not in inp["frames"]:
            assert bool((g_r[f] == 0).all()) and bool((g_t[f] == 0).all()), f
    assert bool((g_r[2] == 0).all()) and bool((g_t[2] == 0).all())
    assert bool(torch.isnan(g_r[4:]).all()) and bool(torch.isnan(g_t[4:]).all())       # rows behind U are untouched
    # two runs: equal bits
    again = backward(inp, inp["frames"], every)
    assert torch.equal(again[0][:4], g_r[:4]) and torch.equal(again[1][:4], g_t[:4])
    # a shorter list, in another order of u: the same rows, nothing else written
    part = [3, 0]
    p_r, p_t = backward(inp, inp["frames"], part, pad_rows=2)
    for u, f in enumerate(part):
        assert torch.equal(p_r[u], g_r[f]) and torch.equal(p_t[u], g_t[f]), f
    assert bool(torch.isnan(p_r[2:]).all()) and bool(torch.isnan(p_t[2:]).all())
    # positions with f = -1 contribute nothing: the chain over the remaining positions
    fewer = [-1 if k % 3 == 0 else f for k, f in enumerate(inp["frames"])]
    _, fr64, ft64 = R.host_chain(inp, F64, frames=fewer)
    _, fr32, ft32 = R.host_chain(inp, F32, frames=fewer)
    f_r, f_t = backward(inp, fewer, every)
    if any(f >= 0 for f in fewer):
        check_split("backward d_rotvec, f = -1 B=%d V=%d" % (B, V), f_r, fr64, fr32)
        check_split("backward d_trans,  f = -1 B=%d V=%d" % (B, V), f_t, ft64, ft32)
    else:
        assert bool((f_r[:4] == 0).all()) and bool((f_t[:4] == 0).all())
    none = backward(inp, [-1] * V, every)
    assert bool((none[0][:4] == 0).all()) and bool((none[1][:4] == 0).all())


# =================================================================================================================
# Adam
# =================================================================================================================
ADAM_F, ADAM_LISTS = 7, ([0, 1, 3], [1, 2, 3, 5], [0, 5])         # rows 4 and 6 are never listed
ADAM_LR = (0.01, 0.003)


def adam_inputs(B):
    g = torch.Generator().manual_seed(400 + B)
    start = [R.rounded(0.1 * torch.randn((ADAM_F, B, 3), generator=g, dtype=F64)) for _ in range(2)]
    grads = [[R.rounded(torch.randn((len(l), B, 3), generator=g, dtype=F64) * 10.0 ** float(k - 1)) for _ in range(2)] for k, l in enumerate(ADAM_LISTS)]
    return start, grads


def adam_checker(start, grads, which, dtype):
    p = start[which].to(dtype).clone().reshape(ADAM_F, -1).requires_grad_(True)
    opt = torch.optim.SparseAdam([p], lr=ADAM_LR[which], betas=(0.9, 0.999), eps=1e-8)
    for l, g in zip(ADAM_LISTS, grads):
        p.grad = torch.sparse_coo_tensor(torch.tensor(l)[None], g[which].to(dtype).reshape(len(l), -1), p.shape)
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("B", R.BONES)
def test_adam_equals_sparse_adam(B):
    from manus_amd._lib import check, lib, ptr, stream
    start, grads = adam_inputs(B)
    x = [_dev(s) for s in start]
    m = [torch.zeros_like(t) for t in x]
    v = [torch.zeros_like(t) for t in x]
    for step, (l, g) in enumerate(zip(ADAM_LISTS, grads), 1):
        lt, g0, g1 = _i32(l), _dev(g[0]), _dev(g[1])
        check(lib().mgr_pose_adam(len(l), B, ptr(lt), ptr(g0), ptr(g1), ptr(x[0]), ptr(x[1]), ptr(m[0]), ptr(v[0]),
                                  ptr(m[1]), ptr(v[1]), ADAM_LR[0], ADAM_LR[1], 0.9, 0.999, 1e-8, step, stream()), "mgr_pose_adam")
    for which, name in enumerate(("rotvec", "trans")):
        r64, r32 = adam_checker(start, grads, which, F64), adam_checker(start, grads, which, F32)
        for what, got, k in ((name, x[which], 0), ("exp_avg", m[which], 1), ("exp_avg_sq", v[which], 2)):
            rows = lambda t: t.reshape(ADAM_F * B, 3)
            check_rows("adam %s %s B=%d" % (name, what, B), rows(got), rows(r64[k]), rows(r32[k]))
        for f in (4, 6):        # never listed: bitwise unchanged
            assert torch.equal(x[which][f], _dev(start[which])[f]) and bool((m[which][f] == 0).all()) and bool((v[which][f] == 0).all())


# =================================================================================================================
# recovery, end to end: the scene of test_gpu_pose_grad.py::test_pose_recovery_end_to_end
# =================================================================================================================
def test_pose_recovery_with_the_refiner():
    """Hand scene, n = 3000, 3 views, 96x64, targets = the fused forward at the true pose, three bones turned by 0.05 rad; 50 steps
    at lr 1e-3 (rotations and translations: the host loop has one Adam rate), the Gaussians frozen.  Driven by `PoseRefiner`:
    the loss ends below its start and the mean geodesic angle of the three bones below its start.  The host-driven loop of the
    existing test runs beside it and both pairs of figures are printed (LAB.md)."""
    from test_gpu_pose_grad import _geodesic, _scene
    from manus_amd.engine import HipViewCompute
    from manus_amd.pose import PoseCorrection, PoseRefiner, _exp_so3, pose_backward
    from manus_amd.transforms import bone_transforms
    views, ids, steps = 3, [0, 1, 2], 50
    sc, ct = _scene("hand", 3000, views)
    rest, nb = sc["rest"], sc["rest"].shape[0]
    posed_true = sc["posed"].clone()
    hc = HipViewCompute(sc, torch.zeros((views, 3, 64, 96), device=DEV), ct, fused=True, pose_grad=True, loss="l1+ssim")
    with torch.no_grad():
        hc.targets = hc.forward_views_fused(ids)[0].clone()
    bones = [3, 7, 12]
    delta = torch.eye(4, device=DEV).repeat(nb, 1, 1)
    delta[bones, :3, :3] = _exp_so3(0.05 * torch.eye(3, device=DEV))
    posed_bad = (posed_true @ delta).contiguous()

    def angle(corr):
        with torch.no_grad():
            return float(torch.stack([_geodesic(corr(posed_bad[v], v)[bones, :3, :3], posed_true[v][bones, :3, :3]) for v in ids]).mean())

    # -- the device chain
    sc["posed"].copy_(posed_bad)
    ref = PoseRefiner([("capture", v) for v in ids], nb, rest, 1e-3, 1e-3, device=DEV)
    module = ref.as_module()
    dev_losses, dev_a0 = [], angle(module)
    for _ in range(steps):
        ref.apply(hc, ids, ids)
        out = hc(ids, 1.0 / views)
        dev_losses.append(float(out["loss"]))
        ref.step(out["d_transforms"], ids, ids)
    dev_a1 = angle(module)
    assert ref.steps == steps
    # -- the host chain of test_pose_recovery_end_to_end on the same scene
    corr = PoseCorrection(views, nb, device=DEV)
    opt = torch.optim.Adam(corr.parameters(), lr=1e-3)
    host_losses, host_a0 = [], angle(corr)
    for _ in range(steps):
        opt.zero_grad()
        corrected = [corr(posed_bad[v], v) for v in ids]
        with torch.no_grad():
            sc["transforms"][ids] = torch.stack([bone_transforms(c, rest) for c in corrected])
        out = hc(ids, 1.0 / views)
        host_losses.append(float(out["loss"]))
        for v in ids:
            corrected[v].backward(pose_backward(out["d_transforms"][v], corrected[v], rest))
        opt.step()
    host_a1 = angle(corr)
    print("FIGURE pose recovery, PoseRefiner: loss %.6f -> %.6f, mean geodesic angle %.4f -> %.4f rad" % (dev_losses[0], dev_losses[-1], dev_a0, dev_a1))
    print("FIGURE pose recovery, host loop:   loss %.6f -> %.6f, mean geodesic angle %.4f -> %.4f rad" % (host_losses[0], host_losses[-1], host_a0, host_a1))
    assert dev_losses[-1] < dev_losses[0]
    assert dev_a1 < dev_a0


# =================================================================================================================
# HipViewCompute.transforms_changed()
# =================================================================================================================
def _clone(o):
    return {k: ({q: t.clone() for q, t in v.items()} if isinstance(v, dict) else v.clone()) for k, v in o.items() if k in ("loss", "grads", "d_transforms")}


def _same(a, b, what):
    assert torch.equal(a["loss"], b["loss"]), (what, "loss")
    assert torch.equal(a["d_transforms"], b["d_transforms"]), (what, "d_transforms")
    for k, g in b["grads"].items():
        assert torch.equal(a["grads"][k], g), (what, k)


def _refined_scene(n=3000, views=3):
    from test_gpu_pose_grad import _scene
    from manus_amd.pose import PoseRefiner
    sc, ct = _scene("hand", n, views)
    nb = sc["rest"].shape[0]
    ref = PoseRefiner([("capture", f) for f in range(2)], nb, sc["rest"], 1e-3, 1e-3, device=DEV)
    g = torch.Generator().manual_seed(3)
    ref.rotvec.copy_((0.03 * torch.randn(ref.rotvec.shape, generator=g)).to(DEV))
    ref.trans.copy_((0.002 * torch.randn(ref.trans.shape, generator=g)).to(DEV))
    tg = torch.rand((views, 3, 64, 96), generator=g).to(DEV)
    return sc, ct, ref, tg


def test_transforms_changed_equals_view_constants_changed():
    from manus_amd.engine import HipViewCompute
    sc, ct, ref, tg = _refined_scene()
    ids, frames = [0, 1, 2], [1, 0, 1]
    hc = HipViewCompute(sc, tg, ct, fused=True, pose_grad=True, loss="l1+ssim", persistent_grads=False)
    before = _clone(hc(ids, 1.0 / 3))
    gathered = hc.gathered_transforms(ids)
    assert gathered is not None and hc.gathered_transforms([0, 1]) is None
    version = sc["transforms"]._version
    # (a) the gathered copy of the cached view set is written by apply itself
    ref.apply(hc, ids, frames)
    assert sc["transforms"]._version == version and hc.gathered_transforms(ids) is gathered          # nothing was dropped
    assert torch.equal(gathered, sc["transforms"][ids])
    a = _clone(hc(ids, 1.0 / 3))
    assert not torch.equal(a["loss"], before["loss"])                                                  # the correction is seen
    hc.view_constants_changed()
    _same(a, _clone(hc(ids, 1.0 / 3)), "apply into the gathered copy")
    # (b) apply to another view list: the cached set is refreshed from the table by transforms_changed()
    gathered = hc.gathered_transforms(ids)
    ref.rotvec.mul_(-1.5)
    ref.apply(hc, [2, 0], [0, 1])
    assert hc.gathered_transforms(ids) is gathered and torch.equal(gathered, sc["transforms"][ids])
    b = _clone(hc(ids, 1.0 / 3))
    assert not torch.equal(b["loss"], a["loss"])
    hc.view_constants_changed()
    _same(b, _clone(hc(ids, 1.0 / 3)), "cached set refreshed from the table")
    # (c) the modular route reads the same cache
    hm = HipViewCompute(sc, tg, ct, fused=False, pose_grad=True, loss="l1+ssim")
    hm(ids, 1.0 / 3)
    ref.rotvec.mul_(0.5)
    ref.apply(hm, ids, frames)
    c = _clone(hm(ids, 1.0 / 3))
    hm.view_constants_changed()
    d = _clone(hm(ids, 1.0 / 3))
    assert torch.equal(c["loss"], d["loss"])              # (the forward: this route's backward is not held to equal bits)


def test_transforms_changed_keeps_the_cached_lpips_target_taps():
    """lpips_cache_targets=True, stand-in weights: a counting wrapper around LPIPS.target_taps sees one call over a first step and
    three refined steps; view_constants_changed() makes it two."""
    import lpips_ref
    from manus_amd.engine import HipViewCompute
    from manus_amd.lpips import LPIPS
    sc, ct, ref, tg = _refined_scene(n=2000)
    net = LPIPS.from_state_dicts(*lpips_ref.state_dicts("vgg", lpips_ref.make_weights("vgg", 0)), net="vgg")
    calls, inner = [], net.target_taps

    def counted(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    net.target_taps = counted
    ids, frames = [0, 1, 2], [1, 0, 1]
    rects = [(8, 6, 64, 40), (0, 0, 48, 32), (20, 16, 70, 44)]
    hc = HipViewCompute(sc, tg, ct, fused=True, pose_grad=True, loss="l1+ssim", persistent_grads=False, lpips=net, w_lpips=0.1,
                        lpips_rects=rects, lpips_cache_targets=True)
    losses = [float(hc(ids, 1.0 / 3)["loss"])]
    assert len(calls) == 1
    taps = hc._cache[tuple(ids)]["lpips"]["taps"]
    for _ in range(3):
        ref.apply(hc, ids, frames)
        out = hc(ids, 1.0 / 3)
        losses.append(float(out["loss"]))
        ref.step(out["d_transforms"], ids, frames)
    assert len(calls) == 1 and hc._cache[tuple(ids)]["lpips"]["taps"] is taps
    assert len(set(losses)) == 4                               # every step saw other transforms
    hc.view_constants_changed()
    hc(ids, 1.0 / 3)
    assert len(calls) == 2

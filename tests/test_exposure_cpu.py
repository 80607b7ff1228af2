"""No GPU: the ABI of the exposure entries (header, binding, built library), the restatement's analytic backward against fp64
autograd, the refusals of HipViewCompute / ExposureRefiner / Trainer that need no device, the rate schedule, the state dict, and
the conditions the recovery fixture itself has to meet."""
import ctypes
import os
import re

import pytest
import torch

import exposure_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_exposure_block": 0, "mgr_exposure_workspace_bytes": 3, "mgr_exposure_apply": 9, "mgr_exposure_backward": 13,
               "mgr_exposure_adam": 15}


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    assert "exposure.hip" in build.SOURCES
    build.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in NEW_ENTRIES.items():
        assert _declared_args(header, name) == arity, name
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == arity, (name, len(args), arity)
        assert res is (ctypes.c_size_t if name.endswith("_workspace_bytes") else ctypes.c_int), name
        assert hasattr(so, name), "%s is not exported by the built library" % name
    # the rates of the Adam entry travel as doubles, like mgr_pose_adam's
    assert _lib.SIGNATURES["mgr_exposure_adam"][1][9:13] == [ctypes.c_double] * 4
    L = _lib.lib()
    block = L.mgr_exposure_block()
    assert block > 0 and block % 4 == 0
    # 12 doubles per workgroup and view, nothing for a size the entries refuse
    assert L.mgr_exposure_workspace_bytes(3, 1, block + 1) >= 3 * 2 * 96 > L.mgr_exposure_workspace_bytes(3, 1, block) >= 3 * 96
    assert L.mgr_exposure_workspace_bytes(0, 4, 4) == 0 and L.mgr_exposure_workspace_bytes(1, 0, 4) == 0


def test_host_refusals_of_the_entries_need_no_device():
    """Every refusal is decided on the arguments, before any launch.  Only NULL pointers are passed here, so no call could launch
    whatever it decided; the refusals that need real buffers (a short workspace, aliasing) are in tests/test_gpu_exposure.py."""
    from manus_amd import _lib
    L = _lib.lib()
    for V, H, W, C in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (70000, 4, 4, 1), (1, 65536, 65536, 1)):
        assert L.mgr_exposure_apply(V, H, W, C, None, None, None, None, None) == _lib.MGR_EINVAL
        assert b"null" not in L.mgr_last_error()
        assert L.mgr_exposure_backward(V, H, W, C, None, None, None, None, None, None, None, 1 << 20, None) == _lib.MGR_EINVAL
        assert b"null" not in L.mgr_last_error()
    assert b"image too large" in L.mgr_last_error()
    assert L.mgr_exposure_apply(1, 4, 4, 1, None, None, None, None, None) == _lib.MGR_EINVAL
    assert b"mgr_exposure_apply: null" in L.mgr_last_error()
    assert L.mgr_exposure_backward(1, 4, 4, 1, None, None, None, None, None, None, None, 1 << 20, None) == _lib.MGR_EINVAL
    assert b"mgr_exposure_backward: null" in L.mgr_last_error()
    nul = (None,) * 5
    assert L.mgr_exposure_adam(1, 1, None, 1, *nul, 0.01, 0.9, 0.999, 1e-8, 0, None) == _lib.MGR_EINVAL
    assert b"step" in L.mgr_last_error()
    for lr in (float("nan"), float("inf")):
        assert L.mgr_exposure_adam(1, 1, None, 1, *nul, lr, 0.9, 0.999, 1e-8, 1, None) == _lib.MGR_EINVAL
        assert b"rate" in L.mgr_last_error()
    for C, U, V in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.mgr_exposure_adam(C, U, None, V, *nul, 0.01, 0.9, 0.999, 1e-8, 1, None) == _lib.MGR_EINVAL
        assert b"at least 1" in L.mgr_last_error()
    assert L.mgr_exposure_adam(1, 1, None, 1, *nul, 0.01, 0.9, 0.999, 1e-8, 1, None) == _lib.MGR_EINVAL
    assert b"null" in L.mgr_last_error()


@pytest.mark.parametrize("rows", [[0, 1, 2], [1, 1, 0], [0, -1, 1], [5, 0, 0]])
def test_analytic_backward_equals_fp64_autograd(rows):
    V, H, W = 3, 5, 7
    E = R.table(3)
    img, g = R.images(V, H, W)
    g_ad, dE_ad = R.backward_autograd(img, E, rows, g)
    g_an, dE_an = R.backward_ref(img, E, rows, g)
    eg = float((g_ad - g_an).abs().max() / g_ad.abs().max())
    eE = float((dE_ad - dE_an).abs().max() / dE_ad.abs().max())
    print("analytic vs autograd: g %.3e  dE %.3e" % (eg, eE))
    assert eg <= 1e-12 and eE <= 1e-12
    for k, r in enumerate(rows):
        if not 0 <= r < 3:      # no correction: the view and its gradient pass through, nothing reaches the table
            assert torch.equal(R.apply_ref(img, E, rows)[k], img[k]) and torch.equal(g_an[k], g[k])
            assert bool((dE_an[k] == 0).all()) and bool((dE_ad[k] == 0).all())


def _cpu_object_scene():
    from manus_amd.synthetic import camera_table, make_scene
    sc = make_scene(n_gaussians=50, kind="object", seed=1, grid_res=8, n_cameras=2, width=24, height=16, device="cpu")
    return sc, camera_table(sc["cameras"], "cpu")


def test_refusals_of_the_compute_object():
    from manus_amd.engine import HipViewCompute
    sc, ct = _cpu_object_scene()
    tg = torch.zeros((2, 3, 16, 24))
    good = torch.zeros((2, 3, 4))
    hc = HipViewCompute(sc, tg, ct, exposure=good)
    assert hc.exposure is good and hc.exposure_on is True and hc.exposure_ids is None      # the table is not copied
    assert hc._exposure_table() is good
    hc.exposure_on = False
    assert hc._exposure_table() is None
    assert HipViewCompute(sc, tg, ct)._exposure_table() is None
    three = torch.zeros((3, 3, 4))
    assert HipViewCompute(sc, tg, ct, exposure=three, exposure_ids=[2, -1])._exposure_table() is three
    for bad in (torch.zeros((2, 4, 3)), torch.zeros((2, 12)), torch.zeros((2, 3, 4), dtype=torch.float64), torch.zeros((2, 3, 4), device="meta"),
                torch.zeros((2, 3, 8))[:, :, ::2], [[0.0] * 4] * 3):
        with pytest.raises(ValueError, match="exposure"):
            HipViewCompute(sc, tg, ct, exposure=bad)
    with pytest.raises(ValueError, match="exposure_ids"):
        HipViewCompute(sc, tg, ct, exposure=three)                          # C != V_all without ids
    for ids in ([0], [0, 1, 2]):
        with pytest.raises(ValueError, match="exposure_ids"):
            HipViewCompute(sc, tg, ct, exposure=three, exposure_ids=ids)
    # the attributes are plain: a table set after construction is refused at the step's own check
    hc = HipViewCompute(sc, tg, ct)
    hc.exposure = three
    with pytest.raises(ValueError, match="exposure_ids"):
        hc._exposure_table()
    hc.exposure_ids = [0, 2]
    assert hc._exposure_table() is three


def test_refusals_of_the_refiner_and_the_trainer():
    from manus_amd.engine import HipViewCompute, Trainer
    from manus_amd.exposure import ExposureRefiner
    with pytest.raises(ValueError, match="at least one camera"):
        ExposureRefiner([], device="cpu")
    with pytest.raises(ValueError, match="frozen"):
        ExposureRefiner(["a", "b"], frozen=("c",), device="cpu")
    for kw in (dict(lr_init=0.0), dict(lr_final=-1.0), dict(lr_init=float("nan")), dict(max_steps=0)):
        with pytest.raises(ValueError):
            ExposureRefiner(["a"], device="cpu", **kw)
    r = ExposureRefiner(["a", "b", "a", None, "c"], frozen=("b",), device="cpu")
    assert r.camera_keys == ["a", "b", "c"] and r.frozen == frozenset([1]) and tuple(r.E.shape) == (3, 3, 4)
    assert torch.equal(r.E, R.identity_table(3).float())
    d = torch.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="one row per view"):
        r.step(d, [0, 1], [0])
    with pytest.raises(ValueError, match="d_exposure"):
        r.step(torch.zeros((2, 12)), [0, 1], [0, 1])
    with pytest.raises(ValueError, match="beyond"):
        r.step(d, [0, 1], [0, 3])
    r.step(d, [0, 1], [1, -1])              # only a frozen camera and a view without one: nothing to move, no launch, no step
    assert r.steps == 0 and r.last_listed == []

    class Store:
        camera_keys = ["c", "a", "zz"]
        row = {10: 0, 11: 1, 12: 2}
    assert r.rows_of(Store, [12, 10, 11, 10]) == [-1, 2, 0, 2]
    with pytest.raises(ValueError, match="camera keys"):
        r.rows_of(object(), [0])
    # attach: one table row per view row
    sc, ct = _cpu_object_scene()
    hc = HipViewCompute(sc, torch.zeros((2, 3, 16, 24)), ct)
    with pytest.raises(ValueError, match="view rows"):
        r.attach(hc)
    with pytest.raises(ValueError, match="ids"):
        r.attach(hc, [0])
    r.attach(hc, [2, -1])
    assert hc.exposure is r.E and hc.exposure_ids == [2, -1]
    two = ExposureRefiner(["a", "b"], device="cpu")
    two.attach(hc)
    assert hc.exposure is two.E and hc.exposure_ids == [0, 1]
    # the Trainer: the gradient is not reduced across ranks
    with pytest.raises(ValueError, match="world_size == 1"):
        Trainer(hc, 2, 1.0, world_size=2, exposure=two)
    with pytest.raises(ValueError, match="exposure_every"):
        Trainer(hc, 2, 1.0, exposure=two, exposure_every=0)
    with pytest.raises(ValueError, match="exposure table"):
        Trainer(object(), 2, 1.0, exposure=two)


def test_rate_schedule_ends():
    from manus_amd.exposure import ExposureRefiner
    r = ExposureRefiner(["a"], device="cpu")
    assert r.lr(0) == pytest.approx(0.01, rel=1e-12) and r.lr(30000) == pytest.approx(0.001, rel=1e-12)
    assert r.lr(10 ** 6) == pytest.approx(0.001, rel=1e-12)                    # held behind max_steps
    assert r.lr(15000) == pytest.approx((0.01 * 0.001) ** 0.5, rel=1e-12)      # log-linear between
    r = ExposureRefiner(["a"], lr_init=0.02, lr_final=0.02, max_steps=10, device="cpu")
    assert r.lr(0) == r.lr(5) == r.lr(10) == pytest.approx(0.02, rel=1e-12)


def test_state_dict_round_trip_and_key_mismatch():
    from manus_amd.exposure import ExposureRefiner
    a = ExposureRefiner(["a", "b", "c"], device="cpu")
    gen = torch.Generator().manual_seed(0)
    a.E += 0.1 * torch.randn(a.E.shape, generator=gen)
    a.m += torch.randn(a.m.shape, generator=gen)
    a.v += torch.rand(a.v.shape, generator=gen)
    a.steps = 17
    st = a.state_dict()
    assert set(st) == {"camera_keys", "steps", "E", "m", "v"}          # the rates are configuration
    a.E.zero_()                                                        # the state holds copies
    b = ExposureRefiner(["a", "b", "c"], lr_init=0.5, lr_final=0.5, device="cpu")
    table = b.E
    b.load_state_dict(st)
    assert b.E is table                                                # in place: an attached compute object keeps seeing it
    assert torch.equal(b.E, st["E"]) and torch.equal(b.m, st["m"]) and torch.equal(b.v, st["v"]) and b.steps == 17
    assert b.lr(0) == pytest.approx(0.5)
    with pytest.raises(ValueError, match="other cameras"):
        ExposureRefiner(["a", "c", "b"], device="cpu").load_state_dict(st)
    with pytest.raises(ValueError, match="other cameras"):
        ExposureRefiner(["a", "b"], device="cpu").load_state_dict(st)


def test_recovery_fixture_is_well_posed():
    """The recovery test of the device kernels is only worth its bound if the problem itself is well conditioned and the fp64
    loop solves it: both are asserted here, on the host."""
    img, planted, tgt = R.recovery_fixture()
    conds = R.condition_numbers(img)
    print("condition numbers of [img; 1] per view:", ["%.0f" % c for c in conds])
    assert max(conds) < 1e3
    losses, E = R.recovery_host_loop(img, tgt)
    print("fp64 loop: loss %.3e -> %.3e after %d steps" % (losses[0], losses[-1], len(losses) - 1))
    assert len(losses) == R.RECOVERY_STEPS + 1
    assert losses[-1] < losses[0] / 100.0
    assert float((E - planted).abs().max()) < float((R.identity_table(3) - planted).abs().max())

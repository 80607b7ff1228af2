"""No GPU: the ABI of the skin-grid refinement step (mgr_skin_grid_refine and its workspace query) -- header, binding, built
library --, its refusals, which are all decided before anything touches a device, the restatement of tests/skin_refine_ref.py
(prior gradient against central differences, the projection's rules), `optim.SkinGridRefiner`'s arguments and state on CPU
tensors, and the two conditions the GPU file's recovery test puts on its own reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import skin_refine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity, res in (("mgr_skin_grid_refine_workspace_bytes", 1, ctypes.c_size_t), ("mgr_skin_grid_refine", 24, ctypes.c_int)):
        args = _declared_args(header, name)
        assert len(args) == arity, (name, args)
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        r, bound = _lib.SIGNATURES[name]
        assert len(bound) == arity and r is res, (name, len(bound), r)
        assert hasattr(so, name), "%s is not exported by the built library" % name
    args = _declared_args(header, "mgr_skin_grid_refine")
    assert args[-1] == "void* stream" and args[:4] == ["const int32_t* voxel", "const float* grad", "const uint32_t* count", "int capacity"]
    # lr, beta1, beta2, eps and prior_weight travel as doubles, in the header and in the binding
    doubles = [k for k, a in enumerate(args) if a.startswith("double ")]
    assert [args[k] for k in doubles] == ["double lr", "double beta1", "double beta2", "double eps", "double prior_weight"]
    bound = _lib.SIGNATURES["mgr_skin_grid_refine"][1]
    assert [k for k, t in enumerate(bound) if t is ctypes.c_double] == doubles
    assert args[20] == "double* prior_value" and bound[20] is ctypes.c_void_p


def test_workspace_is_one_double_per_eight_rows():
    from manus_amd._lib import lib
    L = lib()
    assert L.mgr_skin_grid_refine_workspace_bytes(0) == 0 and L.mgr_skin_grid_refine_workspace_bytes(-5) == 0
    for cap in (1, 8, 9, 257, 100000):
        n = L.mgr_skin_grid_refine_workspace_bytes(cap)
        assert n >= 8 * ((cap + 7) // 8) and n % 256 == 0 and n < 8 * ((cap + 7) // 8) + 256, (cap, n)


class _Buffers:
    """Host arrays behind the pointers of a call: a refusal dereferences none of them, and leaves all of them as they were."""
    NAMES = ("voxel", "grad", "count", "grid", "grid0", "exp_avg", "exp_avg_sq", "prior_value", "workspace")

    def __init__(self):
        g = np.random.default_rng(0)
        self.a = dict(voxel=np.arange(16, dtype=np.int32), grad=g.random((16, 24), dtype=np.float32), count=np.array([16], np.uint32),
                      grid=g.random((64, 24), dtype=np.float32), grid0=g.random((64, 24), dtype=np.float32),
                      exp_avg=g.random((64, 24), dtype=np.float32), exp_avg_sq=g.random((64, 24), dtype=np.float32),
                      prior_value=np.array([123.5]), workspace=np.full(64, 7.0))
        self.before = {k: v.copy() for k, v in self.a.items()}

    def ptr(self, k):
        return ctypes.c_void_p(self.a[k].ctypes.data)

    def untouched(self):
        return all(np.array_equal(self.a[k], self.before[k]) for k in self.NAMES)


def _call(buf, capacity=16, stride=24, B=21, step=1, prior_weight=0.5, min_sum=1e-12, ws_bytes=None, null=()):
    from manus_amd._lib import lib
    p = {k: (None if k in null else buf.ptr(k)) for k in buf.NAMES}
    need = int(lib().mgr_skin_grid_refine_workspace_bytes(capacity))
    return lib().mgr_skin_grid_refine(p["voxel"], p["grad"], p["count"], capacity, p["grid"], p["grid0"], stride, B, p["exp_avg"],
                                      p["exp_avg_sq"], 0.01, 0.9, 0.999, 1e-8, step, 1, 0.0, prior_weight, 1, min_sum, p["prior_value"],
                                      p["workspace"], need if ws_bytes is None else ws_bytes, None)


REFUSALS = [
    ("B = 0", dict(B=0, stride=24)), ("B = -1", dict(B=-1, stride=24)), ("B = 33", dict(B=33, stride=33)),
    ("stride neither B nor 24", dict(B=21, stride=22)), ("stride 24 below B", dict(B=25, stride=24)),
    ("capacity < 0", dict(capacity=-1)), ("step = 0", dict(step=0)), ("step < 0", dict(step=-3)),
    ("prior_weight < 0", dict(prior_weight=-0.5)), ("prior_weight inf", dict(prior_weight=float("inf"))),
    ("prior_weight nan", dict(prior_weight=float("nan"))),
    ("prior without grid0", dict(null=("grid0",))), ("prior without prior_value", dict(null=("prior_value",))),
    ("min_sum < 0", dict(min_sum=-1e-3)),
] + [("null %s" % k, dict(null=(k,))) for k in ("voxel", "grad", "count", "grid", "exp_avg", "exp_avg_sq")] \
  + [("null %s at weight 0" % k, dict(null=(k, "grid0", "prior_value"), prior_weight=0.0)) for k in ("voxel", "grid", "exp_avg_sq")]


@pytest.mark.parametrize("tag,kw", REFUSALS, ids=[t for t, _ in REFUSALS])
def test_refusals_before_the_device(tag, kw):
    from manus_amd._lib import MGR_EINVAL, lib
    buf = _Buffers()
    rc = _call(buf, **kw)
    err = lib().mgr_last_error()
    assert rc == MGR_EINVAL, (tag, rc, err)
    assert err.startswith(b"mgr_skin_grid_refine"), err
    assert buf.untouched(), tag


def test_short_workspace_is_enomem():
    from manus_amd._lib import MGR_ENOMEM, lib
    need = int(lib().mgr_skin_grid_refine_workspace_bytes(16))
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(null=("workspace",)), dict(ws_bytes=need - 1, prior_weight=0.0)):
        buf = _Buffers()
        rc = _call(buf, **kw)
        assert rc == MGR_ENOMEM and lib().mgr_last_error().startswith(b"mgr_skin_grid_refine"), (kw, rc)
        assert buf.untouched(), kw


# -- the restatement -----------------------------------------------------------------------------------------------------
def test_prior_gradient_equals_central_differences():
    g = torch.Generator().manual_seed(3)
    x, x0 = torch.rand((7, 21), generator=g, dtype=F64), torch.rand((7, 21), generator=g, dtype=F64)
    w, h = 0.37, 1e-6
    an = R.prior_grad(x, x0, w)
    for k in torch.randperm(x.numel(), generator=g)[:20].tolist():
        up, dn = x.clone(), x.clone()
        up.reshape(-1)[k] += h
        dn.reshape(-1)[k] -= h
        fd = (R.prior_value(up, x0, w) - R.prior_value(dn, x0, w)) / (2 * h)
        assert abs(fd - float(an.reshape(-1)[k])) <= 1e-8 * max(1.0, abs(fd)), (k, fd, float(an.reshape(-1)[k]))
    assert R.prior_value(x0, x0, w) == 0.0 and bool((R.prior_grad(x0, x0, w) == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, F64])
def test_projection_rules(dtype):
    g = torch.Generator().manual_seed(4)
    x = torch.rand((40, 21), generator=g, dtype=F64).to(dtype)
    x[3] = 0.0                                  # all zero: S = 0 is not above min_sum
    x[5, 2] = float("nan")                      # a NaN row: S > min_sum is false
    x[7] = 1e-15                                # a tiny row below min_sum
    x[9] = -x[9]                                # a negative sum (no clamp): not above min_sum either
    p = R.project_rows(x, 1e-12)
    eps = torch.finfo(dtype).eps
    rest = [k for k in range(40) if k not in (3, 5, 7, 9)]
    assert float((p[rest].double().sum(1) - 1.0).abs().max()) <= 8 * eps
    for k in (3, 7, 9):
        assert torch.equal(p[k], x[k]), k
    assert bool(torch.isnan(p[5, 2])) and torch.equal(p[5, :2], x[5, :2]) and torch.equal(p[5, 3:], x[5, 3:])
    assert int(torch.isnan(p).sum()) == 1       # no NaN is created
    # idempotent: a projected row has sum 1 to rounding, so a second projection moves it by rounding only
    assert float((R.project_rows(p, 1e-12)[rest] - p[rest]).abs().max()) <= 4 * eps


def test_chain_with_the_extras_off_is_sparse_adam():
    import test_gpu_skin_grid_grad as G
    grid, sets, grads = G.adam_inputs(21)
    for clamp_min in (None, 0.3):
        a = G.adam_checker(grid, sets, grads, F64, clamp_min)
        b = R.refine_chain(grid, sets, grads, F64, clamp_min=clamp_min, prior_weight=0.0, project=False)
        assert all(torch.equal(x, y) for x, y in zip(a, b[:3])) and b[3] == [0.0, 0.0, 0.0]


# -- SkinGridRefiner on CPU tensors ----------------------------------------------------------------------------------------
def _grid(B=21, dims=(3, 4, 5)):
    from manus_amd import ops
    return ops.SkinGrid(torch.rand(dims + (B,), generator=torch.Generator().manual_seed(B)))


def test_refiner_argument_errors():
    from manus_amd._lib import ManusHipError
    from manus_amd.optim import SkinGridRefiner
    sg = _grid()
    with pytest.raises(ManusHipError):
        SkinGridRefiner(sg.data, lr=0.01)
    for kw in (dict(prior_weight=-1.0), dict(prior_weight=float("nan")), dict(prior_weight=float("inf")), dict(min_sum=-1e-3)):
        with pytest.raises(ValueError):
            SkinGridRefiner(sg, lr=0.01, **kw)
    r = SkinGridRefiner(sg, lr=0.01)
    assert r.project is True and r.prior_weight == 0.0 and r.clamp_min == 0.0 and r.min_sum == 1e-12 and r.steps == 0
    assert torch.equal(r.prior, sg.data) and r.prior.data_ptr() != sg.data.data_ptr()          # a copy
    assert r.last_prior.dtype == F64 and r.last_prior.numel() == 1
    with pytest.raises(ValueError):
        r.set_prior(torch.zeros((3, 4, 5, 20)))
    new = torch.rand((3, 4, 5, 21))
    r.set_prior(new)
    assert torch.equal(r.prior[..., :21], new) and bool((r.prior[..., 21:] == 0).all())
    from manus_amd import ops
    other = ops.SkinGridGrad(torch.zeros(4, dtype=torch.int32), torch.zeros((4, 24)), torch.zeros(1, dtype=torch.int32), (3, 4, 6, 21))
    with pytest.raises(ManusHipError):
        r.step(other)


def test_refiner_state_dict_keys_and_round_trip():
    from manus_amd.optim import SkinGridRefiner
    sg = _grid()
    r = SkinGridRefiner(sg, lr=0.02, betas=(0.8, 0.99), eps=1e-7, clamp_min=None, prior_weight=0.25, project=False, min_sum=1e-9)
    sd = r.state_dict()
    assert set(sd) == {"shape", "stride", "steps", "exp_avg", "exp_avg_sq", "prior", "hyper"}
    assert set(sd["hyper"]) == {"lr", "betas", "eps", "clamp_min", "prior_weight", "project", "min_sum"}
    assert sd["exp_avg"] is None and sd["steps"] == 0 and sd["shape"] == (3, 4, 5, 21) and sd["stride"] == 24
    # moments as a run would have left them
    r.exp_avg, r.exp_avg_sq, r.steps = torch.rand_like(sg.data), torch.rand_like(sg.data), 5
    r.prior.mul_(0.5)
    sd = r.state_dict()
    fresh = SkinGridRefiner(sg, lr=0.5)
    fresh.load_state_dict(sd)
    assert fresh.steps == 5 and fresh.lr == 0.02 and fresh.betas == (0.8, 0.99) and fresh.eps == 1e-7 and fresh.clamp_min is None
    assert fresh.prior_weight == 0.25 and fresh.project is False and fresh.min_sum == 1e-9
    for k in ("exp_avg", "exp_avg_sq", "prior"):
        assert torch.equal(getattr(fresh, k), getattr(r, k)) and getattr(fresh, k).data_ptr() != getattr(r, k).data_ptr()
    # a grid of another shape, and one of another stride
    with pytest.raises(ValueError):
        SkinGridRefiner(_grid(dims=(3, 4, 6)), lr=0.01).load_state_dict(sd)
    with pytest.raises(ValueError):
        SkinGridRefiner(_grid(B=25), lr=0.01).load_state_dict(sd)
    with pytest.raises(ValueError):
        SkinGridRefiner(sg, lr=0.01).load_state_dict(dict(sd, exp_avg=torch.zeros((3, 4, 5, 21))))


def test_refiner_state_passes_through_a_checkpoint(tmp_path):
    from manus_amd import checkpoint
    from manus_amd.optim import SkinGridRefiner
    sg = _grid()
    r = SkinGridRefiner(sg, lr=0.02, prior_weight=0.25)
    r.exp_avg, r.exp_avg_sq, r.steps = torch.rand_like(sg.data), torch.rand_like(sg.data), 3
    params = {"_xyz": torch.rand((5, 3)), "_features_dc": torch.rand((5, 1, 3)), "_features_rest": torch.rand((5, 15, 3)),
              "_opacity": torch.rand((5, 1)), "_scaling": torch.rand((5, 3)), "_rotation": torch.rand((5, 4))}
    path = checkpoint.save_checkpoint(str(tmp_path), params, 0, 3, 0.5, extra_state={"skin_grid_refiner": r.state_dict()})
    back = checkpoint.load_checkpoint(path, return_checkpoint=True)[2]["skin_grid_refiner"]      # the safe loader: no pickled objects
    fresh = SkinGridRefiner(sg, lr=0.5, project=False)
    fresh.load_state_dict(back)
    a, b = r.state_dict(), fresh.state_dict()
    assert a["hyper"] == b["hyper"] and a["steps"] == b["steps"] and tuple(a["shape"]) == tuple(b["shape"])
    assert all(torch.equal(a[k], b[k]) for k in ("exp_avg", "exp_avg_sq", "prior"))


# -- the conditions on the GPU file's own reference ------------------------------------------------------------------------
def test_recovery_checker_with_projection_converges_and_the_prior_holds_the_grid():
    """Measured when the test was written: rho_ref 7.9e-5 with the projection (1.56e-4 without), row sums 1 to 4e-16;
    dist(w = 1) / dist(w = 0) = 0.79 / 2.31 = 0.34."""
    free, held = R.recovery_reference(0.0, True), R.recovery_reference(1.0, True)
    print("FIGURE recovery reference: project rho %.3e dist %.3f sums [%.17g, %.17g] rows %d; prior 1: rho %.3e dist %.3f"
          % (free["rho_ref"], free["dist"], free["sum_min"], free["sum_max"], free["touched"], held["rho_ref"], held["dist"]))
    assert free["rho_ref"] < 0.1, free["rho_ref"]
    assert abs(free["sum_min"] - 1.0) < 1e-14 and abs(free["sum_max"] - 1.0) < 1e-14
    assert held["dist"] <= 0.5 * free["dist"], (held["dist"], free["dist"])

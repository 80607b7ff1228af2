"""GPU: densify_and_prune(remove_outliers=True) (manus_amd.optim over manus_amd.outliers) on an optimizer of 3 000 Gaussians
-- a blob with rows that clone, rows that split, rows the opacity / size tests prune, and planted floaters -- with fixed
noise.  Everything is compared `torch.equal`: leaves, both moments, skin weights and the three statistics."""
import numpy as np
import pytest
import torch

import outlier_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_BLOB, N_FLOAT = 2988, 12
N = N_BLOB + N_FLOAT
MAX_GRAD, MIN_OPACITY, EXTENT, SIZE_THR = 0.0002, 0.005, 1.0, 20
OPTS = dict(percent_dense=0.01, remove_outliers_step=200)


def make_optimizer():
    """Fresh optimizer, identical every call: blob rows 0 .. N_BLOB-1, floaters behind them.  A third of the blob carries a
    gradient above the threshold (small scales clone, large ones split), 40 rows have an opacity below the threshold, 5 a
    world size above 0.1 * extent; the floaters carry no gradient, so they are neither cloned nor split."""
    from manus_amd.optim import GaussianOptimizer
    g = torch.Generator().manual_seed(5)
    xyz = torch.as_tensor(R.planted(3, N_BLOB, N_FLOAT))
    # largest scale 3 .. 30 mm against a clone / split boundary of percent_dense * extent = 10 mm
    scal = torch.log(torch.empty(N, 1).uniform_(0.003, 0.03, generator=g) * torch.empty(N, 3).uniform_(0.7, 1.0, generator=g))
    scal[100:105] = float(np.log(0.2))
    opac = torch.randn(N, 1, generator=g) + 1.0
    opac[200:240] = -7.0
    rot = torch.randn(N, 4, generator=g)
    params = dict(_xyz=xyz, _features_dc=torch.randn(N, 1, 3, generator=g), _features_rest=torch.randn(N, 15, 3, generator=g) * 0.1,
                  _opacity=opac, _scaling=scal, _rotation=rot)
    skin = torch.rand(N, 4, generator=g)
    go = GaussianOptimizer({k: v.to(DEV) for k, v in params.items()}, opts=OPTS, skin_weights=skin.to(DEV))
    for a in go.m:
        go.m[a].copy_(torch.randn(go.m[a].shape, generator=g).to(DEV))
        go.v[a].copy_(torch.rand(go.v[a].shape, generator=g).to(DEV))
    accum = torch.zeros(N, 1)
    accum[:N_BLOB:3] = 0.001
    accum[100:105] = 0.0
    go.xyz_gradient_accum.copy_(accum.to(DEV))
    go.denom.fill_(1.0)
    return go


def noise_pool():
    return torch.randn(2 * N, 3, generator=torch.Generator().manual_seed(9)).to(DEV)


def state(go):
    out = {}
    for name, d in (("p", go.p), ("m", go.m), ("v", go.v)):
        for a, t in d.items():
            out[name + a] = t
    out["skin"] = go.skin_weights
    out["accum"], out["denom"], out["radii"] = go.xyz_gradient_accum, go.denom, go.max_radii2D
    return out


def assert_same_state(a, b, what):
    sa, sb = state(a), state(b)
    for k in sa:
        assert sa[k].shape == sb[k].shape, (what, k, sa[k].shape, sb[k].shape)
        assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), (what, k)


def floaters_left(go):
    fl = torch.as_tensor(R.planted(3, N_BLOB, N_FLOAT)[N_BLOB:], device=DEV)
    return int((go.p["_xyz"][:, None, :] == fl[None]).all(-1).any(1).sum())


def test_remove_outliers_equals_the_hand_composition():
    from manus_amd.optim import ALL_GROUPS
    from manus_amd.outliers import outlier_mask
    noise = noise_pool()
    go = make_optimizer()
    info = go.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, SIZE_THR, remove_outliers=True, noise=noise, noise_is_pool=True)
    # by hand, through public methods: densify with pruning disabled, the outlier mask on the resulting centres, one prune
    ref = make_optimizer()
    first = ref.densify_and_prune(MAX_GRAD, float("-inf"), EXTENT, None, noise=noise, noise_is_pool=True)
    assert first["cloned"] > 100 and first["split_selected"] > 100 and first["total"] > N
    assert floaters_left(ref) == N_FLOAT
    outl = outlier_mask(ref.p["_xyz"], prob=0.8, neighbors=512)
    tests = ref.prune_mask(MIN_OPACITY, EXTENT, SIZE_THR)
    assert int(tests.sum()) >= 45 and int(outl.sum()) >= N_FLOAT
    M = ref.prune_points(outl | tests)
    assert_same_state(go, ref, "remove_outliers=True vs hand composition")
    assert info["outliers"] == int(outl.sum()) and info["total"] == M == go.N
    assert info["kept"] + info["cloned"] + info["split_children"] == M
    assert floaters_left(go) == 0, "planted floaters survived"
    assert go.replaced == ALL_GROUPS


def test_nothing_flagged_equals_the_flag_off(monkeypatch):
    """With the scores' threshold forced to 1 nothing is flagged (a score is at most 1), and the two-pass route must then
    give the one-pass result bit for bit: same rows, same order."""
    from manus_amd import optim
    noise = noise_pool()
    # the flag off, before the flag is exercised anywhere in this test: the existing path's own outputs
    before = make_optimizer()
    info_b = before.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, SIZE_THR, noise=noise, noise_is_pool=True)
    monkeypatch.setattr(optim, "OUTLIER_PROB", 1.0)
    go = make_optimizer()
    info = go.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, SIZE_THR, remove_outliers=True, noise=noise, noise_is_pool=True)
    assert info["outliers"] == 0
    assert_same_state(go, before, "threshold 1 vs remove_outliers=False")
    for key in ("kept", "cloned", "split_selected", "split_kept", "total"):
        assert info[key] == info_b[key], (key, info[key], info_b[key])
    assert info_b["kept"] < N - info_b["split_selected"] and floaters_left(before) == N_FLOAT      # the tests did prune; floaters stay
    # ... and the flag off after the flag was exercised gives the same bits again
    after = make_optimizer()
    info_a = after.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, SIZE_THR, remove_outliers=False, noise=noise, noise_is_pool=True)
    assert info_a == info_b and "outliers" not in info_a
    assert_same_state(after, before, "remove_outliers=False before vs after")


def test_density_update_reaches_the_outlier_path():
    noise = noise_pool()
    go = make_optimizer()
    stats = dict(grad2d=torch.zeros(N, device=DEV), vis=torch.zeros(N, device=DEV), radii=torch.zeros(N, dtype=torch.int32, device=DEV))
    assert go.density_update(stats, EXTENT, 200, bg_white=True, noise=noise, noise_is_pool=True)
    assert go.last_densify["outliers"] >= N_FLOAT and floaters_left(go) == 0
    ref = make_optimizer()
    ref.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, remove_outliers=True, noise=noise, noise_is_pool=True)
    assert_same_state(go, ref, "density_update at remove_outliers_step")
    other = make_optimizer()
    assert other.density_update(stats, EXTENT, 300, bg_white=True, noise=noise, noise_is_pool=True)
    assert "outliers" not in other.last_densify and floaters_left(other) == N_FLOAT


def test_reference_named_mask():
    from manus_amd.outliers import outlier_mask, update_mask_based_on_outliers
    x = make_optimizer().p["_xyz"]
    got = update_mask_based_on_outliers(x)
    assert got.dtype == torch.bool and got.is_cuda and got.shape == (N,)
    assert torch.equal(got, outlier_mask(x, prob=0.5, neighbors=128))
    assert got[N_BLOB:].all()

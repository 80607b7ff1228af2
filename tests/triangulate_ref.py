"""The checker of the robust multi-view triangulation (mgr_triangulate, csrc/triangulate.hip; `pose.triangulate_keypoints`,
`pose.KinematicPoseRefiner.triangulate`): the algorithm of the header comment above the entry as numpy, run whole in one dtype
(fp64 or fp32), and the committed inputs of the tests.

    active     s > (float)min_conf, finite target, both plane norms finite and > 0
    planes     a_u = t_x P2 - P0, a_v = t_y P2 - P1, each over the norm of its first three components -> (n, d)
    solve      N = sum w (n_u n_u^T + n_v n_v^T), b = -sum w (d_u n_u + d_v n_v), accepted iff det N > det_min (tr N / 3)^3
    inlier     active, q2 > z_min, |q[:2] / q2 - t| < tau
    seed       pairs a < b of active cameras in lexicographic order, the first accepted pair with the most inliers
    refit      refit_rounds times X = solve(inliers(X), s); then S = inliers(X), the final set
    polish     gn_iters Gauss-Newton steps on sum_S s |u(X) - t|^2 over the fixed S

The kernel forms planes, seed and classifications in fp32 and the refit's and polish's products and sums in fp64; this
restatement is one dtype throughout, so its fp32 run is the coarser of the two.  Tolerance of the GPU tests: `check_rows`,
e_kernel <= 8 * max(e32, 2^-23) against the fp64 run, e32 the fp32 run's own error.  The decisions (active, accepted, inlier,
the seed) are discontinuous: `test_triangulate_cpu.py` asserts on the fixtures the margins that make the fp32 kernel decide as
the fp64 run does.  The thresholds enter both runs through fp32, as they enter the kernel.

Parity with the reference's `batch_triangulate` is unpinned: its module imports `easymocap`, which this project does not carry."""
import functools
import math

import numpy as np
import torch

DEFAULTS = dict(tau=25.0, min_conf=0.1, min_views=3, z_min=1e-2, det_min=1e-6, refit_rounds=2, gn_iters=2)
F32, F64 = np.float32, np.float64


def _solve(N, b, det_min):
    """N (...,6) = N00 N01 N02 N11 N12 N22, b (...,3) -> accepted (...), X (...,3), ratio det / m^3 (...)."""
    dt = N.dtype.type
    n0, n1, n2, n3, n4, n5 = (N[..., i] for i in range(6))
    with np.errstate(all="ignore"):
        c00, c01, c02 = n3 * n5 - n4 * n4, n2 * n4 - n1 * n5, n1 * n4 - n2 * n3
        c11, c12, c22 = n0 * n5 - n2 * n2, n1 * n2 - n0 * n4, n0 * n3 - n1 * n1
        det = (n0 * c00 + n1 * c01) + n2 * c02
        m = ((n0 + n3) + n5) / dt(3)
        m3 = (m * m) * m
        ok = det > dt(det_min) * m3
        X = np.stack([((c00 * b[..., 0] + c01 * b[..., 1]) + c02 * b[..., 2]) / det,
                      ((c01 * b[..., 0] + c11 * b[..., 1]) + c12 * b[..., 2]) / det,
                      ((c02 * b[..., 0] + c12 * b[..., 1]) + c22 * b[..., 2]) / det], -1)
        ratio = det / m3
    assert X.dtype == N.dtype
    return ok, X, ratio


def _view(P, t, X):
    """Cameras P (C,3,4), targets t (C,2) at X (...,3) -> q2 (...,C), u (...,C,2), r (...,C,2), d (...,C)."""
    Xe = X[..., None, :]
    with np.errstate(all="ignore"):
        q = [((P[:, i, 0] * Xe[..., 0] + P[:, i, 1] * Xe[..., 1]) + P[:, i, 2] * Xe[..., 2]) + P[:, i, 3] for i in range(3)]
        u = np.stack([q[0] / q[2], q[1] / q[2]], -1)
        r = u - t
        d = np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1])
    return q[2], u, r, d


def _sym(a, b):
    """(C,3), (C,3) -> (C,6): a_i a_j + b_i b_j over (00, 01, 02, 11, 12, 22)."""
    ij = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return np.stack([a[:, i] * a[:, j] + b[:, i] * b[:, j] for i, j in ij], -1)


def _sum(terms, S):
    """Sequential sum over the cameras of S in ascending order, in the terms' dtype."""
    return np.cumsum(terms[S], 0)[-1]


def problem(P, t, s, dtype=F64, seed=None, light=False, **par):
    """One (frame, keypoint) problem: P (C,3,4), t (C,2), s (C,) -> dict(valid, X (3,), S (C,) bool, n, conf, dist (C,), active,
    pairs (n,2), counts (n,) with -1 for a pair not accepted, points (n,3) and sets (n, bits of C) the pairs' X_ab and inliers(X_ab),
    seed (index into pairs), rounds: the classified distances (NaN
    where not active and in front) of every refit round and of the final set, ratios: det / m^3 of every pair's solve).
    `seed`: start from that pair index instead of the best one.  `light`: the lists of the pairs are left out."""
    par = dict(DEFAULTS, **par)
    dt = dtype
    C = P.shape[0]
    tau, zmin, minconf, detmin32 = (dt(F32(par[k])) for k in ("tau", "z_min", "min_conf", "det_min"))
    detmin = dt(par["det_min"])
    P, t = P.astype(dt), t.astype(dt)
    s32 = s.astype(F32)
    out = dict(valid=False, X=np.full(3, np.nan, dt), S=np.zeros(C, bool), n=0, conf=dt(0), dist=np.full(C, np.nan, dt), pairs=np.zeros((0, 2), int),
               counts=np.zeros(0, int), seed=-1, rounds=[], ratios=np.zeros(0, dt))
    with np.errstate(all="ignore"):
        active = (s32 > F32(par["min_conf"])) & np.isfinite(t).all(1)
        au, av = t[:, 0:1] * P[:, 2] - P[:, 0], t[:, 1:2] * P[:, 2] - P[:, 1]
        lu = np.sqrt((au[:, 0] * au[:, 0] + au[:, 1] * au[:, 1]) + au[:, 2] * au[:, 2])
        lv = np.sqrt((av[:, 0] * av[:, 0] + av[:, 1] * av[:, 1]) + av[:, 2] * av[:, 2])
        active &= np.isfinite(lu) & (lu > 0) & np.isfinite(lv) & (lv > 0)
        zero = lambda x: np.where(active.reshape((C,) + (1,) * (x.ndim - 1)), x, dt(0)).astype(dt)
        nu, nv, du, dv = zero(au[:, :3] / lu[:, None]), zero(av[:, :3] / lv[:, None]), zero(au[:, 3] / lu), zero(av[:, 3] / lv)
    s, t = zero(s.astype(dt)), zero(t)
    out["active"] = active
    M, m = _sym(nu, nv), -(du[:, None] * nu + dv[:, None] * nv)
    idx = np.flatnonzero(active)
    if len(idx) < 2:
        return out
    ia, ib = np.triu_indices(len(idx), 1)
    A, B = idx[ia], idx[ib]
    ok, Xp, ratio = _solve(M[A] + M[B], m[A] + m[B], detmin32)
    q2, _, _, d = _view(P, t, Xp)
    front = active & (q2 > zmin)
    rows = np.arange(len(A))
    accepted = ok & front[rows, A] & front[rows, B]
    sets = front & (d < tau)
    counts = sets.sum(1)
    counts[~accepted] = -1
    if not light:
        out.update(pairs=np.stack([A, B], 1), counts=counts, ratios=ratio, points=Xp, sets=np.packbits(sets, 1))
    if not accepted.any():
        return out
    out["seed"] = int(np.argmax(counts)) if seed is None else int(seed)
    assert counts[out["seed"]] >= 0
    return _from_seed(out, P, t, s, M, m, active, Xp[out["seed"]], par)


def from_point(p, P, X, **par):
    """The refit and the polish of problem `p` (a dict of `problem`, run with the same P and keywords, that reached its seed)
    started from the point X in place of that seed -> a dict as `problem` gives, without the lists of the pairs."""
    par = dict(DEFAULTS, **par)
    dt = p["X"].dtype.type
    C = P.shape[0]
    out = dict(valid=False, X=np.full(3, np.nan, dt), S=np.zeros(C, bool), n=0, conf=dt(0), dist=np.full(C, np.nan, dt), rounds=[])
    return _from_seed(out, P.astype(dt), *p["tables"], np.asarray(X, dt), par)


def _from_seed(out, P, t, s, M, m, active, X, par):
    dt = P.dtype.type
    tau, zmin = dt(F32(par["tau"])), dt(F32(par["z_min"]))
    detmin = dt(par["det_min"])
    out["tables"] = (t, s, M, m, active)

    def classify(X):
        q2, u, r, d = _view(P, t, X)
        front = active & (q2 > zmin)
        out["rounds"].append(np.where(front, d, dt(np.nan)))
        return front & (d < tau), (q2, u, r, d, front)
    for _ in range(par["refit_rounds"]):
        S, _ = classify(X)
        if S.sum() < 2:
            return out
        ok, X, _ = _solve(_sum(s[:, None] * M, S), _sum(s[:, None] * m, S), detmin)
        if not ok:
            return out
    S, _ = classify(X)
    n = int(S.sum())
    if n < par["min_views"]:
        return out
    for _ in range(par["gn_iters"]):
        q2, u, r, d = _view(P, t, X)
        with np.errstate(all="ignore"):
            J0 = (P[:, 0, :3] - u[:, 0:1] * P[:, 2, :3]) / q2[:, None]
            J1 = (P[:, 1, :3] - u[:, 1:2] * P[:, 2, :3]) / q2[:, None]
            H = _sum(s[:, None] * _sym(J0, J1), S)
            g = _sum(s[:, None] * (J0 * r[:, 0:1] + J1 * r[:, 1:2]), S)
        ok, e, _ = _solve(H, g, detmin)
        if not ok:
            break
        X = X - e
    q2, _, _, d = _view(P, t, X)
    out.update(valid=True, X=X, S=S, n=n, conf=_sum(s, S) / dt(n), dist=np.where(active & (q2 > zmin), d, dt(np.nan)))
    assert X.dtype == dt and out["dist"].dtype == dt
    return out


def triangulate(proj, targets, weights, dtype=F64, detail=False, **par):
    """proj (C,3,4), targets (F,C,K,2), weights (F,C,K) -> dict(xyz (F,K,3), conf (F,K), n_inliers (F,K) int32, inliers (F,C,K) bool,
    dist (F,C,K)) in `dtype`; with `detail` also problems[f][k], the dicts of `problem`."""
    proj, targets, weights = (np.asarray(x) for x in (proj, targets, weights))
    F, C, K = weights.shape
    assert proj.shape == (C, 3, 4) and targets.shape == (F, C, K, 2)
    res = dict(xyz=np.full((F, K, 3), np.nan, dtype), conf=np.zeros((F, K), dtype), n_inliers=np.zeros((F, K), np.int32),
               inliers=np.zeros((F, C, K), bool), dist=np.full((F, C, K), np.nan, dtype), problems=[])
    for f in range(F):
        res["problems"].append([])
        for k in range(K):
            p = problem(proj, targets[f, :, k], weights[f, :, k], dtype, light=not detail, **par)
            res["xyz"][f, k], res["conf"][f, k], res["n_inliers"][f, k] = p["X"], p["conf"], p["n"]
            res["inliers"][f, :, k], res["dist"][f, :, k] = p["S"], p["dist"]
            res["problems"][f].append(p)
    if not detail:
        del res["problems"]
    return res


def reprojection_gradient(P, t, s, S, X):
    """The Gauss-Newton gradient g = sum_S s J^T r at X in fp64 and the value E = sum_S s |r|^2 / 2 it is the gradient of."""
    P, t, s, X = (np.asarray(x, F64) for x in (P, t, s, X))
    q2, u, r, _ = _view(P, t, X)
    J0 = (P[:, 0, :3] - u[:, 0:1] * P[:, 2, :3]) / q2[:, None]
    J1 = (P[:, 1, :3] - u[:, 1:2] * P[:, 2, :3]) / q2[:, None]
    g = (s[:, None] * (J0 * r[:, 0:1] + J1 * r[:, 1:2]))[S].sum(0)
    return g, 0.5 * float((s * (r * r).sum(1))[S].sum())


# ------------------------------------------------------------------------------------------------------------------------------
# the fixtures: a ring of cameras looking at the origin, points planted inside a 0.2 m box
# ------------------------------------------------------------------------------------------------------------------------------
FOCAL, CENTRE = 500.0, (320.0, 240.0)
BOX = 0.2                      # the planted points lie in [-BOX / 2, BOX / 2]^3
NOISE, OUTLIER = 0.5, (80.0, 200.0)      # pixels: the inlier noise (uniform on a disc), the range of an outlier's displacement
# (C, F, K, seed): F * K = 1, 21 and 5 * 21 (the last two end in a partial workgroup of four problems)
SHAPES = [(2, 1, 1, 0), (3, 1, 21, 0), (8, 1, 1, 0), (8, 1, 21, 0), (8, 5, 21, 0), (53, 1, 21, 0), (64, 1, 21, 0), (53, 5, 21, 0)]
DEAD, RICH = 1, 8              # rigs of RICH cameras and more: camera DEAD is a copy of camera 0, camera C - 1 looks away
ROGUE, ROGUE_SHAPES = 4, [(53, 1, 21), (64, 1, 21)]      # the camera that is wrong in every problem, and the rigs that get one
CROWD = 16                     # rigs of CROWD cameras and more draw their outliers by rate, smaller ones plant one per problem


def _look_at(centre, axis):
    z = axis / np.linalg.norm(axis)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, -(R @ centre)[:, None]], 1)


def ring(C):
    """proj (C,3,4) float32 through `pose.projection_matrices`: cameras on a ring of radius 1 m around the origin at heights
    0.5 + 0.2 sin(3 phi), looking at the origin, focal 500, centre (320, 240).  With C >= 8 camera 1 is a copy of camera 0 (the
    degenerate pair) and camera C - 1 stands at (0.5, 0, 0.1) looking AWAY from the origin: every planted point is behind it."""
    from manus_amd.pose import projection_matrices
    ext = []
    for c in range(C):
        phi = 2.0 * math.pi * c / C
        pos = np.array([math.cos(phi), math.sin(phi), 0.5 + 0.2 * math.sin(3.0 * phi)])
        ext.append(_look_at(pos, -pos))
    if C >= RICH:
        ext[DEAD] = ext[0].copy()
        pos = np.array([0.5, 0.0, 0.1])
        ext[C - 1] = _look_at(pos, pos)
    Kin = np.array([[FOCAL, 0.0, CENTRE[0]], [0.0, FOCAL, CENTRE[1]], [0.0, 0.0, 1.0]])
    return projection_matrices(torch.tensor(np.repeat(Kin[None], C, 0)), torch.tensor(np.stack(ext))).numpy()


def project(proj, X):
    """(..., C, 2) fp64 pixels of the points X (...,3), nothing clipped."""
    P = np.asarray(proj, F64)
    q = np.einsum("cij,...j->...ci", P[:, :, :3], np.asarray(X, F64)) + P[:, :, 3]
    return q[..., :2] / q[..., 2:]


def fixture(C, F, K, seed=0, invalid=False, rogue=None):
    """-> dict(proj (C,3,4), targets (F,C,K,2), weights (F,C,K) float32; points (F,K,3) fp64; par: the entry's keywords; invalid:
    the (f, k) of the planted invalid problems by kind).

    Detections: the fp64 projection of the planted point plus noise uniform on a disc of 0.5 px; weights uniform in [0.3, 1].
    C = 2 runs with min_views = 2 and nothing else planted; C = 3 has one outlier in problem (0, K - 1) when K > 1 (two inliers
    are left: invalid by min_views).  Rigs of 8 cameras and more: a detection of a ring camera can be an outlier displaced by
    80 .. 200 px, or of a weight in [0, 0.08] < min_conf (a detector that saw nothing: its target is anywhere in the image) -- with 16
    cameras and more with probability 0.2 and 0.1 each; below, with six ring cameras, exactly one outlier per problem and one weak
    detection in every third problem, so that four inliers are left and a seed of one inlier less is still a set of inliers; camera 1, the copy of camera 0, has weight 0 throughout; the last camera, looking away,
    carries confident detections (the mirrored projections) of a point behind it; detection (0, 2, 0) is a NaN target with a
    positive weight.  `rogue` = c: camera c is an outlier in every problem, the others of the ring keep their draw.
    `invalid`: on F * K >= 6 problems of a rig of 8 and more, in place of what the draw put there --
        few1   (0, 1): one active camera                           few2 (0, 2): two active cameras, both inliers: |S| = 2 < min_views
        twin   (0, 3): only cameras 0 and 1 active, on one detection: the pair's normal matrix has rank 2
        behind (0, 4): the point (0, 0, 5) is behind every camera of the ring; their detections confident and exact."""
    g = np.random.default_rng(7700 + 1000 * C + 10 * F + K + 100000 * seed)
    proj = ring(C)
    pts = (g.random((F, K, 3)) - 0.5) * BOX
    uv = np.moveaxis(project(proj, pts), 1, 2)                                                  # (F,K,C,2) -> (F,C,K,2)
    ang, rad = 2.0 * math.pi * g.random((F, C, K)), NOISE * np.sqrt(g.random((F, C, K)))
    t = uv + rad[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    s = 0.3 + 0.7 * g.random((F, C, K))
    par = dict(DEFAULTS)
    planted = {}
    oang, orad = 2.0 * math.pi * g.random((F, C, K)), OUTLIER[0] + (OUTLIER[1] - OUTLIER[0]) * g.random((F, C, K))
    shift = orad[..., None] * np.stack([np.cos(oang), np.sin(oang)], -1)
    draw, low, anywhere = g.random((F, C, K)), 0.08 * g.random((F, C, K)), g.random((F, C, K, 2)) * np.array([640.0, 480.0])
    if C == 2:
        par["min_views"] = 2
    elif C < RICH:
        if K > 1:
            t[0, 0, K - 1] += shift[0, 0, K - 1]
    else:
        ringc = np.ones(C, bool)
        ringc[[DEAD, C - 1]] = False
        if C >= CROWD:
            out = (draw < 0.2) & ringc[None, :, None]
            weak = (draw >= 0.2) & (draw < 0.3) & ringc[None, :, None]
        else:                # six ring cameras: exactly one outlier per problem, one weak detection in every third problem
            order = np.argsort(np.where(ringc[None, :, None], draw, 2.0), 1)                    # (F,C,K): ring cameras first, in drawn order
            out, weak = np.zeros((F, C, K), bool), np.zeros((F, C, K), bool)
            ff, kk = np.meshgrid(np.arange(F), np.arange(K), indexing="ij")
            out[ff, order[:, 0], kk] = True
            third = (ff * K + kk) % 3 == 1
            weak[ff[third], order[:, 1][third], kk[third]] = True
        if rogue is not None:
            out[:, rogue] = True
            weak[:, rogue] = False
        t[out] += shift[out]
        t[weak], s[weak] = anywhere[weak], low[weak]
        s[:, DEAD] = 0.0
        t[0, 2, 0], s[0, 2, 0] = np.nan, 0.9
        if invalid:
            assert F * K >= 6 and K >= 5
            clean = uv + rad[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)
            s[0, :, 1] = 0.0
            s[0, 3, 1] = 0.9
            s[0, :, 2], t[0, :, 2] = 0.0, clean[0, :, 2]
            s[0, [3, 5], 2] = 0.9
            s[0, :, 3] = 0.0
            s[0, [0, DEAD], 3], t[0, DEAD, 3] = 0.9, t[0, 0, 3]
            t[0, :, 4], s[0, :, 4] = project(proj, np.array([0.0, 0.0, 5.0])), 0.9
            s[0, C - 1, 4] = 0.0
            planted = dict(few1=(0, 1), few2=(0, 2), twin=(0, 3), behind=(0, 4))
    return dict(C=C, F=F, K=K, proj=proj, targets=t.astype(F32), weights=s.astype(F32), points=pts, par=par, invalid=planted)


@functools.lru_cache(maxsize=None)
def case(C, F, K, seed=0, invalid=False, rogue=None):
    """`fixture` of these arguments: computed once, shared, left unchanged."""
    return fixture(C, F, K, seed, invalid, rogue)


@functools.lru_cache(maxsize=None)
def reference(C, F, K, seed=0, invalid=False, rogue=None, refit_rounds=None, gn_iters=None):
    """(fp64 run, fp32 run) of `triangulate` with `detail` on `case(...)`, with the case's keywords and, where given, another
    refit_rounds / gn_iters: computed once, shared, left unchanged."""
    fx = case(C, F, K, seed, invalid, rogue)
    par = dict(fx["par"])
    par.update({k: v for k, v in (("refit_rounds", refit_rounds), ("gn_iters", gn_iters)) if v is not None})
    return tuple(triangulate(fx["proj"], fx["targets"], fx["weights"], dt, detail=True, **par) for dt in (F64, F32))


# ------------------------------------------------------------------------------------------------------------------------------
# the refiner fixture: the golden hand seen by 8 cameras, detections only
# ------------------------------------------------------------------------------------------------------------------------------
HAND = dict(frames=4, cameras=8, steps=200, lr_rot=0.05, lr_trans=0.01, delta=5.0, w_kp=10.0, w_kp2d=0.01, rot_off=0.6, trans_off=0.25)


@functools.lru_cache(maxsize=None)
def hand_inputs():
    """`fk_terms_ref.recovery_inputs()`'s golden hand (K = 21, both global rows free) on 4 frames with theta0 = 0; theta_true = mask *
    0.3 uniform(+-1) on the fingers, a global rotation of 0.6 rad about a drawn axis and a global translation of 0.25 m along another.
    8 cameras on a sphere of four hand radii around the keypoints at theta_true; detections = the fp64 projections plus 0.5 px
    of noise, weights uniform in [0.5, 1]; in frame f cameras f and f + 3 are wrong about EVERY keypoint by 80 .. 200 px.  No 3-D
    target is given: `kp_target` / `kp_weight` are absent until a triangulation supplies them."""
    import fk_chain_ref as R
    import fk_kp2d_ref as K2
    import fk_terms_ref as T
    from manus_amd.pose import dof_mask, keypoint_offsets, project_keypoints, projection_matrices
    cfg = HAND
    d = np.load(R.GOLDEN)
    parents = [int(p) for p in d["parents"]]
    rest = torch.tensor(d["world_rest_matrixs"], dtype=torch.float64)
    J, F, C = len(parents), cfg["frames"], cfg["cameras"]
    bones, offsets = keypoint_offsets(rest, d["world_rest_heads"], d["world_rest_tails"])
    mask = dof_mask(["bone_%d" % i for i in range(J)], True, True).double()
    g = torch.Generator().manual_seed(2525)
    uni = lambda *s: 2 * torch.rand(s, generator=g, dtype=torch.float64) - 1
    true = mask * 0.3 * uni(F, J + 2, 3)
    axis, along = torch.nn.functional.normalize(uni(F, 3), dim=1), torch.nn.functional.normalize(uni(F, 3), dim=1)
    true[:, 0], true[:, -1] = cfg["rot_off"] * axis, cfg["trans_off"] * along
    true = R.rounded(true * (mask != 0))
    base = torch.eye(4, dtype=torch.float64).repeat(F, 1, 1)
    K = J + 1
    p = T.keypoints_of(R.fk(true, rest, parents, base), bones.tolist(), offsets.double())
    centroid = p.reshape(-1, 3).mean(0)
    radius = float((p.reshape(-1, 3) - centroid).norm(dim=1).max())
    Kin = torch.tensor([[FOCAL, 0.0, CENTRE[0]], [0.0, FOCAL, CENTRE[1]], [0.0, 0.0, 1.0]], dtype=torch.float64)
    ext = torch.stack([K2.look_at(centroid + 4.0 * radius * v, -v) for v in K2.sphere(C, g)])
    proj = projection_matrices(Kin.repeat(C, 1, 1), ext).double()
    ang, rad = math.pi * uni(F, C, K), NOISE * torch.rand((F, C, K), generator=g, dtype=torch.float64).sqrt()
    t = project_keypoints(proj, p) + rad[..., None] * torch.stack([ang.cos(), ang.sin()], -1)
    oang, orad = math.pi * uni(F, C, K), OUTLIER[0] + (OUTLIER[1] - OUTLIER[0]) * torch.rand((F, C, K), generator=g, dtype=torch.float64)
    wrong = torch.zeros((F, C, K), dtype=torch.bool)
    for f in range(F):
        wrong[f, [f % C, (f + 3) % C]] = True
    t = t + wrong[..., None] * orad[..., None] * torch.stack([oang.cos(), oang.sin()], -1)
    s = 0.75 + 0.25 * uni(F, C, K)
    keys = [("take", f) for f in range(F)]
    return dict(case="hand8", J=J, F=F, K=K, C=C, parents=parents, rest=rest, base=base, theta=torch.zeros((F, J + 2, 3), dtype=torch.float64),
                theta_true=true, theta_ref=torch.zeros((F, J + 2, 3), dtype=torch.float64), mask=mask, kp_bone=bones.tolist(),
                kp_offset=offsets.double(), frame_keys=keys, neighbours=T.neighbours(keys), points=p, wrong=wrong, kp2d_proj=proj,
                kp2d_target=R.rounded(t), kp2d_weight=R.rounded(s), kp2d_delta=cfg["delta"], kp2d_zmin=DEFAULTS["z_min"])


def keypoint_error(fx, theta):
    """The mean distance (m) of the posed keypoints at theta from those at theta_true, in fp64."""
    import fk_chain_ref as R
    import fk_terms_ref as T
    p = T.keypoints_of(R.fk(theta.detach().cpu().double(), fx["rest"], fx["parents"], fx["base"]), fx["kp_bone"], fx["kp_offset"])
    return float((p - fx["points"]).norm(dim=-1).mean())


@functools.lru_cache(maxsize=None)
def hand_recovery():
    """The pipeline of `KinematicPoseRefiner.triangulate()` + `fit_keypoints` as a host fp64 loop on the restatements: `triangulate`
    (fp64) of the detections -> 3-D targets xyz with weights conf, 2-D weights times the inlier flags; then `fk_kp2d_ref.adam_loop`
    with w_kp and w_kp2d on from theta0 = 0.  -> dict(tri: the triangulation, fx: the inputs with the tables filled in, theta: the
    final angles, start / final: the mean keypoint error in m before and after).  Computed once, shared, left unchanged."""
    import fk_kp2d_ref as K2
    cfg = HAND
    fx = dict(hand_inputs())
    tri = triangulate(fx["kp2d_proj"].numpy(), fx["kp2d_target"].numpy(), fx["kp2d_weight"].numpy(), F64)
    fx["kp_target"], fx["kp_weight"] = torch.tensor(tri["xyz"]), torch.tensor(tri["conf"])
    fx["kp2d_weight"] = fx["kp2d_weight"] * torch.tensor(tri["inliers"]).double()
    w = dict(K2.ZERO, w_kp=cfg["w_kp"], w_kp2d=cfg["w_kp2d"])
    theta, _ = K2.adam_loop(fx, torch.float64, w, cfg["delta"], cfg["steps"], list(range(fx["F"])), cfg["lr_rot"], cfg["lr_trans"])
    return dict(tri=tri, fx=fx, theta=theta, start=keypoint_error(fx, fx["theta"]), final=keypoint_error(fx, theta))

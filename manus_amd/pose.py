"""Pose refinement on top of the pose gradient (`HipViewCompute(pose_grad=True)`, `ops.lbs_cov` with a differentiable
`transforms`): a per-frame, per-bone correction of the posed bone matrices and the chain rule from dL/d(bone transforms) back
to them.

Two forms of the same chain.  `PoseCorrection` / `pose_backward` are plain host torch on B small matrices under autograd: the
form the tests check against, and what validation and contact renders call.  `PoseRefiner` is the chain on the device (csrc/pose.hip: apply,
backward, row Adam; three launches per step -- four with priors on the corrections, whose value is folded by a launch of its own --,
no autograd graph, no read-back), which `engine.Trainer(pose=...)` schedules.

`KinematicPoseRefiner` has the same surface on another parametrisation: joint angles per frame through forward kinematics on
the device (csrc/fk.hip), 23 constrained angles for the hand (`dof_mask`), optionally a global rotation and translation, joint
limits (`joint_limits`).  Where the free-form correction can pull the skeleton apart at the joints, this one keeps bone lengths
and joint centres by construction.  `triangulate_keypoints` (csrc/triangulate.hip) is the input side of its keypoint terms: 2-D
detections of many cameras into 3-D keypoints with outlier rejection, on the device.

The reference's config/model/pose_optimizer.yaml names `src.models.pose_optimizer`, which was never released: the free-form
correction has no reference counterpart; the kinematic one follows that config's parametrisation and the host machinery of
src/utils/transforms.py (euler_angles_to_armature_space, apply_constraints_to_poses, apply_limits_to_poses)."""
import collections

import torch

from ._lib import MGR_FK_MAX_KEYPOINTS, MGR_MAX_BONES, check, lib, ptr, stream


def _exp_so3(r):
    """Rodrigues: (...,3) rotation vectors -> (...,3,3).  The exact identity at r = 0, differentiable there (series below
    |r|^2 = 1e-6, where they are exact to fp32 rounding)."""
    t2 = (r * r).sum(-1)
    small = t2 < 1e-6
    t2s = torch.where(small, torch.ones_like(t2), t2)
    th = torch.sqrt(t2s)
    a = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(th)) / t2s)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(r.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=r.dtype, device=r.device)
    return eye + a[..., None, None] * K + b[..., None, None] * (K @ K)


class PoseCorrection(torch.nn.Module):
    """rotvec (F,B,3) and trans (F,B,3), zero-initialised: frame f, bone b is corrected in the bone's local frame,
    posed_b @ [[exp(rotvec_b), trans_b], [0, 0, 0, 1]] -- the identity (bit for bit) at zero."""

    def __init__(self, n_frames, n_bones, dtype=torch.float32, device=None):
        super().__init__()
        self.rotvec = torch.nn.Parameter(torch.zeros((n_frames, n_bones, 3), dtype=dtype, device=device))
        self.trans = torch.nn.Parameter(torch.zeros((n_frames, n_bones, 3), dtype=dtype, device=device))

    def forward(self, posed, frame):
        """posed (B,4,4) of frame `frame` -> corrected (B,4,4)."""
        rv, tr = self.rotvec[frame], self.trans[frame]
        top = torch.cat([_exp_so3(rv), tr[..., None]], -1)                             # (B,3,4)
        last = torch.zeros((rv.shape[0], 1, 4), dtype=rv.dtype, device=rv.device)
        last[..., 3] = 1.0
        return posed @ torch.cat([top, last], -2).to(posed.dtype)


def pose_backward(d_transforms, posed, rest, background=True):
    """dL/dposed from dL/dT of T_b = posed_b @ inv(rest_b) (`transforms.bone_transforms`): d_posed_b = dT_b @ inv(rest_b)^T.
    d_transforms (...,B[+1],4,4) -- with `background` the last row is the identity transform's and is dropped; posed
    (...,B,4,4) gives the shape and dtype of the result, rest is (B,4,4).  A caller of the fused step, which has no autograd
    graph, finishes the chain with `corrected.backward(pose_backward(out["d_transforms"][k], corrected, rest))`."""
    dT = d_transforms[..., :-1, :, :] if background else d_transforms
    if dT.shape[-3:] != posed.shape[-3:]:
        raise ValueError("pose_backward: %s transforms for %s posed matrices" % (tuple(dT.shape), tuple(posed.shape)))
    inv_t = torch.linalg.inv(rest.to(device=dT.device, dtype=posed.dtype)).transpose(-1, -2)
    return dT.to(posed.dtype) @ inv_t


def neighbour_table(frame_keys, max_gap=None):
    """(F,2) int32 on the host: (prev, next) of every row of `frame_keys` along its take, -1 = none -- the edges of the
    smoothness prior of `PoseRefiner`.  The rows are the distinct (action, frame_id) pairs in first-seen order, as `PoseRefiner`
    numbers them.  Within an action the rows are ordered by int(frame_id) (equal numbers: first seen first) and rows adjacent in
    that order are neighbours, unless `max_gap` is given and their ids differ by more than it.  An action with an id that does
    not convert keeps its first-seen order, and `max_gap`, which has no numbers to compare there, does not cut it.  Rows of
    different actions are never neighbours."""
    keys = list(dict.fromkeys((k[0], k[1]) for k in frame_keys))
    if max_gap is not None and not float(max_gap) >= 0.0:
        raise ValueError("neighbour_table: max_gap must be None or >= 0 (got %r)" % (max_gap,))
    table = torch.full((len(keys), 2), -1, dtype=torch.int32)
    takes = {}
    for row, (action, _) in enumerate(keys):
        takes.setdefault(action, []).append(row)
    for rows in takes.values():
        try:
            ids = [int(keys[r][1]) for r in rows]
        except (TypeError, ValueError):
            ids = None
        if ids is not None:
            order = sorted(range(len(rows)), key=lambda j: ids[j])          # (stable: first seen first among equal ids)
            rows, ids = [rows[j] for j in order], [ids[j] for j in order]
        for j in range(len(rows) - 1):
            if ids is not None and max_gap is not None and ids[j + 1] - ids[j] > max_gap:
                continue
            table[rows[j], 1] = rows[j + 1]
            table[rows[j + 1], 0] = rows[j]
    return table


class _FrameRows:
    """What `PoseRefiner` and `KinematicPoseRefiner` share on the host: the rows of their tables are the distinct
    (action, frame_id) pairs of `frame_keys` in first-seen order, and the int32 lists of one step -- view rows, the frame of every
    view, the frames listed -- are built once per (view ids, frames) and cached on the device.  A subclass sets `frame_keys`,
    `row`, `n_frames`, `device` and an empty `_lists`."""

    @staticmethod
    def _keys(frame_keys):
        return list(dict.fromkeys((k[0], k[1]) for k in frame_keys))

    # -- host lists ------------------------------------------------------------------------------------------------------
    def frames_of(self, store, items):
        """The rows of the dataset items `items` of a `frames.FrameStore` built by `from_dataset`; -1 (no correction) for an
        item whose frame is not among `frame_keys`."""
        if getattr(store, "frame_keys", None) is None:
            raise ValueError("frames_of needs the frame keys of a store built by FrameStore.from_dataset")
        return [self.row.get(store.frame_keys[store.row[int(i)]], -1) for i in items]

    def _device_lists(self, view_ids, frames):
        """(view rows, frame of view, frames listed: int32 device tensors; the listed frames on the host) of one step.  The
        host drew the views, so the unique frames are listed here, ascending: nothing is read back from the device."""
        name = type(self).__name__
        key = (tuple(int(v) for v in view_ids), tuple(int(f) for f in frames))
        if len(key[0]) != len(key[1]) or not key[0]:
            raise ValueError("%s: one frame row per view, at least one view (got %d views, %d frames)" % (name, len(key[0]), len(key[1])))
        ent = self._lists.get(key)
        if ent is None:
            if any(f >= self.n_frames for f in key[1]):
                raise ValueError("%s: a frame row beyond the %d frames" % (name, self.n_frames))
            if min(key[0]) < 0:
                raise ValueError("%s: negative view id" % name)
            listed = sorted({f for f in key[1] if f >= 0})
            # the three lists in one host buffer and one copy (pinned and asynchronous where the host allows it): a shuffled
            # schedule brings a new key almost every step
            V, U = len(key[0]), len(listed)
            host = torch.tensor(list(key[0]) + list(key[1]) + listed, dtype=torch.int32)
            if self.device.type == "cuda":
                try:
                    host = host.pin_memory()
                except RuntimeError:
                    pass
            buf = host.to(self.device, non_blocking=True)
            ent = (buf[:V], buf[V:2 * V], buf[2 * V:] if U else None, listed, host)      # (host: alive until the copy has run)
            if len(self._lists) >= 256:
                self._lists.clear()
            self._lists[key] = ent
        return ent


class PoseRefiner(_FrameRows):
    """The correction tables of `PoseCorrection` -- rotvec and trans (F,B,3), zero at the start -- kept, applied, differentiated
    and stepped on the device (mgr_pose_apply / mgr_pose_backward / mgr_pose_adam).

    frame_keys: the (action, frame_id) pairs the rows stand for, e.g. those of `SequenceDataset.index_list` (its triples are
    accepted, the camera is ignored; repeats count once, in first-seen order).  rest (B,4,4): the rest matrices of the bones.
    The optimizer is the row Adam of `optim.SkinGridAdam` (torch.optim.SparseAdam's semantics: only the frames a step shows
    move, the bias correction uses the global count `steps`), with a rate each for rotations and translations and no clamp;
    the moments are allocated at the first step.

    Priors (all weights 0: none, today's two entries exactly).  For x = rotvec and x = trans, each with its own weights,
        E = w_mag sum_f |x_f|^2 + w_smooth sum_edges |x_f - x_next(f)|^2
    over the edges of `neighbour_table(frame_keys, max_gap)`: a pull towards zero and towards the neighbouring frames of the
    take.  With any weight non-zero `step` calls mgr_pose_backward_prior in place of mgr_pose_backward: the listed rows'
    gradient gains the true dE/dx_f, taken at the tables before the step (a listed neighbour's update is not seen; a neighbour
    that is not listed is read and stays), and `last_prior` is the part of E that touches the listed rows, each term once --
    a device double scalar, not read back.  The weights are configuration, not state: `state_dict()` does not carry them.

        frames = refiner.frames_of(store, items)             # one row per view, -1: no correction
        refiner.apply(compute, view_ids, frames)             # corrected transforms into the compute object's tables
        out = compute(view_ids, scale)                       # HipViewCompute(pose_grad=True)
        refiner.step(out["d_transforms"], view_ids, frames)

    `hold` is `apply` for a step that no `step` follows."""

    def __init__(self, frame_keys, n_bones, rest, lr_rot, lr_trans, betas=(0.9, 0.999), eps=1e-8, device=None, w_mag_rot=0.0,
                 w_smooth_rot=0.0, w_mag_trans=0.0, w_smooth_trans=0.0, max_gap=None):
        self.frame_keys = list(dict.fromkeys((k[0], k[1]) for k in frame_keys))
        self.row = {k: j for j, k in enumerate(self.frame_keys)}
        F, B = len(self.frame_keys), int(n_bones)
        if F < 1:
            raise ValueError("PoseRefiner needs at least one frame")
        if not 1 <= B <= MGR_MAX_BONES:
            raise ValueError("PoseRefiner: n_bones must be 1 .. %d (got %d)" % (MGR_MAX_BONES, B))
        rest = torch.as_tensor(rest)
        self.device = torch.device(device if device is not None else rest.device)
        if tuple(rest.shape) != (B, 4, 4):
            raise ValueError("PoseRefiner: rest must be (%d,4,4) (got %s)" % (B, tuple(rest.shape)))
        self.rest = rest.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.n_frames, self.n_bones = F, B
        self.lr_rot, self.lr_trans = float(lr_rot), float(lr_trans)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.rotvec = torch.zeros((F, B, 3), dtype=torch.float32, device=self.device)
        self.trans = torch.zeros((F, B, 3), dtype=torch.float32, device=self.device)
        self.m_r = self.v_r = self.m_t = self.v_t = None
        self.steps = 0
        self.last_grad = None           # (frames listed, d_rotvec (U,B,3), d_trans (U,B,3)) of the last step
        self.weights = tuple(float(w) for w in (w_mag_rot, w_smooth_rot, w_mag_trans, w_smooth_trans))
        for name, w in zip(("w_mag_rot", "w_smooth_rot", "w_mag_trans", "w_smooth_trans"), self.weights):
            if not (w >= 0.0 and w != float("inf")):
                raise ValueError("PoseRefiner: %s must be finite and >= 0 (got %r)" % (name, w))
        self.has_prior = any(w != 0.0 for w in self.weights)
        self.max_gap = max_gap
        self.neighbours = neighbour_table(self.frame_keys, max_gap).to(self.device)      # (F,2) int32: prev, next; -1 none
        self.last_prior = None          # with a prior: its value on the rows of the last step (device double scalar)
        self._prior_ws = None           # the per-thread shares of mgr_pose_backward_prior (kept across steps)
        self._posed = None              # the posed table of the compute object last applied to
        self._lists = {}                # (view ids, frames) -> their device lists

    # -- the three launches -----------------------------------------------------------------------------------------------
    def apply(self, compute, view_ids, frames):
        """Corrected bone transforms of the views `view_ids` (frame rows `frames`, -1: uncorrected) from `compute.s["posed"]`
        into `compute.s["transforms"]`, and into the gathered copy of that view set when the compute object holds one; then
        `compute.transforms_changed()`.  Rows of other views stay as they are."""
        s, B = compute.s, self.n_bones
        posed, tfm = s.get("posed"), s.get("transforms")
        if not torch.is_tensor(posed) or not torch.is_tensor(tfm):
            raise ValueError("PoseRefiner.apply: the scene holds no posed / transforms tables")
        n_all = tfm.shape[0]
        if tuple(posed.shape) != (n_all, B, 4, 4) or tuple(tfm.shape) != (n_all, B + 1, 4, 4) or posed.dtype != torch.float32 \
                or tfm.dtype != torch.float32:
            raise ValueError("PoseRefiner.apply: posed %s / transforms %s are not the float32 tables (V,%d,4,4) / (V,%d,4,4)"
                             % (tuple(posed.shape), tuple(tfm.shape), B, B + 1))
        rows, fov = self._device_lists(view_ids, frames)[:2]
        if max(int(v) for v in view_ids) >= n_all:
            raise ValueError("PoseRefiner.apply: a view id beyond the %d views of the tables" % n_all)
        gathered = compute.gathered_transforms(view_ids)
        check(lib().mgr_pose_apply(len(view_ids), B, self.n_frames, ptr(rows), ptr(fov), ptr(posed), ptr(self.rest), ptr(self.rotvec),
                                   ptr(self.trans), ptr(tfm), ptr(gathered), stream()), "mgr_pose_apply")
        self._posed = posed
        compute.transforms_changed(written=view_ids if gathered is not None else None)

    def hold(self, compute, view_ids, frames):
        """`apply` on a step at which the corrections do not move: the step's frames are rendered at their corrected
        transforms and no `step` follows."""
        self.apply(compute, view_ids, frames)

    def step(self, d_transforms, view_ids, frames):
        """One Adam step of the frames the views show, from the step's `out["d_transforms"]` (len(view_ids),B+1,4,4) at the
        transforms the last `apply` wrote.  Views with frame -1 contribute nothing; with no frame at all nothing happens.
        With a prior its gradient is added at the tables before the step and `last_prior` is its value on the listed rows."""
        if self._posed is None:
            raise ValueError("PoseRefiner.step before apply")
        B, V = self.n_bones, len(view_ids)
        if tuple(d_transforms.shape) != (V, B + 1, 4, 4) or d_transforms.dtype != torch.float32:
            raise ValueError("PoseRefiner.step: d_transforms %s is not float32 (%d,%d,4,4)" % (tuple(d_transforms.shape), V, B + 1))
        rows, fov, listed_t, listed = self._device_lists(view_ids, frames)[:4]
        if not listed:
            return
        U = len(listed)
        if self.m_r is None:
            self.m_r, self.v_r, self.m_t, self.v_t = (torch.zeros_like(self.rotvec) for _ in range(4))
        g_r = torch.empty((U, B, 3), dtype=torch.float32, device=self.device)
        g_t = torch.empty((U, B, 3), dtype=torch.float32, device=self.device)
        L = lib()
        if self.has_prior:
            nbytes = int(L.mgr_pose_prior_workspace_bytes(U, B))
            if self._prior_ws is None or self._prior_ws.numel() < nbytes:
                self._prior_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            value = torch.empty((), dtype=torch.float64, device=self.device)
            check(L.mgr_pose_backward_prior(V, B, self.n_frames, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(self._posed), ptr(self.rest),
                                            ptr(self.rotvec), ptr(self.trans), ptr(d_transforms), ptr(g_r), ptr(g_t), ptr(self.neighbours),
                                            *self.weights, ptr(value), ptr(self._prior_ws), self._prior_ws.numel(), stream()),
                  "mgr_pose_backward_prior")
            self.last_prior = value
        else:
            check(L.mgr_pose_backward(V, B, self.n_frames, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(self._posed), ptr(self.rest),
                                      ptr(self.rotvec), ptr(self.trans), ptr(d_transforms), ptr(g_r), ptr(g_t), stream()), "mgr_pose_backward")
        self.steps += 1
        check(L.mgr_pose_adam(U, B, ptr(listed_t), ptr(g_r), ptr(g_t), ptr(self.rotvec), ptr(self.trans), ptr(self.m_r), ptr(self.v_r),
                              ptr(self.m_t), ptr(self.v_t), self.lr_rot, self.lr_trans, self.betas[0], self.betas[1], self.eps, self.steps,
                              stream()), "mgr_pose_adam")
        self.last_grad = (listed, g_r, g_t)

    # -- state --------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return dict(frame_keys=list(self.frame_keys), steps=self.steps, rotvec=self.rotvec.clone(), trans=self.trans.clone(),
                    **{k: (getattr(self, k).clone() if getattr(self, k) is not None else None) for k in ("m_r", "v_r", "m_t", "v_t")})

    def load_state_dict(self, state):
        if [tuple(k) for k in state["frame_keys"]] != self.frame_keys:
            raise ValueError("PoseRefiner.load_state_dict: the state is of other frames")
        for k in ("rotvec", "trans"):
            if tuple(state[k].shape) != tuple(self.rotvec.shape):
                raise ValueError("PoseRefiner.load_state_dict: %s %s, expected %s" % (k, tuple(state[k].shape), tuple(self.rotvec.shape)))
            getattr(self, k).copy_(state[k])
        for k in ("m_r", "v_r", "m_t", "v_t"):
            t = state.get(k)
            setattr(self, k, None if t is None else t.detach().to(device=self.device, dtype=torch.float32).clone().contiguous())
        self.steps = int(state["steps"])

    def as_module(self):
        """A `PoseCorrection` on the SAME storage (its parameters see every later step): what validation and contact renders
        pose with, `module(posed, frame)`.  Just above the series threshold (|r|^2 in [1e-6, ~1e-5]) the module's fp32
        `_exp_so3` forms (1 - cos th) / th^2 with up to 2.7 % error where the kernel takes it from sin^2(th / 2): the two
        rotations differ by about 1e-8 there, the rounding of the host form, not another function."""
        m = PoseCorrection(self.n_frames, self.n_bones, device=self.device)
        m.rotvec = torch.nn.Parameter(self.rotvec, requires_grad=False)
        m.trans = torch.nn.Parameter(self.trans, requires_grad=False)
        return m


# ---------------------------------------------------------------------------------------------------------------------------
# Kinematic refinement: joint angles through forward kinematics (csrc/fk.hip)
# ---------------------------------------------------------------------------------------------------------------------------
LIMITS_XZ = ("bone_5", "bone_9", "bone_13", "bone_17")
LIMITS_X = ("bone_6", "bone_7", "bone_10", "bone_11", "bone_14", "bone_15", "bone_18", "bone_19")


def dof_mask(bnames, optimize_global_R=False, optimize_global_T=False):
    """(J+2,3) float32 of 0 / 1, the free entries of a `KinematicPoseRefiner`'s theta (row 0 the global angles, rows 1..J the
    bones, row J+1 the global translation), after the reference's apply_constraints_to_poses (src/utils/transforms.py:371-419):
    a bone in `dataset.DOF_XZ` frees its angles 0 and 2, a bone in `dataset.DOF_X` its angle 2 -- as the reference's code does,
    despite the name --, every other bone none: 23 ones for the hand's names (`num_pose_parameters: 23`).  The two flags of
    config/model/pose_optimizer.yaml free row 0 and row J+1."""
    from .dataset import DOF_X, DOF_XZ
    names = [str(n) for n in bnames]
    mask = torch.zeros((len(names) + 2, 3), dtype=torch.float32)
    for i, bn in enumerate(names):
        if bn in DOF_XZ:
            mask[1 + i, 0] = mask[1 + i, 2] = 1.0
        elif bn in DOF_X:
            mask[1 + i, 2] = 1.0
    if optimize_global_R:
        mask[0] = 1.0
    if optimize_global_T:
        mask[-1] = 1.0
    return mask


def joint_limits(bnames):
    """(lo, hi), each (J+2,3) float32: the explicit ranges of the reference's apply_limits_to_poses (src/utils/transforms.py:325-368)
    on the entries `dof_mask` frees -- bones 5 / 9 / 13 / 17: [-pi/6, pi/6] on angle 0 and [-pi/2, pi/9] on angle 2; its
    `limits_x` bones (6, 7, 10, 11, 14, 15, 18, 19): [-pi/2, 0] on angle 2 -- and +-pi on every other angle; the global
    translation (row J+1) has no limit (+-inf).  NOT reproduced: the reference's `else` branch clamps column i of the CONSTRAINED
    vector for a bone of INDEX i, i.e. it indexes the 23 free angles by bone index and so clamps entries that belong to other
    bones; here every bone without an explicit range simply keeps +-pi on its own angles."""
    import math
    names = [str(n) for n in bnames]
    J = len(names)
    lo = torch.full((J + 2, 3), -math.pi, dtype=torch.float32)
    hi = torch.full((J + 2, 3), math.pi, dtype=torch.float32)
    for i, bn in enumerate(names):
        if bn in LIMITS_XZ:
            lo[1 + i, 0], hi[1 + i, 0] = -math.pi / 6, math.pi / 6
            lo[1 + i, 2], hi[1 + i, 2] = -math.pi / 2, math.pi / 9
        elif bn in LIMITS_X:
            lo[1 + i, 2], hi[1 + i, 2] = -math.pi / 2, 0.0
    lo[-1], hi[-1] = -float("inf"), float("inf")
    return lo, hi


def theta_from_bones(bones_posed):
    """theta0 (F,J+2,3) float32 from a list of `bones_posed` records (one per frame row; `SequenceDataset` items carry them):
    row 0 = root_rotation, rows 1..J = eulers, row J+1 = root_translation."""
    rows = []
    for b in bones_posed:
        get = (lambda k: b[k]) if isinstance(b, dict) else (lambda k: getattr(b, k))
        e = torch.as_tensor(get("eulers"), dtype=torch.float32).reshape(-1, 3)
        g = torch.as_tensor(get("root_rotation"), dtype=torch.float32).reshape(1, 3)
        t = torch.as_tensor(get("root_translation"), dtype=torch.float32).reshape(1, 3)
        rows.append(torch.cat([g, e, t], 0))
    if not rows:
        raise ValueError("theta_from_bones: no frames")
    return torch.stack(rows)


def check_parents(parents, n_bones):
    """The kinematic tree as a list of ints, refused unless parents[i] is -1 (a root) or an index below i: the walk of
    `transforms.get_pose_wrt_root` and of csrc/fk.hip takes a parent before its children."""
    if isinstance(parents, dict):                        # `transforms.build_kintree`'s {str(i): parent}
        parents = [parents[str(i)] for i in range(len(parents))]
    parents = [int(p) for p in (parents.tolist() if hasattr(parents, "tolist") else parents)]
    if len(parents) != n_bones:
        raise ValueError("parents: %d entries for %d bones" % (len(parents), n_bones))
    for i, p in enumerate(parents):
        if not (p == -1 or 0 <= p < i):
            raise ValueError("parents[%d] = %d: a parent must be -1 or an index below its child's" % (i, p))
    return parents


def keypoint_offsets(rest, rest_heads, rest_tails):
    """(bones (K,) int32, offsets (K,3) float32) of the dataset's keypoint convention -- K = J+1: the first bone's head, then every
    bone's tail (`FrameStore.keypoints`) -- for `KinematicPoseRefiner.set_keypoints`: keypoints 0 and 1 ride on bone 0, keypoint
    k > 1 on bone k-1, and the offset is the rest point in its bone's own frame, inv(rest_b) [point; 1], formed in fp64."""
    rest = torch.as_tensor(rest).detach().cpu().double()
    heads, tails = (torch.as_tensor(x).detach().cpu().double() for x in (rest_heads, rest_tails))
    J = rest.shape[0] if rest.dim() == 3 else 0
    if J < 1 or tuple(rest.shape) != (J, 4, 4) or tuple(heads.shape) != (J, 3) or tuple(tails.shape) != (J, 3):
        raise ValueError("keypoint_offsets: rest (J,4,4), rest_heads (J,3), rest_tails (J,3) (got %s, %s, %s)"
                         % (tuple(rest.shape), tuple(heads.shape), tuple(tails.shape)))
    bones = [0] + list(range(J))
    points = torch.cat([heads[:1], tails], 0)
    hom = torch.cat([points, torch.ones((J + 1, 1), dtype=torch.float64)], 1)
    off = (torch.linalg.inv(rest)[bones] @ hom[..., None])[:, :3, 0]
    return torch.tensor(bones, dtype=torch.int32), off.to(torch.float32)


def keypoints_of_store(store, frame_keys):
    """(F,J+1,3) on the store's device: the 3-D keypoints of the frame rows of `frame_keys` (distinct (action, frame_id) pairs in
    first-seen order, as the refiners number them) from `FrameStore.keypoints` -- of every frame its first stored item (the
    keypoints do not depend on the camera).  Raises for a key the store lacks."""
    if getattr(store, "frame_keys", None) is None or getattr(store, "keypoints", None) is None:
        raise ValueError("keypoints_of_store needs the frame keys and keypoints of a store built by FrameStore.from_dataset")
    first = {}
    for j, k in enumerate(store.frame_keys):
        first.setdefault((k[0], k[1]), j)
    rows = []
    for k in _FrameRows._keys(frame_keys):
        if k not in first:
            raise ValueError("keypoints_of_store: the store holds no item of frame %r" % (k,))
        rows.append(first[k])
    return store.keypoints[rows]


def projection_matrices(K, extr):
    """P (C,3,4) float32 = K_c E_c[:3,:4], formed in fp64 on the host: intrinsics K (C,3,3), extrinsics extr (C,3,4) or (C,4,4)
    world to camera -- mgr_project_points' convention, q = K (E [x; 1]), pixel = q[:2] / q[2] -- for
    `KinematicPoseRefiner.set_keypoints_2d`."""
    K, E = (torch.as_tensor(x).detach().cpu().double() for x in (K, extr))
    C = K.shape[0] if K.dim() == 3 else 0
    if C < 1 or tuple(K.shape) != (C, 3, 3) or tuple(E.shape) not in ((C, 3, 4), (C, 4, 4)):
        raise ValueError("projection_matrices: K (C,3,3) and extr (C,3,4) or (C,4,4) (got %s, %s)" % (tuple(K.shape), tuple(E.shape)))
    return (K @ E[:, :3, :4]).to(torch.float32)


def project_keypoints(proj, xyz):
    """(...,C,K,2) float64 on the host: the points xyz (...,K,3) through the projections proj (C,3,4), u = q[:2] / q[2] with
    q = P_c [x; 1], in fp64.  Nothing is clipped: a point behind a camera comes out mirrored."""
    P, x = torch.as_tensor(proj).detach().cpu().double(), torch.as_tensor(xyz).detach().cpu().double()
    if P.dim() != 3 or tuple(P.shape[1:]) != (3, 4) or x.dim() < 2 or x.shape[-1] != 3:
        raise ValueError("project_keypoints: proj (C,3,4) and xyz (...,K,3) (got %s, %s)" % (tuple(P.shape), tuple(x.shape)))
    q = torch.einsum("cij,...kj->...cki", P[:, :, :3], x) + P[:, None, :, 3]
    return q[..., :2] / q[..., 2:]


Triangulation = collections.namedtuple("Triangulation", "xyz conf n_inliers inliers dist")
Triangulation.__doc__ = """What `triangulate_keypoints` returns, all on the device: xyz (F,K,3) float32 (NaN for an invalid problem), conf (F,K)
float32 (the mean weight of the inliers; 0 for an invalid problem), n_inliers (F,K) int32, inliers (F,C,K) bool -- the set the fit
used, classified before the polish --, dist (F,C,K) float32 -- the pixel distance at the final point, after the polish, NaN for
a camera that is not active or not in front."""


def triangulate_keypoints(proj, targets, weights=None, tau=25.0, min_conf=0.1, min_views=3, z_min=1e-2, det_min=1e-6, refit_rounds=2,
                          gn_iters=2, device=None):
    """Robust multi-view triangulation on the device (mgr_triangulate, csrc/triangulate.hip; the algorithm stands above the entry
    there): proj (C,3,4) (`projection_matrices`), targets (F,C,K,2), weights (F,C,K), (C,K), (K,) or None (ones) -- the layouts of
    `KinematicPoseRefiner.set_keypoints_2d` -- -> `Triangulation`.  Per (frame, keypoint): the pair of cameras whose triangulated
    point the most detections agree with to `tau` pixels seeds the set, `refit_rounds` weighted least-squares fits on the planes of
    the agreeing detections and `gn_iters` Gauss-Newton steps on their reprojection error follow.  A detection takes part only
    with a weight > `min_conf` and a finite target; a point needs `min_views` agreeing cameras, `z_min` in front of each.
    Deterministic; at most 64 cameras.  tau / min_conf / min_views default to what the reference's preprocess/scripts/keypoints_3d.py
    passes.  Tensors already on the device in float32 are used as they are; nothing is read back."""
    from ._lib import MGR_TRI_MAX_CAMERAS
    proj, targets = torch.as_tensor(proj), torch.as_tensor(targets)
    C = int(proj.shape[0]) if proj.dim() == 3 else 0
    if C < 1 or tuple(proj.shape) != (C, 3, 4):
        raise ValueError("triangulate_keypoints: proj must be (C,3,4) with C >= 1 (got %s)" % (tuple(proj.shape),))
    if C > MGR_TRI_MAX_CAMERAS:
        raise ValueError("triangulate_keypoints: at most %d cameras (got %d)" % (MGR_TRI_MAX_CAMERAS, C))
    if targets.dim() != 4 or targets.shape[1] != C or targets.shape[3] != 2 or targets.shape[0] < 1 or targets.shape[2] < 1:
        raise ValueError("triangulate_keypoints: targets must be (F,%d,K,2) with F, K >= 1 (got %s)" % (C, tuple(targets.shape)))
    F, K = int(targets.shape[0]), int(targets.shape[2])
    for name, x in (("tau", tau), ("z_min", z_min), ("det_min", det_min)):
        if not (float(x) > 0.0 and float(x) != float("inf")):
            raise ValueError("triangulate_keypoints: %s must be finite and > 0 (got %r)" % (name, x))
    if not (float(min_conf) >= 0.0 and float(min_conf) != float("inf")):
        raise ValueError("triangulate_keypoints: min_conf must be finite and >= 0 (got %r)" % (min_conf,))
    for name, x, lo in (("min_views", min_views, 2), ("refit_rounds", refit_rounds, 1), ("gn_iters", gn_iters, 0)):
        if int(x) != x or int(x) < lo:
            raise ValueError("triangulate_keypoints: %s must be an integer >= %d (got %r)" % (name, lo, x))
    if device is None:
        device = proj.device if proj.device.type == "cuda" else "cuda"
    device = torch.device(device)
    if weights is None:
        w = torch.ones((F, C, K), dtype=torch.float32, device=device)
    else:
        weights = torch.as_tensor(weights)
        if tuple(weights.shape) in ((K,), (C, K)):
            weights = weights.expand(F, C, K)
        if tuple(weights.shape) != (F, C, K):
            raise ValueError("triangulate_keypoints: weights must be (F,C,K), (C,K) or (K,) = %s (got %s)" % ((F, C, K), tuple(weights.shape)))
        w = weights.detach().to(device=device, dtype=torch.float32).contiguous()
    P = proj.detach().to(device=device, dtype=torch.float32).contiguous()
    t = targets.detach().to(device=device, dtype=torch.float32).contiguous()
    xyz = torch.empty((F, K, 3), dtype=torch.float32, device=device)
    conf = torch.empty((F, K), dtype=torch.float32, device=device)
    n_inliers = torch.empty((F, K), dtype=torch.int32, device=device)
    inliers = torch.empty((F, C, K), dtype=torch.uint8, device=device)
    dist = torch.empty((F, C, K), dtype=torch.float32, device=device)
    check(lib().mgr_triangulate(F, C, K, ptr(P), ptr(t), ptr(w), float(tau), float(min_conf), int(min_views), float(z_min), float(det_min),
                                int(refit_rounds), int(gn_iters), ptr(xyz), ptr(conf), ptr(n_inliers), ptr(inliers), ptr(dist), stream()),
          "mgr_triangulate")
    return Triangulation(xyz, conf, n_inliers, inliers.view(torch.bool), dist)


class KinematicPoseRefiner(_FrameRows):
    """Pose refinement in joint angles: theta (F,J+2,3) per frame row -- row 0 the global Euler angles, rows 1..J the bones'
    Euler angles (XYZ intrinsic, `transforms.euler_angles_to_matrix`), row J+1 the global translation -- through forward
    kinematics on the device (mgr_fk_apply / mgr_fk_backward / mgr_fk_adam, include/manus_hip.h), with `PoseRefiner`'s surface,
    so `engine.Trainer(pose=...)` schedules it unchanged.  Bone lengths and joint centres are fixed by construction: only
    the entries `mask` frees move, and they stay inside `limits`.

    frame_keys as for `PoseRefiner`; rest (J,4,4); parents: J ints, -1 or an index below the child's (several roots allowed;
    `transforms.build_kintree`'s dict is accepted); theta0 (F,J+2,3), e.g. `theta_from_bones`; mask (J+2,3) of 0 / 1 (None: all
    free), e.g. `dof_mask(bnames)`; limits = (lo, hi), each (J+2,3) (None: none), e.g. `joint_limits(bnames)`; base (F,4,4): a
    fixed left transform per frame from armature to world (None: identity; `fit_base` computes it from a dataset's matrices).
    The constants local_i = inv(rest_parent(i)) rest_i are formed in fp64 on the host.  The optimizer is `PoseRefiner`'s row
    Adam with a clamp to the limits behind it.  mask, limits, base and the rates are configuration, not state.

    Terms on the angles (all five weights 0: none, today's two entries exactly), per frame row over the free elements:
        E_dev    = sum_f w_dev |theta_f - theta_ref_f|^2                 a pull towards a kept table: theta0 until `set_reference`
        E_smooth = sum_edges w_smooth |theta_f - theta_next(f)|^2        over `neighbour_table(frame_keys, max_gap)`, no angle wrap
        E_kp     = w_kp sum_f sum_k c[f,k] |p_k(theta_f) - y[f,k]|^2     p_k = M_bone[k] [o_k; 1]: 3-D keypoints (`set_keypoints`)
    with a weight each for the rotations (rows 0..J) and the translation (row J+1).  With any weight non-zero `step` calls
    mgr_fk_backward_terms in place of mgr_fk_backward: the listed rows' gradient gains the true dE/dtheta_f at the tables before
    the step; `last_terms` is the (4,) device double (E_dev, E_smooth, E_kp, their sum) of the part that touches the listed
    rows, each term once, and `last_prior` a view of its last element -- neither is read back.  `fit_keypoints` runs the terms
    alone, without a rendered frame.  Weights, theta_ref and keypoints are configuration, not state: `state_dict()` does not
    carry them.

    A fourth term, also opt-in (w_kp2d = 0: none of it is run), fits the same keypoints to 2-D detections of C cameras:
        E_kp2d   = w_kp2d sum_f sum_c sum_k s[f,c,k] rho(|P_c [p_k(theta_f); 1] dehomogenised - t[f,c,k]|)
    with rho the square, or Huber's function of radius `kp2d_delta` > 0 (`set_keypoints_2d`; detections with a weight not > 0 or
    nearer than `kp2d_zmin` in front of their camera are skipped).  With w_kp2d non-zero `step` and `fit_keypoints` call
    mgr_fk_backward_terms2d; `last_terms` / `last_prior` then include the term and `last_kp2d` is its own value, all three views of
    one (5,) device double.  `reprojection_error` returns the per-detection pixel distances.

        refiner.residual(compute, view_ids, frames)          # does FK at theta0 reproduce the dataset's posed matrices?
        refiner.apply(compute, view_ids, frames)             # as PoseRefiner: transforms of the step's views
        out = compute(view_ids, scale)
        refiner.step(out["d_transforms"], view_ids, frames)"""

    def __init__(self, frame_keys, rest, parents, theta0, lr_rot, lr_trans, mask=None, limits=None, base=None, betas=(0.9, 0.999),
                 eps=1e-8, device=None, w_dev_rot=0.0, w_smooth_rot=0.0, w_dev_trans=0.0, w_smooth_trans=0.0, max_gap=None, w_kp=0.0,
                 w_kp2d=0.0, kp2d_delta=0.0, kp2d_zmin=1e-2):
        self.frame_keys = self._keys(frame_keys)
        self.row = {k: j for j, k in enumerate(self.frame_keys)}
        rest = torch.as_tensor(rest)
        F, J = len(self.frame_keys), int(rest.shape[0]) if rest.dim() == 3 else 0
        if F < 1:
            raise ValueError("KinematicPoseRefiner needs at least one frame")
        if not 1 <= J <= MGR_MAX_BONES or tuple(rest.shape) != (J, 4, 4):
            raise ValueError("KinematicPoseRefiner: rest must be (J,4,4) with J 1 .. %d (got %s)" % (MGR_MAX_BONES, tuple(rest.shape)))
        self.parents_host = check_parents(parents, J)
        self.device = torch.device(device if device is not None else rest.device)
        self.n_frames, self.n_bones = F, J
        self.lr_rot, self.lr_trans = float(lr_rot), float(lr_trans)
        for name, lr in (("lr_rot", self.lr_rot), ("lr_trans", self.lr_trans)):
            if lr != lr or lr in (float("inf"), -float("inf")):
                raise ValueError("KinematicPoseRefiner: %s must be finite (got %r)" % (name, lr))
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)

        def table(x, shape, what):
            x = torch.as_tensor(x)
            if tuple(x.shape) != shape:
                raise ValueError("KinematicPoseRefiner: %s must be %s (got %s)" % (what, shape, tuple(x.shape)))
            return x.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()
        self.rest = table(rest, (J, 4, 4), "rest")
        self.theta = table(theta0, (F, J + 2, 3), "theta0")
        self.mask = table(torch.ones((J + 2, 3)) if mask is None else mask, (J + 2, 3), "mask")
        if bool(((self.mask != 0) & (self.mask != 1)).any()):
            raise ValueError("KinematicPoseRefiner: mask must hold 0 / 1 only")
        inf = torch.full((J + 2, 3), float("inf"))
        lo, hi = (-inf, inf) if limits is None else limits
        self.lo, self.hi = table(lo, (J + 2, 3), "limits[0]"), table(hi, (J + 2, 3), "limits[1]")
        if not bool((self.lo <= self.hi).all()):
            raise ValueError("KinematicPoseRefiner: limits need lo <= hi everywhere")
        self.base = table(torch.eye(4).repeat(F, 1, 1) if base is None else base, (F, 4, 4), "base")
        rest64 = rest.detach().cpu().double()
        inv64 = torch.linalg.inv(rest64)
        self.local64 = torch.stack([rest64[i] if p < 0 else inv64[p] @ rest64[i] for i, p in enumerate(self.parents_host)])
        self.local = self.local64.to(device=self.device, dtype=torch.float32).contiguous()
        self.parents = torch.tensor(self.parents_host, dtype=torch.int32, device=self.device)
        self.m = self.v = None
        self.steps = 0
        self.last_grad = None           # (frames listed, d_theta (U,J+2,3)) of the last step
        self.weights = tuple(float(w) for w in (w_dev_rot, w_smooth_rot, w_dev_trans, w_smooth_trans))
        self.w_kp = float(w_kp)
        for name, w in zip(("w_dev_rot", "w_smooth_rot", "w_dev_trans", "w_smooth_trans", "w_kp"), self.weights + (self.w_kp,)):
            if not (w >= 0.0 and w != float("inf")):
                raise ValueError("KinematicPoseRefiner: %s must be finite and >= 0 (got %r)" % (name, w))
        self.w_kp2d, self.kp2d_delta, self.kp2d_zmin = float(w_kp2d), float(kp2d_delta), float(kp2d_zmin)
        for name, w in (("w_kp2d", self.w_kp2d), ("kp2d_delta", self.kp2d_delta)):
            if not (w >= 0.0 and w != float("inf")):
                raise ValueError("KinematicPoseRefiner: %s must be finite and >= 0 (got %r)" % (name, w))
        if not (self.kp2d_zmin > 0.0 and self.kp2d_zmin != float("inf")):
            raise ValueError("KinematicPoseRefiner: kp2d_zmin must be finite and > 0 (got %r)" % self.kp2d_zmin)
        self.has_terms = any(w != 0.0 for w in self.weights) or self.w_kp != 0.0 or self.w_kp2d != 0.0
        self.max_gap = max_gap
        self.neighbours = neighbour_table(self.frame_keys, max_gap).to(self.device)      # (F,2) int32: prev, next; -1 none
        self.theta_ref = self.theta.clone()
        self.kp = None                  # (bones (K,) int32, offsets (K,3), targets (F,K,3), weights (F,K)) of `set_keypoints`
        self.last_prior = None          # with a term on: the terms' sum on the rows of the last step (device double scalar)
        self.last_terms = None          # with a term on: (E_dev, E_smooth, E_kp, sum) of the last step (device double (4,))
        self.kp2d = None                # (proj (C,3,4), targets (F,C,K,2), weights (F,C,K)) of `set_keypoints_2d`
        self._kp_geom = None            # (bones (K,) int32, offsets (K,3)) the two setters share, and the bones on the host
        self.last_kp2d = None           # with w_kp2d on: E_kp2d of the last step (device double scalar, a view beside last_terms)
        self._terms_ws = None           # the per-frame shares of mgr_fk_backward_terms (kept across steps)
        self._posed = None              # the posed table of the compute object last applied to
        self._lists = {}

    # -- configuration of the terms -------------------------------------------------------------------------------------
    def set_keypoints(self, bones, offsets, targets, weights=None):
        """The keypoints of E_kp: bones (K,) ints in [0,J), offsets (K,3) in the bones' own frames (`keypoint_offsets`), targets
        (F,K,3) per frame row (`keypoints_of_store`), weights (F,K), (K,) or None (ones); K <= 64.  A keypoint of a frame whose
        weight is not > 0 (zero, negative, NaN) is skipped, whatever its target holds."""
        F, J = self.n_frames, self.n_bones
        bones = torch.as_tensor(bones)
        K = int(bones.shape[0]) if bones.dim() == 1 else 0
        if not 1 <= K <= MGR_FK_MAX_KEYPOINTS:
            raise ValueError("KinematicPoseRefiner.set_keypoints: bones must be (K,) with K 1 .. %d (got %s)" % (MGR_FK_MAX_KEYPOINTS, tuple(bones.shape)))
        if bones.dtype.is_floating_point or bones.dtype == torch.bool:
            raise ValueError("KinematicPoseRefiner.set_keypoints: bones must be integers")
        host = [int(b) for b in bones.tolist()]
        if any(not 0 <= b < J for b in host):
            raise ValueError("KinematicPoseRefiner.set_keypoints: a bone outside [0,%d)" % J)

        def table(x, shape, what):
            x = torch.as_tensor(x)
            if tuple(x.shape) != shape:
                raise ValueError("KinematicPoseRefiner.set_keypoints: %s must be %s (got %s)" % (what, shape, tuple(x.shape)))
            return x.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()
        off, tgt = table(offsets, (K, 3), "offsets"), table(targets, (F, K, 3), "targets")
        if weights is None:
            w = torch.ones((F, K), dtype=torch.float32, device=self.device)
        else:
            weights = torch.as_tensor(weights)
            w = table(weights.expand(F, K) if tuple(weights.shape) == (K,) else weights, (F, K), "weights")
        if self.kp2d is not None:
            self._same_geometry("set_keypoints", host, off)
        self.kp = (torch.tensor(host, dtype=torch.int32, device=self.device), off, tgt, w)
        self._kp_geom = (self.kp[0], off, host)

    def _same_geometry(self, who, host, off):
        """Both setters name one set of keypoints: the same K, bones and offsets."""
        if self._kp_geom is not None and (host != self._kp_geom[2] or not torch.equal(off, self._kp_geom[1])):
            raise ValueError("KinematicPoseRefiner.%s: bones / offsets differ from those already set: the 3-D and the 2-D term share "
                             "one set of keypoints" % who)

    def set_keypoints_2d(self, proj, targets, weights=None, bones=None, offsets=None):
        """The detections of E_kp2d: proj (C,3,4), the cameras' projections (`projection_matrices`; pre-scale them and the targets
        to fit in another unit than pixels), targets (F,C,K,2) per frame row and camera, weights (F,C,K), (C,K), (K,) or None
        (ones): the detections' confidences.  A detection whose weight is not > 0 (zero, negative, NaN) is skipped, whatever its
        target holds -- store a missing detection as weight 0 with any target, NaN included.  bones (K,) / offsets (K,3) as for
        `set_keypoints`; needed only when `set_keypoints` has not set them, and when both are given they must be the same."""
        F, J = self.n_frames, self.n_bones
        if (bones is None) != (offsets is None):
            raise ValueError("KinematicPoseRefiner.set_keypoints_2d: give bones and offsets together")
        if bones is None and self._kp_geom is None:
            raise ValueError("KinematicPoseRefiner.set_keypoints_2d: bones and offsets are needed (set_keypoints has not set them)")

        def table(x, shape, what):
            x = torch.as_tensor(x)
            if tuple(x.shape) != shape:
                raise ValueError("KinematicPoseRefiner.set_keypoints_2d: %s must be %s (got %s)" % (what, shape, tuple(x.shape)))
            return x.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()
        if bones is not None:
            bones = torch.as_tensor(bones)
            K = int(bones.shape[0]) if bones.dim() == 1 else 0
            if not 1 <= K <= MGR_FK_MAX_KEYPOINTS:
                raise ValueError("KinematicPoseRefiner.set_keypoints_2d: bones must be (K,) with K 1 .. %d (got %s)"
                                 % (MGR_FK_MAX_KEYPOINTS, tuple(bones.shape)))
            if bones.dtype.is_floating_point or bones.dtype == torch.bool:
                raise ValueError("KinematicPoseRefiner.set_keypoints_2d: bones must be integers")
            host = [int(b) for b in bones.tolist()]
            if any(not 0 <= b < J for b in host):
                raise ValueError("KinematicPoseRefiner.set_keypoints_2d: a bone outside [0,%d)" % J)
            off = table(offsets, (K, 3), "offsets")
            self._same_geometry("set_keypoints_2d", host, off)
            geom = (torch.tensor(host, dtype=torch.int32, device=self.device), off, host) if self._kp_geom is None else self._kp_geom
        else:
            geom = self._kp_geom
        K = len(geom[2])
        proj = torch.as_tensor(proj)
        C = int(proj.shape[0]) if proj.dim() == 3 else 0
        if C < 1:
            raise ValueError("KinematicPoseRefiner.set_keypoints_2d: proj must be (C,3,4) with C >= 1 (got %s)" % (tuple(proj.shape),))
        P, tgt = table(proj, (C, 3, 4), "proj"), table(targets, (F, C, K, 2), "targets")
        if weights is None:
            w = torch.ones((F, C, K), dtype=torch.float32, device=self.device)
        else:
            weights = torch.as_tensor(weights)
            w = table(weights.expand(F, C, K) if tuple(weights.shape) in ((K,), (C, K)) else weights, (F, C, K), "weights")
        self._kp_geom, self.kp2d = geom, (P, tgt, w)

    def triangulate(self, set_3d=True, mask_2d=True, **kw):
        """`triangulate_keypoints` on the tables `set_keypoints_2d` stored (keywords: tau, min_conf, min_views, z_min, det_min,
        refit_rounds, gn_iters) -> its `Triangulation`.  The detections so feed both keypoint terms:
        set_3d: the triangulated points become E_kp's targets and their confidences its weights, on the shared bones and offsets
        -- what `set_keypoints(bones, offsets, xyz, conf)` stores; an invalid keypoint has weight 0 and a NaN target, which the
        term skips exactly;
        mask_2d: the stored 2-D weights are multiplied by `inliers`, so E_kp2d no longer sees a detection the consensus rejected
        (Huber's function only down-weights it).  Calling it again triangulates the masked weights.
        Nothing is read back."""
        if self.kp2d is None:
            raise ValueError("KinematicPoseRefiner.triangulate: no detections are set (set_keypoints_2d)")
        P, tgt, w = self.kp2d
        res = triangulate_keypoints(P, tgt, w, device=self.device, **kw)
        self._adopt(res, set_3d, mask_2d)
        return res

    def _adopt(self, res, set_3d, mask_2d):
        """The bookkeeping of `triangulate`: tensors of the tables' shapes on the refiner's device in, `kp` / `kp2d` replaced."""
        P, tgt, w = self.kp2d
        F, C, K = tuple(w.shape)
        if tuple(res.xyz.shape) != (F, K, 3) or tuple(res.conf.shape) != (F, K) or tuple(res.inliers.shape) != (F, C, K):
            raise ValueError("KinematicPoseRefiner.triangulate: the result is not of the stored detections' shape %s" % ((F, C, K),))
        if set_3d:
            self.kp = (self._kp_geom[0], self._kp_geom[1], res.xyz, res.conf)
        if mask_2d:
            self.kp2d = (P, tgt, w * res.inliers.to(w.dtype))

    def set_reference(self, theta=None):
        """Re-anchors E_dev: theta_ref = theta (F,J+2,3), by default the current table."""
        src = self.theta if theta is None else torch.as_tensor(theta)
        if tuple(src.shape) != tuple(self.theta.shape):
            raise ValueError("KinematicPoseRefiner.set_reference: theta must be %s (got %s)" % (tuple(self.theta.shape), tuple(src.shape)))
        self.theta_ref.copy_(src.detach().to(device=self.device, dtype=torch.float32))

    # -- host fp64 ----------------------------------------------------------------------------------------------------------
    def fk_host(self, theta=None, base=None):
        """M (F,J,4,4) in fp64 on the host from theta (default: the current table) and base (default: the refiner's): the
        reference's walk, `transforms.euler_angles_to_armature_space`, with base in front.  For set-up and checks, not the step."""
        from . import transforms as T
        theta = (self.theta if theta is None else torch.as_tensor(theta)).detach().cpu().double()
        base = (self.base if base is None else torch.as_tensor(base)).detach().cpu().double()
        J = self.n_bones
        tree = {str(i): p for i, p in enumerate(self.parents_host)}
        M = T.euler_angles_to_armature_space(theta[:, :J + 1], tree, self.rest.detach().cpu().double(), theta[:, J + 1])
        return base[:, None] @ M

    def fit_base(self, posed_table):
        """The per-frame transform that aligns FK at the current theta to a dataset's posed matrices `posed_table` (F,J,4,4),
        from the first root r: base_f = posed_table[f,r] inv(M_r) with M at base = identity, in fp64 on the host.  Sets `base`
        (fp32) and returns the fp64 table.  A dataset whose matrices live in world space while its angles are in armature
        space differs from FK by exactly such a transform per frame."""
        posed_table = torch.as_tensor(posed_table).detach().cpu().double()
        F, J = self.n_frames, self.n_bones
        if tuple(posed_table.shape) != (F, J, 4, 4):
            raise ValueError("fit_base: posed_table must be (%d,%d,4,4) (got %s)" % (F, J, tuple(posed_table.shape)))
        r = self.parents_host.index(-1)
        M = self.fk_host(base=torch.eye(4, dtype=torch.float64).repeat(F, 1, 1))
        base = posed_table[:, r] @ torch.linalg.inv(M[:, r])
        self.base.copy_(base.to(torch.float32))
        return base

    # -- the three launches -------------------------------------------------------------------------------------------------
    def _tables(self, compute):
        s, J = compute.s, self.n_bones
        posed, tfm = s.get("posed"), s.get("transforms")
        if not torch.is_tensor(posed) or not torch.is_tensor(tfm):
            raise ValueError("KinematicPoseRefiner: the scene holds no posed / transforms tables")
        n_all = tfm.shape[0]
        if tuple(posed.shape) != (n_all, J, 4, 4) or tuple(tfm.shape) != (n_all, J + 1, 4, 4) or posed.dtype != torch.float32 \
                or tfm.dtype != torch.float32:
            raise ValueError("KinematicPoseRefiner: posed %s / transforms %s are not the float32 tables (V,%d,4,4) / (V,%d,4,4)"
                             % (tuple(posed.shape), tuple(tfm.shape), J, J + 1))
        return posed, tfm, n_all

    def _fk_apply(self, V, rows, fov, posed, tfm, gathered, posed_out):
        check(lib().mgr_fk_apply(V, self.n_bones, self.n_frames, ptr(rows), ptr(fov), ptr(posed), ptr(self.rest), ptr(self.local),
                                 ptr(self.parents), ptr(self.base), ptr(self.theta), ptr(tfm), ptr(gathered), ptr(posed_out), stream()),
              "mgr_fk_apply")

    def apply(self, compute, view_ids, frames):
        """Bone transforms of the views `view_ids` (frame rows `frames`; -1: the dataset's own posed row, uncorrected) from
        theta into `compute.s["transforms"]`, and into the gathered copy of that view set when the compute object holds one;
        then `compute.transforms_changed()`.  Rows of other views stay as they are."""
        posed, tfm, n_all = self._tables(compute)
        rows, fov = self._device_lists(view_ids, frames)[:2]
        if max(int(v) for v in view_ids) >= n_all:
            raise ValueError("KinematicPoseRefiner.apply: a view id beyond the %d views of the tables" % n_all)
        gathered = compute.gathered_transforms(view_ids)
        self._fk_apply(len(view_ids), rows, fov, posed, tfm, gathered, None)
        self._posed = posed
        compute.transforms_changed(written=view_ids if gathered is not None else None)

    def hold(self, compute, view_ids, frames):
        """`apply` on a step at which the angles do not move."""
        self.apply(compute, view_ids, frames)

    def posed(self, view_ids, frames, compute=None):
        """The posed matrices M_i (len(view_ids),J,4,4) of FK at the current theta, one row per view; a view with frame -1 gets
        its row of the posed table of `compute` (default: of the compute object last applied to).  Nothing of the compute
        object is written."""
        V, J = len(view_ids), self.n_bones
        src = self._tables(compute)[0] if compute is not None else self._posed
        if src is None:
            if any(int(f) < 0 for f in frames):
                raise ValueError("KinematicPoseRefiner.posed: a view without a frame needs a compute object's posed table")
            sel = torch.zeros((V, J, 4, 4), dtype=torch.float32, device=self.device)
        else:
            if max(int(v) for v in view_ids) >= src.shape[0]:
                raise ValueError("KinematicPoseRefiner.posed: a view id beyond the %d views of the tables" % src.shape[0])
            sel = src[[int(v) for v in view_ids]].contiguous()
        rows, fov = self._device_lists(range(V), frames)[:2]
        tfm = torch.empty((V, J + 1, 4, 4), dtype=torch.float32, device=self.device)
        out = torch.empty((V, J, 4, 4), dtype=torch.float32, device=self.device)
        self._fk_apply(V, rows, fov, sel, tfm, None, out)
        return out

    def residual(self, compute, view_ids, frames):
        """max |M_i - compute.s["posed"]| over the views (a float; one read-back): how closely FK at the current theta -- at
        theta0, before any step -- reproduces the dataset's posed matrices.  Large: the dataset needs a `base` (`fit_base`)."""
        want = self._tables(compute)[0][[int(v) for v in view_ids]]
        return float((self.posed(view_ids, frames, compute=compute) - want).abs().max())

    def step(self, d_transforms, view_ids, frames):
        """One Adam step, then the clamp to the limits, of the free angles of the frames the views show, from the step's
        `out["d_transforms"]` (len(view_ids),J+1,4,4) at the transforms the last `apply` wrote.  Views with frame -1 contribute
        nothing; with no frame at all nothing happens."""
        if self._posed is None:
            raise ValueError("KinematicPoseRefiner.step before apply")
        J, V = self.n_bones, len(view_ids)
        if tuple(d_transforms.shape) != (V, J + 1, 4, 4) or d_transforms.dtype != torch.float32:
            raise ValueError("KinematicPoseRefiner.step: d_transforms %s is not float32 (%d,%d,4,4)" % (tuple(d_transforms.shape), V, J + 1))
        rows, fov, listed_t, listed = self._device_lists(view_ids, frames)[:4]
        if not listed:
            return
        U = len(listed)
        if self.m is None:
            self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        g = torch.empty((U, J + 2, 3), dtype=torch.float32, device=self.device)
        L = lib()
        if self.has_terms:
            self._backward_terms(V, U, listed_t, rows, fov, d_transforms, g)
        else:
            check(L.mgr_fk_backward(V, J, self.n_frames, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(self.rest), ptr(self.local), ptr(self.parents),
                                    ptr(self.base), ptr(self.theta), ptr(self.mask), ptr(d_transforms), ptr(g), stream()), "mgr_fk_backward")
        self.steps += 1
        check(L.mgr_fk_adam(U, J, ptr(listed_t), ptr(g), ptr(self.theta), ptr(self.m), ptr(self.v), ptr(self.mask), ptr(self.lo), ptr(self.hi),
                            self.lr_rot, self.lr_trans, self.betas[0], self.betas[1], self.eps, self.steps, stream()), "mgr_fk_adam")
        self.last_grad = (listed, g)

    def _backward_terms(self, V, U, listed_t, rows, fov, d_transforms, g):
        """mgr_fk_backward_terms into g (U,J+2,3) with the configured weights (d_transforms None: the terms alone); sets
        `last_terms` and `last_prior`."""
        J, L = self.n_bones, lib()
        if self.w_kp != 0.0 and self.kp is None:
            raise ValueError("KinematicPoseRefiner: w_kp is non-zero and no keypoints are set (set_keypoints)")
        if self.w_kp2d != 0.0:
            values = self._terms2d(V, U, listed_t, rows, fov, d_transforms, g, self.weights, self.w_kp, self.w_kp2d, None)
            self.last_terms, self.last_prior, self.last_kp2d = values[:4], values[3], values[4]
            return
        kp = self.kp if self.w_kp != 0.0 else (None, None, None, None)
        K = int(kp[0].shape[0]) if kp[0] is not None else 0
        nbytes = int(L.mgr_fk_terms_workspace_bytes(U, J, K))
        if self._terms_ws is None or self._terms_ws.numel() < nbytes:
            self._terms_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        values = torch.empty(4, dtype=torch.float64, device=self.device)
        check(L.mgr_fk_backward_terms(V, J, self.n_frames, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(self.rest), ptr(self.local),
                                      ptr(self.parents), ptr(self.base), ptr(self.theta), ptr(self.mask), ptr(d_transforms), ptr(g),
                                      ptr(self.theta_ref), ptr(self.neighbours), *self.weights, K, ptr(kp[0]), ptr(kp[1]), ptr(kp[2]),
                                      ptr(kp[3]), self.w_kp, ptr(values), ptr(self._terms_ws), self._terms_ws.numel(), stream()),
              "mgr_fk_backward_terms")
        self.last_terms, self.last_prior = values, values[3]

    def _terms2d(self, V, U, listed_t, rows, fov, d_transforms, g, weights, w_kp, w_kp2d, dist):
        """One call of mgr_fk_backward_terms2d into g (U,J+2,3) and dist ((U,C,K) or None) -> values (5,) device double."""
        J, L = self.n_bones, lib()
        if self.kp2d is None:
            raise ValueError("KinematicPoseRefiner: the 2-D keypoint term needs detections (set_keypoints_2d)")
        bones, off = self._kp_geom[:2]
        K, C = int(bones.shape[0]), int(self.kp2d[0].shape[0])
        tgt3, w3 = (self.kp[2], self.kp[3]) if w_kp != 0.0 else (None, None)
        nbytes = int(L.mgr_fk_terms2d_workspace_bytes(U, J, K, C))
        if self._terms_ws is None or self._terms_ws.numel() < nbytes:
            self._terms_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        values = torch.empty(5, dtype=torch.float64, device=self.device)
        check(L.mgr_fk_backward_terms2d(V, J, self.n_frames, U, ptr(listed_t), ptr(rows), ptr(fov), ptr(self.rest), ptr(self.local),
                                        ptr(self.parents), ptr(self.base), ptr(self.theta), ptr(self.mask), ptr(d_transforms), ptr(g),
                                        ptr(self.theta_ref), ptr(self.neighbours), *weights, K, ptr(bones), ptr(off), ptr(tgt3), ptr(w3),
                                        w_kp, C, ptr(self.kp2d[0]), ptr(self.kp2d[1]), ptr(self.kp2d[2]), w_kp2d, self.kp2d_delta,
                                        self.kp2d_zmin, ptr(dist), ptr(values), ptr(self._terms_ws), self._terms_ws.numel(), stream()),
              "mgr_fk_backward_terms2d")
        return values

    def reprojection_error(self, frames=None):
        """(U,C,K) device float32: the distances |P_c [p_k; 1] dehomogenised - t[f,c,k]| of the detections of `set_keypoints_2d` at
        the current angles, for the frame rows `frames` in the order given (default: all rows), NaN where a detection is skipped
        (weight not > 0, or not `kp2d_zmin` in front of its camera).  One call of mgr_fk_backward_terms2d with the 2-D term
        alone; its gradient goes to a scratch buffer: nothing is stepped, and `last_terms`, `last_prior`, `last_kp2d`, the moments
        and `steps` stay as they are.  Nothing is read back."""
        if self.kp2d is None:
            raise ValueError("KinematicPoseRefiner.reprojection_error: no detections are set (set_keypoints_2d)")
        F, J = self.n_frames, self.n_bones
        listed = [int(f) for f in (range(F) if frames is None else frames)]
        if not listed or min(listed) < 0 or max(listed) >= F:
            raise ValueError("KinematicPoseRefiner.reprojection_error: frames must be rows in [0,%d), at least one" % F)
        U, C, K = len(listed), int(self.kp2d[0].shape[0]), int(self._kp_geom[0].shape[0])
        listed_t = torch.tensor(listed, dtype=torch.int32, device=self.device)
        g = torch.empty((U, J + 2, 3), dtype=torch.float32, device=self.device)
        dist = torch.empty((U, C, K), dtype=torch.float32, device=self.device)
        self._terms2d(0, U, listed_t, None, None, None, g, (0.0, 0.0, 0.0, 0.0), 0.0, self.w_kp2d if self.w_kp2d != 0.0 else 1.0, dist)
        return dist

    def fit_keypoints(self, steps, frames=None, lr_rot=None, lr_trans=None):
        """`steps` Adam steps of the terms alone -- mgr_fk_backward_terms (mgr_fk_backward_terms2d with w_kp2d on; the 2-D term alone
        is a fit to the cameras' detections) without d_transforms, then mgr_fk_adam -- on the frame
        rows `frames` (default: all), with the configured weights: the best constrained angles for the keypoints, found without
        rendering a frame.  lr_rot / lr_trans default to the refiner's.  The moments and the step count of this loop are its own:
        `m`, `v` and `steps` of training are untouched, only `theta` moves.  Nothing is read back; `last_terms` holds the values
        of the last iteration (at the angles before its step)."""
        if not self.has_terms:
            raise ValueError("KinematicPoseRefiner.fit_keypoints: every weight is zero")
        F, J = self.n_frames, self.n_bones
        listed = sorted({int(f) for f in (range(F) if frames is None else frames)})
        if not listed or listed[0] < 0 or listed[-1] >= F:
            raise ValueError("KinematicPoseRefiner.fit_keypoints: frames must be rows in [0,%d), at least one" % F)
        lr_rot, lr_trans = (self.lr_rot if lr_rot is None else float(lr_rot)), (self.lr_trans if lr_trans is None else float(lr_trans))
        U, L = len(listed), lib()
        listed_t = torch.tensor(listed, dtype=torch.int32, device=self.device)
        m, v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        g = torch.empty((U, J + 2, 3), dtype=torch.float32, device=self.device)
        for it in range(1, int(steps) + 1):
            self._backward_terms(0, U, listed_t, None, None, None, g)
            check(L.mgr_fk_adam(U, J, ptr(listed_t), ptr(g), ptr(self.theta), ptr(m), ptr(v), ptr(self.mask), ptr(self.lo), ptr(self.hi),
                                lr_rot, lr_trans, self.betas[0], self.betas[1], self.eps, it, stream()), "mgr_fk_adam")

    def keypoints(self, view_ids, frames, compute=None):
        """The posed keypoints p_k = (M_bone[k] [o_k; 1])[:3] (len(view_ids),K,3) of the views, from `posed()` and the offsets of
        `set_keypoints`: a host torch product on device tensors, for callers that want corrected keypoints."""
        if self.kp is None:
            raise ValueError("KinematicPoseRefiner.keypoints: no keypoints are set (set_keypoints)")
        bones, off = self.kp[0].long(), self.kp[1]
        M = self.posed(view_ids, frames, compute=compute)[:, bones]                           # (V,K,4,4)
        hom = torch.cat([off, torch.ones((off.shape[0], 1), dtype=off.dtype, device=off.device)], 1)
        return (M @ hom[None, :, :, None])[:, :, :3, 0]

    # -- state --------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return dict(frame_keys=list(self.frame_keys), steps=self.steps, theta=self.theta.clone(),
                    m=None if self.m is None else self.m.clone(), v=None if self.v is None else self.v.clone())

    def load_state_dict(self, state):
        if [tuple(k) for k in state["frame_keys"]] != self.frame_keys:
            raise ValueError("KinematicPoseRefiner.load_state_dict: the state is of other frames")
        if tuple(state["theta"].shape) != tuple(self.theta.shape):
            raise ValueError("KinematicPoseRefiner.load_state_dict: theta %s, expected %s" % (tuple(state["theta"].shape), tuple(self.theta.shape)))
        self.theta.copy_(state["theta"])
        for k in ("m", "v"):
            t = state.get(k)
            setattr(self, k, None if t is None else t.detach().to(device=self.device, dtype=torch.float32).clone().contiguous())
        self.steps = int(state["steps"])

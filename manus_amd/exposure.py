"""Per-camera exposure refinement: one learnt affine colour transform per camera of the rig, trained on the step.

A capture has some fifty cameras, each with its own gain and white balance; what the Gaussians cannot explain per camera they
bake into view-dependent colour and floaters.  Upstream 3DGS' answer is a learnt 3x4 colour transform per image on the render
before the loss; this is that option per CAMERA (csrc/exposure.hip: mgr_exposure_apply / mgr_exposure_backward /
mgr_exposure_adam).  The reference (brown-ivl/manus) has no counterpart.

    refiner = ExposureRefiner(store.camera_keys, frozen=(store.camera_keys[0],))
    refiner.attach(compute, refiner.rows_of(store, items))      # compute.exposure / compute.exposure_ids
    out = compute(view_ids, scale)                              # out["d_exposure"] (V,3,4) by position
    refiner.step(out["d_exposure"], view_ids, [compute.exposure_ids[v] for v in view_ids])

`engine.Trainer(exposure=refiner)` does the three lines on its schedule.
"""
import math

import torch

from ._lib import check, lib, ptr, stream
from .optim import get_expon_lr_func


class ExposureRefiner:
    """The table E (C,3,4) -- A = E[:,:,:3], b = E[:,:,3], identity at the start --, its Adam moments and step count.

    camera_keys: the camera names the rows stand for (repeats count once, in first-seen order; None entries are dropped).  The
    optimizer is the row Adam of `pose.PoseRefiner` (torch.optim.SparseAdam's semantics: only the cameras a step shows move, the
    bias correction uses the global count `steps`); `lr(step)` decays log-linearly from lr_init to lr_final over max_steps
    (`optim.get_expon_lr_func`).  frozen: camera names whose rows never move.  They anchor the gauge: a global gain can travel
    between the Gaussians' colours and the table, and a frozen camera pins it.  Default: none frozen.  The rates, betas, eps and
    `frozen` are configuration, not state: `state_dict()` carries the keys, the table, the moments and `steps`."""

    def __init__(self, camera_keys, lr_init=0.01, lr_final=0.001, max_steps=30000, betas=(0.9, 0.999), eps=1e-8, frozen=(), device=None):
        self.camera_keys = list(dict.fromkeys(k for k in camera_keys if k is not None))
        self.row = {k: j for j, k in enumerate(self.camera_keys)}
        C = len(self.camera_keys)
        if C < 1:
            raise ValueError("ExposureRefiner needs at least one camera")
        self.lr_init, self.lr_final, self.max_steps = float(lr_init), float(lr_final), int(max_steps)
        if not (self.lr_init > 0.0 and self.lr_final > 0.0 and math.isfinite(self.lr_init) and math.isfinite(self.lr_final)):
            raise ValueError("ExposureRefiner: lr_init and lr_final must be finite and positive (got %r, %r)" % (lr_init, lr_final))
        if self.max_steps < 1:
            raise ValueError("ExposureRefiner: max_steps must be at least 1")
        self._lr = get_expon_lr_func(self.lr_init, self.lr_final, max_steps=self.max_steps)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        unknown = [k for k in frozen if k not in self.row]
        if unknown:
            raise ValueError("ExposureRefiner: frozen names cameras that are not among camera_keys: %r" % (unknown,))
        self.frozen = frozenset(self.row[k] for k in frozen)
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.n_cameras = C
        self.E = torch.zeros((C, 3, 4), dtype=torch.float32, device=self.device)
        self.E[:, 0, 0] = self.E[:, 1, 1] = self.E[:, 2, 2] = 1.0
        self.m = torch.zeros_like(self.E)
        self.v = torch.zeros_like(self.E)
        self.steps = 0
        self.last_listed = None         # the rows the last step moved (host)
        self._lists = {}                # rows of a step -> (device rows, device list, host list)

    def lr(self, step):
        """The rate of the step taken after `step` earlier ones: lr_init at 0, lr_final from max_steps on, log-linear between."""
        return self._lr(int(step))

    # -- rows ---------------------------------------------------------------------------------------------------------------
    def rows_of(self, store, items):
        """The table rows of the dataset items `items` of a `frames.FrameStore` built by `from_dataset`; -1 (no correction) for an
        item whose camera is not among `camera_keys`."""
        if getattr(store, "camera_keys", None) is None:
            raise ValueError("rows_of needs the camera keys of a store built by FrameStore.from_dataset")
        return [self.row.get(store.camera_keys[store.row[int(i)]], -1) for i in items]

    def attach(self, compute, ids=None):
        """Point a `HipViewCompute` at the table: `compute.exposure` is E itself (every later step of this refiner is seen),
        `compute.exposure_ids` the table row of each of its view rows -- `ids`, or 0 .. V_all - 1 when the table has one row per
        view row."""
        n_all = int(compute.cams.shape[0])
        if ids is None:
            if self.n_cameras != n_all:
                raise ValueError("ExposureRefiner.attach: %d cameras for %d view rows: pass the row of every view row" % (self.n_cameras, n_all))
            ids = range(n_all)
        ids = [int(r) for r in ids]
        if len(ids) != n_all:
            raise ValueError("ExposureRefiner.attach: %d ids for %d view rows" % (len(ids), n_all))
        compute.exposure, compute.exposure_ids = self.E, ids
        compute._exposure_table()

    def _device_lists(self, rows):
        key = tuple(int(r) for r in rows)
        ent = self._lists.get(key)
        if ent is None:
            if any(r >= self.n_cameras for r in key):
                raise ValueError("ExposureRefiner: a row beyond the %d cameras" % self.n_cameras)
            listed = sorted({r for r in key if r >= 0 and r not in self.frozen})
            buf = torch.tensor(list(key) + listed, dtype=torch.int32).to(self.device)
            ent = (buf[:len(key)], buf[len(key):] if listed else None, listed)
            if len(self._lists) >= 256:
                self._lists.clear()
            self._lists[key] = ent
        return ent

    # -- the step -----------------------------------------------------------------------------------------------------------
    def step(self, d_exposure, view_ids, rows):
        """One Adam step of the cameras the views show, from the step's `out["d_exposure"]` (len(view_ids),3,4) by position;
        rows: the table row of every position (-1: none).  The distinct rows that are not frozen are listed in ascending order
        and stepped by ONE launch; views that share a camera are summed there, in ascending position.  With no row to move
        nothing happens, `steps` included."""
        V = len(view_ids)
        if len(rows) != V or V < 1:
            raise ValueError("ExposureRefiner.step: one row per view, at least one view (got %d views, %d rows)" % (V, len(rows)))
        if not torch.is_tensor(d_exposure) or tuple(d_exposure.shape) != (V, 3, 4) or d_exposure.dtype != torch.float32:
            raise ValueError("ExposureRefiner.step: d_exposure is not float32 (%d,3,4)" % V)
        cov, listed_t, listed = self._device_lists(rows)
        self.last_listed = listed
        if not listed:
            return
        rate = self.lr(self.steps)
        self.steps += 1
        check(lib().mgr_exposure_adam(self.n_cameras, len(listed), ptr(listed_t), V, ptr(cov), ptr(d_exposure.contiguous()), ptr(self.E),
                                      ptr(self.m), ptr(self.v), rate, self.betas[0], self.betas[1], self.eps, self.steps, stream()),
              "mgr_exposure_adam")

    # -- state --------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return dict(camera_keys=list(self.camera_keys), steps=self.steps, E=self.E.clone(), m=self.m.clone(), v=self.v.clone())

    def load_state_dict(self, state):
        if list(state["camera_keys"]) != self.camera_keys:
            raise ValueError("ExposureRefiner.load_state_dict: the state is of other cameras")
        for k in ("E", "m", "v"):
            if tuple(state[k].shape) != tuple(self.E.shape):
                raise ValueError("ExposureRefiner.load_state_dict: %s %s, expected %s" % (k, tuple(state[k].shape), tuple(self.E.shape)))
        for k in ("E", "m", "v"):      # in place: a compute object attached to E keeps seeing it
            getattr(self, k).copy_(state[k])
        self.steps = int(state["steps"])

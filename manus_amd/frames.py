"""Device frame store: the RGBA crops of a capture kept on the GPU as stored (uint8), decoded into the float targets and
masks of a step by one kernel (mgr_frames_decode, csrc/frames.hip).

`SequenceDataset.view_batch` builds a step's targets on the host: a full frame per view, the crop pasted at its bbox, the
division by 255 and the composite in float64, 33 MB per 1080p view copied to the device.  Kept as float targets a sequence
does not fit on the device either (25 MB per image); as its stored crops it is a few hundred KB per item.  A `FrameStore`
reads every item's crop and bbox once, packs the crops into one device pool and rewrites rows of caller-owned tables from
it -- bit for bit what `fetch_images` computes (tests/test_frames_cpu.py, tests/test_gpu_frames.py).

    store = FrameStore.from_dataset(ds, device="cuda:0")
    store.load_step(compute, items)          # targets, masks, cameras and poses of `items` into the rows 0 .. len(items) - 1
    out = compute(view_ids, scale)

No fallback: a resize factor other than 1 or 1/k (sizes divisible by k) is refused -- the host path needs OpenCV there."""
import weakref

import numpy as np
import torch

from . import transforms as T
from ._lib import MgrFrameView, check, lib, ptr, stream

ALIGN = 16      # every crop of the pool starts at a multiple of this


def factor_k(resize_factor):
    """k of a resize factor 1/k (1 for the factor 1); ValueError for anything else."""
    f = float(resize_factor)
    if f == 1.0:
        return 1
    k = round(1.0 / f) if f > 0 else 0
    if k < 2 or abs(1.0 / k - f) >= 1e-9:
        raise ValueError("resize_factor %r: the frame store decodes the factors 1 and 1/k only" % (resize_factor,))
    return k


def out_rect(bbox, k):
    """A bbox (x0,y0,x1,y1) in source pixels as a rectangle of output pixels, rounded outwards; (0,0,0,0) when it is empty."""
    x0, y0, x1, y1 = (int(t) for t in bbox)
    if x1 <= x0 or y1 <= y0:
        return (0, 0, 0, 0)
    return (x0 // k, y0 // k, -(-x1 // k), -(-y1 // k))


def union_rect(a, b):
    """Bounding rectangle of two rectangles (an empty one counts for nothing)."""
    if a[2] <= a[0] or a[3] <= a[1]:
        return b
    if b[2] <= b[0] or b[3] <= b[1]:
        return a
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))


class FrameStore:
    """The crops of a set of dataset items in one device pool, and the host tables that go with them.

    pool      (bytes,) uint8 on the device: the crops as stored, (h, w, 4) RGBA with packed rows, each at a multiple of 16 bytes
    offsets   (n,) int64, host: byte offset of every item's crop
    bboxes    (n, 4) int64, host: xmin, ymin, xmax, ymax of the crop in the SOURCE frame (height k x width k)
    items     the dataset indices the rows stand for (`decode` and `load_step` take dataset indices)
    height, width, k    output size and the block size of the resize (source frame = output size times k)
    cam_rows (n,40), transforms (n,J+1,4,4), posed (n,J,4,4), keypoints (n,J+1,3)    on the device, only from `from_dataset`: the
              per-item camera rows and poses `load_step` copies into a compute object's tables
    frame_keys    per row the (action, frame_id) of the item, host, only from `from_dataset`
    camera_keys   per row the camera name of the item, host, only from `from_dataset`
    """

    def __init__(self, pool, offsets, bboxes, height, width, k=1, items=None):
        self.pool = pool
        self.offsets = np.asarray(offsets, np.int64).reshape(-1)
        self.bboxes = np.asarray(bboxes, np.int64).reshape(-1, 4)
        self.height, self.width, self.k = int(height), int(width), int(k)
        self.items = list(range(len(self.offsets))) if items is None else [int(i) for i in items]
        self.row = {it: j for j, it in enumerate(self.items)}
        self.cam_rows = self.transforms = self.posed = self.keypoints = None
        self.cameras = None          # per row the camera dict of the dataset (host)
        self.frame_keys = None       # per row the (action, frame_id) of the item (host; `from_dataset`): the rows of `pose.PoseRefiner`
        self.camera_keys = None      # per row the camera name of the item (host; `from_dataset`): the rows of `exposure.ExposureRefiner`
        self._state = {}             # (targets.data_ptr(), slot) -> (weak reference to the table, rectangle, background, masks pointer)
        self._scene_masks = None     # (targets.data_ptr(), float table): masks decoded for a scene's pruning masks alone (`load_step(scene_masks=True)`)
        self._bg_host = None         # (id, version) of a compute object's background tensor and its three floats
        self.lpips_fit = None        # keywords of `lpips_rects` for `load_step(lpips_rects=True)`, e.g. dict(margin=16, quantum=32, common=True)
        if len(self.offsets) != len(self.items) or len(self.bboxes) != len(self.items):
            raise ValueError("offsets, bboxes and items must have one entry per crop")
        if (self.offsets % ALIGN).any():
            raise ValueError("crop offsets must be multiples of %d" % ALIGN)

    # -- construction ---------------------------------------------------------------------------------------------------
    @staticmethod
    def pack(crops):
        """crops: list of (h,w,4) uint8 arrays -> (pool (bytes,) uint8 ndarray, offsets (n,) int64): each crop at the next
        multiple of 16 bytes, the padding zero."""
        offsets, at = [], 0
        for c in crops:
            offsets.append(at)
            at += -(-int(c.size) // ALIGN) * ALIGN
        pool = np.zeros(at, np.uint8)
        for c, o in zip(crops, offsets):
            pool[o: o + c.size] = np.ascontiguousarray(c, np.uint8).reshape(-1)
        return pool, np.asarray(offsets, np.int64)

    @classmethod
    def from_dataset(cls, ds, indices=None, device="cuda:0", max_bytes=None):
        """Every item's crop and bbox read once from the container of `ds` (a `SequenceDataset` with one camera per item)."""
        from .dataset import _skeleton_batch, open_sequence
        from .synthetic import camera_table
        k = factor_k(ds.resize_factor)
        if ds.height % k or ds.width % k:
            raise ValueError("resize_factor 1/%d needs a frame size divisible by %d (got %d x %d)" % (k, k, ds.width, ds.height))
        indices = list(range(len(ds))) if indices is None else [int(i) for i in indices]
        crops, bboxes, total = [], [], 0
        for i in indices:
            action, frame_id, cam = ds.index_list[i]
            if cam is None:
                raise ValueError("item %d draws its cameras at random (rand_views_per_timestep): the frame store holds one crop per item" % i)
            with open_sequence(ds._path(action)) as f:
                data = f.get("frames")[str(frame_id)]
                bbox = [int(t) for t in data["bbox"][cam][:]]
                crop = np.asarray(data["images"][cam][:], np.uint8)
            if crop.shape != (bbox[3] - bbox[1], bbox[2] - bbox[0], 4):
                raise ValueError("item %d: crop %s does not fill its bbox %s" % (i, crop.shape, bbox))
            if bbox[0] < 0 or bbox[1] < 0 or bbox[2] > ds.width or bbox[3] > ds.height:
                raise ValueError("item %d: bbox %s outside the %d x %d frame" % (i, bbox, ds.width, ds.height))
            total += -(-crop.size // ALIGN) * ALIGN
            if max_bytes is not None and total > max_bytes:
                raise ValueError("the crop pool exceeds max_bytes = %d at item %d" % (max_bytes, i))
            crops.append(crop)
            bboxes.append(bbox)
        pool, offsets = cls.pack(crops)
        host = torch.from_numpy(pool)
        if torch.device(device).type == "cuda":
            try:
                host = host.pin_memory()      # (staged through pinned memory when the host allows it)
            except RuntimeError:
                pass
        st = cls(host.to(device), offsets, np.asarray(bboxes, np.int64).reshape(-1, 4), ds.height // k, ds.width // k, k, indices)
        # the camera rows and poses of the items, built the way a compute object's tables are (hand_scene_from_batch,
        # synthetic.camera_table): the same arithmetic, so a re-pointed row holds the bits construction would have given it
        cam_rows, tfs, posed, keyp, cams = [], [], [], [], []
        for i in indices:
            it = ds.fetch_data(i, images=False)
            sk = _skeleton_batch([it], "cpu", camera_row=0)
            cam = {k_: (v.cpu().numpy() if torch.is_tensor(v) else v) for k_, v in sk["cameras"][0].items()}
            cams.append(cam)
            cam_rows.append(camera_table([cam], "cpu")[0])
            p = sk["posed"][0].cpu().float()
            posed.append(p)
            tfs.append(T.bone_transforms(p, it["bones_rest"].transforms.cpu().float()))
            keyp.append(sk["keypoints"][0].float())
        st.cameras = cams
        st.frame_keys = [tuple(ds.index_list[i][:2]) for i in indices]
        st.camera_keys = [ds.index_list[i][2] for i in indices]
        if indices:
            st.cam_rows = torch.stack(cam_rows).to(device)
            st.transforms, st.posed, st.keypoints = torch.stack(tfs).to(device), torch.stack(posed).to(device), torch.stack(keyp).to(device)
        return st

    @property
    def nbytes(self):
        return int(self.pool.numel())

    # -- decode ---------------------------------------------------------------------------------------------------------
    def invalidate(self, targets=None):
        """Forget what the store knows about the tables it wrote (all of them, or `targets` alone): the next decode into them
        writes whole images.  Call it when someone else wrote into a table."""
        if targets is None:
            self._state.clear()
        else:
            p = targets.data_ptr()
            self._state = {key: v for key, v in self._state.items() if key[0] != p}

    def _records(self, items, bg, targets, masks, slots, dirty):
        """The MgrFrameView array of one decode and the dirty-rectangle state it leaves.  With `dirty`, a slot whose last
        write by this store (into the same table object, with the same background, the masks table in step) is known gets
        the union of the old and the new bbox in output pixels; every other slot the whole image."""
        V = len(items)
        slots = list(range(V)) if slots is None else [int(s) for s in slots]
        if len(slots) != V:
            raise ValueError("one slot per item")
        if len(set(slots)) != V:
            raise ValueError("two items of one decode name the same slot")
        bg = np.asarray(bg.detach().cpu() if torch.is_tensor(bg) else bg, np.float32)
        if bg.shape == (3,):
            bg = np.broadcast_to(bg, (V, 3))
        if bg.shape != (V, 3):
            raise ValueError("bg must be (3,) or (V,3)")
        H, W, k = self.height, self.width, self.k
        n_slots = int(targets.shape[0])
        if tuple(targets.shape) != (n_slots, 3, H, W) or targets.dtype != torch.float32 or not targets.is_contiguous():
            raise ValueError("targets must be a contiguous float32 table (n_slots,3,%d,%d)" % (H, W))
        if masks is not None and (tuple(masks.shape) != (n_slots, H, W) or masks.dtype != torch.float32 or not masks.is_contiguous()
                                  or masks.device != targets.device):
            raise ValueError("masks must be a contiguous float32 table (n_slots,%d,%d) next to targets" % (H, W))
        tp, mp = targets.data_ptr(), (masks.data_ptr() if masks is not None else None)
        recs = (MgrFrameView * max(V, 1))()
        new_state = {}
        for j, (it, slot) in enumerate(zip(items, slots)):
            if int(it) not in self.row:
                raise KeyError("item %r is not in the frame store" % (it,))
            if not 0 <= slot < n_slots:
                raise ValueError("slot %d outside the table of %d rows" % (slot, n_slots))
            r = self.row[int(it)]
            box = tuple(int(t) for t in self.bboxes[r])
            rect_new = out_rect(box, k)
            color = tuple(float(c) for c in bg[j])
            rect = (0, 0, W, H)
            old = self._state.get((tp, slot))
            if dirty and old is not None and old[0]() is targets and old[2] == color and (mp is None or old[3] == mp):
                rect = union_rect(old[1], rect_new)
            v = recs[j]
            v.offset = int(self.offsets[r])
            v.x0, v.y0, v.x1, v.y1 = box
            v.rx0, v.ry0, v.rx1, v.ry1 = rect
            v.bg[0], v.bg[1], v.bg[2] = color
            v.slot = slot
            new_state[(tp, slot)] = (weakref.ref(targets), rect_new, color, mp)
        return recs, new_state, n_slots

    def _launch(self, V, recs, targets, masks, n_slots):
        """mgr_frames_decode on the current stream (GPU tables only: `ptr` refuses anything else)."""
        check(lib().mgr_frames_decode(V, self.height, self.width, self.k, ptr(self.pool), self.nbytes, recs, ptr(targets),
                                      ptr(masks), n_slots, stream()), "mgr_frames_decode")

    def decode(self, items, bg, targets, masks=None, slots=None, dirty=True):
        """Write the rows `slots` (default 0 .. len(items) - 1) of the caller's `targets` (n_slots,3,H,W) -- and `masks`
        (n_slots,H,W) when given -- from the crops of the dataset items `items`, composited on `bg` ((3,) or (V,3)).  Rows not
        named stay as they are.  The write goes through the tables' raw pointers: torch's version counters do not move."""
        items = list(items)
        recs, new_state, n_slots = self._records(items, bg, targets, masks, slots, dirty)
        if items:
            self._launch(len(items), recs, targets, masks, n_slots)
        self._state.update(new_state)
        if len(self._state) > 65536:      # (tables long gone: forget them all, the next writes are whole images)
            self._state = dict(new_state)

    # -- LPIPS windows ---------------------------------------------------------------------------------------------------
    def lpips_rects(self, items, margin=16, net="vgg", quantum=0, common=False):
        """(len(items),4) int32 x0, y0, w, h: every item's bbox in output pixels (`out_rect`), grown by `margin`, clamped to the
        frame and brought to the network's minimum size (`lpips.fit_rects`) -- the windows of `HipViewCompute.lpips_rects`.  An
        empty bbox gives an empty rectangle.  quantum / common: `fit_rects`' -- sides rounded up to a multiple of the quantum,
        one size for the whole set -- for a batched term (`HipViewCompute.lpips_batch`).  Host arithmetic only."""
        from .lpips import fit_rects
        rects = []
        for it in items:
            if int(it) not in self.row:
                raise KeyError("item %r is not in the frame store" % (it,))
            x0, y0, x1, y1 = out_rect(self.bboxes[self.row[int(it)]], self.k)
            rects.append((x0, y0, x1 - x0, y1 - y0))
        return fit_rects(np.asarray(rects, np.int64).reshape(-1, 4), self.height, self.width, net, margin, quantum, common)

    # -- one step of a compute object -----------------------------------------------------------------------------------
    def _compute_bg(self, compute):
        """The three floats of the compute object's background colour (read back once per tensor version)."""
        bg = compute.s["bg"]
        key = (id(bg), bg._version)
        if self._bg_host is None or self._bg_host[0] != key:
            self._bg_host = (key, np.asarray(bg.detach().cpu(), np.float32).reshape(3))
        return self._bg_host[1]

    def load_step(self, compute, items, slots=None, masks=False, lpips_rects=False, scene_masks=False):
        """Point the rows `slots` (default 0 .. len(items) - 1) of an `engine.HipViewCompute` at the dataset items `items`:
        their targets decoded into `compute.targets`, their masks into `compute.mask_targets` (when that is set; masks=True
        allocates a zero table and sets it when it is not), their camera rows into `compute.cams`, their bone transforms (and
        posed transforms, keypoints, camera dicts, pruning masks where the scene holds them) into the scene's tables, all in
        place; the compute object is told, so its next step rebuilds what it derives from them.  lpips_rects=True also writes
        the slots' rows of `compute.lpips_rects` with the items' windows (`lpips_rects(items, **self.lpips_fit)`; the store's
        `lpips_fit` is None, today's rows, or a dict of margin / net / quantum / common), allocating a table of full-frame
        rectangles first when the compute object has none.  scene_masks=True: when the compute object has NO mask table but the
        scene holds pruning masks (`s["masks"]`, what `HipViewCompute.prune_views` hands the pruning tests), the items' masks are
        decoded into a table the store keeps and copied into the scene's rows all the same -- the mask loss term stays off --,
        so that a pruning test never meets a drawn item's camera with another item's mask."""
        if self.cam_rows is None:
            raise ValueError("load_step needs the camera rows and poses of a store built by FrameStore.from_dataset")
        items = [int(i) for i in items]
        slots = list(range(len(items))) if slots is None else [int(s) for s in slots]
        s = compute.s
        mt = compute.mask_targets
        if mt is None and masks:
            mt = torch.zeros((compute.targets.shape[0], self.height, self.width), dtype=torch.float32, device=compute.targets.device)
        if mt is None and scene_masks and torch.is_tensor(s.get("masks")) and \
                tuple(s["masks"].shape) == (int(compute.targets.shape[0]), self.height, self.width):
            key = compute.targets.data_ptr()
            if self._scene_masks is None or self._scene_masks[0] != key or self._scene_masks[1].device != compute.targets.device \
                    or self._scene_masks[1].shape != s["masks"].shape:
                self._scene_masks = (key, torch.zeros(tuple(s["masks"].shape), dtype=torch.float32, device=compute.targets.device))
                self.invalidate(compute.targets)      # (a new masks table: the next decode writes whole images)
            mt = self._scene_masks[1]
            decoded_for_scene = True
        else:
            decoded_for_scene = False
        self.decode(items, self._compute_bg(compute), compute.targets, mt, slots)
        dev = compute.cams.device
        rows_t = torch.tensor([self.row[i] for i in items], dtype=torch.long, device=dev)
        slots_t = torch.tensor(slots, dtype=torch.long, device=dev)
        compute.cams.index_copy_(0, slots_t, self.cam_rows.index_select(0, rows_t))
        if compute.is_hand:
            if tuple(s["transforms"].shape[1:]) != tuple(self.transforms.shape[1:]):
                raise ValueError("the scene poses %s bones, the store's items %s" % (tuple(s["transforms"].shape[1:]), tuple(self.transforms.shape[1:])))
            s["transforms"].index_copy_(0, slots_t, self.transforms.index_select(0, rows_t))
        for name, table in (("posed", self.posed), ("keypoints", self.keypoints)):
            if torch.is_tensor(s.get(name)) and tuple(s[name].shape[1:]) == tuple(table.shape[1:]):
                s[name].index_copy_(0, slots_t, table.index_select(0, rows_t).to(s[name].dtype))
        if isinstance(s.get("cameras"), list):
            for i, slot in zip(items, slots):
                s["cameras"][slot] = self.cameras[self.row[i]]
        if mt is not None and torch.is_tensor(s.get("masks")) and s["masks"] is not mt and s["masks"].shape == mt.shape:
            s["masks"].index_copy_(0, slots_t, mt.index_select(0, slots_t).to(s["masks"].dtype))
        if mt is not compute.mask_targets and not decoded_for_scene:
            compute.mask_targets = mt
        if lpips_rects:
            table = compute.lpips_rects
            if table is None:
                table = np.tile(np.asarray([0, 0, self.width, self.height], np.int32), (int(compute.targets.shape[0]), 1))
            else:
                table = np.array(table, dtype=np.int32).reshape(-1, 4)
            table[slots] = self.lpips_rects(items, **(self.lpips_fit or {}))
            compute.lpips_rects = table
        compute.view_constants_changed()

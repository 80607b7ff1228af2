"""No GPU: the numpy restatement of the frame decode (tests/frames_ref.py) against SequenceDataset.fetch_images bit for bit, the
ABI of mgr_frames_decode, its refusals (all in front of any launch: no device needed), and FrameStore's packing tables and
dirty-rectangle bookkeeping with the launch stubbed out."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from frames_ref import decode_ref, out_rect

from manus_amd import dataset as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(bg_color="white", subject="s1", rand_views_per_timestep=-1, n_bones=20, num_time_steps=-1, split_ratio=1.0,
            sequences="all", split_by_action=False)


def write_sequence(path, seed, width, height, crops=None, n_frames=2, n_cams=3):
    """One synthetic action file; crops: {(frame position, camera position): (crop, bbox)} replace the generated ones."""
    arr = D.synthetic_sequence(seed, n_frames=n_frames, n_cams=n_cams, width=width, height=height)
    frames = D.natsorted({key.split("/")[1] for key in arr if key.startswith("frames/")})
    for (f, c), (crop, bbox) in (crops or {}).items():
        arr["frames/%s/images/cam%02d" % (frames[f], c)] = np.asarray(crop, np.uint8)
        arr["frames/%s/bbox/cam%02d" % (frames[f], c)] = np.asarray(bbox, np.int64)
    D.write_tree(os.path.join(path, "grasp_1.npz"), arr)


def hand_crops(width, height, seed=0):
    """Crops the generator does not make: odd offsets, all four borders, the whole frame, one pixel, nothing; alpha 0, 255, 1, 254
    and random."""
    rng = np.random.default_rng(seed)

    def crop(box, alpha):
        h, w = box[3] - box[1], box[2] - box[0]
        c = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if alpha == "mix":
            c[..., 3] = rng.choice(np.array([0, 255, 1, 254], np.uint8), (h, w))
        elif alpha != "random":
            c[..., 3] = alpha
        return c, box
    boxes = [((3, 5, width - 7, height - 3), "mix"), ((0, 0, width, height), "random"), ((1, 1, 2, 2), 254),
             ((7, 9, 7, 9), 0), ((0, 3, width, height - 5), 1), ((5, 0, width - 3, height), 255)]
    return {(i // 3, i % 3): crop(b, a) for i, (b, a) in enumerate(boxes)}


@pytest.mark.parametrize("width,height,k", [(64, 48, 1), (64, 48, 2), (63, 45, 3), (62, 46, 2)])
@pytest.mark.parametrize("bg", ["white", "black"])
def test_reference_equals_the_host_path_bit_for_bit(tmp_path, width, height, k, bg):
    write_sequence(str(tmp_path), 5, width, height, hand_crops(width, height))
    ds = D.SequenceDataset(str(tmp_path), dict(BASE, width=width, height=height, resize_factor=1.0 / k, bg_color=bg), "train")
    assert len(ds) == 6
    H, W = height // k, width // k
    for i in range(len(ds)):
        action, frame, cam = ds.index_list[i]
        with D.open_sequence(ds._path(action)) as f:
            data = f["frames"][str(frame)]
            crop, bbox = data["images"][cam][:], data["bbox"][cam][:]
        it = ds[i]
        tgt, mask = decode_ref(crop, bbox, ds.get_bg_color(), H, W, k)
        assert it["rgb"].shape == (1, H, W, 3)
        assert torch.equal(it["rgb"][0].permute(2, 0, 1), torch.from_numpy(tgt)), (i, bbox)
        assert torch.equal(it["mask"][0, ..., 0], torch.from_numpy(mask)), (i, bbox)


def test_reference_with_a_random_background(tmp_path):
    """A background that is no 0 or 1: the composite's second product is a real fp64 multiplication."""
    write_sequence(str(tmp_path), 6, 64, 48)
    ds = D.SequenceDataset(str(tmp_path), dict(BASE, width=64, height=48, resize_factor=0.5), "train")
    bg = np.random.default_rng(3).random(3).astype(np.float32)
    ds.get_bg_color = lambda: bg
    with D.open_sequence(ds._path("grasp_1")) as f:
        data = f["frames"][str(ds.index_list[2][1])]
        cam = ds.index_list[2][2]
        img = ds.fetch_images(data, cam)
        tgt, mask = decode_ref(data["images"][cam][:], data["bbox"][cam][:], bg, 24, 32, 2)
    assert torch.equal(D.to_tensor(img[..., :3]).permute(2, 0, 1), torch.from_numpy(tgt))
    assert torch.equal(D.to_tensor(img[..., 3]), torch.from_numpy(mask))


def test_entry_is_declared_bound_and_exported():
    from manus_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    m = re.search(r"\bint\s+mgr_frames_decode\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, "include/manus_hip.h does not declare mgr_frames_decode"
    n_decl = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    res, args = _lib.SIGNATURES["mgr_frames_decode"]
    assert n_decl == len(args) == 11 and res is ctypes.c_int
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mgr_frames_decode")
    assert "frames.hip" in build.SOURCES
    assert int(re.search(r"#define\s+MGR_FRAMES_MAX_VIEWS\s+(\d+)", header).group(1)) == _lib.MGR_FRAMES_MAX_VIEWS == 16
    assert ctypes.sizeof(_lib.MgrFrameView) == 56 and _lib.MgrFrameView.slot.offset == 52 and _lib.MgrFrameView.bg.offset == 40


def _view(offset=0, box=(0, 0, 4, 4), rect=(0, 0, 8, 6), slot=0, bg=(1.0, 1.0, 1.0)):
    from manus_amd._lib import MgrFrameView
    v = MgrFrameView()
    v.offset = offset
    v.x0, v.y0, v.x1, v.y1 = box
    v.rx0, v.ry0, v.rx1, v.ry1 = rect
    v.bg[0], v.bg[1], v.bg[2] = bg
    v.slot = slot
    return v


def test_refusals_need_no_device():
    """Every refusal of the entry comes before its first launch.  The pointers are never dereferenced: any non-null value does."""
    from manus_amd._lib import MGR_EINVAL, MgrFrameView, lib
    L = lib()
    H, W, pool, tables, pool_bytes, n_slots = 6, 8, 4096, 8192, 1024, 4

    def call(views, k=1, pool=pool, pool_bytes=pool_bytes, n_slots=n_slots, H=H, W=W):
        arr = (MgrFrameView * len(views))(*views)
        return L.mgr_frames_decode(len(views), H, W, k, pool, pool_bytes, arr, tables, None, n_slots, None)

    def refused(rc, text):
        assert rc == MGR_EINVAL and text in L.mgr_last_error(), (rc, L.mgr_last_error())

    refused(call([_view()], k=0), b"k < 1")
    refused(call([_view()], k=-2), b"k < 1")
    refused(call([_view(box=(0, 0, 9, 4))]), b"bbox")                       # beyond W k
    refused(call([_view(box=(0, 0, 4, 7))]), b"bbox")                       # beyond H k
    refused(call([_view(box=(-1, 0, 4, 4))]), b"bbox")
    refused(call([_view(box=(5, 0, 4, 4))]), b"bbox")                       # x1 < x0
    refused(call([_view(box=(0, 5, 4, 4))]), b"bbox")
    refused(call([_view(box=(0, 0, 17, 4), rect=(0, 0, 8, 6))], k=2), b"bbox")    # W k = 16
    refused(call([_view(offset=8)]), b"multiple of 16")
    refused(call([_view(offset=-16)]), b"multiple of 16")
    refused(call([_view(offset=pool_bytes - 48)]), b"beyond the pool")      # 64 bytes of crop, 48 left
    refused(call([_view(offset=pool_bytes + 16, box=(0, 0, 0, 0))]), b"beyond the pool")
    refused(call([_view(rect=(0, 0, 9, 6))]), b"rectangle")
    refused(call([_view(rect=(0, 0, 8, 7))]), b"rectangle")
    refused(call([_view(rect=(-1, 0, 8, 6))]), b"rectangle")
    refused(call([_view(rect=(5, 0, 4, 6))]), b"rectangle")
    refused(call([_view(slot=4)]), b"slot")
    refused(call([_view(slot=-1)]), b"slot")
    refused(call([_view(slot=1), _view(offset=64, slot=2), _view(offset=128, slot=1)]), b"same slot")
    refused(call([_view(slot=s % 3) for s in range(20)]), b"same slot")     # across the chunks of 16 views
    refused(call([_view()], pool=None), b"null pool")
    refused(call([_view()], H=0), b"bad sizes")
    # a bad view anywhere in the call refuses all of it (the check runs over every chunk first)
    refused(call([_view(slot=s) for s in range(17)] + [_view(slot=17, offset=8)], n_slots=32), b"multiple of 16")
    # nothing to do is no error; an empty crop needs no pool
    assert call([]) == 0
    assert L.mgr_frames_decode(0, H, W, 1, None, 0, None, None, None, 0, None) == 0


class Stub:
    """FrameStore._launch replaced: records what would have been launched."""

    def __init__(self, store):
        self.calls = []
        store._launch = self

    def __call__(self, V, recs, targets, masks, n_slots):
        self.calls.append([dict(offset=r.offset, box=(r.x0, r.y0, r.x1, r.y1), rect=(r.rx0, r.ry0, r.rx1, r.ry1), bg=tuple(r.bg), slot=r.slot)
                           for r in list(recs)[:V]])
        return self.calls[-1]


def test_store_tables_and_dirty_rectangles(tmp_path):
    from manus_amd.frames import FrameStore, out_rect as store_rect, union_rect
    width, height, k = 64, 48, 2
    left, right = (2, 3, 31, 45), (51, 20, 58, 27)
    rng = np.random.default_rng(1)
    crops = {(0, 0): (rng.integers(0, 256, (42, 29, 4), dtype=np.uint8), left), (0, 1): (rng.integers(0, 256, (7, 7, 4), dtype=np.uint8), right),
             (0, 2): (np.zeros((0, 0, 4), np.uint8), (9, 9, 9, 9))}
    write_sequence(str(tmp_path), 2, width, height, crops)
    ds = D.SequenceDataset(str(tmp_path), dict(BASE, width=width, height=height, resize_factor=0.5), "train")
    st = FrameStore.from_dataset(ds, device="cpu")
    # -- packing: one row per item, offsets multiples of 16 and disjoint, bbox copied, the pool holds the crops as stored
    assert st.items == list(range(len(ds))) and (st.height, st.width, st.k) == (24, 32, 2)
    assert st.pool.dtype == torch.uint8 and (st.offsets % 16 == 0).all() and st.offsets[0] == 0
    pool = st.pool.numpy()
    end = 0
    for j, (action, frame, cam) in enumerate(ds.index_list):
        with D.open_sequence(ds._path(action)) as f:
            crop, bbox = f["frames"][str(frame)]["images"][cam][:], f["frames"][str(frame)]["bbox"][cam][:]
        assert list(st.bboxes[j]) == [int(t) for t in bbox]
        assert st.offsets[j] >= end and st.offsets[j] - end < 16
        assert np.array_equal(pool[st.offsets[j]: st.offsets[j] + crop.size], crop.reshape(-1))
        end = st.offsets[j] + crop.size
    assert 29 * 42 * 4 % 16 != 0 and st.nbytes == -(-end // 16) * 16
    assert st.cam_rows.shape == (len(ds), 40) and st.transforms.shape == (len(ds), 21, 4, 4)
    with pytest.raises(ValueError, match="max_bytes"):
        FrameStore.from_dataset(ds, device="cpu", max_bytes=1000)
    sub = FrameStore.from_dataset(ds, indices=[4, 1], device="cpu")
    assert sub.items == [4, 1] and list(sub.bboxes[1]) == list(st.bboxes[1]) and sub.row == {4: 0, 1: 1}
    # -- rectangles: outwards
    assert store_rect(left, 2) == out_rect(left, 2) == (1, 1, 16, 23) and store_rect(right, 2) == (25, 10, 29, 14)
    assert store_rect((9, 9, 9, 9), 2) == (0, 0, 0, 0) and union_rect((0, 0, 0, 0), (1, 2, 3, 4)) == (1, 2, 3, 4)
    assert union_rect((1, 1, 16, 23), (25, 10, 29, 14)) == (1, 1, 29, 23)
    # -- bookkeeping (launch stubbed): first write whole, then unions; per table and slot; background and invalidate reset it
    stub = Stub(st)
    tg, other = torch.zeros((3, 3, 24, 32)), torch.zeros((3, 3, 24, 32))
    mk = torch.zeros((3, 24, 32))
    full = (0, 0, 32, 24)
    white, black = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    st.decode([0], white, tg, slots=[2])
    assert stub.calls[-1] == [dict(offset=0, box=left, rect=full, bg=white, slot=2)]
    st.decode([1], white, tg, slots=[2])
    assert stub.calls[-1][0]["rect"] == (1, 1, 29, 23) and stub.calls[-1][0]["box"] == right and stub.calls[-1][0]["offset"] == int(st.offsets[1])
    st.decode([1], white, tg, slots=[2])
    assert stub.calls[-1][0]["rect"] == (25, 10, 29, 14)                      # the union with itself
    st.decode([2], white, tg, slots=[2])
    assert stub.calls[-1][0]["rect"] == (25, 10, 29, 14)                      # an empty crop: only the old box is rewritten
    st.decode([2], white, tg, slots=[2])
    assert stub.calls[-1][0]["rect"] == (0, 0, 0, 0)
    st.decode([0], white, tg, slots=[1])
    assert stub.calls[-1][0]["rect"] == full                                  # another slot
    st.decode([0], white, other, slots=[2])
    assert stub.calls[-1][0]["rect"] == full                                  # another table
    st.decode([0], black, tg, slots=[2])
    assert stub.calls[-1][0]["rect"] == full and stub.calls[-1][0]["bg"] == black     # another background
    st.decode([1], black, tg, slots=[2], dirty=False)
    assert stub.calls[-1][0]["rect"] == full
    st.decode([0], black, tg, slots=[2])
    assert stub.calls[-1][0]["rect"] == (1, 1, 29, 23)                        # (a whole write leaves its box behind too)
    st.decode([1], black, tg, mk, slots=[2])
    assert stub.calls[-1][0]["rect"] == full                                  # the masks table was not written along so far
    st.decode([0], black, tg, mk, slots=[2])
    assert stub.calls[-1][0]["rect"] == (1, 1, 29, 23)
    st.invalidate(other)
    st.decode([1], black, tg, mk, slots=[2])
    assert stub.calls[-1][0]["rect"] == (1, 1, 29, 23)                        # (forgot the other table only)
    st.invalidate()
    st.decode([1], black, tg, mk, slots=[2])
    assert stub.calls[-1][0]["rect"] == full
    # per-view backgrounds, default slots, one record per item
    st.decode([0, 1, 2], np.array([white, black, (0.25, 0.5, 0.75)], np.float32), tg)
    assert [r["slot"] for r in stub.calls[-1]] == [0, 1, 2] and [r["bg"] for r in stub.calls[-1]] == [white, black, (0.25, 0.5, 0.75)]
    # what the store refuses itself
    for bad in (dict(slots=[0, 0]), dict(slots=[3, 1]), dict(slots=[0])):
        with pytest.raises(ValueError):
            st.decode([0, 1], white, tg, **bad)
    with pytest.raises(KeyError):
        sub.decode([0], white, tg)
    with pytest.raises(ValueError):
        st.decode([0], white, torch.zeros((3, 3, 24, 31)))
    with pytest.raises(ValueError):
        st.decode([0], white, tg, torch.zeros((2, 24, 32)))
    with pytest.raises(ValueError):
        st.decode([0, 1], (1.0, 1.0), tg)


def test_store_refuses_what_the_kernel_does_not_decode(tmp_path):
    from manus_amd.frames import FrameStore, factor_k
    assert factor_k(1.0) == 1 and factor_k(0.5) == 2 and factor_k(1.0 / 3) == 3
    for bad in (0.3, 2.0, 0.0, -0.5):
        with pytest.raises(ValueError):
            factor_k(bad)
    write_sequence(str(tmp_path), 4, 62, 46)
    ds = D.SequenceDataset(str(tmp_path), dict(BASE, width=62, height=46, resize_factor=1.0), "train")
    ds.resize_factor = 0.25                      # 62 x 46 is not divisible by 4
    with pytest.raises(ValueError, match="divisible"):
        FrameStore.from_dataset(ds, device="cpu")
    rand = D.SequenceDataset(str(tmp_path), dict(BASE, width=62, height=46, resize_factor=1.0, rand_views_per_timestep=2), "train")
    with pytest.raises(ValueError, match="random"):
        FrameStore.from_dataset(rand, device="cpu")
    # without a device there is no decode: no fallback
    from manus_amd._lib import ManusHipError
    st = FrameStore.from_dataset(ds.__class__(str(tmp_path), dict(BASE, width=62, height=46, resize_factor=1.0), "train"), device="cpu")
    with pytest.raises(ManusHipError):
        st.decode([0], (1.0, 1.0, 1.0), torch.zeros((1, 3, 46, 62)))

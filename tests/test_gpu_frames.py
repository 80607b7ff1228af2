"""GPU: mgr_frames_decode through frames.FrameStore against its numpy restatement (tests/frames_ref.py, pinned to
SequenceDataset.fetch_images by tests/test_frames_cpu.py) -- every output compared BIT FOR BIT, no tolerance --, the dirty
rectangles, `SequenceDataset.view_batch(store=...)` against the host path, and `FrameStore.load_step` re-pointing a fused
HipViewCompute step.

Shapes are tiny on purpose: 64x48 at k = 1 and 2, 62x46 at k = 2 (31x23: odd width, the scalar-store path, unaligned rows),
63x45 at k = 3.  Crop byte sizes are no multiples of 16 (the pool's padding is in use)."""
import os

import numpy as np
import pytest
import torch

from frames_ref import decode_ref, out_rect
from util import max_rel_err

from manus_amd import dataset as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {"64x48k1": (64, 48, 1), "64x48k2": (64, 48, 2), "62x46k2": (62, 46, 2), "63x45k3": (63, 45, 3)}
BASE = dict(bg_color="white", subject="s1", rand_views_per_timestep=-1, n_bones=20, num_time_steps=-1, split_ratio=1.0,
            sequences="all", split_by_action=False)
SENTINEL = -7.0
N_FRAMES, N_CAMS = 6, 3            # 18 items: V = 17 crosses the 16-view chunk


def hand_crops(width, height, seed=0):
    """Item 0: a large box on the left at odd offsets (k x k blocks straddle its edges and average with zeros); 1: a small box on
    the right; 2: touching all four borders = the whole frame; 3: one pixel; 4: nothing; 5: full height at odd x."""
    rng = np.random.default_rng(seed)

    def crop(box, alpha):
        h, w = box[3] - box[1], box[2] - box[0]
        c = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if alpha == "mix":
            c[..., 3] = rng.choice(np.array([0, 255, 1, 254], np.uint8), (h, w))
        elif alpha != "random":
            c[..., 3] = alpha
        return c, box
    boxes = [((1, 3, width // 2 - 3, height - 5), "mix"), ((width - 13, 19, width - 6, 26), "random"), ((0, 0, width, height), "random"),
             ((5, 7, 6, 8), 254), ((9, 9, 9, 9), 0), ((3, 0, width - 7, height), 1)]
    return {(i // N_CAMS, i % N_CAMS): crop(b, a) for i, (b, a) in enumerate(boxes)}


class Capture:
    """One synthetic capture on disk, its dataset, its store, and the reference decode of its items (computed once per
    (item, background), shared by the tests)."""

    def __init__(self, path, width, height, k):
        arr = D.synthetic_sequence(21, n_frames=N_FRAMES, n_cams=N_CAMS, width=width, height=height)
        frames = D.natsorted({key.split("/")[1] for key in arr if key.startswith("frames/")})
        for (f, c), (crop, bbox) in hand_crops(width, height).items():
            arr["frames/%s/images/cam%02d" % (frames[f], c)] = crop
            arr["frames/%s/bbox/cam%02d" % (frames[f], c)] = np.asarray(bbox, np.int64)
        D.write_tree(os.path.join(path, "grasp_1.npz"), arr)
        from manus_amd.frames import FrameStore
        self.ds = D.SequenceDataset(path, dict(BASE, width=width, height=height, resize_factor=1.0 / k), "train")
        assert len(self.ds) == N_FRAMES * N_CAMS
        self.store = FrameStore.from_dataset(self.ds, device=DEV)
        self.H, self.W, self.k = height // k, width // k, k
        self.raw = []
        for action, frame, cam in self.ds.index_list:
            with D.open_sequence(self.ds._path(action)) as f:
                data = f["frames"][str(frame)]
                self.raw.append((data["images"][cam][:], [int(t) for t in data["bbox"][cam][:]]))
        assert any(c.size % 16 for c, _ in self.raw)
        self._ref = {}

    def ref(self, item, bg):
        key = (item, tuple(float(np.float32(c)) for c in bg))
        if key not in self._ref:
            t, m = decode_ref(self.raw[item][0], self.raw[item][1], bg, self.H, self.W, self.k)
            self._ref[key] = (torch.from_numpy(t), torch.from_numpy(m))
        return self._ref[key]

    def tables(self, n):
        return (torch.full((n, 3, self.H, self.W), SENTINEL, device=DEV), torch.full((n, self.H, self.W), SENTINEL, device=DEV))


@pytest.fixture(scope="module")
def captures(tmp_path_factory):
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = Capture(str(tmp_path_factory.mktemp(tag)), *CASES[tag])
        return made[tag]
    return get


@pytest.mark.parametrize("V", [1, 3, 17])
@pytest.mark.parametrize("tag", list(CASES))
def test_decode_is_bitwise_the_reference(captures, tag, V):
    cap = captures(tag)
    st = cap.store
    rng = np.random.default_rng(V)
    items = [int(i) for i in (rng.permutation(18)[:V] if V > 1 else [0])]
    if V == 3:
        items = [4, 2, 0]                                    # the empty crop, the whole frame, the odd box
    n_slots = V + 4
    slots = [int(s) for s in rng.permutation(n_slots)[:V]]   # permuted, with holes
    for name, bg in (("white", np.ones(3, np.float32)), ("black", np.zeros(3, np.float32)), ("random", rng.random((V, 3)).astype(np.float32))):
        tg, mk = cap.tables(n_slots)
        st.decode(items, bg, tg, mk, slots=slots, dirty=False)
        got_t, got_m = tg.cpu(), mk.cpu()
        for j, (it, slot) in enumerate(zip(items, slots)):
            rt, rm = cap.ref(it, bg if bg.ndim == 1 else bg[j])
            assert torch.equal(got_t[slot], rt), (tag, name, it, slot, float((got_t[slot] - rt).abs().max()))
            assert torch.equal(got_m[slot], rm), (tag, name, it, slot)
        rest = [s for s in range(n_slots) if s not in slots]
        assert bool((got_t[rest] == SENTINEL).all()) and bool((got_m[rest] == SENTINEL).all())
        # masks=None leaves no write behind
        tg2, mk2 = cap.tables(n_slots)
        st.decode(items, bg, tg2, None, slots=slots, dirty=False)
        assert torch.equal(tg2.cpu(), got_t) and bool((mk2 == SENTINEL).all())
    # the empty crop is background and a zero mask; alpha 254 / 1 are the fp32 of 254 / 255 and 1 / 255
    tg, mk = cap.tables(1)
    st.decode([4], np.array([0.25, 0.5, 0.75], np.float32), tg, mk, dirty=False)
    assert bool((mk == 0).all()) and torch.equal(tg[0, :, 0, 0].cpu(), torch.tensor([0.25, 0.5, 0.75]))
    if cap.k == 1:
        st.decode([3], np.ones(3, np.float32), tg, mk, dirty=False)
        assert float(mk[0, 7, 5]) == float(np.float32(254 / 255.0)) and float(mk[0, 7, 6]) == 0.0
        st.decode([5], np.ones(3, np.float32), tg, mk, dirty=False)
        assert float(mk[0, 0, 3]) == float(np.float32(1 / 255.0))


@pytest.mark.parametrize("tag", ["64x48k1", "64x48k2", "62x46k2"])
def test_dirty_rectangles(captures, tag):
    cap = captures(tag)
    st = cap.store
    A, B, slot = 0, 1, 1                                     # a large box on the left, a small one on the right
    white, grey = np.ones(3, np.float32), np.array([0.5, 0.25, 0.125], np.float32)
    ra, rb = out_rect(cap.raw[A][1], cap.k), out_rect(cap.raw[B][1], cap.k)
    assert ra[2] < rb[0]                                     # disjoint: the union is more than either
    inside = torch.zeros((cap.H, cap.W), dtype=torch.bool)
    inside[min(ra[1], rb[1]): max(ra[3], rb[3]), min(ra[0], rb[0]): max(ra[2], rb[2])] = True
    assert bool((~inside).any())

    def check(tg, mk, item, bg, poisoned):
        rt, rm = cap.ref(item, bg)
        got_t, got_m = tg[slot].cpu(), mk[slot].cpu()
        if poisoned:                                         # the union was rewritten, the poison outside it is still there
            assert torch.equal(got_t[:, inside], rt[:, inside]) and torch.equal(got_m[inside], rm[inside])
            assert bool((got_t[:, ~inside] == 9.0).all()) and bool((got_m[~inside] == 9.0).all())
        else:
            assert torch.equal(got_t, rt) and torch.equal(got_m, rm)
        assert bool((tg[0] == SENTINEL).all()) and bool((tg[2] == SENTINEL).all()) and bool((mk[0] == SENTINEL).all())

    def poison(tg, mk):
        tg[slot][:, ~inside.to(DEV)] = 9.0
        mk[slot][~inside.to(DEV)] = 9.0

    st.invalidate()
    tg, mk = cap.tables(3)
    st.decode([A], white, tg, mk, slots=[slot])              # nothing known about the slot: the whole image
    check(tg, mk, A, white, False)
    st.decode([B], white, tg, mk, slots=[slot])              # the union of the two boxes ...
    check(tg, mk, B, white, False)                           # ... is a full decode of B
    # that the dirty write IS partial: poison outside both boxes survives it
    st.decode([A], white, tg, mk, slots=[slot])
    poison(tg, mk)
    st.decode([B], white, tg, mk, slots=[slot])
    check(tg, mk, B, white, True)
    # a changed background forces the whole image: the poison is gone
    st.decode([A], grey, tg, mk, slots=[slot])
    check(tg, mk, A, grey, False)
    poison(tg, mk)
    st.decode([B], grey, tg, mk, slots=[slot])
    check(tg, mk, B, grey, True)
    # and so does invalidate()
    st.invalidate()
    st.decode([A], grey, tg, mk, slots=[slot])
    check(tg, mk, A, grey, False)
    poison(tg, mk)
    st.invalidate(tg)
    st.decode([B], grey, tg, mk, slots=[slot])
    check(tg, mk, B, grey, False)
    # dirty=False never trusts the table
    poison(tg, mk)
    st.decode([A], grey, tg, mk, slots=[slot], dirty=False)
    check(tg, mk, A, grey, False)


@pytest.mark.parametrize("tag", ["64x48k1", "62x46k2"])
def test_view_batch_with_a_store_equals_the_host_path(captures, tag):
    cap = captures(tag)
    idx = [7, 0, 4, 2, 16]
    host = cap.ds.view_batch(idx)
    dev = cap.ds.view_batch(idx, DEV, store=cap.store)
    assert set(host) == set(dev)
    for key, h in host.items():
        d = dev[key]
        if key == "cameras":
            assert len(d) == len(h)
            for ch, cd in zip(h, d):
                assert set(ch) == set(cd)
                for f, v in ch.items():
                    assert (torch.equal(cd[f], v) and cd[f].dtype == v.dtype) if torch.is_tensor(v) else np.array_equal(cd[f], v), f
        else:
            assert d.device.type == "cuda" and d.dtype == h.dtype and d.shape == h.shape, key
            assert torch.equal(d.cpu(), h), key
    assert dev["targets"].shape == (5, 3, cap.H, cap.W) and dev["masks"].shape == (5, cap.H, cap.W)


def test_load_step_repoints_a_fused_step(captures):
    """Compute object X is built from the host batch of items A; Y from items B, then re-pointed at A by `load_step`.  X run twice
    says whether the step is bit-reproducible here: if so Y must equal X bit for bit, otherwise within the project's
    fused-gradient bar (tensor-wide max-rel-err 1e-4)."""
    from manus_amd.engine import HipViewCompute
    from manus_amd.synthetic import camera_table
    cap = captures("64x48k1")
    ds, st = cap.ds, cap.store
    A, B = [0, 1, 2], [9, 10, 11]                            # the three cameras of the first frame / of the fourth
    ids, V = [0, 1, 2], 3

    def build(items):
        batch = ds.view_batch(items)
        scene, targets = D.hand_scene_from_batch(batch, ds[0]["bones_rest"], 2000, grid_res=24, seed=1, device=DEV)
        assert targets.shape == (V, 3, 48, 64)
        hc = HipViewCompute(scene, targets, camera_table(scene["cameras"], DEV), loss="l1+ssim", fused=True, persistent_grads=False,
                            mask_targets=scene["masks"].float().contiguous().clone())
        return hc

    def step(hc):
        out = hc(ids, 1.0 / V)
        torch.cuda.synchronize()
        return dict(loss=out["loss"].detach().clone().cpu(), **{k: g.detach().clone().cpu() for k, g in out["grads"].items()})

    def same(a, b, exact, what):
        worst = 0.0
        for key in a:
            if exact:
                assert torch.equal(a[key], b[key]), (what, key, max_rel_err(a[key].numpy(), b[key].numpy()))
            else:
                worst = max(worst, max_rel_err(a[key].numpy(), b[key].numpy()))
        print("%s: %s" % (what, "bit for bit" if exact else "max-rel-err %.3g" % worst))
        assert worst < 1e-4, (what, worst)

    X, Y = build(A), build(B)
    for k_ in X.params:
        assert torch.equal(X.params[k_], Y.params[k_])       # (the model is the same: only the views differ)
    x1, x2 = step(X), step(X)
    exact = all(torch.equal(x1[k_], x2[k_]) for k_ in x1)
    print("X run to run:", "bit for bit" if exact else "not bit for bit")
    y0 = step(Y)
    assert float(y0["loss"]) != float(x1["loss"])            # negative control: Y looks at other views
    assert not torch.equal(Y.targets, X.targets)
    st.load_step(Y, A)
    assert torch.equal(Y.targets, X.targets) and torch.equal(Y.mask_targets, X.mask_targets)
    assert torch.equal(Y.cams, X.cams) and torch.equal(Y.s["transforms"], X.s["transforms"])
    assert torch.equal(Y.s["keypoints"], X.s["keypoints"]) and torch.equal(Y.s["posed"], X.s["posed"])
    same(step(Y), x1, exact, "Y re-pointed at A against X")
    # the mask term on the decoded masks against the host masks
    X.w_mask = Y.w_mask = 0.5
    xm1, xm2 = step(X), step(X)
    exact_m = all(torch.equal(xm1[k_], xm2[k_]) for k_ in xm1)
    assert float(xm1["loss"]) != float(x1["loss"])
    same(step(Y), xm1, exact_m, "mask term: Y against X")
    # and back again through the dirty rectangles, in other slots: Y's rows 2, 0 take the items 10, 9
    st.load_step(Y, [10, 9], slots=[2, 0])
    Z = build([9, 1, 10])
    Z.w_mask = 0.5
    z1, z2 = step(Z), step(Z)
    assert torch.equal(Y.targets, Z.targets) and torch.equal(Y.mask_targets, Z.mask_targets) and torch.equal(Y.cams, Z.cams)
    same(step(Y), z1, all(torch.equal(z1[k_], z2[k_]) for k_ in z1), "two rows re-pointed: Y against Z")

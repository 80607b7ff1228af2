"""Deterministic inputs for the contact-evaluation kernels at seams, borders, ties and ragged sizes (numpy, seeded; no
torch, nothing of the code under test but the PALETTE).  tests/test_contact_eval_cases_cpu.py proves on the restatement
(contact_eval_ref.py) that every case holds what it was built for; tests/test_gpu_contact_eval_edges.py runs them.

Geometry the cases aim at: k_ceval_labels owns 64 x 16 pixels per workgroup (seams x = 63|64, y = 15|16) with one 16 x 16
occupancy tile per wave; k_ceval_fill walks tiles in rings; k_ceval_counts folds one record per 4096 pixels in groups of
16; k_ceval_fill's grid stride is 1024 * 256 residual pixels."""
import numpy as np

from manus_amd.contact_eval import PALETTE

TILE = 16
CHAIN_SIZES = [(1, 1, 1), (1, 1, 5), (2, 3, 2), (1, 5, 4), (1, 15, 63), (1, 16, 64), (2, 17, 65), (1, 16, 68), (3, 33, 130), (1, 47, 128)]
EDGE_BYTES = np.array([0, 127, 128, 129, 255], np.uint8)
# the +-10 boxes of entries 3 and 16 (173,198,231 / 156,217,228) share R 163..166, G 207..208, B 221..238: the only overlap
OVERLAP_LO, OVERLAP_HI = np.array([163, 207, 221]), np.array([166, 208, 238])
GROUND = np.array([60, 60, 60], np.uint8)            # in no box


def _rng(*key):
    return np.random.default_rng([20261021] + [int(k) for k in key])


def _cuts(n, first, step=6, least=3):
    """Cell borders along an axis of n pixels: first, first + step, ... with no cell thinner than `least` at either end.
    `first` is odd and `step` even, so no border falls on a multiple of 16: a cell straddles every tile edge."""
    cuts = [c for c in range(first, n, step) if c >= least and n - c >= least]
    return [0] + cuts + [n]


def _blob(g, H, W, lo=0.25, hi=0.6):
    """A random union of three ellipses with half-axes of lo .. hi of the image's sides (the default: about half the image)."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(3):
        cy, cx = g.uniform(0, H), g.uniform(0, W)
        ry, rx = g.uniform(lo, hi) * max(H, 2), g.uniform(lo, hi) * max(W, 2)
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return m


def _skin(g, H, W, shift):
    """The left half: a quilt of cells of palette colours (kind 0..15), of the 3 / 16 overlap (kind 16) and of ground
    (gaps: residual pixels), with per-channel jitter in [-12, 12]; then lines, exact +-10 / +-11 cells, 3 | overlap | 16
    stripes and an entry-15 block where they fit."""
    img = np.empty((H, W, 3), np.int64)
    ys, xs = _cuts(H, 3), _cuts(W, 3)
    n = 0
    for a in range(len(ys) - 1):
        for b in range(len(xs) - 1):
            y0, y1, x0, x1 = ys[a], ys[a + 1], xs[b], xs[b + 1]
            on_seam = any(y0 < e <= y1 - 1 for e in range(TILE, H, TILE)) or any(x0 < e <= x1 - 1 for e in range(TILE, W, TILE))
            on_border = y0 == 0 or x0 == 0 or y1 == H or x1 == W
            kind = (n + shift) % 17
            n += 1
            shape = (y1 - y0, x1 - x0, 3)
            if not on_seam and not on_border and (a * 5 + b * 3 + shift) % 7 == 0:
                img[y0:y1, x0:x1] = g.integers(0, 256, shape)                 # a gap: noise, mostly in no box
                continue
            if kind == 16:
                img[y0:y1, x0:x1] = g.integers(OVERLAP_LO, OVERLAP_HI + 1, shape)
                continue
            jit = g.integers(-10, 11, shape)
            out = g.random(shape[:2]) < 0.05                                  # some pixels just outside, on one channel
            ch = g.integers(0, 3, shape[:2])
            far = g.choice(np.array([-12, -11, 11, 12]), shape[:2])
            for c in range(3):
                jit[..., c] = np.where(out & (ch == c), far, jit[..., c])
            if (a + b) % 5 == 0:                                              # the whole cell exactly on / just off the box's faces
                face = (a + 2 * b) % 4
                jit[:] = np.array([(10, -10, 10), (-10, 10, -10), (11, 0, 0), (0, 0, -11)])[face % 2 if on_seam or on_border else face]
            img[y0:y1, x0:x1] = PALETTE[kind].astype(np.int64) + jit
    if H >= 15 and W >= 60:
        img[4:10, 20:31] = GROUND                                             # one-pixel-wide lines: the opening removes them
        img[7, 20:31] = PALETTE[6]
        img[4:10, 25] = PALETTE[6]
        img[4:10, 36:39] = PALETTE[2].astype(np.int64) + (5, -5, 3)           # entry 3 only
        img[4:10, 39:42] = g.integers(OVERLAP_LO, OVERLAP_HI + 1, (6, 3, 3))  # both: the first match, label 3
        img[4:10, 42:45] = PALETTE[15].astype(np.int64) + (-5, 5, -3)         # entry 16 only
        img[4:10, 48:54] = PALETTE[14]                                        # entry 15
    return np.clip(img, 0, 255).astype(np.uint8)


def chain_case(V, H, W):
    """(frame uint8 (V,H,2W,3), seg (V,H,W,3), rgba (V,H,W,4)).  Right half and seg: bytes of {0,127,128,129,255}; alpha of
    the same set, above 128 inside the hand.  Hands: the image with random blobs cut out; with V >= 2 the last view's is empty and the one before
    it full."""
    g = _rng(1, V, H, W)
    frame = np.empty((V, H, 2 * W, 3), np.uint8)
    for v in range(V):
        frame[v, :, :W] = _skin(g, H, W, 5 * v + H + W)
    frame[:, :, W:] = g.choice(EDGE_BYTES, (V, H, W, 3), p=[0.1, 0.15, 0.25, 0.25, 0.25])
    seg = g.choice(EDGE_BYTES, (V, H, W, 3), p=[0.1, 0.15, 0.25, 0.25, 0.25])
    rgba = g.integers(0, 256, (V, H, W, 4)).astype(np.uint8)
    for v in range(V):
        hand = ~_blob(g, H, W, 0.05, 0.18) if H * W > 16 else g.random((H, W)) < 0.7      # the image but for three blobs
        if V == 1 and H * W <= 16:
            hand[:] = True                                                    # (one pixel / one row: keep the hand)
        if V >= 2 and v == V - 1:
            hand[:] = False
        if V >= 2 and v == V - 2:
            hand[:] = True
        rgba[v, ..., 3] = np.where(hand, g.choice(np.array([129, 255], np.uint8), (H, W)), g.choice(np.array([0, 127, 128], np.uint8), (H, W)))
    return frame, seg, rgba


# ---------------------------------------------------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------------------------------------------------
def _cross(frame, hand, cy, cx, entry):
    """A 5-pixel cross of an exact palette colour, clipped to the image: the smallest thing the opening keeps."""
    H, W = hand.shape
    for dy, dx in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        y, x = cy + dy, cx + dx
        if 0 <= y < H and 0 <= x < W:
            frame[y, x] = PALETTE[entry % 16]
            hand[y, x] = 1


def _residual(hand, y, x, around=True):
    H, W = hand.shape
    for dy, dx in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)) if around else ((0, 0),):
        if 0 <= y + dy < H and 0 <= x + dx < W:
            hand[y + dy, x + dx] = 1


def _ties(H, W):
    """Per tile two motifs, each a residual pixel R with two crosses of different colours whose nearest pixels lie at
    d^2 = 16: the loser in R's own tile (ring 0), the winner -- the lower index -- in the tile above / to the left (ring 1),
    on that tile's last row / column, so that it stands exactly at the least distance ring 1 can have from R (1 + 3 pixels)
    and at the least distance its tile can have: a search that gives up a ring or a tile at 'not nearer' loses it.
        up:    R = (Y + 3, X + 9); loser left (Y + 3, X + 5) or right (Y + 3, X + 13); winner (Y - 1, X + 9)
        left:  R = (Y + 8, X + 3); loser right (Y + 8, X + 7) or below (Y + 12, X + 3); winner (Y + 8, X - 1)
    R's four neighbours are residual too (no tie: the nearer cross wins)."""
    frame, hand = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    k = 0
    for ty in range((H + TILE - 1) // TILE):
        for tx in range((W + TILE - 1) // TILE):
            Y, X = ty * TILE, tx * TILE
            if ty >= 1 and Y + 4 < H and X + 15 < W:
                _cross(frame, hand, Y + 3, X + 14 if tx % 2 else X + 4, 2 * k)
                _cross(frame, hand, Y - 2, X + 9, 2 * k + 1)
                _residual(hand, Y + 3, X + 9)
                k += 1
            if tx >= 1 and Y + 14 < H and X + 9 < W:
                if ty % 2:
                    _cross(frame, hand, Y + 13, X + 3, 2 * k)
                else:
                    _cross(frame, hand, Y + 8, X + 8, 2 * k)
                _cross(frame, hand, Y + 8, X - 2, 2 * k + 1)
                _residual(hand, Y + 8, X + 3)
                k += 1
    return frame[None], hand[None]


def _corner(H, W, cy, cx, entry):
    frame, hand = np.zeros((H, W, 3), np.uint8), np.ones((H, W), np.uint8)
    _cross(frame, hand, cy, cx, entry)
    return frame[None], hand[None]


def _far_box():
    H, W = 40, 200
    frame, hand = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    for cy, cx, e in ((5, 196, 3), (20, 195, 7), (35, 197, 14)):
        _cross(frame, hand, cy, cx, e)
    hand[:, :TILE] = 1
    return frame[None], hand[None]


def _every_pixel():
    H = W = 520
    frame, hand = np.zeros((H, W, 3), np.uint8), np.ones((H, W), np.uint8)
    _cross(frame, hand, 260, 260, 4)
    _cross(frame, hand, 260 + 2 * TILE, 260 - 2 * TILE, 9)
    return frame[None], hand[None]


def _mixed_batch():
    """view 0 normal; view 1 residual pixels and nothing labelled; view 2 nothing at all"""
    V, H, W = 3, 33, 47
    g = _rng(2, V, H, W)
    frame, hand = np.zeros((V, H, W, 3), np.uint8), np.zeros((V, H, W), np.uint8)
    for cy, cx, e in ((3, 4, 0), (16, 15, 5), (31, 45, 15), (20, 33, 10)):
        _cross(frame[0], hand[0], cy, cx, e)
    hand[0] |= _blob(g, H, W).astype(np.uint8)
    hand[1] = _blob(g, H, W)
    hand[1, 0, 0] = 1
    frame[1] = 3                                                              # in no box
    return frame, hand


FILL_CASES = ["ties-48x80", "ties-33x130", "far-box", "corner-16", "corner-17", "corner-5x7", "every-pixel", "mixed-batch"]


def fill_case(name):
    """(frame_left (V,H,W,3) uint8, hand (V,H,W) uint8)"""
    if name == "ties-48x80":
        return _ties(48, 80)
    if name == "ties-33x130":
        return _ties(33, 130)
    if name == "far-box":
        return _far_box()
    if name == "corner-16":
        return _corner(16, 16, 0, 0, 1)                                       # clipped to three pixels in the corner
    if name == "corner-17":
        return _corner(17, 17, 16, 16, 12)                                    # in the one-pixel edge tile
    if name == "corner-5x7":
        return _corner(5, 7, 4, 0, 8)
    if name == "every-pixel":
        return _every_pixel()
    if name == "mixed-batch":
        return _mixed_batch()
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------
# counts, collage, fp32 frame
# ---------------------------------------------------------------------------------------------------------------------
COUNT_SIZES = [(1, 260, 260), (2, 259, 261), (1, 1, 3), (3, 64, 64)]


def count_case(V, H, W):
    """(pred, gt, labels) (V,H,W) uint8: pred / gt of {0, 1, 255}, empty outside blobs; labels 0..16.  V = 3: view 1 is zero."""
    g = _rng(3, V, H, W)
    vals = np.array([0, 1, 255], np.uint8)
    pred, gt = g.choice(vals, (V, H, W)), g.choice(vals, (V, H, W))
    labels = g.integers(0, 17, (V, H, W)).astype(np.uint8)
    if H * W > 16:
        for v in range(V):
            pred[v] *= _blob(g, H, W).astype(np.uint8)
            gt[v] *= _blob(g, H, W).astype(np.uint8)
    if V == 3:
        pred[1] = 0
        gt[1] = 0
    return pred, gt, labels


COLLAGE_SIZES = [(2, 3, 5), (1, 16, 64)]
COLLAGE_M = [0, 1, 16]


def collage_case(V, H, W, M):
    """(rgba (V,H,W,4), masks (M,V,H,W)).  At H * W = 1024 every photo byte 0..255 occurs in every channel with alpha both
    sides of the threshold; alpha of {0,127,128,129,255}; masks of {0,1,255}."""
    g = _rng(4, V, H, W, M)
    rgba = g.integers(0, 256, (V, H, W, 4)).astype(np.uint8)
    rgba[..., 3] = g.choice(EDGE_BYTES, (V, H, W))
    if H * W % 1024 == 0:
        p = g.permutation(H * W)
        for c in range(3):
            rgba[0, ..., c].reshape(-1)[p] = (np.arange(H * W) + 85 * c) % 256
        rgba[0, ..., 3].reshape(-1)[p] = np.array([127, 129, 128, 255], np.uint8)[(np.arange(H * W) // 256) % 4]
    masks = g.choice(np.array([0, 1, 255], np.uint8), (M, V, H, W))
    return rgba, masks


def f32_frame_case():
    """(frame float32 (1,8,256,3), seg, rgba) at (1,8,128): float32(k / 255) and its neighbours both ways for every k, -0.0,
    +-inf, NaN, -0.3, 1.7 and subnormals, all of them in both halves."""
    V, H, W = 1, 8, 128
    g = _rng(5, V, H, W)
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    vals = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2)),
                           np.array([-0.0, np.inf, -np.inf, np.nan, -0.3, 1.7, 1e-45, -1e-45, 1e-39, 5.8e-39, 0.5, 1.0], np.float32)]).astype(np.float32)
    frame = np.empty((V, H, 2 * W, 3), np.float32)
    for half in (0, 1):
        n = H * W * 3
        fill = np.concatenate([vals, g.uniform(-0.1, 1.1, n - len(vals)).astype(np.float32)])
        frame[0, :, half * W:(half + 1) * W] = g.permutation(fill).reshape(H, W, 3)
    seg = g.choice(EDGE_BYTES, (V, H, W, 3))
    rgba = g.integers(0, 256, (V, H, W, 4)).astype(np.uint8)
    return frame, seg, rgba, vals

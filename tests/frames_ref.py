"""numpy restatement of mgr_frames_decode (include/manus_hip.h): the crop inside its bbox and zeros outside, the integer block
mean, the fp64 composite rounded to fp32 once.  tests/test_frames_cpu.py pins it to SequenceDataset.fetch_images bit for bit;
the GPU tests compare the kernel with it bit for bit."""
import numpy as np

LUT = np.arange(256, dtype=np.float64) / 255.0


def block_mean(frame, k):
    """(H k, W k, 4) uint8 -> (H, W, 4) integers: (2 s + k^2) // (2 k^2) of the block sums s."""
    if k == 1:
        return frame.astype(np.int64)
    Hs, Ws = frame.shape[:2]
    assert Hs % k == 0 and Ws % k == 0
    s = frame.reshape(Hs // k, k, Ws // k, k, 4).astype(np.int64).sum((1, 3))
    return (2 * s + k * k) // (2 * k * k)


def decode_ref(crop, bbox, bg, H, W, k=1):
    """target (3,H,W) float32 and mask (H,W) float32 of one view.  crop (h,w,4) uint8 at bbox = (x0,y0,x1,y1) in source pixels
    of the (H k, W k) source frame; bg: three floats (taken as float32, like the kernel's record)."""
    x0, y0, x1, y1 = (int(t) for t in bbox)
    frame = np.zeros((H * k, W * k, 4), np.uint8)
    if x1 > x0 and y1 > y0:
        frame[y0:y1, x0:x1] = np.asarray(crop, np.uint8).reshape(y1 - y0, x1 - x0, 4)
    m = block_mean(frame, k)
    c, a = LUT[m[..., :3]], LUT[m[..., 3:]]
    b = np.asarray(bg, np.float32).astype(np.float64)
    rgb = c * a + b * (1.0 - a)
    return np.ascontiguousarray(rgb.astype(np.float32).transpose(2, 0, 1)), a[..., 0].astype(np.float32)


def out_rect(bbox, k):
    """The bbox in output pixels, rounded outwards; (0,0,0,0) for an empty crop."""
    x0, y0, x1, y1 = (int(t) for t in bbox)
    if x1 <= x0 or y1 <= y0:
        return (0, 0, 0, 0)
    return (x0 // k, y0 // k, -(-x1 // k), -(-y1 // k))

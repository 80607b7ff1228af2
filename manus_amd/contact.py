"""Hand <-> object contact distances over the HIP kernel of `csrc/contact.hip`.

Mirrors src/utils/gaussian_utils.py of brown-ivl/manus:

    get_contact_map(pt1, pt2, chunk)    :514-518   chunked torch.cdist(...).min(1)[0]
    get_contact_dist(pt1, pt2)          :521-549   taichi brute-force nearest point, distance + index
    get_cmap(pt1, pt2, c_thresh)        :571-577   1 - clamp(dist, 0, c_thresh) / c_thresh (+ a matplotlib colour map,
                                                   which stays with the caller)
    get_cmap / get_cmap_near / get_colors_from_cmap (below) add the colour map on the device: see their docstrings

GPU tensors only; there is no CPU fallback.
"""
import torch

from . import colormap
from ._lib import ManusHipError, check, f32c, lib, ptr, stream


def _nearest(pt1, pt2, want_idx):
    pt1, pt2 = f32c(pt1), f32c(pt2)
    if not pt1.is_cuda or not pt2.is_cuda:
        raise ManusHipError("manus_amd.contact needs GPU tensors; there is no CPU fallback")
    if pt1.dim() != 2 or pt1.shape[1] != 3 or pt2.dim() != 2 or pt2.shape[1] != 3:
        raise ManusHipError("contact: points are (N,3)")
    n1, n2 = pt1.shape[0], pt2.shape[0]
    dist = torch.empty((n1,), dtype=torch.float32, device=pt1.device)
    idx = torch.empty((n1,), dtype=torch.int32, device=pt1.device) if want_idx else None
    nbytes = int(lib().mgr_contact_workspace_bytes(n1, n2))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=pt1.device)
    check(lib().mgr_contact_dist(n1, ptr(pt1), n2, ptr(pt2), ptr(dist), ptr(idx), ptr(ws), nbytes, stream()),
          "mgr_contact_dist")
    return dist, idx


def get_contact_dist(pt1, pt2):
    """(distance to the nearest point of pt2, its index as float32 like the reference's taichi ndarray)."""
    dist, idx = _nearest(pt1, pt2, True)
    return dist, idx.to(torch.float32)


def get_contact_map(pt1, pt2, chunk=1024):
    """Distance of every point of pt1 to its nearest point of pt2 (`chunk` kept for signature parity)."""
    return _nearest(pt1, pt2, False)[0]


def get_cmap_values(pt1, pt2, c_thresh=0.004):
    """(1 - clamp(dist, 0, c_thresh)/c_thresh, indices): get_cmap without the colour-map lookup."""
    dist, idx = get_contact_dist(pt1, pt2)
    return 1 - torch.clamp(dist.clone(), 0, c_thresh) / c_thresh, idx


# ---------------------------------------------------------------------------------------------------------------------
# Contact maps with their colours on the device: get_cmap (gaussian_utils.py:571-577) and get_colors_from_cmap
# (src/utils/vis_util.py:22-25) without the device -> numpy -> matplotlib -> device round trip.
# ---------------------------------------------------------------------------------------------------------------------
def _points(pt1, pt2, what):
    pt1, pt2 = f32c(pt1), f32c(pt2)
    if not pt1.is_cuda or not pt2.is_cuda:
        raise ManusHipError("manus_amd.contact needs GPU tensors; there is no CPU fallback")
    if pt1.dim() != 2 or pt1.shape[1] != 3 or pt2.dim() != 2 or pt2.shape[1] != 3:
        raise ManusHipError(what + ": points are (N,3)")
    return pt1, pt2


def contact_values(dist, c_thresh=0.004):
    """1 - clamp(dist, 0, c_thresh) / c_thresh in fp32 with an IEEE division (`mgr_contact_values`).  `get_cmap_values`
    leaves the division to torch, which on the device multiplies by the rounded reciprocal of a Python scalar; the contact
    renders and their CPU references divide."""
    dist = f32c(dist)
    out = torch.empty_like(dist)
    check(lib().mgr_contact_values(dist.numel(), ptr(dist), float(c_thresh), ptr(out), stream()), "mgr_contact_values")
    return out


def contact_near(pt1, pt2, c_thresh=0.004, want_dist=False):
    """`mgr_contact_near`: (value (N1,), index (N1,) int32, distance (N1,) or None) of the nearest point of pt2 within
    c_thresh.  value is that of the brute-force search for every point; index is -1 and distance 1e9 where value is 0."""
    pt1, pt2 = _points(pt1, pt2, "contact_near")
    n1, n2 = pt1.shape[0], pt2.shape[0]
    value = torch.empty((n1,), dtype=torch.float32, device=pt1.device)
    idx = torch.empty((n1,), dtype=torch.int32, device=pt1.device)
    dist = torch.empty((n1,), dtype=torch.float32, device=pt1.device) if want_dist else None
    nbytes = int(lib().mgr_contact_near_workspace_bytes(n1, n2))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=pt1.device)
    check(lib().mgr_contact_near(n1, ptr(pt1), n2, ptr(pt2), float(c_thresh), ptr(value), ptr(idx), ptr(dist), ptr(ws), nbytes,
                                 stream()), "mgr_contact_near")
    return value, idx, dist


def contact_colors(values, cmap="gray", base=None, alpha=0.0):
    """(N,3) colours of `values` (N,) on the 256-entry map `cmap` (a name or a (256,3) table), exactly matplotlib's lookup;
    with `base` (N,3): base * alpha + (1 - alpha) * colours, the blend of composite.py:153,160 in its operation order."""
    values = f32c(values).reshape(-1)
    table = colormap.lut(cmap, values.device)
    n = values.shape[0]
    if base is not None:
        base = f32c(base)
        if tuple(base.shape) != (n, 3):
            raise ManusHipError("contact_colors: base is (N,3)")
    out = torch.empty((n, 3), dtype=torch.float32, device=values.device)
    # the reference multiplies by the Python float (1 - alpha), rounded to fp32 by torch: not by 1.0f - (float)alpha
    check(lib().mgr_contact_colors(n, ptr(values), ptr(table), ptr(base), float(alpha), float(1.0 - float(alpha)), None, 0, None,
                                   ptr(out), stream()), "mgr_contact_colors")
    return out


def contact_table_colors(values, table, idx_nn=None):
    """NOCS renders (composite.py:165-183): table[idx_nn[n]] (or table[n]) where values[n] > 0, black elsewhere."""
    values, table = f32c(values).reshape(-1), f32c(table)
    n = values.shape[0]
    if table.dim() != 2 or table.shape[1] != 3:
        raise ManusHipError("contact_table_colors: table is (M,3)")
    if idx_nn is not None:
        idx_nn = idx_nn.to(torch.int32).contiguous()
        if idx_nn.shape[0] != n:
            raise ManusHipError("contact_table_colors: one index per value")
    out = torch.empty((n, 3), dtype=torch.float32, device=values.device)
    check(lib().mgr_contact_colors(n, ptr(values), None, None, 0.0, 1.0, ptr(table), table.shape[0], ptr(idx_nn), ptr(out),
                                   stream()), "mgr_contact_colors")
    return out


def get_colors_from_cmap(values, cmap_name="viridis"):
    """vis_util.py:22-25 on a device tensor: `plt.get_cmap(cmap_name)(values)[..., :3]` as fp32, shape values.shape + (3,)."""
    return contact_colors(values, cmap_name).reshape(tuple(values.shape) + (3,))


def get_cmap(pt1, pt2, c_thresh=0.004, cmap_type="gray"):
    """gaussian_utils.py:571-577: (value, indices as float32, (N,3) colours), on the brute-force search, so the indices are
    the reference's for every point."""
    dist, idx = get_contact_dist(pt1, pt2)
    value = contact_values(dist, c_thresh)
    return value, idx, contact_colors(value, cmap_type)


def get_cmap_near(pt1, pt2, c_thresh=0.004, cmap_type="gray"):
    """`get_cmap` on the grid search: same value and colours for every point, same index wherever value > 0, index -1
    elsewhere (the reference reads indices only under the mask value > 0, composite.py:176-183)."""
    value, idx, _ = contact_near(pt1, pt2, c_thresh)
    return value, idx.to(torch.float32), contact_colors(value, cmap_type)

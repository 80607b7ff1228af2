"""256-entry colour tables on the device for the contact renders.

The reference colours a contact map with matplotlib on the host (`plt.get_cmap(name)(values)`,
src/utils/vis_util.py:22-25): device -> numpy -> matplotlib -> device on every render.  Here the
table of a map is uploaded once and the lookup is part of `mgr_contact_colors`.
"""
import numpy as np
import torch

from ._lib import ManusHipError

_CACHE = {}      # (name, device) -> (256,3) fp32 tensor


def _table(name):
    if name == "gray":       # i / 255, what matplotlib's 'gray' holds in its 256 entries: no matplotlib needed
        return np.repeat((np.arange(256, dtype=np.float64) / 255.0)[:, None], 3, axis=1).astype(np.float32)
    try:
        import matplotlib
    except ImportError:
        raise ManusHipError("colour map %r needs matplotlib, which is not installed: pass a (256,3) array of colours "
                            "instead of a name (only 'gray' is built in)" % (name,))
    return np.asarray(matplotlib.colormaps[name].resampled(256)(np.arange(256))[:, :3]).astype(np.float32)


def lut(name_or_tensor, device):
    """(256,3) fp32 table on `device` of a map name (cached per name and device) or of a (256,3) array / tensor."""
    device = torch.device(device)
    if isinstance(name_or_tensor, str):
        key = (name_or_tensor, str(device))
        t = _CACHE.get(key)
        if t is None:
            t = _CACHE[key] = torch.from_numpy(_table(name_or_tensor)).to(device)
        return t
    t = torch.as_tensor(name_or_tensor, dtype=torch.float32)
    if tuple(t.shape) != (256, 3):
        raise ManusHipError("a colour table is (256,3), got %s" % (tuple(t.shape),))
    return t.to(device).contiguous()

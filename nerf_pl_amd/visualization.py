"""`utils/visualization.py` of the reference (visualization.py:6-17) on the GPU: `visualize_depth` is two HIP launches
(`nerfhip_depth_colormap`); the depth image never visits the host and there is no cv2 / PIL / torchvision dependency."""
import torch

from . import ops
from ._lib import NerfHipError, require_gpu

COLORMAP_JET = 2          # cv2.COLORMAP_JET, the reference's default

_TABLES = {}


def _table(kind, device):
    key = (kind, str(device))
    if key not in _TABLES:
        if kind == "jet":
            from .imageio_min import jet_table
            t = torch.from_numpy(jet_table())
        else:
            t = torch.arange(256, dtype=torch.uint8).unsqueeze(1).repeat(1, 3)
        _TABLES[key] = t.to(device)
    return _TABLES[key]


def visualize_depth(depth, cmap=COLORMAP_JET):
    """depth: (H, W) on the GPU -> (3, H, W) float32 in [0, 1] on the same device (NaN -> 0, +-inf -> +-FLT_MAX, normalised by
    the image's minimum and maximum, 8-bit index, colour table, byte / 255: numpy's float32 arithmetic bit for bit).

    cmap: 2 (cv2.COLORMAP_JET, the built-in table), None (no colours: the 8-bit index on all three channels) or a (256, 3)
    uint8 tensor, e.g. `cv2.applyColorMap(np.arange(256, dtype=np.uint8), m).reshape(256, 3)` of any cv2 map m.
    Channel order is the reference's: it hands cv2's BGR image to PIL as if it were RGB, so channel 0 of the result is the
    colour map's BLUE and channel 2 its red; a table's columns are in that (output) order."""
    if not (cmap is None or torch.is_tensor(cmap) or (type(cmap) is int and cmap == COLORMAP_JET)):
        raise ValueError("visualize_depth: cmap must be 2 (JET), None or a (256, 3) uint8 tensor, got %r" % (cmap,))
    if not torch.is_tensor(depth):
        raise NerfHipError("visualize_depth: expected a torch tensor, got %s" % type(depth).__name__)
    require_gpu(depth)
    if depth.dim() != 2:
        raise ValueError("visualize_depth: depth must be (H, W), got %s" % (tuple(depth.shape),))
    if torch.is_tensor(cmap):
        table = cmap
    else:
        table = _table("index" if cmap is None else "jet", depth.device)
    return ops.depth_colormap(depth, table, want_float=True, want_bytes=False)[0]

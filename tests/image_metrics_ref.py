"""Restatements that the image-metric tests compare the HIP kernels with (CPU, torch / numpy only).

* `ssim_map(img1, img2, ws, dtype)`: kornia 0.2.0's `kornia.losses.ssim` behind the reference's `metrics.ssim`
  (metrics.py:15-20) as include/nerfhip.h states it — a ws x ws Gaussian window (sigma 1.5), depth-wise `F.conv2d` with zero
  padding, the five filtered products, `1 - 2 * clamp(1 - map, 0, 1) / 2` — in float64 (the yardstick) or float32 (what the
  reference's own arithmetic gives: its distance from the float64 map is the tests' tolerance).
* `depth_index(depth)` / `depth_colors(depth, table)`: `visualize_depth` (utils/visualization.py:6-17) in numpy float32.
"""
import numpy as np
import torch
import torch.nn.functional as F


def gaussian_window(ws, dtype=torch.float64):
    """(ws, ws) outer product of g[i] = exp(-(i - ws//2)^2 / (2 * 1.5^2)), normalised to sum 1 along each axis."""
    g = torch.tensor([np.exp(-((i - ws // 2) ** 2) / (2.0 * 1.5 ** 2)) for i in range(ws)], dtype=dtype)
    g = g / g.sum()
    return g[:, None] * g[None, :]


def ssim_map(img1, img2, ws, dtype=torch.float64):
    """img1, img2 (B,C,H,W) -> the (B,C,H,W) map of `metrics.ssim(..., reduction='none')`, computed in `dtype`."""
    a, b = img1.to(dtype), img2.to(dtype)
    C = a.shape[1]
    win = gaussian_window(ws, dtype)[None, None].repeat(C, 1, 1, 1)
    pad = (ws - 1) // 2

    def filt(x):
        return F.conv2d(x, win, padding=pad, groups=C)
    mu1, mu2 = filt(a), filt(b)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11 = filt(a * a) - mu1_sq
    s22 = filt(b * b) - mu2_sq
    s12 = filt(a * b) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2))
    dssim = torch.clamp(1 - m, 0, 1) / 2
    return 1 - 2 * dssim


def depth_index(depth):
    """The 8-bit index image of visualize_depth, numpy float32 arithmetic.  A NaN quotient (inf / inf: an image that holds both
    infinities overflows `ma - mi`) becomes 0, which is what `astype(np.uint8)` gives on x86-64; stated here so that the
    restatement does not depend on the platform."""
    x = np.nan_to_num(np.asarray(depth, dtype=np.float32))
    mi, ma = np.min(x), np.max(x)
    with np.errstate(all="ignore"):
        x = (x - mi) / (ma - mi + np.float32(1e-8))
        v = np.float32(255) * x
        assert v.dtype == np.float32
        return np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)


def depth_colors(depth, table):
    """-> ((3,H,W) float32 = ToTensor of the table lookup, (H,W,3) uint8); table (256,3) uint8 in output channel order."""
    idx = depth_index(depth)
    rgb = np.asarray(table, dtype=np.uint8)[idx]
    return np.moveaxis(rgb.astype(np.float32) / np.float32(255), -1, 0), rgb

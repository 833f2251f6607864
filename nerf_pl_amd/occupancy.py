"""Skipping empty space at eval: an occupancy bitfield of the trained density and a renderer wrapper that runs
the inner renderer only on the rays that cross occupied cells, each with [near, far] tightened to the occupied stretch.

    grid = OccupancyGrid.from_model(nerf_fine, 128, (-1.2, 1.2), (-1.2, 1.2), (-1.2, 1.2), sigma_threshold=0.0, dilate=1)
    renderer = CulledRenderer(GraphRenderer(models, embeddings, white_back=True), grid, white_back=True, tighten="none")
    inference.evaluate(dataset, renderer)

Opt-in, and entirely beside the render path: rays carry their own near and far (columns 6 and 7), so a tightened interval is
an edit of the ray rows and no render kernel changes.  The reference has no counterpart; without these classes every output
is what it was.  Cull, compaction and scatter are HIP kernels (csrc/occupancy.hip); there is no torch-indexing stand-in.
"""
import numpy as np
import torch

from . import grid as _grid
from . import ops
from ._lib import NerfHipError

__all__ = ["OccupancyGrid", "CulledRenderer"]


def _pair(r):
    lo, hi = (float(v) for v in r)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("an axis range must be finite with lo < hi, got %r" % (r,))
    return lo, hi


class OccupancyGrid:
    """One bit per cell of the (N-1)^3 cells between the points of an N^3 sigma lattice (include/nerfhip.h holds the format):
    `bits` (int32 words on the device), `M` cells per axis, `ranges` = ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi))."""

    def __init__(self, bits, M, ranges, sigma_threshold=0.0, dilate=0):
        self.M = int(M)
        self.ranges = tuple(_pair(r) for r in ranges)
        if len(self.ranges) != 3:
            raise ValueError("ranges must be three (lo, hi) pairs")
        if not torch.is_tensor(bits) or not bits.is_cuda:
            raise NerfHipError("nerf_pl_amd runs on MI355X only: the bitfield must be a device tensor (no CPU fallback)")
        if bits.dtype != torch.int32 or bits.dim() != 1 or self.M < 1 or bits.numel() != ops.occupancy_words(self.M):
            raise ValueError("a grid of %d^3 cells needs %d int32 words, got %s %s"
                             % (self.M, ops.occupancy_words(max(self.M, 0)), tuple(bits.shape), bits.dtype))
        self.bits = bits.contiguous()
        self.sigma_threshold = float(sigma_threshold)
        self.dilate = int(dilate)

    @classmethod
    def from_sigma(cls, sigma, x_range, y_range, z_range, sigma_threshold=0.0, dilate=1):
        """sigma (N, N, N) on the device, indexed [iy, ix, iz] as `grid.sigma_grid` returns it, on the lattice whose first and
        last points are the ranges' ends.  A cell is occupied iff one of its 8 corners is > sigma_threshold (or NaN); the set is
        then dilated by `dilate` cells."""
        bits = ops.occupancy_build(sigma, sigma_threshold, dilate)
        return cls(bits, sigma.shape[0] - 1, (x_range, y_range, z_range), sigma_threshold, dilate)

    @classmethod
    def from_model(cls, model, N, x_range, y_range, z_range, sigma_threshold=0.0, dilate=1, embedding_xyz=None):
        """`grid.sigma_grid(model, N, ...)` (the fused sigma-only kernel; a non-default NeRF needs `embedding_xyz`), then
        `from_sigma`."""
        sigma = _grid.sigma_grid(model, N, x_range, y_range, z_range, embedding_xyz=embedding_xyz)
        return cls.from_sigma(sigma, x_range, y_range, z_range, sigma_threshold, dilate)

    def occupied_fraction(self):
        """Occupied cells / M^3 (one host read; the unused bits of the last word are zero)."""
        w = self.bits.cpu().numpy().view(np.uint32)
        return float(np.unpackbits(w.view(np.uint8)).sum()) / float(self.M ** 3)

    def save(self, path):
        """One .npz holding the settings and the words, nothing else."""
        np.savez(path, words=self.bits.cpu().numpy(), M=np.int64(self.M), ranges=np.asarray(self.ranges, np.float64),
                 sigma_threshold=np.float64(self.sigma_threshold), dilate=np.int64(self.dilate))

    @classmethod
    def load(cls, path, device=None):
        z = np.load(path, allow_pickle=False)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return cls(torch.from_numpy(np.ascontiguousarray(z["words"], np.int32)).to(dev), int(z["M"]),
                   [tuple(r) for r in z["ranges"].tolist()], float(z["sigma_threshold"]), int(z["dilate"]))

    def cull(self, rays):
        """rays (n, 8) on the device -> (hit (n,) uint8, t0 (n,), t1 (n,)): the ray crosses occupied cells inside [t0, t1], a
        sub-interval of its [near, far]; a miss has hit == 0."""
        return ops.cull_rays(rays, self.bits, self.M, self.ranges)


class CulledRenderer:
    """`renderer` (any callable rays (n, 8) -> dict of (n, ...) tensors: a `GraphRenderer`, a closure over
    `batched_inference`) run on the rays that hit `grid` only, with their near and far tightened; the other rows of every output
    are the background: 1.0 (white_back) or 0.0 for keys starting with 'rgb', 0.0 for the rest — what the reference's
    compositing gives for all-zero weights.  Per call: cull, compact, one 4-byte read of the number of hits, the inner render,
    one scatter launch per four outputs.  `stats` counts rays seen and rays rendered.

    `tighten`: which ends of [near, far] the hits get from the cull — "both" (t0 and t1), "near" (t0 only; far stays) or "none"
    (the rays go to the inner renderer as they came: culling only).  The time of a call depends on the number of rays rendered,
    not on the interval, so this is a choice of sampling, not of speed.  WARNING: "both" is the default because it is what the class
    was specified to do, but moving `far` cost 5 dB and more on the one scene measured (the reference's compositing gives the last
    sample of a ray an unbounded thickness): prefer "near" or "none" unless the scene has been checked.

    A call with any hit costs at least one whole chunk of the inner renderer where that pads a ragged tail, as `GraphRenderer`
    does: the time follows the number of chunks, not the exact share of rays."""

    def __init__(self, renderer, grid, white_back, tighten="both"):
        if tighten not in ("both", "near", "none"):
            raise ValueError("tighten must be 'both', 'near' or 'none', got %r" % (tighten,))
        self.renderer = renderer
        self.grid = grid
        self.white_back = bool(white_back)
        self.tighten = tighten
        self.stats = {"rays": 0, "rendered": 0, "calls": 0}
        self._keys = None             # the inner renderer's keys and row shapes, known after its first call

    def _background(self, n, dev):
        """Every ray missed before the inner renderer ever ran: its keys are not known, so the reference's test-time set is
        returned."""
        keys = self._keys or {"opacity_coarse": (), "rgb_fine": (3,), "depth_fine": (), "opacity_fine": ()}
        out = {}
        slot = torch.full((n,), -1, device=dev, dtype=torch.int32)
        for k, tail in keys.items():
            empty = torch.empty((0,) + tail, device=dev, dtype=torch.float32)
            if tail == (3,):
                out[k] = ops.cull_scatter(slot, self.white_back and k.startswith("rgb"), rgb=empty)[0]
            else:
                out[k] = ops.cull_scatter(slot, False, depth=empty)[1]
        return out

    @torch.no_grad()
    def __call__(self, rays):
        n = rays.shape[0]
        hit, t0, t1 = self.grid.cull(rays)
        slot, _, compact, n_hit = ops.cull_compact(hit, rays, t0 if self.tighten != "none" else None,
                                                   t1 if self.tighten == "both" else None)
        k = int(n_hit.item())                              # the one host read
        self.stats["rays"] += n
        self.stats["rendered"] += k
        self.stats["calls"] += 1
        if k == 0:
            return self._background(n, rays.device)
        inner = self.renderer(compact[:k])
        self._keys = {key: tuple(v.shape[1:]) for key, v in inner.items()}
        out = {}
        vec, scal = [], []
        for key, v in inner.items():
            if v.shape[0] != k or v.dtype != torch.float32 or tuple(v.shape[1:]) not in ((3,), ()):
                raise NerfHipError("CulledRenderer: output %r is %s %s; per-ray fp32 (n, 3) or (n,) outputs can be scattered"
                                   % (key, tuple(v.shape), v.dtype))
            (vec if v.dim() == 2 else scal).append(key)
        # one launch takes a 3-channel output and up to three scalars; 3-channel keys that are not colours get a zero background
        while vec or scal:
            kv = vec.pop(0) if vec else None
            ks = [scal.pop(0) for _ in range(min(3, len(scal)))]
            args = [inner[kv] if kv is not None else None] + [inner[s] for s in ks] + [None] * (3 - len(ks))
            res = ops.cull_scatter(slot, self.white_back and kv is not None and kv.startswith("rgb"), *args)
            if kv is not None:
                out[kv] = res[0]
            for s, r in zip(ks, res[1:]):
                out[s] = r
        return {key: out[key] for key in inner}            # the inner renderer's own key order

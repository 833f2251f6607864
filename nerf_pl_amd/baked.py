"""Rendering the baked RGBA volume: the lattice of a .vol file (volume.export_vol, README_Unity.md
"VolumeRender") kept on the device in 8^3-point bricks, and a ray march through it — a preview renderer without an MLP.

    vol = BakedVolume.from_model(nerf_fine, 256, (-1.2, 1.2), (-1.2, 1.2), (-1.2, 1.2))      # or .from_file("lego.vol", 512, ranges)
    out = inference.evaluate(dataset, BakedRenderer(vol, white_back=True))

Opt-in, and beside everything else: nothing of training, rendering or export changes.  The reference's consumer of the file is a
Unity shader; the semantics of the march are this project's own (include/nerfhip.h, csrc/baked_core.h).  What a baked volume
cannot show is view-dependent colour: export_vol queries the network with a zero direction.  Build and march are HIP kernels
(csrc/baked.hip); the numpy functions below restate the two layouts for hosts without a GPU and for tests.

    python -m nerf_pl_amd.baked --vol lego.vol --N 512 --x_range -1.2 1.2 --y_range -1.2 1.2 --z_range -1.2 1.2 \\
        --dataset_name blender --root_dir data/nerf_synthetic/lego --split test --img_wh 400 400 --out results/baked --gif lego.gif
"""
import numpy as np
import torch

from . import ops
from ._lib import NerfHipError
from .occupancy import OccupancyGrid, _pair

__all__ = ["BakedVolume", "BakedRenderer"]


# ---- the two layouts in numpy: for the tests and for callers of ops.baked_render_host, not part of the public surface ------------
def bricks_from_dense_host(rgba):
    """A dense (N, N, N, 4) uint8 lattice indexed [iy, ix, iz] -> the bricked volume as a flat uint8 array of
    ops.baked_bytes(N) bytes (include/nerfhip.h: brick (by NB + bx) NB + bz, local ((iy & 7) 8 + (ix & 7)) 8 + (iz & 7))."""
    rgba = np.asarray(rgba)
    if rgba.dtype != np.uint8 or rgba.ndim != 4 or rgba.shape[3] != 4 or len(set(rgba.shape[:3])) != 1:
        raise ValueError("expected (N, N, N, 4) uint8, got %s %s" % (rgba.shape, rgba.dtype))
    N = rgba.shape[0]
    NB = (N + 7) // 8
    pad = np.zeros((NB * 8, NB * 8, NB * 8, 4), np.uint8)
    pad[:N, :N, :N] = rgba
    # [by, ly, bx, lx, bz, lz, ch] -> [by, bx, bz, ly, lx, lz, ch]
    return np.ascontiguousarray(pad.reshape(NB, 8, NB, 8, NB, 8, 4).transpose(0, 2, 4, 1, 3, 5, 6)).reshape(-1)


def dense_from_bricks_host(data, N):
    """The inverse of `bricks_from_dense_host`: the flat bricked volume -> (N, N, N, 4) uint8."""
    NB = (int(N) + 7) // 8
    b = np.asarray(data, np.uint8).reshape(NB, NB, NB, 8, 8, 8, 4).transpose(0, 3, 1, 4, 2, 5, 6)
    return np.ascontiguousarray(b.reshape(NB * 8, NB * 8, NB * 8, 4)[:N, :N, :N])


def brick_bits_host(rgba):
    """The bitfield of the occupied cell bricks of a dense (N, N, N, 4) lattice as int32 words: brick (by, bx, bz) of 8^3 cells
    is occupied iff a point with every index in [8 b, 8 b + 8] (clipped) has A > 0; brick c = (by MB + bx) MB + bz is bit c & 31
    of word c >> 5."""
    a = np.asarray(rgba)[..., 3] > 0
    N = a.shape[0]
    MB = (N - 1 + 7) // 8
    occ = np.zeros((MB, MB, MB), bool)
    for by in range(MB):
        for bx in range(MB):
            for bz in range(MB):
                occ[by, bx, bz] = a[8 * by:8 * by + 9, 8 * bx:8 * bx + 9, 8 * bz:8 * bz + 9].any()
    flat = occ.reshape(-1)
    bits = np.zeros(ops.baked_brick_words(N) * 32, np.uint8)
    bits[:flat.size] = flat
    return np.packbits(bits, bitorder="little").view(np.int32)


# ---- the volume on the device -------------------------------------------------------------------------------------------------
class BakedVolume:
    """The bricked lattice on the device: `data` (uint8, ops.baked_bytes(N)), `bits` (int32 words: the occupied cell bricks),
    `N`, `ranges` = ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)) with the first and last lattice points on the ranges' ends, and
    `cell`, the thickness the stored opacities belong to: (x_hi - x_lo) / N unless given, as in volume.export_vol."""

    def __init__(self, data, N, ranges, cell=None, bits=None):
        self.N = int(N)
        self.ranges = tuple(_pair(r) for r in ranges)
        if len(self.ranges) != 3:
            raise ValueError("ranges must be three (lo, hi) pairs")
        if not torch.is_tensor(data) or not data.is_cuda:
            raise NerfHipError("nerf_pl_amd runs on MI355X only: the volume must be a device tensor (no CPU fallback)")
        self.cell = float((self.ranges[0][1] - self.ranges[0][0]) / self.N if cell is None else cell)
        if not self.cell > 0:
            raise ValueError("cell must be > 0, got %r" % (cell,))
        self.data = data
        self.bits = ops.baked_bricks(data, self.N) if bits is None else bits

    @classmethod
    def from_records(cls, records, N, ranges, cell=None):
        """records (K, 2) int32 on the device: what volume.vol_records / export_vol return (the bytes of the file).  ValueError
        for an index outside the lattice."""
        return cls(ops.baked_scatter(records, N), N, ranges, cell)

    @classmethod
    def from_file(cls, path, N, ranges, cell=None, device=None):
        """A .vol file (volume.write_vol) -> the volume on `device` (the current GPU unless given).  ValueError for a length that
        is not a whole number of records or an index outside the lattice."""
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) % 8:
            raise ValueError("from_file: %d bytes is not a whole number of 8-byte records" % len(raw))
        rec = np.frombuffer(raw, dtype="<u4").astype(np.uint32).view(np.int32).reshape(-1, 2)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return cls.from_records(torch.from_numpy(rec.copy()).to(dev), N, ranges, cell)

    @classmethod
    def from_dense(cls, rgba, ranges, cell=None):
        """rgba (N, N, N, 4) uint8 on the device, indexed [iy, ix, iz] as volume.read_vol returns it."""
        data = ops.baked_from_dense(rgba)
        return cls(data, rgba.shape[0], ranges, cell)

    @classmethod
    def from_model(cls, model, N, x_range, y_range, z_range, embeddings=None):
        """volume.export_vol followed by `from_records`: the records never leave the device."""
        from . import volume
        records = volume.export_vol(model, N, x_range, y_range, z_range, embeddings=embeddings)
        return cls.from_records(records, N, (x_range, y_range, z_range))

    def to_dense(self):
        """(N, N, N, 4) uint8 on the device, indexed [iy, ix, iz]: volume.read_vol of the file the volume came from."""
        N, NB = self.N, (self.N + 7) // 8
        b = self.data.view(NB, NB, NB, 8, 8, 8, 4).permute(0, 3, 1, 4, 2, 5, 6)
        return b.reshape(NB * 8, NB * 8, NB * 8, 4)[:N, :N, :N].contiguous()

    def occupancy_grid(self, dilate=1):
        """The `OccupancyGrid` of the lattice's (N - 1)^3 cells: a cell is occupied iff one of its corners has A > 0, dilated by
        `dilate` cells — for `CulledRenderer`."""
        alpha = self.to_dense()[..., 3].to(torch.float32).contiguous()
        return OccupancyGrid.from_sigma(alpha, *self.ranges, sigma_threshold=0.0, dilate=dilate)

    def occupied_fraction(self):
        """Occupied cell bricks / all cell bricks (one host read)."""
        w = self.bits.cpu().numpy().view(np.uint32)
        return float(np.unpackbits(w.view(np.uint8)).sum()) / float(((self.N - 1 + 7) // 8) ** 3)


class BakedRenderer:
    """A callable rays (n, 8) -> {'rgb_fine' (n, 3), 'depth_fine' (n,), 'opacity_fine' (n,)} that marches `volume` in segments
    of `step` cells: usable as `inference.evaluate(dataset, BakedRenderer(...))` and inside `occupancy.CulledRenderer`.
    `t_stop` > 0 ends a ray once its transmittance falls below it; `skip=False` marches without the brick bitfield (the same
    bits of output, more gathers)."""

    def __init__(self, volume, white_back, step=0.5, t_stop=0.0, skip=True):
        if not 1.0 / 16 <= float(step) <= 8.0:
            raise ValueError("step must be in [1/16, 8] cells, got %r" % (step,))
        if not 0.0 <= float(t_stop) < 1.0:
            raise ValueError("t_stop must be in [0, 1), got %r" % (t_stop,))
        self.volume = volume
        self.white_back = bool(white_back)
        self.step = float(step)
        self.t_stop = float(t_stop)
        self.skip = bool(skip)

    @torch.no_grad()
    def __call__(self, rays):
        v = self.volume
        rgb, depth, opacity = ops.baked_render(rays, v.data, v.bits if self.skip else None, v.N, v.ranges, v.cell, self.step,
                                               self.t_stop, self.white_back)
        return {"rgb_fine": rgb, "depth_fine": depth, "opacity_fine": opacity}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Render the poses of a dataset split from a .vol file (no network involved)")
    ap.add_argument("--vol", required=True, help="the .vol file (python -m nerf_pl_amd.volume)")
    ap.add_argument("--N", type=int, default=512)
    for ax in "xyz":
        ap.add_argument("--%s_range" % ax, nargs=2, type=float, default=[-1.2, 1.2])
    ap.add_argument("--dataset_name", default="blender", choices=["blender", "llff"])
    ap.add_argument("--root_dir", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--img_wh", nargs=2, type=int, default=[800, 800])
    ap.add_argument("--step", type=float, default=0.5, help="segment length in cells")
    ap.add_argument("--out", default=None, help="directory for the PNG frames")
    ap.add_argument("--gif", default=None, help="path of an animated GIF of the frames")
    a = ap.parse_args(argv)
    from .inference import evaluate
    if a.dataset_name == "blender":
        from .datasets.blender import BlenderDataset
        dataset = BlenderDataset(a.root_dir, split=a.split, img_wh=tuple(a.img_wh))
    else:
        from .datasets.llff import LLFFDataset
        dataset = LLFFDataset(a.root_dir, split=a.split, img_wh=tuple(a.img_wh))
    ranges = (tuple(a.x_range), tuple(a.y_range), tuple(a.z_range))
    vol = BakedVolume.from_file(a.vol, a.N, ranges)
    out = evaluate(dataset, BakedRenderer(vol, white_back=getattr(dataset, "white_back", a.dataset_name == "blender"), step=a.step),
                   dir_name=a.out, gif_path=a.gif)
    print("%d frames from %s (N = %d, %.1f %% of the bricks occupied)" % (len(out["images"]), a.vol, a.N, 100 * vol.occupied_fraction()))
    if out["mean_psnr"] is not None:
        print("mean PSNR %.2f dB, mean SSIM %.4f against the split's images" % (out["mean_psnr"], out["mean_ssim"]))


if __name__ == "__main__":
    main()

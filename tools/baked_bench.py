#!/usr/bin/env python3
"""Frame time of the baked-volume ray march on a synthetic scene, and the time of its build steps.

    python tools/baked_bench.py [--size 800] [--reps 9] [--out profiles/baked_bench.json]

The scene is a solid ball and a slab in [-1.2, 1.2]^3 (about 8 % of the lattice points carry alpha), sampled onto an N^3 RGBA8
lattice on the device, N = 128, 256, 512.  One frame is size x size rays (800 x 800 = 640 k) from a camera at radius 4.  Per N and
step (1 and 0.5 cells), ms per frame from device events for three arms that alternate within every repetition, the median of
--reps: the march with the brick bitfield, without it, and with it inside CulledRenderer (dilate 1, tighten "none").  Per N
also the build steps alone: scatter of the .vol records (the operator with its allocation and host read, and its two launches
alone), the dense permutation and the brick bitfield, 5 calls per sample.  Needs a GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANGE = (-1.2, 1.2)
LATTICES, STEPS = (128, 256, 512), (1.0, 0.5)


def scene(N, dev):
    """(N, N, N, 4) uint8 indexed [iy, ix, iz]: a ball of radius 0.55 and a slab, coloured by position."""
    ax = torch.linspace(RANGE[0], RANGE[1], N, device=dev)
    y, x, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    ball = (x * x + y * y + (z - 0.1) ** 2) < 0.55 ** 2
    slab = (x.abs() < 0.9) & (y.abs() < 0.7) & ((z + 0.6).abs() < 0.08)
    solid = ball | slab
    rgba = torch.zeros(N, N, N, 4, device=dev, dtype=torch.uint8)
    for ch, coord in enumerate((x, y, z)):
        rgba[..., ch] = ((coord / 2.4 + 0.5) * 255).to(torch.uint8).expand(N, N, N)
    rgba[..., 3] = 160
    rgba[~solid] = 0
    return rgba


def records_of(rgba):
    """the (K, 2) int32 records of the .vol file of a dense lattice, on the device"""
    flat = rgba.reshape(-1, 4).to(torch.int64)
    idx = torch.nonzero(flat[:, 3] > 0).squeeze(1)
    p = flat[idx]
    packed = (p[:, 0] << 24) | (p[:, 1] << 16) | (p[:, 2] << 8) | p[:, 3]
    both = torch.stack([idx, packed], 1)
    return torch.where(both >= 2 ** 31, both - 2 ** 32, both).to(torch.int32).contiguous()


def look_at_pose(pos):
    z = torch.nn.functional.normalize(pos, dim=0)
    x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0]), z), dim=0)
    return torch.stack([x, torch.linalg.cross(z, x), z, pos], 1)


def timed(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lattices", type=int, nargs="+", default=list(LATTICES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baked_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("baked_bench needs a GPU")
    dev = torch.device("cuda:0")
    from nerf_pl_amd import _lib, ops, rays as rays_mod
    from nerf_pl_amd.baked import BakedRenderer, BakedVolume
    from nerf_pl_amd.occupancy import CulledRenderer

    pos = torch.nn.functional.normalize(torch.tensor([0.5, -0.7, 0.45]), dim=0) * 4.0
    rays = rays_mod.gen_rays(look_at_pose(pos).to(dev), a.size, a.size, 1111.0 * a.size / 800, 2.0, 6.0)
    report = {"recipe": "ball + slab in %s^3, one %d x %d frame (%d rays) from radius 4, focal %.0f; device events, the arms alternating, "
                        "median of %d" % (list(RANGE), a.size, a.size, rays.shape[0], 1111.0 * a.size / 800, a.reps),
              "device": torch.cuda.get_device_name(0), "rows": [], "build": []}
    ranges = (RANGE,) * 3
    lib = _lib.load()
    for N in a.lattices:
        rgba = scene(N, dev)
        rec = records_of(rgba)
        vol = BakedVolume.from_dense(rgba, ranges)
        assert torch.equal(ops.baked_scatter(rec, N), vol.data)
        build = {"N": N, "records": int(rec.shape[0]), "points_with_alpha": rec.shape[0] / float(N ** 3),
                 "bricks_occupied": vol.occupied_fraction(), "volume_MiB": ops.baked_bytes(N) / 2.0 ** 20}
        # the scatter's two launches alone, into buffers that exist: no allocation, no host read of the count
        out, n_bad = torch.empty_like(vol.data), torch.empty(1, device=dev, dtype=torch.int32)

        def scatter_launches():
            _lib.check(lib.nerfhip_baked_scatter(_lib.ptr(rec), rec.shape[0], N, _lib.ptr(out), _lib.ptr(n_bad), _lib.stream_ptr()),
                       "nerfhip_baked_scatter")
        for name, fn in (("scatter_ms", lambda: ops.baked_scatter(rec, N)), ("scatter_launches_ms", scatter_launches),
                         ("from_dense_ms", lambda: ops.baked_from_dense(rgba)), ("bricks_ms", lambda: ops.baked_bricks(vol.data, N))):
            fn()
            torch.cuda.synchronize()
            build[name] = median([timed(fn, 5) for _ in range(a.reps)])
        assert torch.equal(out, vol.data) and int(n_bad.item()) == 0
        del out
        report["build"].append(build)
        print("N %3d build: %d records (%.3f of the points, %.3f of the bricks) | scatter %.3f ms with its allocation and host read, "
              "%.3f ms its two launches alone, from_dense %.3f ms, bricks %.3f ms"
              % (N, build["records"], build["points_with_alpha"], build["bricks_occupied"], build["scatter_ms"],
                 build["scatter_launches_ms"], build["from_dense_ms"], build["bricks_ms"]), flush=True)
        grid = vol.occupancy_grid(dilate=1)
        del rgba
        for step in STEPS:
            skip = BakedRenderer(vol, True, step=step)
            noskip = BakedRenderer(vol, True, step=step, skip=False)
            culled = CulledRenderer(skip, grid, True, tighten="none")
            arms = (("skip", skip), ("noskip", noskip), ("culled", culled))
            want = skip(rays)
            for name, fn in arms[1:]:                      # the arms compute the same bits
                got = fn(rays)
                assert all(torch.equal(got[k], want[k]) for k in want), name
            ms = {name: [] for name, _ in arms}
            for rep in range(a.reps):
                for name, fn in (arms if rep % 2 == 0 else arms[::-1]):
                    ms[name].append(timed(lambda: fn(rays), 5))
            row = {"N": N, "step": step, "rays": int(rays.shape[0]), "rays_culled_share": 1.0 - culled.stats["rendered"] / float(culled.stats["rays"]),
                   "opaque_share": float((want["opacity_fine"] > 0.5).float().mean())}
            for name in ms:
                row["ms_" + name] = median(ms[name])
                row["ms_%s_all" % name] = ms[name]
            report["rows"].append(row)
            print("N %3d step %.2f: skip %.3f ms  noskip %.3f ms  culled %.3f ms  (%.3f of the rays culled, %.3f opaque)"
                  % (N, step, row["ms_skip"], row["ms_noskip"], row["ms_culled"], row["rays_culled_share"], row["opaque_share"]), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(report, fh, indent=1)
        del vol, grid
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

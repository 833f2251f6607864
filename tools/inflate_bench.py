#!/usr/bin/env python3
"""Inflating a Blender scene's PNG frames: the host path (serial zlib.decompress, then the raw scanlines go up) against the device
path (the IDAT bytes go up, then nerfhip_inflate), on the GPU that is visible.

    python tools/inflate_bench.py [--out profiles/inflate_bench.json] [--rounds 11]

Frames: procedural 800 x 800 RGBA, Blender-like (transparent background, a shaded and textured object), written as PNG files
with zlib level 6 and level 1; batches of 16 (the loader's) and 32 / 64 / 100 (a whole training split).  One process; device
events for what runs on the device, the host clock for what runs on the host; median and range of the rounds.  Per batch size and
level: (a) zlib ms, H2D ms and bytes of the scanlines; (b) H2D ms and bytes of the IDAT data, kernel ms; the whole
BlenderDataset._load on the host clock with both settings."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZE = 800


def frame(seed, size=SIZE):
    """RGBA: a lit sphere with a noisy texture and a soft edge over a transparent background"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    cx, cy, rad = size * (0.4 + 0.2 * rng.random()), size * (0.4 + 0.2 * rng.random()), size * (0.25 + 0.1 * rng.random())
    r = np.hypot(x - cx, y - cy) / rad
    z = np.sqrt(np.clip(1 - r * r, 0, 1))
    light = np.clip(0.2 + 0.8 * (0.5 * z + 0.3 * (cx - x) / rad + 0.3 * (cy - y) / rad), 0, 1)
    texture = 0.85 + 0.15 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0) + 0.02 * rng.standard_normal((size, size))
    img = np.zeros((size, size, 4), np.uint8)
    for k, tint in enumerate((0.9, 0.6, 0.3)):
        img[..., k] = np.where(r < 1, np.clip(255 * tint * light * texture, 0, 255), 0)
    img[..., 3] = np.clip(255 * (1 - r) * 40, 0, 255)
    return img


def png_file(img, level):
    """imageio's choice for a uint8 array: filter 0 on every row (the Blender sets themselves are written by Blender; both are
    plain zlib streams)"""
    from nerf_pl_amd.imageio_min import _chunk
    h, w, _ = img.shape
    rows = np.zeros((h, 1 + 4 * w), np.uint8)
    rows[:, 1:] = img.reshape(h, 4 * w)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) \
        + _chunk(b"IEND", b"")


def stats(values):
    return {"median_ms": round(statistics.median(values), 4), "min_ms": round(min(values), 4), "max_ms": round(max(values), 4)}


def device_ms(fn, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def host_ms(fn, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_bench.json"))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--batches", default="16,32,64,100")
    args = ap.parse_args()
    from nerf_pl_amd import _lib, ops
    from nerf_pl_amd.datasets import BlenderDataset
    from nerf_pl_amd.imageio_min import png_idat
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    sizes = [int(v) for v in args.batches.split(",")]
    frames = [frame(s) for s in range(16)]                 # 16 distinct frames, repeated to fill the larger batches
    out_bytes = SIZE * (1 + 4 * SIZE)
    result = {"frame": "%d x %d RGBA, procedural" % (SIZE, SIZE), "raw_bytes_per_frame": out_bytes, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "zlib": zlib.ZLIB_RUNTIME_VERSION, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for level in (6, 1):
            files = [png_file(f, level) for f in frames]
            scene = os.path.join(tmp, "level%d" % level)
            os.makedirs(os.path.join(scene, "train"))
            meta = {"camera_angle_x": 0.69, "frames": []}
            for i in range(max(sizes)):
                with open(os.path.join(scene, "train", "r_%d.png" % i), "wb") as f:
                    f.write(files[i % len(files)])
                meta["frames"].append({"file_path": "./train/r_%d" % i, "transform_matrix": np.eye(4).tolist()})
            with open(os.path.join(scene, "transforms_val.json"), "w") as f:      # the val split loads nothing in its constructor
                json.dump(meta, f)
            loaders = {kind: BlenderDataset(scene, "val", (SIZE, SIZE), device=dev, png_inflate=kind) for kind in ("host", "gpu")}
            for n in sizes:
                paths = [os.path.join(scene, "train", "r_%d.png" % i) for i in range(n)]
                streams = [png_idat(p)[3] for p in paths]
                raws = [zlib.decompress(s) for s in streams]
                offsets = np.zeros(n + 1, np.int64)
                offsets[1:] = np.cumsum([len(s) for s in streams])
                joined = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy())
                raw_host = torch.from_numpy(np.stack([np.frombuffer(r, np.uint8) for r in raws]))
                d_off = torch.from_numpy(offsets).to(dev)
                d_in = joined.to(dev)
                d_out = torch.empty((n, out_bytes), device=dev, dtype=torch.uint8)
                status = torch.zeros(n, device=dev, dtype=torch.int32)

                def kernel():
                    _lib.check(lib.nerfhip_inflate(d_in.data_ptr(), d_off.data_ptr(), d_in.numel(), n, d_out.data_ptr(), out_bytes, out_bytes,
                                                   status.data_ptr(), _lib.stream_ptr()), "nerfhip_inflate")
                kernel()
                assert not bool(status.any()) and torch.equal(d_out.cpu(), raw_host)
                case = {"level": level, "frames": n, "idat_bytes": int(joined.numel()), "raw_bytes": int(raw_host.numel()),
                        "host_zlib": host_ms(lambda: [zlib.decompress(s) for s in streams], args.rounds),
                        "h2d_raw": device_ms(lambda: raw_host.to(dev), args.rounds),
                        "h2d_idat": device_ms(lambda: joined.to(dev), args.rounds),
                        "kernel": device_ms(kernel, args.rounds),
                        "inflate_batch_host_clock": host_ms(lambda: ops.inflate_batch(streams, out_bytes, dev), args.rounds),
                        "load_host": host_ms(lambda: loaders["host"]._load(paths), args.rounds),
                        "load_gpu": host_ms(lambda: loaders["gpu"]._load(paths), args.rounds)}
                case["path_a_ms"] = round(case["host_zlib"]["median_ms"] + case["h2d_raw"]["median_ms"], 4)
                case["path_b_ms"] = round(case["h2d_idat"]["median_ms"] + case["kernel"]["median_ms"], 4)
                case["b_over_a"] = round(case["path_b_ms"] / case["path_a_ms"], 4)
                case["kernel_ms_per_frame"] = round(case["kernel"]["median_ms"] / n, 4)
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
                del d_in, d_out, raw_host
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

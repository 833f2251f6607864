"""Load time of a Blender scene (nerf_pl_amd/datasets) by stage, at the reference's sizes: 100 RGBA PNGs of 800 x 800, loaded at
img_wh 400 (the reference recipe's --img_wh 400 400: every image resized) and 800 (no resize).

    python tools/dataset_load_bench.py [--images 100] [--size 800] [--repeats 5] [--out profiles/dataset_load.json]

The files are synthetic (a shaded, lightly noisy disc on a transparent background, 10 distinct images written 10 times each; by
PIL with its adaptive scanline filters where PIL is importable, else unfiltered by imageio_min) in a temporary directory.  Per
size the stages of BlenderDataset._load are run as the dataset runs them, in batches of 16 files, and timed apart: file read +
inflate with the host clock, the host-to-device copy, the unfilter launch and resize + blend with device events (each batch's
events are read after the batch; the figures are sums over the batches).  `total` is the host clock around building
BlenderDataset('train') and a device synchronise.  One warm-up pass per size, then `repeats` passes alternating between the
sizes; medians are reported, with the extremes.  Where PIL is importable the reference's way — PIL open + resize(LANCZOS) +
the torch blend on the CPU, one process — is timed on the same files in the same alternation.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nerf_pl_amd import ops  # noqa: E402
from nerf_pl_amd.datasets import BlenderDataset, blender  # noqa: E402
from nerf_pl_amd.imageio_min import png_bytes, png_inflate  # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None


def synth_image(k, size):
    rng = np.random.default_rng(k)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    cx, cy, r = size * (0.5 + 0.05 * np.cos(k)), size * (0.5 + 0.05 * np.sin(k)), size * 0.33
    d = np.hypot(x - cx, y - cy)
    alpha = np.clip((r - d) * 0.5 + 0.5, 0.0, 1.0)                           # one-pixel soft edge
    shade = np.clip(1.0 - d / r, 0.0, 1.0)
    rgb = np.stack([0.9 * shade + 0.1, 0.6 * shade * (x / size) + 0.2, 0.8 * (y / size) * shade + 0.1], -1)
    rgb = rgb * 255 + rng.normal(0.0, 2.0, rgb.shape)                        # render noise
    img = np.concatenate([np.clip(rgb, 0, 255) * (alpha[..., None] > 0), alpha[..., None] * 255], -1)
    return img.astype(np.uint8)


def write_scene(root, n_images, size):
    os.makedirs(os.path.join(root, "train"))
    distinct = [synth_image(k, size) for k in range(min(10, n_images))]
    frames = []
    for i in range(n_images):
        path = os.path.join(root, "train", "r_%d.png" % i)
        img = distinct[i % len(distinct)]
        if Image is not None:
            Image.fromarray(img, "RGBA").save(path)
        else:
            with open(path, "wb") as f:
                f.write(png_bytes(img))
        m = np.eye(4)
        m[:3, 3] = (0.0, 0.0, 4.0)
        frames.append({"file_path": "./train/r_%d" % i, "transform_matrix": m.tolist()})
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f)
    return [os.path.join(root, "train", "r_%d.png" % i) for i in range(n_images)]


def staged_pass(paths, wh, dev):
    """the stages of BlenderDataset._load over all files -> milliseconds per stage"""
    t = dict(read_inflate_ms=0.0, h2d_ms=0.0, unfilter_ms=0.0, resize_blend_ms=0.0)
    out = torch.empty(len(paths) * wh * wh, 3, device=dev)
    for i in range(0, len(paths), blender._BATCH):
        batch = paths[i:i + blender._BATCH]
        t0 = time.perf_counter()
        rows = []
        for p in batch:
            W, H, ch, raw = png_inflate(p)
            rows.append(np.frombuffer(raw, dtype=np.uint8))
        host = torch.from_numpy(np.stack(rows))
        t["read_inflate_ms"] += (time.perf_counter() - t0) * 1e3
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        streams = host.to(dev)
        ev[1].record()
        rgba, _ = ops.decode_png_batch(streams, H, W, 4, return_flags=True)
        ev[2].record()
        rgba = ops.resize_rgba_lanczos(rgba, wh, wh)
        ops.rgba_to_rgb_white(rgba, out=out[i * wh * wh:(i + len(batch)) * wh * wh])
        ev[3].record()
        torch.cuda.synchronize()
        t["h2d_ms"] += ev[0].elapsed_time(ev[1])
        t["unfilter_ms"] += ev[1].elapsed_time(ev[2])
        t["resize_blend_ms"] += ev[2].elapsed_time(ev[3])
    return t


def total_pass(root, wh, dev):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = BlenderDataset(root, "train", (wh, wh), device=dev)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert ds.all_rgbs.shape[0] == len(ds.image_paths) * wh * wh
    return ms


def pil_pass(paths, wh):
    """blender.py:54-58 per file: PIL open + resize + ToTensor's arithmetic + the blend, on the CPU"""
    t0 = time.perf_counter()
    rgbs = []
    for p in paths:
        img = Image.open(p).resize((wh, wh), Image.LANCZOS)
        img = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        img = img.view(4, -1).permute(1, 0)
        rgbs.append(img[:, :3] * img[:, -1:] + (1 - img[:, -1:]))
    torch.cat(rgbs, 0)
    return (time.perf_counter() - t0) * 1e3


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dataset_load_bench needs an MI355X: nothing here is a timing without one")
    dev = torch.device("cuda:0")
    sizes = (a.size // 2, a.size)
    with tempfile.TemporaryDirectory() as root:
        paths = write_scene(root, a.images, a.size)
        file_bytes = sum(os.path.getsize(p) for p in paths)
        filters = np.zeros(5, np.int64)
        for p in paths[:10]:
            W, H, ch, raw = png_inflate(p)
            filters += np.bincount(np.frombuffer(raw, np.uint8).reshape(H, -1)[:, 0], minlength=5)[:5]
        samples = {wh: {"staged": [], "total": [], "pil": []} for wh in sizes}
        for wh in sizes:                                                     # warm-up: code objects, allocator, file cache
            staged_pass(paths, wh, dev)
            total_pass(root, wh, dev)
        for _ in range(a.repeats):
            for wh in sizes:
                samples[wh]["staged"].append(staged_pass(paths, wh, dev))
                samples[wh]["total"].append(total_pass(root, wh, dev))
                if Image is not None:
                    samples[wh]["pil"].append(pil_pass(paths, wh))
    rec = {"images": a.images, "size": a.size, "repeats": a.repeats, "batch": blender._BATCH, "png_bytes": file_bytes,
           "inflated_bytes": a.images * a.size * (1 + 4 * a.size), "writer": "PIL" if Image is not None else "imageio_min (filter 0)",
           "filter_rows_first_10_files": filters.tolist(), "device": torch.cuda.get_device_name(0), "img_wh": {}}
    for wh in sizes:
        s = samples[wh]
        r = {k: summary([p[k] for p in s["staged"]]) for k in s["staged"][0]}
        r["total_ms"] = summary(s["total"])
        r["pil_reference_ms"] = summary(s["pil"]) if s["pil"] else None
        rec["img_wh"][str(wh)] = r
        print("img_wh %d: " % wh + ", ".join("%s %.1f" % (k, v["median"]) for k, v in r.items() if v), flush=True)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

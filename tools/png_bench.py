"""Timing and sizes of the GPU PNG encoder (csrc/png.hip behind imageio_min.png_bytes_device) against the host writer
(imageio_min.png_bytes, filter 0 + zlib level 6) for the file `eval.py:138` writes per image: render-like RGB frames (a shaded,
textured object with sensor-like noise on a white background) of 800 x 800 (Blender) and 1008 x 756 (LLFF), n = 1 and n = 8.

* nerfhip_png_filter and nerfhip_png_deflate: device events around one call each, after a warm-up call; the order of the two
  alternates from round to round (deflate runs on the streams of the same batch);
* `png_bytes_device(batch)` and, frame by frame, `png_bytes(frame, 6)` of the same frames already on the host: wall clock, the
  two alternating from round to round; the device figure includes both copies to the host and the container's CRC-32;
* the file sizes of both.

    python tools/png_bench.py [--rounds 7] [--out profiles/png_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pl_amd import imageio_min, ops  # noqa: E402

SIZES = ((800, 800), (756, 1008))          # (H, W)
BATCHES = (1, 8)


def frames(n, H, W, dev):
    """(n, H, W, 3) uint8 on the device: a lit, textured sphere that turns and drifts over white."""
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for k in range(n):
        a = 6.2831853 * k / 8
        u, v = (x + 0.5) / W - 0.5 - 0.08 * torch.cos(torch.tensor(a)), ((y + 0.5) / H - 0.5) * H / W - 0.05 * torch.sin(torch.tensor(a))
        r2 = (u * u + v * v) / 0.12
        z = torch.sqrt(torch.clamp(1.0 - r2, 0.0, 1.0))
        col = torch.stack([0.5 + 0.4 * torch.sin(9 * u + 5 * v + a) * z, 0.45 + 0.35 * torch.cos(7 * v - 3 * u + 2 * a),
                           0.3 + 0.6 * z * (0.5 + 0.5 * torch.sin(40 * u * v + a))], dim=-1)
        col = col * (0.35 + 0.65 * z[..., None]) + 0.004 * torch.randn(H, W, 3, device=dev, generator=g)
        edge = torch.clamp((1.0 - r2) * 40.0, 0.0, 1.0)[..., None]
        img = torch.where((r2 < 1.0)[..., None], col * edge + (1.0 - edge), torch.ones_like(col))
        out.append((img.clamp(0, 1) * 255).to(torch.uint8))
    return torch.stack(out)


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"unit": "ms", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "strip": ops.PNG_STRIP, "cases": []}
    for H, W in SIZES:
        for n in BATCHES:
            batch = frames(n, H, W, dev)
            host = batch.cpu().numpy()
            ws = ops.png_workspace(n, H * (1 + 3 * W), dev)
            streams = ops.png_filter(batch)
            ops.png_deflate(streams, ws)                                 # warm-up of both
            ours = imageio_min.png_bytes_device(batch)                   # ... and of the whole path
            theirs = [imageio_min.png_bytes(f, 6) for f in host]
            for f, data in zip(host, ours):                              # what is timed is a correct file
                w_, h_, ch, raw = imageio_min.png_inflate(data)
                back = ops.decode_png_batch(torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(1, -1).to(dev), h_, w_, ch)
                assert torch.equal(back[0].cpu(), torch.from_numpy(f))
            torch.cuda.synchronize()
            t_f, t_d, t_dev, t_host = [], [], [], []
            for r in range(a.rounds):
                steps = [(t_f, lambda: ops.png_filter(batch)), (t_d, lambda: ops.png_deflate(streams, ws))]
                for acc, fn in (steps if r % 2 == 0 else steps[::-1]):
                    acc.append(device_ms(fn))
                walls = [(t_dev, lambda: imageio_min.png_bytes_device(batch)),
                         (t_host, lambda: [imageio_min.png_bytes(f, 6) for f in host])]
                for acc, fn in (walls if r % 2 == 0 else walls[::-1]):
                    acc.append(wall_ms(fn)[0])
            out["cases"].append({
                "size": [W, H], "n": n, "workspace_bytes": int(ws.numel() * 8),
                "filter_device": spread(t_f), "deflate_device": spread(t_d),
                "png_bytes_device_wall": spread(t_dev), "png_bytes_level6_host_wall": spread(t_host),
                "png_bytes_device_wall_per_frame": round(statistics.median(t_dev) / n, 3),
                "png_bytes_level6_host_wall_per_frame": round(statistics.median(t_host) / n, 3),
                "file_bytes_device": [len(d) for d in ours], "file_bytes_host": [len(d) for d in theirs]})
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

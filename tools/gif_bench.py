"""Timing of the GPU GIF encoder (csrc/gif.hip behind imageio_min.gif_bytes) for the movie `eval.py:145` writes: 120 frames of
800 x 800, a shaded moving object on a white background.

* nerfhip_gif_quantize and nerfhip_gif_lzw per batch of `imageio_min.GIF_BATCH` frames: device events around one call each,
  after a warm-up call; the order of the two alternates from round to round (lzw runs on the indices of the same batch);
* the whole file, `imageio_min.gif_bytes(frames)`: wall clock including every copy to the host;
* where Pillow is present: `Image.quantize(256, method=0, dither=NONE)` of every frame plus Pillow's `save_all` GIF writer on
  the host, wall clock, once (`--pillow-frames` of the frames; the figure is per frame);
* the file sizes of both.

    python tools/gif_bench.py [--frames 120] [--rounds 7] [--pillow-frames 24] [--out profiles/gif_bench.json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pl_amd import imageio_min, ops  # noqa: E402

H = W = 800


def movie(n, dev):
    """(n, H, W, 3) uint8 on the device: a lit, textured sphere that turns and drifts over white."""
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for k in range(n):
        a = 6.2831853 * k / n
        u, v = (x + 0.5) / W - 0.5 - 0.08 * torch.cos(torch.tensor(a)), (y + 0.5) / H - 0.5 - 0.05 * torch.sin(torch.tensor(a))
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


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pillow-frames", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = movie(a.frames, dev)
    batch = frames[:imageio_min.GIF_BATCH].contiguous()
    n = batch.shape[0]
    ws = ops.gif_workspace(n, H, W, dev)
    indices = ops.gif_quantize(batch, ws)[0]
    ops.gif_lzw(indices, H, W, ws)                                   # warm-up of both
    torch.cuda.synchronize()
    t_q, t_z, t_file = [], [], []
    for r in range(a.rounds):
        steps = [(t_q, lambda: ops.gif_quantize(batch, ws)), (t_z, lambda: ops.gif_lzw(indices, H, W, ws))]
        for acc, fn in (steps if r % 2 == 0 else steps[::-1]):
            acc.append(device_ms(fn))
    data = imageio_min.gif_bytes(frames)                             # warm-up of the whole path
    for r in range(max(1, a.rounds // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = imageio_min.gif_bytes(frames)
        t_file.append((time.perf_counter() - t0) * 1e3)
    out = {"unit": "ms", "device": torch.cuda.get_device_name(0), "frames": a.frames, "size": [W, H], "batch": n, "rounds": a.rounds,
           "workspace_bytes_per_batch": int(ws.numel() * 8),
           "quantize_per_batch": spread(t_q), "lzw_per_batch": spread(t_z), "gif_bytes_whole_movie_wall": spread(t_file),
           "file_bytes": len(data)}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None and a.pillow_frames > 0:
        host = frames[:a.pillow_frames].cpu().numpy()
        t0 = time.perf_counter()
        pf = [Image.fromarray(f).quantize(256, method=0, dither=Image.Dither.NONE) for f in host]
        t1 = time.perf_counter()
        buf = io.BytesIO()
        pf[0].save(buf, "GIF", save_all=True, append_images=pf[1:], duration=30, loop=0)
        t2 = time.perf_counter()
        ours = imageio_min.gif_bytes(frames[:a.pillow_frames])
        out["pillow"] = {"frames": len(host), "quantize_ms_per_frame": round((t1 - t0) * 1e3 / len(host), 2),
                         "save_ms_per_frame": round((t2 - t1) * 1e3 / len(host), 2), "file_bytes": len(buf.getvalue()),
                         "file_bytes_ours_same_frames": len(ours),
                         "note": "Pillow's writer stores only the changed rectangle of each later frame; ours stores whole frames"}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Timing of the image-metric kernels against the same arithmetic through torch ops on the same GPU, and of the per-image tail
of `inference.evaluate` against that of `inference.save_image_outputs`.

* nerfhip_ssim (mean only, renderer layout (H*W,3)) at window 3 and 11 vs kornia 0.2.0's formula through depth-wise `F.conv2d`
  (what a user without the kernel would write), fp32, mean-reduced;
* nerfhip_depth_colormap vs nan_to_num / min / max / normalise / table lookup through torch ops (device-resident: a kinder
  comparison than the reference's host round trip through numpy, cv2 and PIL);
* the evaluate tail (uint8 on the device, 3 B per pixel copied) vs the save_image_outputs tail (12 B per pixel copied, `* 255`
  and `astype` in numpy), both without the PNG encoder: wall clock around a synchronising copy.

Image sizes 800 x 800 (Blender) and 1008 x 756 (LLFF).  One process; device events around REPS back-to-back eager calls; the order
of the configurations alternates from round to round.

    python tools/image_metrics_bench.py [--rounds 9] [--out profiles/image_metrics.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pl_amd import inference, metrics, ops  # noqa: E402
from nerf_pl_amd.visualization import _table  # noqa: E402

REPS = 20
SIZES = ((800, 800), (756, 1008))          # (H, W)


def torch_ssim(pred, gt, win, pad):
    """kornia 0.2.0's ssim loss behind metrics.py:15-20, mean-reduced; pred / gt (1,3,H,W), win (3,1,ws,ws)"""
    def filt(x):
        return F.conv2d(x, win, padding=pad, groups=3)
    mu1, mu2 = filt(pred), filt(gt)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = filt(pred * pred) - mu1_sq, filt(gt * gt) - mu2_sq, filt(pred * gt) - mu12
    m = ((2 * mu12 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1_sq + mu2_sq + 1e-4) * (s11 + s22 + 9e-4))
    return 1 - 2 * torch.mean(torch.clamp(1 - m, 0, 1) / 2)


def torch_depth(depth, table_f):
    x = torch.nan_to_num(depth)
    mi, ma = x.min(), x.max()
    x = (x - mi) / (ma - mi + 1e-8)
    return table_f[(255 * x).to(torch.uint8).long()].permute(2, 0, 1)


def device_us(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def wall_us(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    return (time.perf_counter() - t0) / REPS * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    configs = []
    for H, W in SIZES:
        tag = "%dx%d" % (W, H)
        gt = torch.rand(H * W, 3, device=dev)
        pred = (gt + 0.02 * torch.randn_like(gt)).clamp(0, 1)
        planar = [t.view(H, W, 3).permute(2, 0, 1)[None].contiguous() for t in (pred, gt)]
        depth = 2.0 + 4.0 * torch.rand(H, W, device=dev)
        table = _table("jet", dev)
        table_f = table.float() / 255
        for ws in (3, 11):
            g = torch.tensor([np.exp(-((i - ws // 2) ** 2) / (2.0 * 1.5 ** 2)) for i in range(ws)], dtype=torch.float32, device=dev)
            g = g / g.sum()
            win = (g[:, None] * g[None, :])[None, None].repeat(3, 1, 1, 1)
            configs.append(("ssim_ws%d_%s_hip" % (ws, tag), device_us,
                            lambda pred=pred, gt=gt, H=H, W=W, ws=ws: metrics.ssim_hw3(pred, gt, H, W, window_size=ws)))
            configs.append(("ssim_ws%d_%s_torch" % (ws, tag), device_us,
                            lambda p=planar, win=win, ws=ws: torch_ssim(p[0], p[1], win, ws // 2)))
        configs.append(("depth_%s_hip" % tag, device_us, lambda depth=depth, table=table: ops.depth_colormap(depth, table)))
        configs.append(("depth_%s_torch" % tag, device_us, lambda depth=depth, table_f=table_f: torch_depth(depth, table_f)))
        configs.append(("tail_%s_u8_on_device" % tag, wall_us,
                        lambda pred=pred, H=H, W=W: inference.image_to_u8(pred).reshape(H, W, 3).cpu().numpy()))
        configs.append(("tail_%s_fp32_copy_numpy" % tag, wall_us,
                        lambda pred=pred, H=H, W=W: (pred.reshape(H, W, 3).cpu().numpy() * 255).astype(np.uint8)))
    samples = {name: [] for name, _, _ in configs}
    for r in range(a.rounds):
        for name, timer, fn in (configs if r % 2 == 0 else configs[::-1]):
            samples[name].append(timer(fn))
    out = {"unit": "us per call (ssim_*, depth_*: device events; tail_*: wall clock incl. the synchronising copy)",
           "calls_per_sample": REPS, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, xs in samples.items():
        out["configs"][name] = {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

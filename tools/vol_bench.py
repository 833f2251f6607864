"""Timing of the Unity volume export (nerf_pl_amd/volume.py, csrc/volume.hip) on one GPU.

* nerfhip_vol_pack alone at n = 512^3 on a seeded rgb-sigma with a trained-like share of kept points (about 20 %), against the same
  pack through torch ops on the same device (clamp, exp, mask, nonzero, gather, shifts: what a user without the kernel would write
  once the notebook's arrays live on the device).  Two inputs: `iid` (kept points scattered: every 256-point block holds some,
  so the emit pass reads every point a second time) and `ball` (the same share inside one ball of the lattice, as a trained scene
  has it: the emit pass skips the empty blocks).
* the pack's achieved bytes/s against the bytes it must move (volume export: 16 B per point read once + 8 B per kept
  point written) and against what this implementation moves (the second read of the blocks that keep something added).
* export_vol at N = 512 in bf16 and fp32 beside grid.sigma_grid at the same N (the sigma-only lattice query of the mesh export).

One process; device events around REPS back-to-back calls; the order of the configurations alternates from round to round.

    python tools/vol_bench.py [--rounds 5] [--N 512] [--out profiles/vol_export.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pl_amd import _lib, grid, volume  # noqa: E402
from nerf_pl_amd.models import NeRF  # noqa: E402

REPS = 5
RANGE = (-1.2, 1.2)


def make_input(N, kind, dev, seed):
    """(N^3, 4) float32: sigmoid-like colours; about 20 % of the densities positive (a fifth of those tiny: kept with A == 0)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    n = N ** 3
    x = torch.empty(n, 4, device=dev)
    x[:, :3] = torch.sigmoid(2 * torch.randn(n, 3, device=dev, generator=g))
    pos = torch.exp(3.0 + 1.5 * torch.randn(n, device=dev, generator=g))
    pos = torch.where(torch.rand(n, device=dev, generator=g) < 0.2, pos * 1e-4, pos)
    neg = -torch.rand(n, device=dev, generator=g) * 10 - 1e-3
    if kind == "iid":
        inside = torch.rand(n, device=dev, generator=g) < 0.2
    else:
        c = torch.linspace(-0.5, 0.5, N, device=dev)
        r2 = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2).reshape(-1)
        inside = r2 < (0.2 * 3 / (4 * np.pi)) ** (2.0 / 3.0)
    x[:, 3] = torch.where(inside, pos, neg)
    return x


def torch_pack(x, c):
    sigma = x[:, 3].clamp(min=0)
    a = 1 - torch.exp(c * sigma)
    idx = torch.nonzero(a > 0).squeeze(1)
    rgb = (x[idx, :3] * 255).to(torch.int64)
    s = (rgb[:, 0] << 24) | (rgb[:, 1] << 16) | (rgb[:, 2] << 8) | (a[idx] * 255).to(torch.int64)
    return torch.stack([idx, s], -1).to(torch.int32)


def device_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, n = a.N, a.N ** 3
    cell = (RANGE[1] - RANGE[0]) / N
    c = float(np.float32(-cell))
    lib = _lib.load()
    ws = torch.empty(lib.nerfhip_vol_workspace_bytes(n), device=dev, dtype=torch.uint8)
    records = torch.empty(n, 2, device=dev, dtype=torch.int32)
    cursor = torch.zeros(1, device=dev, dtype=torch.int64)

    def hip_pack(x):
        cursor.zero_()
        _lib.check(lib.nerfhip_vol_pack(_lib.ptr(x), n, 0, c, _lib.ptr(ws), _lib.ptr(records), n, _lib.ptr(cursor), _lib.stream_ptr()),
                   "nerfhip_vol_pack")

    configs, traffic = [], {}
    for kind in ("iid", "ball"):
        x = make_input(N, kind, dev, 1)
        hip_pack(x)
        K = int(cursor.item())
        ref = torch_pack(x, c)
        same = ref.shape[0] == K and bool((ref == records[:K]).all())       # fp32 exp of torch vs the rounded fp64 exp: informative
        blocks = (x[:, 3] > 0).view(-1, 256).any(1).sum().item() if n % 256 == 0 else None
        traffic[kind] = {"kept": K, "kept_share": round(K / n, 4), "equals_torch_pack": same,
                         "must_move_bytes": 16 * n + 8 * K,
                         "moves_bytes": None if blocks is None else 16 * n + 16 * 256 * blocks + 8 * K + 12 * (n // 256)}
        del ref
        configs.append(("pack_%s_hip" % kind, lambda x=x: hip_pack(x), REPS))
        configs.append(("pack_%s_torch" % kind, lambda x=x: torch_pack(x, c), REPS))
    torch.manual_seed(0)
    model = NeRF().to(dev).eval()
    for dtype in ("bf16", "fp32"):
        def export(dtype=dtype):
            model.mlp_dtype = dtype
            return volume.export_vol(model, N, RANGE, RANGE, RANGE)

        def sigma(dtype=dtype):
            model.mlp_dtype = dtype
            return grid.sigma_grid(model, N, RANGE, RANGE, RANGE)
        configs.append(("export_vol_%s" % dtype, export, 1))
        configs.append(("sigma_grid_%s" % dtype, sigma, 1))
    model.mlp_dtype = "bf16"
    kept_model = volume.export_vol(model, N, RANGE, RANGE, RANGE).shape[0]
    samples = {name: [] for name, _, _ in configs}
    for r in range(a.rounds):
        for name, fn, reps in (configs if r % 2 == 0 else configs[::-1]):
            samples[name].append(device_ms(fn, reps))
        print("round %d of %d done" % (r + 1, a.rounds), file=sys.stderr, flush=True)
    out = {"unit": "ms per call (device events)", "N": N, "points": n, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "pack_inputs": traffic, "export_model": {"weights": "NeRF() default init, torch.manual_seed(0)", "kept": kept_model},
           "configs": {}}
    for name, xs in samples.items():
        out["configs"][name] = {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    for kind, t in traffic.items():
        ms = out["configs"]["pack_%s_hip" % kind]["median"]
        t["must_move_TBps"] = round(t["must_move_bytes"] / ms / 1e9, 3)
        if t["moves_bytes"] is not None:
            t["moves_TBps"] = round(t["moves_bytes"] / ms / 1e9, 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

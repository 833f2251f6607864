"""Timing of the optimizer kernels alone over both models' flat buffers (2 x 595,844 floats), each replayed from a hipGraph
(20 launches per replay, device events): adam_kernel twice (its two timings against each other are the run's own spread), the
RAdam kernel at a rectified step, the Ranger kernel at a non-sync step (k beyond every step of the run) and at a sync step (k = 1).
One process; the order of the configurations alternates from round to round.

    python tools/optim_kernel_bench.py [--rounds 11] [--out profiles/radam_kernels.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pl_amd import _lib  # noqa: E402
from nerf_pl_amd._lib import check, ptr, stream_ptr  # noqa: E402
from nerf_pl_amd.models import NeRF  # noqa: E402

LAUNCHES, REPS, START_STEP = 20, 20, 100.0          # t = 101 .. : rectified (N_sma(101) = 95), far from the t = 1 slow-buffer fill


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    numel = sum(p.numel() for p in NeRF().parameters())
    torch.manual_seed(0)
    bufs = {k: [torch.randn(numel, device=dev) * s for _ in range(2)]
            for k, s in (("p", 0.1), ("g", 1e-3), ("m", 1e-3), ("slow", 0.1))}
    bufs["v"] = [torch.rand(numel, device=dev) * 1e-6 for _ in range(2)]
    state = torch.zeros(2, device=dev)
    arr = ctypes.c_void_p * 2
    pa = {k: arr(*[t.data_ptr() for t in v]) for k, v in bufs.items()}
    nn = (ctypes.c_int64 * 2)(numel, numel)
    lr, eps, wd = 5e-4, 1e-8, 0.0

    def adam():
        check(lib.nerfhip_adam_step(pa["p"], pa["g"], pa["m"], pa["v"], nn, 2, ptr(state), lr, 0.9, 0.999, eps, wd, stream_ptr()), "adam")

    def radam():
        check(lib.nerfhip_radam_step(pa["p"], pa["g"], pa["m"], pa["v"], nn, 2, ptr(state), lr, 0.9, 0.999, eps, wd, 1, stream_ptr()), "radam")

    def ranger(k):
        def fn():
            check(lib.nerfhip_ranger_step(pa["p"], pa["g"], pa["m"], pa["v"], nn, 2, ptr(state), pa["slow"], 0.5, k, 5.0, lr, 0.95, 0.999,
                                          eps, wd, stream_ptr()), "ranger")
        return fn

    configs = [("adam_a", adam), ("radam_rectified", radam), ("ranger_nosync", ranger(1 << 30)), ("adam_b", adam),
               ("ranger_sync", ranger(1))]
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in configs:
        state.zero_()
        state[0] = START_STEP
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            for _ in range(LAUNCHES):
                fn()
        graphs[name] = g

    def measure(name):
        state.zero_()
        state[0] = START_STEP
        g = graphs[name]
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (REPS * LAUNCHES) * 1e3

    samples = {name: [] for name, _ in configs}
    for r in range(a.rounds):
        order = configs if r % 2 == 0 else configs[::-1]
        for name, _ in order:
            samples[name].append(measure(name))
    out = {"unit": "us per launch", "numel": [numel, numel], "launches_per_replay": LAUNCHES, "replays_per_sample": REPS,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "kernels": {}}
    for name, xs in samples.items():
        out["kernels"][name] = {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    med = {k: v["median"] for k, v in out["kernels"].items()}
    out["adam_vs_adam_spread"] = round(abs(med["adam_a"] - med["adam_b"]), 3)
    adam_mid = 0.5 * (med["adam_a"] + med["adam_b"])
    out["minus_adam"] = {k: round(med[k] - adam_mid, 3) for k in ("radam_rectified", "ranger_nosync", "ranger_sync")}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

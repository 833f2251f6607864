"""Epoch sampling against sampling with replacement, on one 100 x 800 x 800 store, in one process:

* the batch launch alone — `EpochSampler.sample()` (nerfhip_epoch_batch) against `RayStore.sample(B)` (nerfhip_torch_draws with a
  ray batch), B = 1024 and B = 32768, each replayed from a hipGraph of 20 launches and timed with device events, alternating;
* the graphed training step (bench.py's default: 1024 rays x (64 + 128) samples, bf16) with each as its batch source — the step's
  draws and weight packing ride in RayStore.sample's launch and take one launch more beside EpochSampler's;
* the node counts of both step graphs (expected: epoch = replacement + 1).

    python tools/epoch_sampler_bench.py [--rounds 11] [--out profiles/epoch_sampler.json]
"""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_inputs import synth_params, synth_store  # noqa: E402
from nerf_pl_amd import draws as D  # noqa: E402
from nerf_pl_amd.system import GraphedTrainStep, NeRFSystem, _HipGraphBackend, graph_node_count  # noqa: E402

LAUNCHES, REPS, STEPS = 20, 20, 50


def launch_graph(fn, dev, draw_state):
    """a hipGraph of LAUNCHES calls of fn"""
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    draw_state.arm()
    with D.capturing(draw_state), torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        keep = [fn() for _ in range(LAUNCHES)]
    return g, keep


def time_replays(g):
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (REPS * LAUNCHES) * 1e3


def make_stepper(dev, source_of):
    hp = Namespace(N_samples=64, N_importance=128, use_disp=False, perturb=1.0, noise_std=0.0, chunk=1024 * 32, loss_type="mse", lr=5e-4,
                   weight_decay=0, decay_step=[10 ** 9], decay_gamma=0.5, white_back=True, optimizer="adam", lr_scheduler="steplr")
    system = NeRFSystem(hp)
    system.nerf_coarse.load_state_dict(synth_params(100, 4.0, 0.2))
    system.nerf_fine.load_state_dict(synth_params(101, 4.0, 0.2))
    for m in system.models:
        m.mlp_dtype = "bf16"
    system = system.to(dev)
    (opt,), _ = system.configure_optimizers()
    draws = (hp.N_samples, hp.N_importance, hp.perturb, hp.noise_std)
    stepper = GraphedTrainStep(system, opt, warmup=3, batch_source=source_of(draws, (system.models, "bf16")),
                               backend=_HipGraphBackend(keep_graph=True))
    for _ in range(6):
        stepper()
    torch.cuda.synchronize()
    return stepper


def time_steps(stepper):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stepper()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(STEPS):
        stepper()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS * 1e3


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    store = synth_store(4321, dev, n_img=100, hw=800)
    draw_state = D.GraphDrawState(dev)
    out = {"unit": "us", "store": [100, 800, 800], "launches_per_replay": LAUNCHES, "replays_per_sample": REPS, "steps_per_sample": STEPS,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "launch": {}, "step": {}}

    # ---- the batch launch alone ----
    for B in (1024, 32768):
        sampler = store.epoch_sampler(B, seed=1, last="drop")        # (a captured launch has one batch shape)
        graphs = {"replacement": launch_graph(lambda: store.sample(B), dev, draw_state),
                  "epoch": launch_graph(sampler.sample, dev, draw_state)}
        names = list(graphs)
        samples = {k: [] for k in names}
        for r in range(a.rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                samples[k].append(time_replays(graphs[k][0]))
        res = {k: summary(v) for k, v in samples.items()}
        res["epoch_over_replacement"] = round(res["epoch"]["median"] / res["replacement"]["median"], 3)
        out["launch"]["B%d" % B] = res
        del graphs

    # ---- the training step with each batch source ----
    B = 1024
    sampler = store.epoch_sampler(B, seed=1)                          # 6.4e7 / 1024 = 62500 batches: no partial batch
    steppers = {"replacement": make_stepper(dev, lambda draws, pack: (lambda: store.sample(B, step_draws=draws, pack_models=pack))),
                "epoch": make_stepper(dev, lambda draws, pack: sampler.source(step_draws=draws, pack_models=pack))}
    names = list(steppers)
    samples = {k: [] for k in names}
    for r in range(a.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            samples[k].append(time_steps(steppers[k]))
    res = {k: summary(v) for k, v in samples.items()}
    res["epoch_over_replacement"] = round(res["epoch"]["median"] / res["replacement"]["median"], 4)
    res["graph_nodes"] = {k: graph_node_count(s.graph) for k, s in steppers.items()}
    res["sampler_mirror"] = {"epoch": sampler.epoch, "cursor": sampler.cursor,
                             "device": [int(v) for v in sampler.state.cpu()[1:3]]}
    out["step"] = res

    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""What empty-space skipping at eval buys and costs, measured on the procedural brick scene of
tests/test_gpu_psnr_gate.py:

    python tests/tools/cull_eval.py [--steps 1200] [--views 2] [--size 800] [--out profiles/cull_eval.json]

Trains the brick scene for a fixed number of steps, renders held-out views with the plain GraphRenderer and with CulledRenderer
around the same GraphRenderer, and sweeps sigma_threshold over {0, 1, 5, 20} and dilate over {0, 1, 2} at N = 128 and 256.  Per
setting and each `tighten` mode of CulledRenderer: occupied fraction, share of rays rendered, PSNR against the closed-form ground
truth for both renderers, PSNR between the two (null when they are bit-equal), ms per image for each (device events, the two
renderers alternating), the grid build time, and the time of cull + compact + scatter alone.  The time baseline is the plain
renderer in the same run.  Before the sweep, three grids without scene content: all zeros (a call that renders nothing), all ones
over the sweep's box (near / far edited by the box clip alone) and all ones over a box that contains every ray segment (every ray
rendered, nothing edited: the overhead on a frame the object fills)."""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import scenes  # noqa: E402
from tests import test_gpu_psnr_gate as G  # noqa: E402

RANGE = (-1.2, 1.2)                    # the brick (1.4 x 1.0 x 0.7 box + ball) with a margin
THRESHOLDS, DILATES, LATTICES = (0.0, 1.0, 5.0, 20.0), (0, 1, 2), (128, 256)
MODES = ("both", "near", "none")     # CulledRenderer's `tighten`


def train(dev, data, steps, dtype, seed):
    """G.train_curve's loop, keeping the trained system."""
    from nerf_pl_amd.models import NeRF
    from nerf_pl_amd.system import NeRFSystem
    rays, rgbs, _, _ = data
    hp = Namespace(N_samples=G.S, N_importance=G.N, use_disp=False, perturb=1.0, noise_std=0.0, chunk=32768, loss_type="mse", lr=5e-4,
                   weight_decay=0, decay_step=[10 ** 9], decay_gamma=0.5, white_back=True, optimizer="adam", lr_scheduler="steplr")
    torch.manual_seed(seed)
    init = [NeRF().state_dict(), NeRF().state_dict()]
    system = NeRFSystem(hp)
    system.nerf_coarse.load_state_dict(init[0])
    system.nerf_fine.load_state_dict(init[1])
    for m in system.models:
        m.mlp_dtype = dtype
    system = system.to(dev)
    (opt,), _ = system.configure_optimizers()
    torch.manual_seed(1000 + seed)
    perm = torch.randperm(rays.shape[0], generator=torch.Generator().manual_seed(1000 + seed)).to(dev)
    scale = steps / float(G.STEPS)
    lr_at = {max(1, int(round(k * scale))): v for k, v in G.LR_AT.items()}
    for step in range(1, steps + 1):
        if step in lr_at:
            for grp in opt.param_groups:
                grp["lr"] = lr_at[step]
        idx = perm[((step - 1) * G.B) % (rays.shape[0] - G.B):][:G.B]
        out = system.training_step({"rays": rays[idx], "rgbs": rgbs[idx]}, step)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()
        opt.step()
    return system


def look_at_pose(pos):
    """c2w (3, 4) of a camera at `pos` looking at the origin (the Blender convention: the camera looks along its -z)."""
    z = torch.nn.functional.normalize(pos, dim=0)
    up = torch.tensor([0.0, 0.0, 1.0])
    x = torch.nn.functional.normalize(torch.linalg.cross(up, z), dim=0)
    y = torch.linalg.cross(z, x)
    return torch.stack([x, y, z, pos], 1)


def psnr(a, b):
    return float(-10 * torch.log10(torch.mean((a - b) ** 2)))


def timed(fn, reps):
    """ms per call from device events around `reps` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(og, renderer, views, plain, reps, dev):
    """One grid against the plain renderer on every view: the per-view record of the JSON."""
    from nerf_pl_amd import ops
    from nerf_pl_amd.occupancy import CulledRenderer
    out_views = []
    for (r, gt), p in zip(views, plain):
        view = {"psnr_plain": psnr(p, gt)}
        ms_plain = []
        for mode in MODES:
            culled = CulledRenderer(renderer, og, white_back=True, tighten=mode)
            out = culled(r)["rgb_fine"]
            view["rays_rendered_share"] = culled.stats["rendered"] / float(culled.stats["rays"])
            view["chunks_rendered"] = -(-culled.stats["rendered"] // renderer.chunk)  # a ragged tail is padded to a whole chunk
            view["psnr_culled_" + mode] = psnr(out, gt)
            view["psnr_culled_%s_vs_plain" % mode] = None if torch.equal(out, p) else psnr(out, p)
            # the two renderers alternating, in both orders
            ms_culled = []
            for rep in range(reps):
                order = (("plain", renderer), ("culled", culled)) if rep % 2 == 0 else (("culled", culled), ("plain", renderer))
                for name, fn in order:
                    (ms_plain if name == "plain" else ms_culled).append(timed(lambda: fn(r), 1))
            view["ms_culled_" + mode] = sorted(ms_culled)[len(ms_culled) // 2]
            view["ms_culled_%s_all" % mode] = ms_culled
        view["ms_plain"] = sorted(ms_plain)[len(ms_plain) // 2]
        view["ms_plain_all"] = ms_plain
        # cull + compact + scatter alone: the launches of one call without the inner render and without the host read
        hit, t0, t1 = og.cull(r)
        slot, _, compact, n_hit = ops.cull_compact(hit, r, t0, t1)
        k = int(n_hit.item())
        fake = (torch.zeros(k, 3, device=dev), torch.zeros(k, device=dev), torch.zeros(k, device=dev), torch.zeros(k, device=dev))

        def overhead():
            h, a0, a1 = og.cull(r)
            s, _, _, _ = ops.cull_compact(h, r, a0, a1)
            ops.cull_scatter(s, True, *fake)
        overhead()
        view["ms_cull_kernel"] = timed(lambda: og.cull(r), 5)
        view["ms_cull_compact_scatter"] = timed(overhead, 5)
        out_views.append(view)
    return out_views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=G.STEPS)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull_eval.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from nerf_pl_amd import grid as grid_mod, ops, rays as rays_mod
    from nerf_pl_amd.inference import GraphRenderer
    from nerf_pl_amd.occupancy import CulledRenderer, OccupancyGrid

    t = time.time()
    data = G.make_data(dev)
    system = None
    for seed in range(4):                                  # a seed that never leaves the all-white solution is replaced
        system = train(dev, data, a.steps, a.dtype, seed)
        with torch.no_grad():
            from nerf_pl_amd.inference import batched_inference
            img = batched_inference(system.models, system.embeddings, data[2], G.S, G.N, False, 32768, True)["rgb_fine"]
        held_out = psnr(img, data[3])
        print("trained %d steps (seed %d): %.2f dB on the held-out rays, %.1f s" % (a.steps, seed, held_out, time.time() - t), flush=True)
        if held_out >= G.DEAD_BELOW_DB:
            break
    report = {"recipe": "brick scene, %d steps of %d rays, %d+%d samples, %s; %d held-out views of %d x %d from radius 4, focal %.0f; "
                        "grid over %s^3 from the fine model; eval at 64+128 samples, 32768-ray GraphRenderer chunks"
                        % (a.steps, G.B, G.S, G.N, a.dtype, a.views, a.size, a.size, 1111.0 * a.size / 800, list(RANGE)),
              "train_psnr_held_out_rays": held_out, "settings": []}

    # held-out views and their closed-form ground truth
    g = torch.Generator().manual_seed(99)
    views = []
    for _ in range(a.views):
        pos = torch.nn.functional.normalize(torch.randn(3, generator=g) + torch.tensor([0.0, 0.0, 0.6]), dim=0) * 4.0
        r = rays_mod.gen_rays(look_at_pose(pos).to(dev), a.size, a.size, 1111.0 * a.size / 800, 2.0, 6.0)
        gt = scenes._render_closed_form(lambda p: scenes.brick_field(p, **scenes.BRICK_DEFAULT), r, 768).float()
        views.append((r, gt))
    print("views ready, %.1f s" % (time.time() - t), flush=True)

    renderer = GraphRenderer(system.models, system.embeddings, N_samples=64, N_importance=128, white_back=True)
    plain = [renderer(r)["rgb_fine"] for r, _ in views]
    report["plain_psnr"] = [psnr(p, gt) for p, (_, gt) in zip(plain, views)]
    report["background_share_of_pixels"] = [float((gt == 1.0).all(1).float().mean()) for _, gt in views]

    # reference grids that hold no scene content: what a call costs when nothing is rendered (all zeros), what editing near / far
    # does on its own (all ones over the sweep's box: only the box clip moves them), and the overhead on a frame where every ray
    # hits and nothing is edited (all ones over a box that contains every [near, far] segment)
    report["reference_grids"] = []
    for name, fill, rng in (("zeros", 0, RANGE), ("ones_same_box", -1, RANGE), ("ones_containing_box", -1, (-8.0, 8.0))):
        og = OccupancyGrid(torch.full((ops.occupancy_words(8),), fill, device=dev, dtype=torch.int32), 8, (rng,) * 3)
        row = {"grid": name, "M": 8, "range": list(rng), "views": measure(og, renderer, views, plain, max(a.reps, 7), dev)}
        report["reference_grids"].append(row)
        v = row["views"]
        mean = lambda key: sum(x[key] for x in v) / len(v)  # noqa: E731
        print("%-20s rendered %.3f (%.1f chunks) | PSNR plain %.2f culled both %.2f near %.2f none %.2f | ms plain %.2f culled both %.2f "
              "near %.2f none %.2f | cull %.3f all three %.3f"
              % (name, mean("rays_rendered_share"), mean("chunks_rendered"), mean("psnr_plain"), mean("psnr_culled_both"),
                 mean("psnr_culled_near"), mean("psnr_culled_none"), mean("ms_plain"), mean("ms_culled_both"), mean("ms_culled_near"),
                 mean("ms_culled_none"), mean("ms_cull_kernel"), mean("ms_cull_compact_scatter")), flush=True)

    for N in LATTICES:
        sigma = grid_mod.sigma_grid(system.nerf_fine, N, RANGE, RANGE, RANGE)           # warm-up
        torch.cuda.synchronize()
        t_sigma = timed(lambda: grid_mod.sigma_grid(system.nerf_fine, N, RANGE, RANGE, RANGE), 1)
        sigma = grid_mod.sigma_grid(system.nerf_fine, N, RANGE, RANGE, RANGE)
        for thr in THRESHOLDS:
            for dil in DILATES:
                OccupancyGrid.from_sigma(sigma, RANGE, RANGE, RANGE, thr, dil)          # warm-up
                t_bits = timed(lambda: OccupancyGrid.from_sigma(sigma, RANGE, RANGE, RANGE, thr, dil), 3)
                og = OccupancyGrid.from_sigma(sigma, RANGE, RANGE, RANGE, thr, dil)
                row = {"N": N, "sigma_threshold": thr, "dilate": dil, "occupied_fraction": og.occupied_fraction(),
                       "sigma_grid_ms": t_sigma, "bitfield_ms": t_bits, "views": []}
                row["views"] = measure(og, renderer, views, plain, a.reps, dev)
                report["settings"].append(row)
                v = row["views"]
                mean = lambda key: sum(x[key] for x in v) / len(v)  # noqa: E731
                print("N %3d thr %4.1f dil %d: occupied %.4f rendered %.3f | PSNR plain %.2f culled both %.2f near %.2f none %.2f | "
                      "ms plain %.1f culled both %.1f near %.1f none %.1f | cull %.3f all three %.3f | bitfield %.2f ms (sigma grid %.1f ms)"
                      % (N, thr, dil, row["occupied_fraction"], mean("rays_rendered_share"), mean("psnr_plain"), mean("psnr_culled_both"),
                         mean("psnr_culled_near"), mean("psnr_culled_none"), mean("ms_plain"), mean("ms_culled_both"),
                         mean("ms_culled_near"), mean("ms_culled_none"), mean("ms_cull_kernel"), mean("ms_cull_compact_scatter"),
                         t_bits, t_sigma), flush=True)
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as fh:                # after every setting: a run cut short keeps what it measured
                    json.dump(report, fh, indent=1)
    report["wall_s"] = round(time.time() - t, 1)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

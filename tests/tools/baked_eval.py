"""What the baked RGBA volume shows and costs as a renderer, measured on the procedural brick scene of
tests/test_gpu_psnr_gate.py, trained as tests/tools/cull_eval.py trains it:

    python tests/tools/baked_eval.py [--steps 1200] [--views 2] [--size 800] [--out profiles/baked_eval.json]

Bakes the trained fine model at N = 128, 256 and 512 (volume.export_vol -> BakedVolume, the records never leave the device) and
renders held-out views with BakedRenderer at step 1 and 0.5.  Per setting and view: PSNR of the baked render against the
closed-form ground truth and against the NeRF render of the same view, and ms per frame (device events) next to the plain
GraphRenderer's in the same run, the two alternating.  Also per N: the time of the bake (export + scatter + bricks, the median
of --reps), the occupied share of the bricks and of the lattice points, and one diagnostic: the PSNR of the same lattice with
its alpha rounded to nearest where the file truncates."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cull_eval as C  # noqa: E402
from oracle import scenes  # noqa: E402
from tests import test_gpu_psnr_gate as G  # noqa: E402

RANGE = C.RANGE
LATTICES, STEPS = (128, 256, 512), (1.0, 0.5)


def nearest_alpha_volume(model, N):
    """A diagnostic, not a file format: the same lattice with A = round-to-nearest(255 a) where the file truncates (colours as
    the file has them), to tell the quantisation of a cell-thick alpha apart from everything else the bake loses."""
    from nerf_pl_amd import volume
    from nerf_pl_amd.baked import BakedVolume
    rs = volume.rgbsigma_grid(model, N, RANGE, RANGE, RANGE)
    a = 1.0 - torch.exp(-((RANGE[1] - RANGE[0]) / N) * rs[:, 3].clamp(min=0))
    alpha = torch.floor(a * 255 + 0.5).clamp(0, 255)
    rgba = torch.cat([torch.floor(rs[:, :3].clamp(0, 1) * 255), alpha[:, None]], 1).to(torch.uint8)
    rgba[alpha == 0] = 0
    return BakedVolume.from_dense(rgba.view(N, N, N, 4), (RANGE,) * 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=G.STEPS)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lattices", type=int, nargs="+", default=list(LATTICES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baked_eval.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from nerf_pl_amd import rays as rays_mod
    from nerf_pl_amd.baked import BakedRenderer, BakedVolume
    from nerf_pl_amd.inference import GraphRenderer, batched_inference

    t = time.time()
    data = G.make_data(dev)
    for seed in range(4):                                  # a seed that never leaves the all-white solution is replaced
        system = C.train(dev, data, a.steps, a.dtype, seed)
        with torch.no_grad():
            img = batched_inference(system.models, system.embeddings, data[2], G.S, G.N, False, 32768, True)["rgb_fine"]
        held_out = C.psnr(img, data[3])
        print("trained %d steps (seed %d): %.2f dB on the held-out rays, %.1f s" % (a.steps, seed, held_out, time.time() - t), flush=True)
        if held_out >= G.DEAD_BELOW_DB:
            break
    report = {"recipe": "brick scene, %d steps of %d rays, %d+%d samples, %s; %d held-out views of %d x %d from radius 4, focal %.0f; "
                        "fine model baked over %s^3 with a zero view direction; NeRF eval at 64+128 samples, 32768-ray GraphRenderer chunks"
                        % (a.steps, G.B, G.S, G.N, a.dtype, a.views, a.size, a.size, 1111.0 * a.size / 800, list(RANGE)),
              "train_psnr_held_out_rays": held_out, "settings": []}

    g = torch.Generator().manual_seed(99)
    views = []
    for _ in range(a.views):
        pos = torch.nn.functional.normalize(torch.randn(3, generator=g) + torch.tensor([0.0, 0.0, 0.6]), dim=0) * 4.0
        r = rays_mod.gen_rays(C.look_at_pose(pos).to(dev), a.size, a.size, 1111.0 * a.size / 800, 2.0, 6.0)
        gt = scenes._render_closed_form(lambda p: scenes.brick_field(p, **scenes.BRICK_DEFAULT), r, 768).float()
        views.append((r, gt))
    renderer = GraphRenderer(system.models, system.embeddings, N_samples=64, N_importance=128, white_back=True)
    nerf = [renderer(r)["rgb_fine"] for r, _ in views]
    report["nerf_psnr"] = [C.psnr(p, gt) for p, (_, gt) in zip(nerf, views)]
    print("views ready, NeRF %.2f dB, %.1f s" % (sum(report["nerf_psnr"]) / len(views), time.time() - t), flush=True)

    for N in a.lattices:
        bake = lambda: BakedVolume.from_model(system.nerf_fine, N, RANGE, RANGE, RANGE)  # noqa: E731
        vol = bake()                                       # warm-up
        torch.cuda.synchronize()
        bake_all = [C.timed(bake, 1) for _ in range(a.reps)]
        bake_ms = sorted(bake_all)[len(bake_all) // 2]
        dense_a = vol.to_dense()[..., 3]
        points_share = float((dense_a > 0).float().mean())
        del dense_a
        nearest = nearest_alpha_volume(system.nerf_fine, N)
        nearest_psnr = [C.psnr(BakedRenderer(nearest, white_back=True, step=0.5)(r)["rgb_fine"], gt) for r, gt in views]
        del nearest
        for step in STEPS:
            baked = BakedRenderer(vol, white_back=True, step=step)
            row = {"N": N, "step": step, "bake_ms": bake_ms, "bake_ms_all": bake_all, "bricks_occupied": vol.occupied_fraction(),
                   "points_with_alpha": points_share,
                   "psnr_nearest_alpha_vs_truth_step_0.5": nearest_psnr, "views": []}
            for (r, gt), p in zip(views, nerf):
                out = baked(r)["rgb_fine"]
                ms_nerf, ms_baked = [], []
                for rep in range(a.reps):                  # the two renderers alternating, in both orders
                    order = (("nerf", renderer), ("baked", baked)) if rep % 2 == 0 else (("baked", baked), ("nerf", renderer))
                    for name, fn in order:
                        (ms_nerf if name == "nerf" else ms_baked).append(C.timed(lambda: fn(r), 1))
                row["views"].append({"psnr_baked_vs_truth": C.psnr(out, gt), "psnr_baked_vs_nerf": C.psnr(out, p),
                                     "psnr_nerf_vs_truth": C.psnr(p, gt), "ms_baked": sorted(ms_baked)[len(ms_baked) // 2],
                                     "ms_baked_all": ms_baked, "ms_nerf": sorted(ms_nerf)[len(ms_nerf) // 2], "ms_nerf_all": ms_nerf})
            report["settings"].append(row)
            v = row["views"]
            mean = lambda key: sum(x[key] for x in v) / len(v)  # noqa: E731
            print("N %3d step %.2f: bricks occupied %.4f points %.4f | PSNR baked vs truth %.2f vs NeRF %.2f (NeRF vs truth %.2f) | "
                  "ms baked %.3f NeRF %.1f | bake %.1f ms | alpha to nearest: %.2f dB"
                  % (N, step, row["bricks_occupied"], points_share, mean("psnr_baked_vs_truth"), mean("psnr_baked_vs_nerf"),
                     mean("psnr_nerf_vs_truth"), mean("ms_baked"), mean("ms_nerf"), bake_ms, sum(nearest_psnr) / len(nearest_psnr)),
                  flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as fh:                   # after every setting: a run cut short keeps what it measured
                json.dump(report, fh, indent=1)
        del vol
    report["wall_s"] = round(time.time() - t, 1)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

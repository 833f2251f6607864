#!/usr/bin/env python3
"""Build time and frame time of the mesh ray caster on the trained brick scene's own mesh, beside the other
renderers of the same scene in the same run.

    python tools/meshcast_bench.py [--size 800] [--reps 9] [--out profiles/mesh_cast.json]

The scene is tests/tools/mesh_eval.py's: the procedural brick scene, trained, its mesh extracted at N_grid = 128, 256, 512.  One
frame is size x size rays (800 x 800 = 640 k) from a camera at radius 4.  Per N_grid: the hierarchy's build from device tensors
(keys, torch.sort, boxes; no upload), 5 builds per sample; then ms per frame from device events for arms that alternate within
every repetition, the median of --reps: MeshRenderer, the cast alone, the baked march of the same scene at N = N_grid (step 0.5),
the plain GraphRenderer (64 + 128 samples), and MixedRenderer over the GraphRenderer in both modes with the same mesh moved half a
unit along x.  No timing is asserted.  Needs a GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def timed(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--sigma_threshold", type=float, default=10.0)
    ap.add_argument("--lattices", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cast.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshcast_bench needs a GPU")
    dev = torch.device("cuda:0")
    import mesh_eval as E
    from nerf_pl_amd import ops
    from nerf_pl_amd.baked import BakedRenderer, BakedVolume
    from nerf_pl_amd.inference import GraphRenderer
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer, MixedRenderer

    system, held_out = E.trained_system(dev, a.steps, "bf16", lambda s: print(s, flush=True))
    rays = E.views_of(dev, 1, a.size, 99)[0][0]
    train_views = E.views_of(dev, 12, 200, 7)
    nerf_white = GraphRenderer(system.models, system.embeddings, N_samples=64, N_importance=128, white_back=True)
    nerf_plain = GraphRenderer(system.models, system.embeddings, N_samples=64, N_importance=128, white_back=False)
    report = {"recipe": "brick scene trained %d steps (%.2f dB held out), mesh at sigma %.1f; one %d x %d frame (%d rays) from radius 4; device "
                        "events, 5 calls per sample (GraphRenderer arms: 1), the arms alternating, median of %d"
                        % (a.steps, held_out, a.sigma_threshold, a.size, a.size, rays.shape[0], a.reps),
              "device": torch.cuda.get_device_name(0), "rows": []}
    for N in a.lattices:
        v, tri, c = E.brick_mesh(system, N, a.sigma_threshold, train_views, 200)
        if len(tri) == 0:
            print("N_grid %d: the mesh is empty" % N, flush=True)
            continue
        bvh = MeshBVH(v, tri, c, device=dev)
        moved = MeshBVH(bvh.vertices + torch.tensor([0.5, 0.0, 0.0], device=dev), bvh.triangles, bvh.colors)
        build = lambda: ops.mesh_bvh_build(bvh.vertices, bvh.triangles)  # noqa: E731
        build()
        torch.cuda.synchronize()
        build_all = [timed(build, 5) for _ in range(a.reps)]
        vol = BakedVolume.from_model(system.nerf_fine, N, E.RANGE, E.RANGE, E.RANGE)
        mesh_renderer = MeshRenderer(bvh, white_back=True)
        arms = (("mesh", mesh_renderer, 5), ("cast", bvh.cast, 5), ("baked", BakedRenderer(vol, white_back=True, step=0.5), 5),
                ("nerf", nerf_white, 1), ("mixed_ztest", MixedRenderer(nerf_white, moved, True, mode="ztest"), 1),
                ("mixed_clip", MixedRenderer(nerf_plain, moved, True, mode="clip"), 1))
        for _, fn, _ in arms:                              # warm-up: every shape the timed window uses
            fn(rays)
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in arms}
        for rep in range(a.reps):
            for name, fn, calls in (arms if rep % 2 == 0 else arms[::-1]):
                ms[name].append(timed(lambda: fn(rays), calls))
        mask = arms[4][1](rays)["mesh_mask"]
        row = {"N_grid": N, "vertices": int(len(v)), "triangles": int(len(tri)), "boxes": int(bvh.boxes.shape[0]),
               "rays": int(rays.shape[0]), "hit_share": float(mesh_renderer(rays)["opacity_fine"].mean()),
               "mixed_ztest_mesh_share": float(mask.float().mean()), "build_ms": median(build_all), "build_ms_all": build_all}
        for name in ms:
            row["ms_" + name] = median(ms[name])
            row["ms_%s_all" % name] = ms[name]
        report["rows"].append(row)
        print("N_grid %3d: %d triangles, %d boxes | build %.3f ms | mesh %.3f ms (cast alone %.3f)  baked %.3f ms  NeRF %.1f ms  "
              "mixed ztest %.1f ms  clip %.1f ms | %.3f of the rays hit"
              % (N, row["triangles"], row["boxes"], row["build_ms"], row["ms_mesh"], row["ms_cast"], row["ms_baked"], row["ms_nerf"],
                 row["ms_mixed_ztest"], row["ms_mixed_clip"], row["hit_share"]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
        del bvh, moved, vol
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

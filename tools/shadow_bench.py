#!/usr/bin/env python3
"""Frame times of the shadow units on the trained brick scene's own mesh and baked volume.

    python tools/shadow_bench.py [--size 800] [--reps 9] [--lattice 256] [--out profiles/shadow.json]

The scene is tools/meshcast_bench.py's: the procedural brick scene, trained, its mesh extracted at N_grid = --lattice and its
volume baked at the same N; the inserted object is that mesh moved half a unit along x.  One frame is size x size rays from a
camera at radius 4.  The shadow rows come from the surface of a MixedRenderer frame over the baked volume, towards a directional
light (0.5, 0.3, 1).  ms per call from device events for arms that alternate within every repetition, median and range of --reps:

    occluded / cast   nerfhip_mesh_occluded against nerfhip_mesh_cast on the same rows, at K = 1 (radius 0) and at K = 16
                      (radius 0.05) with the sample sequence shifted per pixel and shared — the first incoherent rays this
                      hierarchy sees
    rows, compose     nerfhip_shadow_rays and nerfhip_light_compose alone, at K = 1 and 16
    frames            MixedRenderer, and LitMixedRenderer without and with the baked volume as scene_occluder, over a
                      BakedRenderer and over a GraphRenderer (64 + 128 samples), at K = 1; the baked pair at K = 16 as well

No timing is asserted.  Needs a GPU."""
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


def alternate(arms, reps):
    """{name: [ms per call] of `reps` repetitions}; arms = [(name, fn, calls per sample)], run in order and in reverse by turns"""
    for _, fn, _ in arms:                                  # warm-up: every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in arms}
    for rep in range(reps):
        for name, fn, calls in (arms if rep % 2 == 0 else arms[::-1]):
            ms[name].append(timed(fn, calls))
    return ms


def summary(ms):
    out = {}
    for name, v in ms.items():
        out["ms_" + name] = sorted(v)[len(v) // 2]
        out["ms_%s_range" % name] = [min(v), max(v)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--sigma_threshold", type=float, default=10.0)
    ap.add_argument("--lattice", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shadow_bench needs a GPU")
    dev = torch.device("cuda:0")
    import mesh_eval as E
    from nerf_pl_amd import ops
    from nerf_pl_amd.baked import BakedRenderer, BakedVolume
    from nerf_pl_amd.inference import GraphRenderer
    from nerf_pl_amd.lighting import Light, LitMixedRenderer
    from nerf_pl_amd.meshcast import MeshBVH, MixedRenderer

    system, held_out = E.trained_system(dev, a.steps, "bf16", lambda s: print(s, flush=True))
    rays = E.views_of(dev, 1, a.size, 99)[0][0]
    n = rays.shape[0]
    train_views = E.views_of(dev, 12, 200, 7)
    v, tri, c = E.brick_mesh(system, a.lattice, a.sigma_threshold, train_views, 200)
    if len(tri) == 0:
        raise SystemExit("the mesh is empty")
    bvh = MeshBVH(v, tri, c, device=dev)
    moved = MeshBVH(bvh.vertices + torch.tensor([0.5, 0.0, 0.0], device=dev), bvh.triangles, bvh.colors)
    vol = BakedVolume.from_model(system.nerf_fine, a.lattice, E.RANGE, E.RANGE, E.RANGE)
    baked, occluder = BakedRenderer(vol, white_back=True), BakedRenderer(vol, white_back=False)
    nerf = GraphRenderer(system.models, system.embeddings, N_samples=64, N_importance=128, white_back=True)
    direction = (0.5, 0.3, 1.0)
    report = {"recipe": "brick scene trained %d steps (%.2f dB held out), mesh at sigma %.1f and baked volume at N = %d, the inserted mesh "
                        "moved 0.5 along x; one %d x %d frame (%d rays) from radius 4; directional light %s; device events, 5 calls per "
                        "sample (GraphRenderer arms: 1), the arms alternating, median and [min, max] of %d"
                        % (a.steps, held_out, a.sigma_threshold, a.lattice, a.size, a.size, n, direction, a.reps),
              "device": torch.cuda.get_device_name(0), "triangles": int(len(tri)), "boxes": int(moved.boxes.shape[0]), "rays": int(n)}

    # the surface the rows start from: a mixed frame over the baked volume
    lit = LitMixedRenderer(baked, moved, Light(direction=direction), True)
    frame = MixedRenderer(baked, moved, True)(rays)
    mask = frame["mesh_mask"]
    s = torch.where(frame["opacity_fine"] >= 0.5, frame["depth_fine"] / frame["opacity_fine"], torch.full_like(frame["depth_fine"], float("inf")))
    hit_tri = torch.where(mask != 0, moved.cast(rays)[0], torch.full((n,), -1, device=dev, dtype=torch.int32))
    report.update(bias=lit.bias, reach=lit.reach, mesh_share=float(mask.float().mean()), surface_share=float(torch.isfinite(s).float().mean()))
    report["rows"] = []
    for K, radius, rotate in ((1, 0.0, 1), (16, 0.05, 1), (16, 0.05, 0)):
        def make_rows():
            return ops.shadow_rays(rays, s, "directional", direction, lit.bias, lit.reach, K, radius, bool(rotate), hit_tri, moved.vertices,
                                   moved.triangles)
        rows, cosine = make_rows()
        hit = ops.mesh_occluded(rows, moved.tris, moved.boxes)
        assert torch.equal(hit != 0, ops.mesh_cast(rows, moved.tris, moved.boxes)[0] >= 0)
        ms = alternate([("occluded", lambda: ops.mesh_occluded(rows, moved.tris, moved.boxes), 5),
                        ("cast", lambda: ops.mesh_cast(rows, moved.tris, moved.boxes), 5),
                        ("rows", make_rows, 5),
                        ("compose", lambda: ops.light_compose(frame["rgb_fine"], mask, cosine, hit, None, 0.3, 0.7), 5)], a.reps)
        row = {"K": K, "radius": radius, "rotate": rotate, "rows": int(rows.shape[0]), "occluded_share": float((hit != 0).float().mean()),
               "live_rows_share": float((rows[:, 3:6] != 0).any(1).float().mean())}
        row.update(summary(ms))
        report["rows"].append(row)
        print("K %2d rotate %d: %d rows, %.3f occluded | occluded %.3f ms  cast %.3f ms (ratio %.2f) | rows %.3f ms  compose %.3f ms"
              % (K, rotate, row["rows"], row["occluded_share"], row["ms_occluded"], row["ms_cast"], row["ms_occluded"] / row["ms_cast"],
                 row["ms_rows"], row["ms_compose"]), flush=True)
        del rows, cosine, hit

    report["frames"] = []
    for inner_name, inner, calls, Ks in (("baked", baked, 5, (1, 16)), ("nerf", nerf, 1, (1,))):
        for K in Ks:
            light = Light(direction=direction, radius=0.0 if K == 1 else 0.05, samples=K)
            arms = [("mixed", MixedRenderer(inner, moved, True), calls),
                    ("lit", LitMixedRenderer(inner, moved, light, True), calls),
                    ("lit_occluder", LitMixedRenderer(inner, moved, light, True, scene_occluder=occluder), calls)]
            ms = alternate([(name, (lambda r=r: r(rays)), k) for name, r, k in arms], a.reps)
            row = {"inner": inner_name, "K": K}
            row.update(summary(ms))
            report["frames"].append(row)
            print("%s K %2d: mixed %.3f ms  lit %.3f ms  lit + scene occluder %.3f ms"
                  % (inner_name, K, row["ms_mixed"], row["ms_lit"], row["ms_lit_occluder"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

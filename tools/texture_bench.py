#!/usr/bin/env python3
"""Where the time of a texture bake goes, and what the textured lookup costs beside the vertex-colour shade.

    python tools/texture_bench.py [--res 4] [--reps 5] [--out profiles/texture_bench.txt]

The scene is tests/tools/mesh_eval.py's: the procedural brick scene, trained, its mesh extracted at N_grid 256 and sigma 5, as it is
and decimated to cells of 2 voxels.  Per mesh, in one process, device events around each entry, one warm-up run of every arm, then
--reps samples in alternating order (10 calls per sample, the render 1), median [min, max]:

  the bake split into its three parts — ops.mesh_tex_points (with normals), the colour callable colours_along_normals (the NeRF
  render: 64 + 64 samples per sample point) on one chunk of at most 2^20 sample points, ops.mesh_tex_atlas;
  ops.mesh_shade_tex (bilinear and nearest) against ops.mesh_shade on the same hits of one 800 x 800 frame.

Beside each figure the bytes the pass must move (every array once, gathers at the bytes they use) and the rate that makes.  No
timing is asserted.  Needs a GPU."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def spread(v):
    s = sorted(v)
    return "%.3f [%.3f, %.3f]" % (s[len(s) // 2], s[0], s[-1])


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--N_grid", type=int, default=256)
    ap.add_argument("--sigma_threshold", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_bench needs a GPU")
    dev = torch.device("cuda:0")
    import mesh_eval as E
    from nerf_pl_amd import mesh, ops, texture
    from nerf_pl_amd.meshcast import MeshBVH

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    system, held_out = E.trained_system(dev, a.steps, "bf16", lambda s: print(s, flush=True))
    rays = E.views_of(dev, 1, a.size, 99)[0][0]
    R, n_tex = a.res, ops.mesh_tex_samples(a.res)
    voxel = (E.RANGE[1] - E.RANGE[0]) / a.N_grid
    colour = texture.colours_along_normals(E.NEAR, E.FAR, system.models[0], system.nerf_fine, system.embeddings, white_back=True)
    say("# %s; brick scene trained %d steps (%.2f dB held out), N_grid %d, sigma %.1f; res %d (%d samples per triangle); one %d x %d "
        "frame; device events, one warm-up, %d samples of 10 calls (render: 1) in alternating order, median [min, max] ms per call"
        % (torch.cuda.get_device_name(0), a.steps, held_out, a.N_grid, a.sigma_threshold, R, n_tex, a.size, a.size, a.reps))
    for cells in (0.0, 2.0):
        v, tri, _ = mesh.extract_color_mesh(system.nerf_fine, system.embeddings, a.N_grid, E.RANGE, E.RANGE, E.RANGE, a.sigma_threshold,
                                            decimate_cell=cells * voxel if cells else None, decimate_placement="quadric")
        dv, dt = torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev)
        V, T = len(v), len(tri)
        K, Wa = T * n_tex, texture.default_width(T, R)
        Ha = ops.mesh_tex_height(T, R, Wa)
        colours = torch.randint(0, 256, (K, 3), device=dev, dtype=torch.uint8)
        vertex_colours = torch.randint(0, 256, (V, 3), device=dev, dtype=torch.uint8)
        chunk_tris = min(T, (1 << 20) // n_tex)
        points, normals = ops.mesh_tex_points(dv, dt[:chunk_tris], R)
        atlas = ops.mesh_tex_atlas(colours, T, R, Wa)
        bvh = MeshBVH(dv, dt)
        hit_tri, _, b1, b2 = bvh.cast(rays)
        n, hits = rays.shape[0], int((hit_tri >= 0).sum())
        arms = [("points", lambda: ops.mesh_tex_points(dv, dt, R), 36 * K + 12 * T + 36 * T),
                ("render", lambda: colour(points, normals), None),
                ("atlas", lambda: ops.mesh_tex_atlas(colours, T, R, Wa), 3 * K + 3 * Wa * Ha),
                ("shade", lambda: ops.mesh_shade(rays, hit_tri, b1, b2, dv, dt, vertex_colours), 56 * n + (12 + 36 + 9) * hits),
                ("shade_tex bilinear", lambda: ops.mesh_shade_tex(rays, hit_tri, b1, b2, dv, dt, atlas, R, "bilinear"),
                 56 * n + (12 + 36 + 12) * hits),
                ("shade_tex nearest", lambda: ops.mesh_shade_tex(rays, hit_tri, b1, b2, dv, dt, atlas, R, "nearest"),
                 56 * n + (12 + 36 + 3) * hits)]
        for _, fn, _ in arms:                              # warm-up: every shape the timed window uses
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in arms}
        for rep in range(a.reps):
            for name, fn, _ in (arms if rep % 2 == 0 else arms[::-1]):
                ms[name].append(timed(fn, 1 if name == "render" else 10))
        say("")
        say("mesh %s: V = %d, T = %d, K = %d samples, atlas %d x %d (%.1f MB); %d of %d rays hit"
            % ("as extracted" if not cells else "decimated to %g voxels (quadric)" % cells, V, T, K, Wa, Ha, 3e-6 * Wa * Ha, hits, n))
        for name, _, moved in arms:
            if moved is None:
                per = median(ms[name]) * 1e6 / points.shape[0]
                say("  %-20s %s ms for %d sample points of one chunk (%.1f ns each; the whole bake: %.0f ms at that rate)"
                    % (name, spread(ms[name]), points.shape[0], per, per * K * 1e-6))
            else:
                say("  %-20s %s ms, must move %.1f MB: %.2f TB/s" % (name, spread(ms[name]), moved * 1e-6, moved / median(ms[name]) * 1e-9))
        say("  shade_tex / shade: bilinear %.2fx, nearest %.2fx"
            % (median(ms["shade_tex bilinear"]) / median(ms["shade"]), median(ms["shade_tex nearest"]) / median(ms["shade"])))
        del bvh, atlas, colours, points, normals
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

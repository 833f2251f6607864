"""What the extracted coloured mesh shows as a renderer, measured on the procedural brick scene of
tests/test_gpu_psnr_gate.py, trained as tests/tools/cull_eval.py trains it:

    python tests/tools/mesh_eval.py [--steps 1200] [--views 2] [--size 800] [--out profiles/mesh_eval.json]

Extracts the trained fine model's mesh at N_grid = 128, 256 and 512 and sigma = 2, 5, 10, 20 (mesh.extract_color_mesh, colours fused from --train_views
closed-form images of the scene), builds its hierarchy (MeshBVH) and renders held-out views with MeshRenderer(ambient = 1).  Per
N_grid and view: PSNR of the mesh render against the closed-form ground truth and against the NeRF render of the same view, and
two diagnostics that tell geometry from colour (the mesh's silhouette filled with the NeRF's pixels; the silhouette's agreement
with the truth's).  Per N_grid also the mesh's size, the time of the extraction and of the hierarchy's build, and ms per frame
(device events).  Measured and written down; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cull_eval as C  # noqa: E402
from oracle import scenes  # noqa: E402
from tests import test_gpu_psnr_gate as G  # noqa: E402

RANGE = C.RANGE
LATTICES = (128, 256, 512)
NEAR, FAR = 2.0, 6.0


def trained_system(dev, steps, dtype, log=print):
    """(system, PSNR on the held-out rays) of the brick scene; a seed that never leaves the all-white solution is replaced"""
    from nerf_pl_amd.inference import batched_inference
    t = time.time()
    data = G.make_data(dev)
    for seed in range(4):
        system = C.train(dev, data, steps, dtype, seed)
        with torch.no_grad():
            img = batched_inference(system.models, system.embeddings, data[2], G.S, G.N, False, 32768, True)["rgb_fine"]
        held_out = C.psnr(img, data[3])
        log("trained %d steps (seed %d): %.2f dB on the held-out rays, %.1f s" % (steps, seed, held_out, time.time() - t))
        if held_out >= G.DEAD_BELOW_DB:
            break
    return system, held_out


def truth(rays):
    return scenes._render_closed_form(lambda p: scenes.brick_field(p, **scenes.BRICK_DEFAULT), rays, 768).float()


def views_of(dev, n, size, seed):
    """[(rays, closed-form image, c2w)] of n seeded cameras at radius 4 looking at the origin"""
    from nerf_pl_amd import rays as rays_mod
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        pos = torch.nn.functional.normalize(torch.randn(3, generator=g) + torch.tensor([0.0, 0.0, 0.6]), dim=0) * 4.0
        c2w = C.look_at_pose(pos)
        r = rays_mod.gen_rays(c2w.to(dev), size, size, 1111.0 * size / 800, NEAR, FAR)
        out.append((r, truth(r), c2w))
    return out


def brick_mesh(system, N_grid, sigma_threshold, train_views, train_size):
    """mesh.extract_color_mesh of the trained fine model over RANGE^3, coloured from `train_views` closed-form images:
    numpy (vertices, triangles, colors)"""
    from nerf_pl_amd import mesh
    poses = torch.stack([c2w for _, _, c2w in train_views]).numpy().astype(np.float32)
    images = torch.stack([(gt.clamp(0, 1) * 255).to(torch.uint8).view(train_size, train_size, 3) for _, gt, _ in train_views])
    return mesh.extract_color_mesh(system.nerf_fine, system.embeddings, N_grid, RANGE, RANGE, RANGE, sigma_threshold, poses=poses,
                                   images=images, focal=1111.0 * train_size / 800, near=NEAR, white_back=True)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=G.STEPS)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--train_views", type=int, default=12)
    ap.add_argument("--train_size", type=int, default=200)
    ap.add_argument("--sigma_thresholds", type=float, nargs="+", default=[2.0, 5.0, 10.0, 20.0])
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lattices", type=int, nargs="+", default=list(LATTICES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_eval.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_eval needs a GPU")
    dev = torch.device("cuda:0")
    from nerf_pl_amd.inference import GraphRenderer
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer

    t = time.time()
    system, held_out = trained_system(dev, a.steps, a.dtype, lambda s: print(s, flush=True))
    report = {"recipe": "brick scene, %d steps of %d rays, %d+%d samples, %s; mesh of the fine model over %s^3 at sigma %s, colours fused "
                        "from %d closed-form images of %d x %d; %d held-out views of %d x %d from radius 4, focal %.0f; MeshRenderer ambient 1; "
                        "NeRF eval at 64+128 samples" % (a.steps, G.B, G.S, G.N, a.dtype, list(RANGE), a.sigma_thresholds, a.train_views,
                                                         a.train_size, a.train_size, a.views, a.size, a.size, 1111.0 * a.size / 800),
              "train_psnr_held_out_rays": held_out, "settings": []}
    views = views_of(dev, a.views, a.size, 99)
    train_views = views_of(dev, a.train_views, a.train_size, 7)
    renderer = GraphRenderer(system.models, system.embeddings, N_samples=64, N_importance=128, white_back=True)
    nerf_out = [renderer(r) for r, _, _ in views]
    nerf = [o["rgb_fine"] for o in nerf_out]
    nerf_solid = [o["opacity_fine"] > 0.5 for o in nerf_out]
    report["nerf_psnr"] = [C.psnr(p, gt) for p, (_, gt, _) in zip(nerf, views)]
    print("views ready, NeRF %.2f dB, %.1f s" % (sum(report["nerf_psnr"]) / len(views), time.time() - t), flush=True)

    for N, sigma_threshold in [(N, th) for N in a.lattices for th in a.sigma_thresholds]:
        t0 = time.time()
        v, tri, c = brick_mesh(system, N, sigma_threshold, train_views, a.train_size)
        torch.cuda.synchronize()
        extract_s = time.time() - t0
        if len(tri) == 0:
            report["settings"].append({"N_grid": N, "sigma_threshold": sigma_threshold, "triangles": 0})
            print("N_grid %d: the mesh is empty at sigma %.1f" % (N, sigma_threshold), flush=True)
            continue
        build = lambda: MeshBVH(v, tri, c, device=dev)  # noqa: E731
        bvh = build()                                      # warm-up
        torch.cuda.synchronize()
        build_all = [C.timed(build, 1) for _ in range(a.reps)]
        mesh_renderer = MeshRenderer(bvh, white_back=True, ambient=1.0)
        row = {"N_grid": N, "sigma_threshold": sigma_threshold, "vertices": int(len(v)), "triangles": int(len(tri)), "bad_triangles": bvh.n_bad, "boxes": int(bvh.boxes.shape[0]),
               "extract_s": extract_s, "build_ms_with_upload": median(build_all), "build_ms_all": build_all, "views": []}
        for (r, gt, _), p, solid in zip(views, nerf, nerf_solid):
            out = mesh_renderer(r)
            ms = [C.timed(lambda: mesh_renderer(r), 5) for _ in range(a.reps)]
            # two diagnostics that tell the geometry from the fused colours: the mesh's silhouette filled with the NeRF's pixels,
            # and the share of pixels on which "the mesh is hit" agrees with "the truth is darker than 0.95 in some channel" (the scene has a soft rim)
            hit = out["opacity_fine"] > 0
            silhouette = torch.where(hit[:, None], p, torch.ones_like(p))
            row["views"].append({"psnr_mesh_vs_truth": C.psnr(out["rgb_fine"], gt), "psnr_mesh_vs_nerf": C.psnr(out["rgb_fine"], p),
                                 "psnr_nerf_vs_truth": C.psnr(p, gt), "hit_share": float(out["opacity_fine"].mean()),
                                 "psnr_silhouette_with_nerf_pixels_vs_truth": C.psnr(silhouette, gt),
                                 "silhouette_agreement": float((hit == (gt < 0.95).any(1)).float().mean()),
                                 "truth_object_share": float((gt < 0.95).any(1).float().mean()),
                                 "nerf_solid_share": float(solid.float().mean()),
                                 "hit_agrees_with_nerf_solid": float((hit == solid).float().mean()),
                                 "object_pixels_missed": float(((gt < 0.95).any(1) & ~hit).float().mean()),
                                 "ms_mesh": median(ms), "ms_mesh_all": ms})
        report["settings"].append(row)
        vv = row["views"]
        mean = lambda key: sum(x[key] for x in vv) / len(vv)  # noqa: E731
        print("N_grid %3d sigma %g: %d vertices, %d triangles (%d bad), %d boxes | PSNR mesh vs truth %.2f vs NeRF %.2f (NeRF vs truth %.2f) | "
              "silhouette with NeRF pixels %.2f, agreement %.4f (with the NeRF's opacity > 0.5: %.4f; object pixels missed %.4f) | %.3f of the rays hit | ms mesh %.3f | extract %.1f s, build %.2f ms"
              % (N, sigma_threshold, row["vertices"], row["triangles"], row["bad_triangles"], row["boxes"], mean("psnr_mesh_vs_truth"), mean("psnr_mesh_vs_nerf"),
                 mean("psnr_nerf_vs_truth"), mean("psnr_silhouette_with_nerf_pixels_vs_truth"), mean("silhouette_agreement"),
                 mean("hit_agrees_with_nerf_solid"), mean("object_pixels_missed"), mean("hit_share"), mean("ms_mesh"), extract_s, row["build_ms_with_upload"]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:                       # after every setting: a run cut short keeps what it measured
            json.dump(report, fh, indent=1)
        del bvh, mesh_renderer
    report["wall_s"] = round(time.time() - t, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

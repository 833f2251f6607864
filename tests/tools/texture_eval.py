"""What a texture buys the extracted mesh, measured on the trained brick scene of tests/tools/mesh_eval.py:

    python tests/tools/texture_eval.py [--steps 1200] [--views 2] [--size 800] [--out profiles/texture_eval.json]

The fine model's mesh at N_grid 256 and sigma 2 and 5, as it is and decimated to cells of 2 and 4 voxels (decimate.py), rendered
by MeshRenderer(ambient = 1) on held-out views three ways: with fused vertex colours (mesh.fuse_vertex_colors on the mesh's own
vertices), and with a texture baked (texture.bake) at res 1, 2, 4, 8 by each of the two colour callables — the training views with
the occlusion ray (12 closed-form images of 200 x 200, as mesh_eval.py fuses them) and rays along the triangle normals through the
NeRF.  Per row: PSNR against the closed-form truth and against the NeRF render of the same view (means over the views), the
atlas' size and the bytes of its PNG (the GPU encoder's), and the same two PSNRs over the interior pixels alone (the mesh is hit and
the NeRF's opacity is above 0.99: without the band where an opaque mesh covers the scene's soft rim).  Per mesh also §20's ceiling:
the mesh's silhouette filled with the NeRF's own pixels.  Measured and written down; nothing is asserted."""
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
import mesh_eval as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=E.G.STEPS)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--train_views", type=int, default=12)
    ap.add_argument("--train_size", type=int, default=200)
    ap.add_argument("--N_grid", type=int, default=256)
    ap.add_argument("--sigma_thresholds", type=float, nargs="+", default=[2.0, 5.0])
    ap.add_argument("--res", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--decimate", type=float, nargs="+", default=[0.0, 2.0, 4.0], help="cells in voxels; 0: the mesh as extracted")
    ap.add_argument("--placement", default="quadric")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_eval.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_eval needs a GPU")
    dev = torch.device("cuda:0")
    from nerf_pl_amd import imageio_min, mesh, texture
    from nerf_pl_amd.inference import GraphRenderer
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer

    t_start = time.time()
    system, held_out = E.trained_system(dev, a.steps, a.dtype, lambda s: print(s, flush=True))
    views = E.views_of(dev, a.views, a.size, 99)
    train_views = E.views_of(dev, a.train_views, a.train_size, 7)
    poses = torch.stack([c2w for _, _, c2w in train_views]).numpy().astype(np.float32)
    images = torch.stack([(gt.clamp(0, 1) * 255).to(torch.uint8).view(a.train_size, a.train_size, 3) for _, gt, _ in train_views])
    focal = 1111.0 * a.train_size / 800
    nerf_out = [GraphRenderer(system.models, system.embeddings, N_samples=64, N_importance=128, white_back=True)(r) for r, _, _ in views]
    nerf = [o["rgb_fine"] for o in nerf_out]
    solid = [o["opacity_fine"] > 0.99 for o in nerf_out]
    voxel = (E.RANGE[1] - E.RANGE[0]) / a.N_grid
    callables = {
        "views": texture.colours_from_views(poses, images, focal, E.NEAR, system.nerf_fine, system.embeddings, white_back=True),
        "normals": texture.colours_along_normals(E.NEAR, E.FAR, system.models[0], system.nerf_fine, system.embeddings, white_back=True)}
    report = {"recipe": "brick scene, %d steps, %s (%.2f dB on the held-out rays); mesh of the fine model over %s^3 at N_grid %d; decimation "
                        "%s placement, cells in voxels of %.5f; vertex colours and the 'views' textures from %d closed-form images of %d x %d, "
                        "the 'normals' textures from rays along the triangle normals (near %.1f, far %.1f, 64 + 64 samples); %d held-out "
                        "views of %d x %d from radius 4; MeshRenderer ambient 1, bilinear; PSNRs are means over the views"
                        % (a.steps, a.dtype, held_out, list(E.RANGE), a.N_grid, a.placement, voxel, a.train_views, a.train_size, a.train_size,
                           E.NEAR, E.FAR, a.views, a.size, a.size),
              "nerf_psnr_vs_truth": sum(C.psnr(p, gt) for p, (_, gt, _) in zip(nerf, views)) / len(views), "rows": []}
    print("NeRF vs truth %.2f dB, %.1f s" % (report["nerf_psnr_vs_truth"], time.time() - t_start), flush=True)

    def score(renderer):
        """means over the views of: PSNR vs truth, vs the NeRF render, of the silhouette filled with the NeRF's pixels vs truth, and
        the first two over the INTERIOR pixels alone — the mesh is hit and the NeRF's opacity is above 0.99, which leaves out the
        band where an opaque mesh covers the scene's soft rim — with the share of the pixels that is"""
        cols = [[] for _ in range(6)]
        for (r, gt, _), p, s in zip(views, nerf, solid):
            out = renderer(r)
            hit = out["opacity_fine"] > 0
            inside = hit & s
            for c, x in zip(cols, (C.psnr(out["rgb_fine"], gt), C.psnr(out["rgb_fine"], p),
                                   C.psnr(torch.where(hit[:, None], p, torch.ones_like(p)), gt),
                                   C.psnr(out["rgb_fine"][inside], gt[inside]), C.psnr(out["rgb_fine"][inside], p[inside]),
                                   float(inside.float().mean()))):
                c.append(x)
        return [sum(c) / len(c) for c in cols]

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:                       # after every row: a run cut short keeps what it measured
            json.dump(report, fh, indent=1)

    for sigma in a.sigma_thresholds:
        for cells in a.decimate:
            v, tri, _ = mesh.extract_color_mesh(system.nerf_fine, system.embeddings, a.N_grid, E.RANGE, E.RANGE, E.RANGE, sigma,
                                                decimate_cell=cells * voxel if cells else None, decimate_placement=a.placement)
            if len(tri) == 0:
                print("sigma %g, %g voxels: the mesh is empty" % (sigma, cells), flush=True)
                continue
            dv, dt = torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev)
            base = {"sigma_threshold": sigma, "decimate_voxels": cells, "vertices": int(len(v)), "triangles": int(len(tri))}
            t0 = time.time()
            colors = mesh.fuse_vertex_colors(dv, poses, images, focal, E.NEAR, system.nerf_fine, system.embeddings, white_back=True)
            vs_truth, vs_nerf, ceiling, in_truth, in_nerf, share = score(MeshRenderer(MeshBVH(dv, dt, colors), white_back=True))
            torch.cuda.synchronize()
            report["rows"].append(dict(base, colouring="vertex", psnr_vs_truth=vs_truth, psnr_vs_nerf=vs_nerf,
                                       psnr_interior_vs_truth=in_truth, psnr_interior_vs_nerf=in_nerf, interior_share=share,
                                       silhouette_with_nerf_pixels_vs_truth=ceiling, colour_s=time.time() - t0,
                                       colour_bytes=3 * int(len(v))))
            print("sigma %g, %g voxels: %d vertices, %d triangles | vertex colours %.2f dB vs truth, %.2f vs NeRF; interior (%.3f of the "
                  "pixels) %.2f, %.2f | silhouette ceiling %.2f"
                  % (sigma, cells, len(v), len(tri), vs_truth, vs_nerf, share, in_truth, in_nerf, ceiling), flush=True)
            save()
            for R in a.res:
                for name, colour in callables.items():
                    t0 = time.time()
                    try:
                        atlas = texture.bake(dv, dt, R, colour)
                    except ValueError as e:                # the atlas would exceed 16384 rows
                        report["rows"].append(dict(base, colouring="texture/" + name, res=R, error=str(e)))
                        print("  res %d %s: %s" % (R, name, e), flush=True)
                        save()
                        continue
                    torch.cuda.synchronize()
                    bake_s = time.time() - t0
                    vs_truth, vs_nerf, _, in_truth, in_nerf, _ = score(MeshRenderer(MeshBVH(dv, dt, texture=atlas), white_back=True))
                    try:
                        png = len(imageio_min.png_bytes_device(atlas.data.unsqueeze(0))[0])
                    except Exception as e:                 # noqa: BLE001  (a size the encoder refuses is a finding, not a failure)
                        png = "encoder: %s" % e
                    report["rows"].append(dict(base, colouring="texture/" + name, res=R, psnr_vs_truth=vs_truth, psnr_vs_nerf=vs_nerf,
                                               psnr_interior_vs_truth=in_truth, psnr_interior_vs_nerf=in_nerf, atlas_width=atlas.width, atlas_height=atlas.height, atlas_bytes=3 * atlas.width * atlas.height,
                                               png_bytes=png, bake_s=bake_s))
                    print("  res %d %-7s %5d x %5d, PNG %s B, baked in %.1f s | %.2f dB vs truth, %.2f vs NeRF; interior %.2f, %.2f"
                          % (R, name, atlas.width, atlas.height, png, bake_s, vs_truth, vs_nerf, in_truth, in_nerf), flush=True)
                    save()
                    del atlas
    report["wall_s"] = round(time.time() - t_start, 1)
    save()
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

"""Timing of the mesh-extraction stages (nerf_pl_amd/mesh.py) at the reference's defaults: N_grid 256, 100 views of 800 x 800,
on a procedural model (tools/_synth.py: default-init NeRF with a sharpened density head).  Device events around each stage
after one warm-up run of it; the PLY write is timed with the host clock.  Marching cubes' kernel time excludes the one
16-byte device-to-host read of (V, T) between its two launches, and is set against the bytes its passes must move.

    python tools/mesh_bench.py [--N 256] [--views 100] [--wh 800] [--dtype bf16] [--out profiles/mesh_bench.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _synth import make_model  # noqa: E402

from nerf_pl_amd import mesh, ops  # noqa: E402
from nerf_pl_amd.grid import sigma_grid  # noqa: E402
from nerf_pl_amd.models import Embedding  # noqa: E402

HBM_PEAK = 8.0e12        # MI355X_MICROARCH.md: HBM3E peak; 6.29 TB/s measured for a float4 copy
HBM_COPY = 6.29e12


def ev_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def mc_split(volume, iso):
    """marching cubes with the count and emit launches timed apart (the same calls ops.marching_cubes makes)"""
    from nerf_pl_amd._lib import load, ptr, stream_ptr
    lib = load()
    n0, n1, n2 = volume.shape
    ws = torch.empty(lib.nerfhip_marching_cubes_workspace_bytes(n0, n1, n2), device=volume.device, dtype=torch.uint8)
    totals = torch.empty(2, device=volume.device, dtype=torch.int64)
    t_count, _ = ev_time(lambda: lib.nerfhip_marching_cubes_count(ptr(volume), n0, n1, n2, float(iso), ptr(ws), ptr(totals),
                                                                  stream_ptr()))
    V, T = (int(x) for x in totals.cpu())
    verts = torch.empty(V, 3, device=volume.device, dtype=torch.float64)
    tris = torch.empty(T, 3, device=volume.device, dtype=torch.int32)
    t_emit, _ = ev_time(lambda: lib.nerfhip_marching_cubes_emit(ptr(volume), n0, n1, n2, float(iso), ptr(ws), ptr(totals), ptr(verts),
                                                                ptr(tris), stream_ptr()))
    return t_count, t_emit, V, T


def look_at(pos):
    back = pos / np.linalg.norm(pos)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(back, right), back, pos], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--wh", type=int, default=800)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--quantile", type=float, default=0.9, help="sigma threshold = this quantile of the grid")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = make_model(0, dev, a.dtype).eval()
    emb = [Embedding(3, 10), Embedding(3, 4)]
    rng = ((-1.0, 1.0),) * 3
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sigma_grid(model, a.N, *rng)                                           # warm-up
    t_grid, sig = ev_time(lambda: sigma_grid(model, a.N, *rng))
    thr = float(torch.quantile(sig.flatten()[:: max(1, sig.numel() // (1 << 23))].float(), a.quantile))
    mc_split(sig, thr)                                                     # warm-up
    t_count, t_emit, V, T = mc_split(sig, thr)
    npts = a.N ** 3
    # bytes each pass must move (every array once): count reads the volume and writes mask + case (6 B/point); the vertex pass
    # reads mask + volume and writes the vertex base (9 B/point) and the vertices (24 B each); the triangle pass reads case,
    # mask and vertex base (6 B/point) and writes the triangles (12 B each)
    mc_bytes = npts * (6 + 9 + 6) + 24 * V + 12 * T
    t_mc = t_count + t_emit
    t_mc_full, (vi, ti) = ev_time(lambda: mesh.marching_cubes(sig, thr))
    vw = torch.from_numpy(mesh.world_coords(vi, a.N, *rng)).to(dev)
    mesh.keep_largest_cluster(vw, ti)                                      # warm-up
    t_clean, (vk, tk) = ev_time(lambda: mesh.keep_largest_cluster(vw, ti))
    say("N_grid %d (%d points), sigma threshold %.4g (quantile %.2f), model %s" % (a.N, npts, thr, a.quantile, a.dtype))
    say("sigma grid            %9.3f ms" % t_grid)
    say("marching cubes        %9.3f ms kernels (count+scan %.3f, emit %.3f); %.3f ms with the size read-back; V %d T %d"
        % (t_mc, t_count, t_emit, t_mc_full, V, T))
    say("  bytes moved         %9.1f MB -> %.2f TB/s = %.1f%% of HBM peak %.1f TB/s (%.1f%% of the %.2f TB/s copy rate)"
        % (mc_bytes / 1e6, mc_bytes / (t_mc * 1e-3) / 1e12, 100 * mc_bytes / (t_mc * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12,
           100 * mc_bytes / (t_mc * 1e-3) / HBM_COPY, HBM_COPY / 1e12))
    say("largest cluster       %9.3f ms (keeps V %d T %d of V %d T %d)" % (t_clean, vk.shape[0], tk.shape[0], V, T))
    W = H = a.wh
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)                     # blender.py: camera_angle_x of the synthetic scenes
    g = np.random.default_rng(0)
    poses = np.stack([look_at(p / np.linalg.norm(p) * 4.0) for p in g.standard_normal((a.views, 3))])
    images = torch.from_numpy(g.integers(0, 256, (a.views, H, W, 3), dtype=np.uint8)).to(dev)
    mesh.fuse_vertex_colors(vk, poses[:1], images[:1], focal, 2.0, model, emb)  # warm-up
    t_fuse, colors = ev_time(lambda: mesh.fuse_vertex_colors(vk, poses, images, focal, 2.0, model, emb))
    # the fusion kernels alone on one view (projection + colour + ray kernel, accumulation kernel), without the render
    w2c = np.linalg.inv(np.concatenate([poses[0], [[0, 0, 0, 1]]], 0).astype(np.float32))[:3]
    acc = torch.zeros(vk.shape[0], 4, device=dev, dtype=torch.float64)
    op = torch.zeros(vk.shape[0], device=dev)
    ops.view_rays(vk, w2c, poses[0][:, 3], focal, images[0], 2.0)
    t_view, (c4, dep, _) = ev_time(lambda: ops.view_rays(vk, w2c, poses[0][:, 3], focal, images[0], 2.0))
    t_acc, _ = ev_time(lambda: ops.color_accumulate(c4, dep, op, 0.2, acc))
    say("colour fusion         %9.3f ms for %d views of %dx%d = %.3f ms per view (of which view-ray kernel %.3f, accumulate %.3f;"
        " the rest is the occlusion render of %d rays x 64 samples)" % (t_fuse, a.views, W, H, t_fuse / a.views, t_view, t_acc,
                                                                     vk.shape[0]))
    vn, tn, cn = vk.cpu().numpy(), tk.cpu().numpy(), colors.cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        mesh.write_ply(os.path.join(d, "m.ply"), vn, tn, cn)
        t_ply = (time.perf_counter() - t0) * 1e3
        size = os.path.getsize(os.path.join(d, "m.ply"))
    say("PLY write             %9.3f ms (host, %.1f MB)" % (t_ply, size / 1e6))
    rec = dict(N=a.N, views=a.views, wh=a.wh, dtype=a.dtype, V=V, T=T, V_kept=int(vk.shape[0]), T_kept=int(tk.shape[0]),
               sigma_grid_ms=t_grid, mc_kernels_ms=t_mc, mc_count_ms=t_count, mc_emit_ms=t_emit, mc_with_readback_ms=t_mc_full,
               mc_bytes=mc_bytes, mc_TBps=mc_bytes / (t_mc * 1e-3) / 1e12, cluster_ms=t_clean, fuse_ms=t_fuse,
               fuse_per_view_ms=t_fuse / a.views, view_rays_ms=t_view, accumulate_ms=t_acc, ply_ms=t_ply)
    say(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

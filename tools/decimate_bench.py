"""Timing of the mesh decimation (nerf_pl_amd/decimate.py) on the mesh of tools/mesh_bench.py: N_grid 256 on a
procedural model (tools/_synth.py), marching cubes, largest cluster — 4.8 M vertices, 9.4 M triangles.  Cells of 2 and 4 voxels,
both placements.  Device events; one warm-up run of every configuration; the configurations run in alternating order (forward,
then backward) over the repetitions; median [min, max].  Per configuration: V' and T'; the time of every pass (C entry point or
torch sort / gather) beside the bytes it must move (every array once, gathers counted at their useful bytes); the total; the
MeshBVH build; an 800 x 800 cast; one view of the colour fusion, before and after; the PSNR of MeshRenderer on the decimated mesh
against the render of the undecimated one (vertex colours = position, 8 views).

    python tools/decimate_bench.py [--N 256] [--reps 5] [--wh 800] [--out profiles/decimate_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _synth import make_model  # noqa: E402
from mesh_bench import ev_time, look_at  # noqa: E402

from nerf_pl_amd import mesh, ops  # noqa: E402
from nerf_pl_amd.grid import sigma_grid  # noqa: E402
from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer  # noqa: E402
from nerf_pl_amd.models import Embedding  # noqa: E402


class Timed(ops._DeviceArrays):
    """the device backend with an event pair around every pass"""
    log = []

    @staticmethod
    def _timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        Timed.log.append(("%02d %s" % (len(Timed.log), name), e0, e1))
        return out

    @staticmethod
    def call(name, *args):
        return Timed._timed(name.replace("nerfhip_mesh_decimate_", ""), lambda: ops._DeviceArrays.call(name, *args))

    @staticmethod
    def sort(keys):
        return Timed._timed("sort (%d keys)" % keys.numel(), lambda: ops._DeviceArrays.sort(keys))

    @staticmethod
    def sort_stable(keys):
        return Timed._timed("sort, stable (%d keys)" % keys.numel(), lambda: ops._DeviceArrays.sort_stable(keys))

    @staticmethod
    def take(a, index):
        return Timed._timed("gather", lambda: ops._DeviceArrays.take(a, index))


def pass_bytes(V, T, C, n_v, n_t, colors, quadric):
    """bytes each pass must move: every array once, a gather at the bytes it uses"""
    k = 3 if colors else 0
    return {"bounds": 12 * V, "keys": 12 * V + 8 * V, "clusters": 8 * V + 8 * V + 4 * V + 4 * C,
            "entries": 12 * T + 12 * T + 24 * T, "place": 8 * V + (12 + k) * V + (24 + 12 + k) * C + (quadric and 24 * T + 144 * T + 36 * C),
            "tri_keys": 12 * T + 12 * T + 17 * T, "duplicates": 16 * T, "mark": 13 * T + 12 * T + T + 2 * C,
            "compact": (1 + 12 + k + 4) * C + (12 + k) * n_v + T + 36 * n_t + 12 * V}


def psnr(a, b):
    return float(-10.0 * torch.log10(torch.mean((a - b) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wh", type=int, default=800)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--quantile", type=float, default=0.9)
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

    sig = sigma_grid(model, a.N, *rng)
    thr = float(torch.quantile(sig.flatten()[:: max(1, sig.numel() // (1 << 23))].float(), a.quantile))
    vi, ti = mesh.marching_cubes(sig, thr)
    v, t = mesh.keep_largest_cluster(torch.from_numpy(mesh.world_coords(vi, a.N, *rng)).to(dev), ti)
    del sig, vi, ti
    V, T = v.shape[0], t.shape[0]
    colors = ((v * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8)
    voxel = 2.0 / a.N
    say("N_grid %d: V %d T %d, voxel %.5f" % (a.N, V, T, voxel))

    W = H = a.wh
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    g = np.random.default_rng(0)
    poses = np.stack([look_at(p / np.linalg.norm(p) * 4.0) for p in g.standard_normal((8, 3))])
    image = torch.from_numpy(g.integers(0, 256, (1, H, W, 3), dtype=np.uint8)).to(dev)

    def view_rays(pose):
        j, i = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
        d = torch.stack([(i - W / 2) / focal, -(j - H / 2) / focal, -torch.ones_like(i)], -1).reshape(-1, 3)
        c2w = torch.from_numpy(pose).to(dev)
        d = d @ c2w[:, :3].T
        o = c2w[:, 3].expand_as(d)
        return torch.cat([o, d, torch.full_like(d[:, :1], 2.0), torch.full_like(d[:, :1], 6.0)], 1).contiguous()

    rays = [view_rays(p) for p in poses]

    def downstream(label, vv, tt, cc):
        MeshBVH(vv, tt, cc)                                                 # warm-up
        t_build, bvh = ev_time(lambda: MeshBVH(vv, tt, cc))
        r = MeshRenderer(bvh, white_back=True)
        r(rays[0])
        t_cast, _ = ev_time(lambda: bvh.cast(rays[0]))
        mesh.fuse_vertex_colors(vv, poses[:1], image, focal, 2.0, model, emb)
        t_fuse, _ = ev_time(lambda: mesh.fuse_vertex_colors(vv, poses[:1], image, focal, 2.0, model, emb))
        say("  %-22s MeshBVH build %8.3f ms, %dx%d cast %7.3f ms, colour fusion %8.3f ms per view (%d rays)" % (label, t_build, W, H, t_cast,
                                                                                                          t_fuse, vv.shape[0]))
        return [r(x)["rgb_fine"] for x in rays], dict(build_ms=t_build, cast_ms=t_cast, fuse_per_view_ms=t_fuse)

    full_rgb, full_rec = downstream("undecimated", v, t, colors)
    configs = [(k, p) for k in (2, 4) for p in ("mean", "quadric")]
    runs = {c: [] for c in configs}
    passes = {c: {} for c in configs}
    outs = {}
    for rep in range(-1, a.reps):                                           # rep -1: warm-up
        for c in (configs if rep % 2 == 0 else configs[::-1]):
            Timed.log = []
            t_all, out = ev_time(lambda: ops._mesh_decimate(Timed, v, t, colors, c[0] * voxel, c[1], None, 1e-3))
            outs[c] = out
            if rep >= 0:
                runs[c].append(t_all)
                for name, e0, e1 in Timed.log:
                    passes[c].setdefault(name, []).append(e0.elapsed_time(e1))
    recs = []
    for c in configs:
        out_v, out_t, out_c, _, counts = outs[c]
        n_v, n_t = out_v.shape[0], out_t.shape[0]
        say("cell %d voxels, %s: V' %d T' %d (%s)" % (c[0], c[1], n_v, n_t, ", ".join("%s %d" % kv for kv in counts.items())))
        say("  total %8.3f ms [%.3f, %.3f] over %d runs, with the two host reads of the bounds and the counts" %
            (statistics.median(runs[c]), min(runs[c]), max(runs[c]), len(runs[c])))
        nbytes = pass_bytes(V, T, counts["clusters"], n_v, n_t, True, c[1] == "quadric")
        for name, ms in passes[c].items():
            med = statistics.median(ms)
            extra = ""
            if name[3:] in nbytes:
                extra = "  %8.1f MB -> %5.2f TB/s" % (nbytes[name[3:]] / 1e6, nbytes[name[3:]] / (med * 1e-3) / 1e12)
            say("    %-28s %8.3f ms [%.3f, %.3f]%s" % (name, med, min(ms), max(ms), extra))
        rgb, rec = downstream("decimated", out_v, out_t, out_c)
        quality = statistics.mean(psnr(x, y) for x, y in zip(rgb, full_rgb))
        say("  PSNR against the undecimated render, mean of %d views of %dx%d: %.2f dB" % (len(rays), W, H, quality))
        recs.append(dict(rec, cell_voxels=c[0], placement=c[1], V_out=n_v, T_out=n_t, counts=counts, total_ms=statistics.median(runs[c]),
                         total_min_ms=min(runs[c]), total_max_ms=max(runs[c]), psnr_db=quality,
                         passes_ms={k: statistics.median(x) for k, x in passes[c].items()}))
    say(json.dumps(dict(N=a.N, V=V, T=T, reps=a.reps, undecimated=full_rec, configs=recs)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

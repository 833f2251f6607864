"""Mesh decimation on the GPU: grid vertex clustering (Rossignac-Borrel) with two placements of a cluster's
representative — "mean", the mean of the member vertices (open3d's simplify_vertex_clustering default), and "quadric", the point
that minimises the summed squared distance to the planes of the member triangles, regularised towards the mean and kept inside the
cell (Lindstrom 2000).  The mean shrinks convex shapes and rounds edges; the quadric placement does not.

    v, t, c = decimate(*mesh.extract_color_mesh(...), cell=2 * voxel, placement="quadric")
    small = MeshBVH.from_ply("lego.ply").decimated(cell=0.02)

One pass, deterministic (two runs give identical bytes), no floating-point atomics: keys -> torch.sort -> scans -> one thread per
vertex, cluster or triangle (csrc/decimate.hip); include/nerfhip.h states the result exactly.  Clustering takes a cell size, not a
triangle budget: the command line prints the counts so that a user can bisect.

    python -m nerf_pl_amd.decimate --ply lego.ply --cell 0.02 --placement quadric --out lego_small.ply
"""
import torch

from . import ops
from .meshcast import _to_device

__all__ = ["decimate"]


def decimate(vertices, triangles, colors=None, cell=None, placement="mean", origin=None, eps=1e-3, return_info=False):
    """vertices (V, 3) fp32, triangles (T, 3) int32, colors (V, 3) uint8 or None — device tensors, or the numpy arrays
    mesh.extract_color_mesh / mesh.read_ply return (copied to the current GPU); a CPU tensor raises NerfHipError — ->
    (vertices' (V', 3), triangles' (T', 3), colors' (V', 3) or None) on the device.  `cell` is the edge of the clustering cells,
    `origin` the corner the cells start at (default: the mesh's minimum), `eps` the quadric's regularisation.  With return_info a
    fourth value: a dict with `cluster_of` (V,) int32 — the output vertex of every input vertex, -1 for a non-finite one or one
    whose cluster no surviving triangle names — and the counts `clusters`, `bad`, `collapsed`, `duplicate`, `unreferenced`."""
    if cell is None:
        raise ValueError("decimate: cell (the edge of the clustering cells) must be given")
    vertices = _to_device("vertices", vertices, torch.float32, None)
    triangles = _to_device("triangles", triangles, torch.int32, vertices.device)
    colors = _to_device("colors", colors, torch.uint8, vertices.device)
    out_v, out_t, out_c, cluster_of, counts = ops.mesh_decimate(vertices, triangles, colors, cell, placement, origin, eps)
    if return_info:
        return out_v, out_t, out_c, dict(counts, cluster_of=cluster_of)
    return out_v, out_t, out_c


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Decimate a PLY mesh by vertex clustering (no network involved)")
    ap.add_argument("--ply", required=True, help="the mesh (python -m nerf_pl_amd.mesh, or any file of mesh.write_ply)")
    ap.add_argument("--cell", type=float, required=True, help="edge of the clustering cells, in the mesh's units")
    ap.add_argument("--placement", default="mean", choices=sorted(ops.DECIMATE_PLACEMENTS))
    ap.add_argument("--eps", type=float, default=1e-3, help="regularisation of the quadric placement")
    ap.add_argument("--out", required=True, help="the PLY file to write")
    a = ap.parse_args(argv)
    from .mesh import read_ply, write_ply
    v, t, c = read_ply(a.ply)
    out_v, out_t, out_c, info = decimate(v, t, c, cell=a.cell, placement=a.placement, eps=a.eps, return_info=True)
    write_ply(a.out, out_v, out_t, out_c)
    print("%s: %d vertices, %d triangles -> %s: %d vertices, %d triangles (cell %g, %s)"
          % (a.ply, len(v), len(t), a.out, out_v.shape[0], out_t.shape[0], a.cell, a.placement))
    print("clusters %(clusters)d, bad %(bad)d, collapsed %(collapsed)d, duplicate %(duplicate)d, unreferenced %(unreferenced)d" % info)


if __name__ == "__main__":
    main()

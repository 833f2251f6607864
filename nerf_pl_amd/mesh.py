"""Coloured mesh extraction from a trained NeRF: the reference's extract_color_mesh.py without mcubes, open3d, cv2 or plyfile.

    sigma_grid (grid.py) -> marching_cubes -> world_coords -> keep_largest_cluster -> fuse_vertex_colors -> write_ply

Every stage runs on the device through HIP kernels (csrc/mesh.hip); the host only reads the sizes of variable-length outputs,
inverts the 4x4 camera poses and maps index coordinates to world coordinates (in numpy, to reproduce the reference's float32
arithmetic exactly).  Dataset I/O stays with the caller: images are loaded and resized exactly as the reference does (PIL)
and passed in as one (n, H, W, 3) uint8 device tensor.

Triangle winding.  Each triangle (i, j, k) of `marching_cubes` has its right-hand normal (v_j - v_i) x (v_k - v_i), taken in
index coordinates (a0, a1, a2), pointing to the side where the volume is BELOW `iso`: for a density grid (occupied = above the
threshold) normals point out of the object and the signed volume of a closed surface is positive.  The reference's world
mapping swaps the first two axes, which mirrors the mesh, so in its world coordinates the normals point inwards.  Whether this
matches PyMCubes' winding has not been checked (mcubes is not available to the tests).
"""
import numpy as np
import torch

from . import ops
from .grid import sigma_grid

__all__ = ["marching_cubes", "keep_largest_cluster", "vertex_normals", "world_coords", "fuse_vertex_colors", "write_ply",
           "extract_color_mesh"]


def marching_cubes(volume, iso):
    """mcubes.marching_cubes(volume, iso) on the device (extract_color_mesh.py:144).

    volume: contiguous float32 CUDA tensor (n0, n1, n2), every dimension >= 2, indexed [a0, a1, a2] like the numpy array.
    Returns (vertices (V, 3) float64, triangles (T, 3) int32), both on the device; vertices are in index coordinates.

    - One vertex per lattice edge whose end values straddle `iso` (one end < iso, compared in fp64), shared by every triangle
      on that edge.  Position a + t along the edge with t = (iso - f_a) / (f_b - f_a) in fp64 from the float32 values, f_a at
      the lower index (the midpoint when f_a == f_b).
    - Cases and triangles from Paul Bourke's tables (bit i of the case set where corner i is below iso).
    - Order: vertices by (owning lattice point in C order, edge axis 0/1/2), the owner being the edge's lower end; triangles by
      (cell in C order, table order).  Two runs give identical bytes.
    - Winding: see the module docstring.
    Raises NerfHipError for a CPU tensor, a dtype other than float32, rank != 3, a dimension < 2, or a mesh whose V or T does
    not fit int32."""
    return ops.marching_cubes(volume, iso)


def keep_largest_cluster(vertices, triangles):
    """open3d's cluster_connected_triangles + argmax + remove_triangles_by_index + remove_unreferenced_vertices
    (extract_color_mesh.py:163-170).

    Triangles are in one cluster when they share an edge (two vertex ids; a shared vertex alone does not connect).  The cluster
    with the most triangles survives; on a tie, the one holding the lowest triangle index (what np.argmax over open3d's
    cluster ids, numbered in order of first triangle, picks).  Surviving triangles and referenced vertices keep their order;
    triangle indices are remapped.  vertices: (V, C) device tensor of any dtype; triangles: (T, 3) int32 device tensor.
    Returns (vertices', triangles') on the device."""
    if not torch.is_tensor(vertices) or vertices.dim() != 2:
        raise ops.NerfHipError("keep_largest_cluster: vertices must be a (V, C) tensor")
    if not vertices.is_cuda:
        raise ops.NerfHipError("nerf_pl_amd runs on MI355X only: vertices is a %s tensor (no CPU fallback)" % vertices.device)
    kept_ids, kept_tris = ops.largest_cluster(triangles, vertices.shape[0])
    return vertices.index_select(0, kept_ids), kept_tris


def vertex_normals(vertices, triangles):
    """open3d's compute_vertex_normals (extract_color_mesh.py:188): per vertex the sum of the unnormalised face normals
    (v1 - v0) x (v2 - v0) of its triangles in fp64, normalised; a zero sum gives (0, 0, 1).  vertices (V, 3) float32,
    triangles (T, 3) int32 -> (V, 3) float64, on the device.  The fp64 sums are formed with atomics, so their last bits
    depend on the order of accumulation."""
    return ops.vertex_normals(vertices, triangles)


def world_coords(vertices, N, x_range, y_range, z_range, coords="reference"):
    """Index-space vertices of marching_cubes(sigma_grid(...)) -> float32 world coordinates, as a numpy (V, 3) array.

    The grid is indexed [iy, ix, iz] (grid.sigma_grid), so a0 runs along y and a1 along x.
      coords="reference": extract_color_mesh.py:148-153 bit for bit in float32: v / N (N, not N - 1), then
                          x = (ymax - ymin) v[:, 1] + ymin and y = (xmax - xmin) v[:, 0] + xmin (the reference's range swap:
                          identical to the true mapping only when the x and y ranges are equal), z = (zmax - zmin) v[:, 2] + zmin.
      coords="exact":     the lattice's own positions: x = xmin + a1 (xmax - xmin) / (N - 1), y = ymin + a0 (ymax - ymin) / (N - 1),
                          z = zmin + a2 (zmax - zmin) / (N - 1), in fp64, rounded once to float32."""
    v = vertices.cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)
    v = v.astype(np.float64, copy=False)
    (xmin, xmax), (ymin, ymax), (zmin, zmax) = x_range, y_range, z_range
    if coords == "reference":
        w = (v / N).astype(np.float32)
        x_ = (ymax - ymin) * w[:, 1] + ymin
        y_ = (xmax - xmin) * w[:, 0] + xmin
        w[:, 0] = x_
        w[:, 1] = y_
        w[:, 2] = (zmax - zmin) * w[:, 2] + zmin
        return w
    if coords == "exact":
        out = np.empty_like(v)
        out[:, 0] = xmin + v[:, 1] * ((xmax - xmin) / (N - 1))
        out[:, 1] = ymin + v[:, 0] * ((ymax - ymin) / (N - 1))
        out[:, 2] = zmin + v[:, 2] * ((zmax - zmin) / (N - 1))
        return out.astype(np.float32)
    raise ValueError("coords must be 'reference' or 'exact', got %r" % (coords,))


def _render(models, embeddings, rays, N_samples, N_importance, chunk, white_back):
    """the reference's batched `f` (extract_color_mesh.py:64-85): render_rays(test_time=True) over chunks of rays"""
    from .models.rendering import render_rays
    out = {}
    for i in range(0, rays.shape[0], chunk):
        r = render_rays(models, embeddings, rays[i:i + chunk], N_samples, False, 0, 0, N_importance, chunk, white_back,
                        test_time=True)
        for k, v in r.items():
            out.setdefault(k, []).append(v)
    return {k: torch.cat(v, 0) for k, v in out.items()}


@torch.no_grad()
def fuse_vertex_colors(vertices, poses, images, focal, near, nerf_fine, embeddings, occ_threshold=0.2, N_samples=64,
                       white_back=False, chunk=32 * 1024, use_vertex_normal=False, triangles=None, far=None, near_t=1.0,
                       nerf_coarse=None, N_importance=64):
    """Per-vertex colours of extract_color_mesh.py:172-285 -> (V, 3) uint8 on the device.

    vertices (V, 3) float32 world coordinates (device tensor or numpy); poses (n, 3, 4) float32 camera-to-world;
    images (n, H, W, 3) uint8 on the device; focal, near (the dataset's bounds.min()) scalars.

    Default mode, per view: w2c = inverse of the float32 4x4 c2w (host); fp64 projection with y and z negated,
    K = [[f, 0, W/2], [0, f, H/2], [0, 0, 1]], depth = z + 1e-5, pixel = float32(xy / depth) clipped to the image; colour =
    bilinear sample of the uint8 image exactly as cv2.remap(INTER_LINEAR) forms it (positions rounded to 1/32 pixel, 15-bit
    weights).  Occlusion: a ray from the camera centre to the vertex (float32 normalised direction, near, far = the float32
    z-depth — the reference's quirk, not the Euclidean distance) through render_rays([nerf_fine], ..., N_samples, 0, test_time)
    -> opacity_coarse.  Weight w = 0.1 / depth + (opacity < occ_threshold), a NaN opacity counting as 0; colour * w and w are
    summed in fp64 on the device; the result is trunc(sum(colour w) / sum(w)).

    use_vertex_normal=True (extract_color_mesh.py:187-205): needs `triangles`, `far` (bounds.max()) and `nerf_coarse`; rays start
    at v - n near near_t along the vertex normal n (vertex_normals), render_rays([nerf_coarse, nerf_fine], ..., N_samples,
    N_importance) and the colour is trunc(rgb_fine * 255); poses and images are not used."""
    dev = next(nerf_fine.parameters()).device
    verts = torch.as_tensor(np.asarray(vertices, np.float32) if not torch.is_tensor(vertices) else vertices).to(dev).contiguous()
    if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise ops.NerfHipError("fuse_vertex_colors: vertices must be (V, 3) float32")
    V = verts.shape[0]
    if use_vertex_normal:
        if triangles is None or far is None or nerf_coarse is None:
            raise ValueError("use_vertex_normal needs triangles, far and nerf_coarse")
        tris = torch.as_tensor(triangles).to(dev, torch.int32).contiguous()
        normals = ops.vertex_normals(verts, tris)
        rays = ops.normal_rays(verts, normals, np.float32(near), np.float32(far), np.float32(near_t))
        rgb = _render([nerf_coarse, nerf_fine], embeddings, rays, N_samples, N_importance, chunk, white_back)["rgb_fine"]
        return ops.rgb_to_u8(rgb.contiguous())
    poses = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, np.float32).reshape(-1, 3, 4)
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[0] != len(poses) or images.shape[3] != 3:
        raise ops.NerfHipError("fuse_vertex_colors: images must be an (n, H, W, 3) uint8 device tensor, one per pose")
    accum = torch.zeros(V, 4, device=dev, dtype=torch.float64)
    for idx in range(len(poses)):
        c2w = np.concatenate([poses[idx], np.array([[0, 0, 0, 1]], np.float32)], 0)
        w2c = np.linalg.inv(c2w)[:3]                                   # float32, as the reference's P_w2c
        colors, depth, rays = ops.view_rays(verts, w2c, poses[idx][:, 3], focal, images[idx], np.float32(near))
        opacity = _render([nerf_fine], embeddings, rays, N_samples, 0, chunk, white_back)["opacity_coarse"]
        ops.color_accumulate(colors, depth, opacity.contiguous(), np.float32(occ_threshold), accum)
    return ops.color_finish(accum)


def write_ply(path, vertices, triangles, colors=None):
    """Binary little-endian PLY with the bytes plyfile writes for the reference's arrays (extract_color_mesh.py:280-297):
    vertex x, y, z float32 [+ red, green, blue uchar], face `list uchar int vertex_indices`."""
    v = np.asarray(vertices.cpu() if torch.is_tensor(vertices) else vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles.cpu() if torch.is_tensor(triangles) else triangles, np.int32).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = np.asarray(colors.cpu() if torch.is_tensor(colors) else colors, np.uint8).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError("write_ply: %d colours for %d vertices" % (len(c), len(v)))
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.empty(len(v), dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(len(t), dtype=[("n", "u1"), ("vertex_indices", "<i4", (3,))])
    frec["n"] = 3
    frec["vertex_indices"] = t
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v),
              "property float x", "property float y", "property float z"]
    if colors is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += ["element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def read_ply(path):
    """(vertices (V,3) float32, triangles (T,3) int32, colors (V,3) uint8 or None) of a file written by write_ply."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    V = int(next(l for l in lines if l.startswith("element vertex")).split()[2])
    T = int(next(l for l in lines if l.startswith("element face")).split()[2])
    has_c = "property uchar red" in lines
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_c else [])
    vrec = np.frombuffer(data, dtype=fields, count=V, offset=end)
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("vertex_indices", "<i4", (3,))], count=T, offset=end + vrec.nbytes)
    if T and not (frec["n"] == 3).all():
        raise ValueError("read_ply: only triangles are supported")
    v = np.stack([vrec["x"], vrec["y"], vrec["z"]], 1)
    c = np.stack([vrec["red"], vrec["green"], vrec["blue"]], 1) if has_c else None
    return v, np.ascontiguousarray(frec["vertex_indices"]), c


@torch.no_grad()
def extract_color_mesh(nerf_fine, embeddings, N_grid, x_range, y_range, z_range, sigma_threshold, poses=None, images=None,
                       focal=None, near=None, far=None, occ_threshold=0.2, N_samples=64, white_back=False, chunk=32 * 1024,
                       use_vertex_normal=False, nerf_coarse=None, N_importance=64, near_t=1.0, coords="reference",
                       decimate_cell=None, decimate_placement="mean"):
    """extract_color_mesh.py end to end: sigma_grid -> marching_cubes -> world_coords -> keep_largest_cluster ->
    fuse_vertex_colors.  Returns numpy (vertices (V,3) float32 world, triangles (T,3) int32, colors (V,3) uint8); colors is None
    when neither poses/images (default mode) nor use_vertex_normal is given.  write_ply(path, *result) writes the reference's file.
    decimate_cell (world units; None: the reference's mesh) clusters the vertices of the largest cluster into cells of that edge
    (decimate.py) before the colour fusion, which then renders one ray per remaining vertex and view."""
    sigma = sigma_grid(nerf_fine, N_grid, x_range, y_range, z_range, embedding_xyz=embeddings[0])
    v_idx, tris = marching_cubes(sigma, sigma_threshold)
    dev = sigma.device
    v_world = torch.from_numpy(world_coords(v_idx, N_grid, x_range, y_range, z_range, coords)).to(dev)
    if tris.shape[0]:
        v_world, tris = keep_largest_cluster(v_world, tris)
    if decimate_cell is not None and tris.shape[0]:
        from .decimate import decimate
        v_world, tris, _ = decimate(v_world, tris, None, cell=decimate_cell, placement=decimate_placement)
    colors = None
    if tris.shape[0] and (use_vertex_normal or poses is not None):
        colors = fuse_vertex_colors(v_world, poses, images, focal, near, nerf_fine, embeddings, occ_threshold, N_samples, white_back,
                                    chunk, use_vertex_normal, tris, far, near_t, nerf_coarse, N_importance).cpu().numpy()
    return v_world.cpu().numpy(), tris.cpu().numpy(), colors

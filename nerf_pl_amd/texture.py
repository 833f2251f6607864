"""Textures for triangle meshes: a per-triangle atlas baked from the trained NeRF, shaded by MeshRenderer /
MixedRenderer, exported as OBJ + MTL + PNG.  Colour resolution no longer follows the triangle count: a decimated mesh keeps its
picture.

    v, t, _ = decimate(*mesh.extract_color_mesh(...)[:2], cell=2 * voxel)                  # bake AFTER decimating
    atlas = bake(v, t, 4, colours_from_views(poses, images, focal, near, nerf_fine, embeddings))
    bvh = MeshBVH(v, t, texture=atlas)                                                     # MeshRenderer(bvh, ...) shows it
    write_obj("lego.obj", v, t, atlas)                                                     # lego.obj, lego.mtl, lego.png

The parametrisation is trivial on purpose (include/nerfhip.h states it): one right-triangle patch of `res` texel intervals per leg
for every triangle, two patches per square block, closed-form addresses — no chart growing, no packing search, no sort, no
atomic.  Every texel is a sample of the colour field at a point of its triangle's plane; the points (ops.mesh_tex_points), the
atlas (ops.mesh_tex_atlas) and the lookup (ops.mesh_shade_tex) are HIP kernels with bit-equal host twins.  The export is for point
or bilinear sampling: a mip chain would bleed across blocks.  The atlas is tied to the triangle numbering.

    python -m nerf_pl_amd.texture --ckpt_path ckpts/lego.ckpt --N_grid 256 --sigma_threshold 20 --decimate 2 --res 4 --out lego.obj
"""
import math
import os

import numpy as np
import torch

from . import ops

__all__ = ["TextureAtlas", "default_width", "bake", "colours_from_views", "colours_along_normals", "write_obj", "read_obj"]


def default_width(n_triangles, res):
    """The width that makes the atlas about square: nb = ceil(sqrt(ceil(T / 2))) blocks per row, more until nb (res + 3) is a
    multiple of 4."""
    B = int(res) + 3
    nb = max(1, math.isqrt(max(0, (int(n_triangles) + 1) // 2 - 1)) + 1)
    while (nb * B) % 4:
        nb += 1
    return nb * B


class TextureAtlas:
    """The texture of one mesh: `res` (texel intervals per patch leg), `width`, `height`, `n_triangles`, and `data`, the
    (height, width, 3) uint8 atlas in the layout of include/nerfhip.h — a device tensor, or a numpy array (host use: uv, write_obj
    with the host encoder, the _host twins)."""

    def __init__(self, data, res, n_triangles):
        self.res, self.n_triangles = int(res), int(n_triangles)
        if data.ndim != 3 or data.shape[2] != 3 or (data.dtype != (torch.uint8 if torch.is_tensor(data) else np.uint8)):
            raise ValueError("TextureAtlas: data must be (height, width, 3) uint8, got %s %s" % (tuple(data.shape), data.dtype))
        self.height, self.width = int(data.shape[0]), int(data.shape[1])
        if self.height != ops.mesh_tex_height(self.n_triangles, self.res, self.width):
            raise ValueError("TextureAtlas: %d triangles at res %d and width %d make %d rows, got %d"
                             % (self.n_triangles, self.res, self.width, ops.mesh_tex_height(self.n_triangles, self.res, self.width),
                                self.height))
        self.data = data

    def uv(self, normalised=False):
        """(T, 3, 2) float32: the texel-centre coordinates, in pixels from the top left, of every triangle's corners — (x + 0.5,
        y + 0.5) of its lattice points (0, 0), (R, 0), (0, R).  Closed form, numpy only.  normalised: what write_obj writes,
        u = px / width and v = 1 - py / height formed in float64 and rounded to float32."""
        if normalised:
            px = self.uv().astype(np.float64)
            return np.stack([px[..., 0] / self.width, 1.0 - px[..., 1] / max(self.height, 1)], -1).astype(np.float32)
        R, B = self.res, self.res + 3
        t = np.arange(self.n_triangles, dtype=np.int64)
        k, odd = t >> 1, (t & 1).astype(bool)
        nb = self.width // B
        x0, y0 = (k % nb) * B, (k // nb) * B
        ij = np.array([(0, 0), (R, 0), (0, R)], np.int64)                                   # (3, 2)
        local = np.where(odd[:, None, None], B - 1 - ij[None], ij[None])                    # (T, 3, 2)
        return (np.stack([x0, y0], 1)[:, None, :] + local + 0.5).astype(np.float32)

    def numpy(self):
        """The atlas bytes on the host."""
        return self.data.cpu().numpy() if torch.is_tensor(self.data) else np.asarray(self.data)


def colours_from_views(poses, images, focal, near, nerf_fine, embeddings, occ_threshold=0.2, N_samples=64, white_back=False,
                       chunk=32 * 1024):
    """A colour callable for `bake`: mesh.fuse_vertex_colors in its default mode on the sample points — every training photograph
    (poses (n, 3, 4), images (n, H, W, 3) uint8 on the device) sampled where the point projects, weighted 0.1 / depth + (the
    occlusion ray's opacity < occ_threshold), truncated; exactly the rule documented there.  Normals are not used."""
    from .mesh import fuse_vertex_colors

    def colour(points, normals):
        return fuse_vertex_colors(points, poses, images, focal, near, nerf_fine, embeddings, occ_threshold, N_samples, white_back, chunk)
    return colour


def colours_along_normals(near, far, nerf_coarse, nerf_fine, embeddings, near_t=1.0, N_samples=64, N_importance=64, white_back=False,
                          chunk=32 * 1024):
    """A colour callable for `bake`: mesh.fuse_vertex_colors' use_vertex_normal rule with the sample's triangle normal n in place of
    the vertex normal — a ray from p - n near near_t along n (ops.normal_rays), rendered by [nerf_coarse, nerf_fine], the colour
    trunc(rgb_fine * 255) (ops.rgb_to_u8)."""
    from .mesh import _render

    @torch.no_grad()
    def colour(points, normals):
        rays = ops.normal_rays(points, normals, np.float32(near), np.float32(far), np.float32(near_t))
        rgb = _render([nerf_coarse, nerf_fine], embeddings, rays, N_samples, N_importance, chunk, white_back)["rgb_fine"]
        return ops.rgb_to_u8(rgb.contiguous())
    return colour


def bake(vertices, triangles, res, colour, width=None, chunk=1 << 22):
    """The atlas of a mesh: vertices (V, 3) fp32 and triangles (T, 3) int32 (device tensors, or numpy arrays copied to the current
    GPU) -> TextureAtlas on the device.  `colour` is any callable (points (k, 3) device fp32, normals (k, 3) device fp64) ->
    (k, 3) uint8 on the device — `colours_from_views`, `colours_along_normals`, or the caller's own.  It is called over whole
    triangles, about `chunk` samples at a time, so memory stays bounded (points and normals: 36 bytes per sample of a chunk;
    what stays is 3 bytes per sample and the atlas).  `width` defaults to `default_width`.  Bake after decimating: the atlas
    belongs to this triangle numbering."""
    from .meshcast import _to_device
    vertices = _to_device("vertices", vertices, torch.float32, None)
    triangles = _to_device("triangles", triangles, torch.int32, vertices.device)
    T, n_tex = triangles.shape[0], ops.mesh_tex_samples(res)
    width = default_width(T, res) if width is None else int(width)
    ops.mesh_tex_height(T, res, width)                                       # refuses a mesh that does not fit before any work
    colours = torch.empty((T * n_tex, 3), device=vertices.device, dtype=torch.uint8)
    step = max(1, int(chunk) // n_tex)
    for t0 in range(0, T, step):
        points, normals = ops.mesh_tex_points(vertices, triangles[t0:t0 + step], res)
        c = colour(points, normals)
        if not torch.is_tensor(c) or c.dtype != torch.uint8 or tuple(c.shape) != tuple(points.shape):
            raise ValueError("bake: the colour callable must return (k, 3) uint8 on the device for k points")
        colours[t0 * n_tex:t0 * n_tex + c.shape[0]] = c
    return TextureAtlas(ops.mesh_tex_atlas(colours, T, res, width), res, T)


def _host(a, dtype):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, dtype)


def write_obj(path, vertices, triangles, atlas, png_encoder="host"):
    """`path` = name.obj, beside it name.mtl and name.png.  The .obj: `mtllib`, `v` per vertex, three `vt` per triangle with
    u = px / width and v = 1 - py / height of `atlas.uv()` (OBJ's v runs upwards), `usemtl`, `f a/1 b/2 c/3` with 1-based indices;
    floats as %.9g, so a float32 survives the round trip.  The .mtl names the PNG in map_Kd.  The PNG is written by
    imageio_min.write_png ("host": atlas data may be numpy) or write_png_device ("gpu": atlas data on the device).  The texture is
    meant for point or bilinear sampling without mip levels."""
    if png_encoder not in ("host", "gpu"):
        raise ValueError("write_obj: png_encoder must be 'host' or 'gpu', got %r" % (png_encoder,))
    v, t = _host(vertices, np.float32).reshape(-1, 3), _host(triangles, np.int32).reshape(-1, 3)
    if len(t) != atlas.n_triangles:
        raise ValueError("write_obj: the atlas is of %d triangles, the mesh has %d" % (atlas.n_triangles, len(t)))
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    from . import imageio_min
    if png_encoder == "gpu":
        if not torch.is_tensor(atlas.data):
            raise ops.NerfHipError("write_obj(png_encoder='gpu'): the atlas must be on the device (no CPU fallback)")
        imageio_min.write_png_device([stem + ".png"], atlas.data.unsqueeze(0))
    else:
        imageio_min.write_png(stem + ".png", atlas.numpy())
    with open(stem + ".mtl", "w") as f:
        f.write("newmtl %s\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd %s.png\n" % (name, name))
    lines = ["mtllib %s.mtl" % name]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]
    lines += ["vt %.9g %.9g" % tuple(p) for p in atlas.uv(normalised=True).reshape(-1, 2).tolist()]
    lines.append("usemtl %s" % name)
    lines += ["f %d/%d %d/%d %d/%d" % (a + 1, 3 * i + 1, b + 1, 3 * i + 2, c + 1, 3 * i + 3) for i, (a, b, c) in enumerate(t.tolist())]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_obj(path, res=None, device=None):
    """A file of `write_obj` -> (vertices (V, 3) float32, triangles (T, 3) int32, TextureAtlas, uv (T, 3, 2) float32 as the file
    has them: `atlas.uv(normalised=True)`).  The patch resolution is not in the file: it is `res`, or else recovered from the first
    triangle's corners (its leg is `res` texels long).  Without `device` the PNG is decoded on the host (imageio_min.read_png: the
    host encoder's files, whose scanlines are unfiltered) and the atlas data is numpy; with `device` the scanline filters are
    reversed on that GPU (ops.decode_png_batch: the GPU encoder's files too) and the atlas data stays there."""
    from . import imageio_min
    v, vt, f, mtl = [], [], [], None
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([np.float32(x) for x in w[1:4]])
            elif w[0] == "vt":
                vt.append([np.float32(x) for x in w[1:3]])
            elif w[0] == "f":
                f.append([[int(x) for x in c.split("/")[:2]] for c in w[1:4]])
            elif w[0] == "mtllib":
                mtl = w[1]
    if mtl is None:
        raise ValueError("read_obj: %s names no material library" % path)
    png = None
    with open(os.path.join(os.path.dirname(path), mtl)) as fh:
        for line in fh:
            w = line.split()
            if w and w[0] == "map_Kd":
                png = w[1]
    if png is None:
        raise ValueError("read_obj: %s names no texture (map_Kd)" % mtl)
    png = os.path.join(os.path.dirname(path), png)
    if device is None:
        try:
            data = imageio_min.read_png(png)
        except NotImplementedError:
            raise ValueError("read_obj: %s has filtered scanlines (write_obj's GPU encoder): pass device= to decode it there" % png)
    else:
        w, h, ch, raw = imageio_min.png_inflate(png)
        if ch != 3:
            raise ValueError("read_obj: %s has %d channels, an atlas has 3" % (png, ch))
        rows = torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(1, -1).to(device)
        data = ops.decode_png_batch(rows, h, w, ch)[0].contiguous()
    f = np.array(f, np.int64).reshape(-1, 3, 2)
    T = len(f)
    if T and not np.array_equal(f[:, :, 1].ravel(), np.arange(1, 3 * T + 1)):
        raise ValueError("read_obj: only files of write_obj are read (three vt per triangle, in order)")
    vertices = np.array(v, np.float32).reshape(-1, 3)
    triangles = (f[:, :, 0] - 1).astype(np.int32)
    if res is None:
        if not T:
            raise ValueError("read_obj: an empty mesh does not tell its res")
        res = int(round(abs(float(vt[1][0]) - float(vt[0][0])) * data.shape[1]))
    return vertices, triangles, TextureAtlas(data, res, T), np.array(vt, np.float32).reshape(-1, 3, 2)


def main(argv=None):
    import argparse
    from .mesh import extract_color_mesh
    from .models import NeRF
    from .models.nerf import Embedding
    from .volume import load_ckpt
    ap = argparse.ArgumentParser(description="A trained NeRF -> mesh -> optional decimation -> texture bake -> name.obj / .mtl / .png")
    ap.add_argument("--ckpt_path", required=True)
    ap.add_argument("--out", required=True, help="the .obj file to write; the .mtl and .png go beside it")
    ap.add_argument("--N_grid", type=int, default=256)
    ap.add_argument("--sigma_threshold", type=float, default=20.0)
    for ax in "xyz":
        ap.add_argument("--%s_range" % ax, nargs=2, type=float, default=[-1.2, 1.2])
    ap.add_argument("--decimate", type=float, default=None, help="cluster the mesh into cells of this many voxels before baking")
    ap.add_argument("--placement", default="quadric", choices=sorted(ops.DECIMATE_PLACEMENTS))
    ap.add_argument("--res", type=int, default=4, help="texel intervals per triangle leg")
    ap.add_argument("--near", type=float, default=2.0)
    ap.add_argument("--far", type=float, default=6.0)
    ap.add_argument("--root_dir", default=None, help="a blender scene: colour from its training photographs (default: rays along the "
                    "triangle normals through the NeRF)")
    ap.add_argument("--img_wh", nargs=2, type=int, default=[800, 800])
    ap.add_argument("--white_back", action="store_true")
    ap.add_argument("--png_encoder", default="gpu", choices=["host", "gpu"])
    a = ap.parse_args(argv)
    coarse, fine = NeRF(), NeRF()
    load_ckpt(coarse, a.ckpt_path, model_name="nerf_coarse")
    load_ckpt(fine, a.ckpt_path, model_name="nerf_fine")
    coarse.cuda().eval(), fine.cuda().eval()
    embeddings = [Embedding(3, 10), Embedding(3, 4)]
    ranges = tuple(a.x_range), tuple(a.y_range), tuple(a.z_range)
    cell = None if a.decimate is None else a.decimate * (a.x_range[1] - a.x_range[0]) / a.N_grid
    v, t, _ = extract_color_mesh(fine, embeddings, a.N_grid, *ranges, a.sigma_threshold, decimate_cell=cell,
                                 decimate_placement=a.placement)
    if a.root_dir:
        from .datasets.blender import BlenderDataset
        ds = BlenderDataset(a.root_dir, split="train", img_wh=tuple(a.img_wh))
        n = len(ds.poses)
        images = (ds.all_rgbs.reshape(n, a.img_wh[1], a.img_wh[0], 3) * 255).round().to(torch.uint8).cuda()
        colour = colours_from_views(np.asarray(ds.poses, np.float32), images, ds.focal, a.near, fine, embeddings, white_back=a.white_back)
    else:
        colour = colours_along_normals(a.near, a.far, coarse, fine, embeddings, white_back=a.white_back)
    atlas = bake(v, t, a.res, colour)
    write_obj(a.out, v, t, atlas, png_encoder=a.png_encoder)
    print("%s: %d vertices, %d triangles, texture %d x %d at res %d (%d samples)"
          % (a.out, len(v), len(t), atlas.width, atlas.height, atlas.res, len(t) * ops.mesh_tex_samples(a.res)))


if __name__ == "__main__":
    main()

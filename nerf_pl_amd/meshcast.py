"""Ray casting against a triangle mesh: the consumer of mesh.extract_color_mesh's mesh, and the reference's third
deliverable, "mixed reality" — a virtual object inside a NeRF render, z-ordered by NeRF's depth.

    bvh = MeshBVH.from_ply("lego.ply")                      # or MeshBVH(*mesh.extract_color_mesh(...)), or device tensors
    out = inference.evaluate(dataset, MeshRenderer(bvh, white_back=True))                  # the mesh gets a PSNR
    mixed = MixedRenderer(GraphRenderer(...), MeshBVH.from_ply("teapot.ply"), white_back=True)

Opt-in, and beside everything else: nothing of training, rendering or extraction changes.  The hierarchy's build, the cast, the
shading and the compositing are HIP kernels (csrc/meshcast.hip); every renderer here obeys the contract of the others:
rays (n, 8) -> {'rgb_fine', 'depth_fine', 'opacity_fine'}.  The mesh is in world space (no NDC rays), has vertex colours, a texture
(texture.py: a per-triangle atlas) or neither, and is static (a moved mesh is built again).

    python -m nerf_pl_amd.meshcast --ply lego.ply --dataset_name blender --root_dir data/nerf_synthetic/lego --split test \\
        --img_wh 400 400 --out results/mesh --gif lego_mesh.gif                 # or --obj lego.obj, a file of texture.write_obj
"""
import numpy as np
import torch

from . import ops
from ._lib import NerfHipError

__all__ = ["MeshBVH", "MeshRenderer", "MixedRenderer"]


_NUMPY = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}


def _to_device(what, a, dtype, device):
    if a is None:
        return None
    if torch.is_tensor(a):
        if not a.is_cuda:
            raise NerfHipError("nerf_pl_amd runs on MI355X only: %s must be a device tensor or a numpy array (no CPU fallback)" % what)
        return a.to(dtype).contiguous()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(a, _NUMPY[dtype])).to(dev)


class MeshBVH:
    """A triangle mesh on the device with its hierarchy of boxes (include/nerfhip.h states the format): `vertices` (V, 3) fp32,
    `triangles` (T, 3) int32, `colors` (V, 3) uint8 or None, and `tris`, `boxes`, `order` of ops.mesh_bvh_build.  The arguments
    are device tensors, or the numpy arrays mesh.extract_color_mesh and mesh.read_ply return (copied to `device`, the current GPU
    unless given).  A triangle with an index outside [0, V) or a non-finite coordinate stays in `triangles` and is never hit;
    `n_bad` counts them.  `texture` is a texture.TextureAtlas of exactly these triangles (its data is copied to the device if it
    is numpy): `shade` then reads it, through `filter` "bilinear" or "nearest", instead of the vertex colours."""

    def __init__(self, vertices, triangles, colors=None, device=None, texture=None, filter="bilinear"):
        self.vertices = _to_device("vertices", vertices, torch.float32, device)
        self.triangles = _to_device("triangles", triangles, torch.int32, device)
        self.colors = _to_device("colors", colors, torch.uint8, device)
        if self.colors is not None and tuple(self.colors.shape) != tuple(self.vertices.shape):
            raise ValueError("MeshBVH: colors must be (V, 3) like vertices, got %s" % (tuple(self.colors.shape),))
        if filter not in ops.TEX_FILTERS:
            raise ValueError("MeshBVH: filter must be 'nearest' or 'bilinear', got %r" % (filter,))
        self.texture, self.filter = None, filter
        if texture is not None:
            if texture.n_triangles != self.triangles.shape[0]:
                raise ValueError("MeshBVH: the texture is of %d triangles, the mesh has %d (an atlas belongs to one triangle numbering)"
                                 % (texture.n_triangles, self.triangles.shape[0]))
            from .texture import TextureAtlas
            self.texture = TextureAtlas(_to_device("texture", texture.data, torch.uint8, self.vertices.device), texture.res,
                                        texture.n_triangles)
        self.tris, self.boxes, self.order, self._n_bad = ops.mesh_bvh_build(self.vertices, self.triangles)

    @classmethod
    def from_ply(cls, path, device=None):
        """A PLY file written by mesh.write_ply."""
        from .mesh import read_ply
        return cls(*read_ply(path), device=device)

    @classmethod
    def from_obj(cls, path, device=None, filter="bilinear", res=None):
        """An OBJ file written by texture.write_obj, with its texture."""
        from .texture import read_obj
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        vertices, triangles, atlas, _ = read_obj(path, res=res, device=dev)
        return cls(vertices, triangles, device=device, texture=atlas, filter=filter)

    @property
    def n_bad(self):
        """Bad triangles of the mesh (one host read)."""
        return int(self._n_bad.item())

    def decimated(self, cell, placement="mean"):
        """A new MeshBVH of this mesh clustered into cells of edge `cell` (decimate.py), colours included — and WITHOUT the
        texture: an atlas is tied to the triangle numbering, which decimation changes.  Bake (texture.bake) after decimating."""
        from .decimate import decimate
        return MeshBVH(*decimate(self.vertices, self.triangles, self.colors, cell=cell, placement=placement))

    def cast(self, rays):
        """rays (n, 8) on the device -> (tri (n,) int32, -1 for a miss; t (n,); b1 (n,); b2 (n,)): ops.mesh_cast."""
        return ops.mesh_cast(rays, self.tris, self.boxes)

    def shade(self, rays, tri, b1, b2, ambient=1.0, background=0.0):
        if self.texture is not None:
            return ops.mesh_shade_tex(rays, tri, b1, b2, self.vertices, self.triangles, self.texture.data, self.texture.res, self.filter,
                                      ambient, background)
        return ops.mesh_shade(rays, tri, b1, b2, self.vertices, self.triangles, self.colors, ambient, background)


class MeshRenderer:
    """A callable rays (n, 8) -> {'rgb_fine' (n, 3), 'depth_fine' (n,), 'opacity_fine' (n,)} that casts `bvh`: the vertex colours
    blended over the hit triangle (or the texture of a textured `bvh` at the hit) times ambient + (1 - ambient) |n . d|, depth =
    the hit's t, opacity 1; a miss is the background (1.0 with white_back, else 0.0), depth 0, opacity 0.  Usable as
    `inference.evaluate(dataset, MeshRenderer(...))` and inside `occupancy.CulledRenderer`.  ambient = 1 shows the fused colours as they are, which is what a PSNR wants."""

    def __init__(self, bvh, white_back, ambient=1.0):
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError("ambient must be in [0, 1], got %r" % (ambient,))
        self.bvh = bvh
        self.white_back = bool(white_back)
        self.ambient = float(ambient)

    @torch.no_grad()
    def layer(self, rays):
        """(tri, t, rgb) of the mesh alone: what MixedRenderer composes"""
        tri, t, b1, b2 = self.bvh.cast(rays)
        return tri, t, self.bvh.shade(rays, tri, b1, b2, self.ambient, 1.0 if self.white_back else 0.0)

    @torch.no_grad()
    def __call__(self, rays):
        tri, t, rgb = self.layer(rays)
        return {"rgb_fine": rgb, "depth_fine": t, "opacity_fine": (tri >= 0).to(torch.float32)}


class MixedRenderer:
    """`renderer` (any callable rays (n, 8) -> dict with 'rgb_fine', 'depth_fine', 'opacity_fine': a `GraphRenderer`, a
    `BakedRenderer`, a `CulledRenderer`) with `mesh` (a MeshBVH, or a MeshRenderer for its ambient term) put into its scene:
    returns the three keys composed, plus 'mesh_mask' (n,) uint8.

    mode "ztest" is the depth test of the reference's Unity demo: the inner render is made as it is, and the mesh pixel replaces
    it where the mesh is hit nearer than s = depth / opacity (+inf where opacity < tau).  A hard switch per pixel: a mesh behind
    a half-transparent part of the scene is hidden by it or not at all.

    mode "clip" renders the scene only up to the mesh — far = min(far, t) on the hit rays, without a background — and lets the
    mesh, or the background on a miss, fill the transmittance that is left: the scene in front of the mesh attenuates it as it
    should.  The inner renderer must not add a white background itself (one whose `white_back` is true is refused), and
    `white_back` here says what a ray that hits nothing ends on.  WARNING, as for CulledRenderer's `tighten`: the
    reference's compositing gives the last sample of a ray an unbounded thickness, so moving `far` changes a pixel wherever the
    density at the cut is above zero — a mesh inside the scene's solid parts is drawn as if the solid ended there."""

    def __init__(self, renderer, mesh, white_back, mode="ztest", tau=0.5):
        if mode not in ops.MIXED_MODES:
            raise ValueError("mode must be 'ztest' or 'clip', got %r" % (mode,))
        if not float(tau) > 0.0:
            raise ValueError("tau must be > 0, got %r" % (tau,))
        if mode == "clip" and getattr(renderer, "white_back", False):
            raise ValueError("MixedRenderer(mode='clip'): the inner renderer adds a white background; build it with white_back=False")
        self.renderer = renderer
        self.white_back = bool(white_back)
        self.mesh = mesh if isinstance(mesh, MeshRenderer) else MeshRenderer(mesh, white_back)
        self.mode = mode
        self.tau = float(tau)

    @torch.no_grad()
    def __call__(self, rays):
        tri, t, rgb_m = self.mesh.layer(rays)
        if self.mode == "clip":
            inner_rays = rays.clone()
            inner_rays[:, 7] = torch.where(tri >= 0, torch.minimum(rays[:, 7], t), rays[:, 7])
        else:
            inner_rays = rays
        inner = self.renderer(inner_rays)
        rgb, depth, opacity, mask = ops.mixed_compose(self.mode, inner["rgb_fine"], inner["depth_fine"], inner["opacity_fine"], tri, t,
                                                      rgb_m, self.tau, 1.0 if self.white_back else 0.0)
        return {"rgb_fine": rgb, "depth_fine": depth, "opacity_fine": opacity, "mesh_mask": mask}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Render the poses of a dataset split from a PLY mesh (no network involved)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ply", help="the mesh (python -m nerf_pl_amd.mesh, or any file of mesh.write_ply)")
    src.add_argument("--obj", help="a textured mesh (python -m nerf_pl_amd.texture, or any file of texture.write_obj)")
    ap.add_argument("--filter", default="bilinear", choices=["nearest", "bilinear"], help="how --obj's texture is sampled")
    ap.add_argument("--dataset_name", default="blender", choices=["blender", "llff"])
    ap.add_argument("--root_dir", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--img_wh", nargs=2, type=int, default=[800, 800])
    ap.add_argument("--ambient", type=float, default=1.0, help="1: the vertex colours as they are; below 1: shaded by |n . d|")
    ap.add_argument("--out", default=None, help="directory for the PNG frames")
    ap.add_argument("--gif", default=None, help="path of an animated GIF of the frames")
    a = ap.parse_args(argv)
    from .inference import evaluate
    if a.dataset_name == "blender":
        from .datasets.blender import BlenderDataset
        dataset = BlenderDataset(a.root_dir, split=a.split, img_wh=tuple(a.img_wh))
    else:
        from .datasets.llff import LLFFDataset
        dataset = LLFFDataset(a.root_dir, split=a.split, img_wh=tuple(a.img_wh))
    bvh = MeshBVH.from_ply(a.ply) if a.ply else MeshBVH.from_obj(a.obj, filter=a.filter)
    white = getattr(dataset, "white_back", a.dataset_name == "blender")
    out = evaluate(dataset, MeshRenderer(bvh, white_back=white, ambient=a.ambient), dir_name=a.out, gif_path=a.gif)
    print("%d frames from %s (%d triangles, %d of them bad, %d boxes)" % (len(out["images"]), a.ply or a.obj, bvh.triangles.shape[0], bvh.n_bad,
                                                                          bvh.boxes.shape[0]))
    if out["mean_psnr"] is not None:
        print("mean PSNR %.2f dB, mean SSIM %.4f against the split's images" % (out["mean_psnr"], out["mean_ssim"]))


if __name__ == "__main__":
    main()

"""Shadows for mixed renders: a virtual object put into a rendered scene is lit by a light in that scene, darkens
the scene behind it and is darkened by the scene — the showpiece the reference's README ends with.

    light = Light(direction=(1, 0, 1), radius=0.05, samples=16)           # or Light(position=(3, 0, 6))
    lit = LitMixedRenderer(BakedRenderer(vol, white_back=True), MeshBVH.from_ply("teapot.ply"), light, white_back=True,
                           scene_occluder=BakedRenderer(vol, white_back=False))
    out = inference.evaluate(dataset, lit)

Opt-in, and beside everything else: `MixedRenderer` and every kernel under it stay as they are.  The secondary rays — formed from
the render's depth, cast for any hit against the mesh's hierarchy, and turned into a factor on the pixel — are HIP kernels
(csrc/shadow.hip); the scene's own occlusion along a shadow row is any renderer's 'opacity_fine' on that row, as the reference
itself takes it in extract_color_mesh.py.

    python -m nerf_pl_amd.lighting --ply teapot.ply --vol lego.vol 512 -1.2 1.2 -1.2 1.2 -1.2 1.2 --light_dir 1 0 1 --samples 16 \\
        --radius 0.05 --dataset_name blender --root_dir data/nerf_synthetic/lego --split test --img_wh 400 400 --gif lit.gif
"""
import math

import torch

from . import ops
from .meshcast import MeshBVH, MeshRenderer, MixedRenderer

__all__ = ["Light", "LitMixedRenderer"]


class Light:
    """One white light: `direction` — the direction TOWARDS a light at infinity, of any non-zero length — or `position` of a point
    light, exactly one of the two.  `radius` > 0 makes it a square of that half-width facing each pixel (for a directional light
    in units of the unit direction: the tangent of its angular half-width) sampled `samples` times per pixel; `rotate` shifts the
    sample sequence per pixel, which trades the banding of a shared sequence for noise."""

    def __init__(self, direction=None, position=None, radius=0.0, samples=1, rotate=True):
        if (direction is None) == (position is None):
            raise ValueError("Light: give exactly one of direction and position")
        self.kind = "directional" if position is None else "point"
        vec = tuple(float(v) for v in (direction if position is None else position))
        if len(vec) != 3 or not all(math.isfinite(v) for v in vec):
            raise ValueError("Light: %s must be three finite numbers, got %r" % ("direction" if position is None else "position", vec))
        if self.kind == "directional" and not any(vec):
            raise ValueError("Light: the direction must not be zero")
        self.vector = vec
        self.radius = float(radius)
        if not (self.radius >= 0.0 and math.isfinite(self.radius)):
            raise ValueError("Light: radius must be finite and >= 0, got %r" % (radius,))
        self.samples = ops._samples_arg("Light", samples)
        self.rotate = bool(rotate)


def _extent(boxes):
    """(lo, hi) of a (k, 2, 3) stack of boxes, or None when there is none with finite ends"""
    boxes = [b for b in boxes if b is not None and all(math.isfinite(v) for v in b[0] + b[1]) and all(l <= h for l, h in zip(*b))]
    if not boxes:
        return None
    return tuple(min(b[0][a] for b in boxes) for a in range(3)), tuple(max(b[1][a] for b in boxes) for a in range(3))


def _diagonal(box):
    return math.sqrt(sum((h - l) ** 2 for l, h in zip(*box)))


def _mesh_box(bvh):
    """the root's box of the hierarchy (one host read), or None for a mesh without a good triangle"""
    if bvh.boxes.shape[0] == 0:
        return None
    root = [float(v) for v in bvh.boxes[-1].cpu()]
    return tuple(root[:3]), tuple(root[3:])


def _volume_box(renderer):
    """the box of a renderer that marches a volume (a BakedRenderer), or None"""
    ranges = getattr(getattr(renderer, "volume", None), "ranges", None)
    if ranges is None:
        return None
    return tuple(float(r[0]) for r in ranges), tuple(float(r[1]) for r in ranges)


class LitMixedRenderer:
    """`MixedRenderer(renderer, mesh, white_back, "ztest", tau)` with `light` applied: returns its dict with 'rgb_fine' lit, plus
    'shadow' (n,) fp32, the visibility V that was applied (1: fully lit).

    Per call: the mixed render (the mesh unshaded, ambient = 1); s = depth / opacity where opacity >= tau, else +inf (a mesh
    pixel has opacity 1 and depth t, so this is the surface of either layer); `ops.shadow_rays` from that surface towards the
    light's samples; `ops.mesh_occluded` on those rows; with `scene_occluder` — any renderer of the rays -> dict contract, meant
    to be a `BakedRenderer(volume, white_back=False)` — the scene's transmittance 1 - opacity_fine along the rows of the mesh's
    pixels; `ops.light_compose`.  A mesh pixel becomes rgb (ambient + (1 - ambient) max(n . l, 0) V), V the mean over the samples
    of (not occluded) x transmittance; a scene pixel rgb (1 - strength (1 - V)), V the mean of (not occluded by the mesh): the
    scene's own shading and self-shadowing are in its radiance already.  ambient = 1 and strength = 0 give `MixedRenderer`'s
    pixels bit for bit.

    `bias` (world units) is where a shadow row starts, so that a surface does not shadow itself: by default 1e-3 of the mesh's
    box diagonal — far above the fp32 error of the surface point (1e-6 of its coordinates), far below the object.  A NeRF depth is
    noisier than that: raise `bias` when the ground under the object shows acne, and know that a bias of the object's size lets
    light leak through it.  `reach` is the far end of a directional light's rows: by default twice the diagonal of the box
    around the mesh and the volume of `renderer` / `scene_occluder` (a row from any point of that box has left it by then), or
    1000 mesh diagonals when no volume is known.  mode "clip" of MixedRenderer is refused: its pixels blend mesh and scene colour
    and cannot be lit apart.  `mask_dtype=torch.float32` returns 'mesh_mask' as fp32, which `occupancy.CulledRenderer` needs to
    scatter it."""

    def __init__(self, renderer, mesh, light, white_back, tau=0.5, ambient=0.3, strength=0.7, bias=None, reach=None, scene_occluder=None,
                 mode="ztest", mask_dtype=torch.uint8):
        if mode != "ztest":
            raise ValueError("LitMixedRenderer: mode %r is not supported: only 'ztest' pixels belong to one layer and can be lit ('clip' "
                             "blends mesh and scene colour)" % (mode,))
        if not isinstance(light, Light):
            raise ValueError("LitMixedRenderer: light must be a Light, got %r" % (light,))
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError("ambient must be in [0, 1], got %r" % (ambient,))
        if not 0.0 <= float(strength) <= 1.0:
            raise ValueError("strength must be in [0, 1], got %r" % (strength,))
        bvh = mesh.bvh if isinstance(mesh, MeshRenderer) else mesh
        if not isinstance(bvh, MeshBVH):
            raise ValueError("LitMixedRenderer: mesh must be a MeshBVH, got %r" % (mesh,))
        self.bvh = bvh
        self.mixed = MixedRenderer(renderer, MeshRenderer(bvh, white_back, ambient=1.0), white_back, "ztest", tau)
        self.light = light
        self.white_back = bool(white_back)
        self.ambient, self.strength = float(ambient), float(strength)
        self.scene_occluder = scene_occluder
        self.mask_dtype = mask_dtype
        mesh_box = _mesh_box(bvh) if bias is None or reach is None else None
        mesh_box = _extent([mesh_box])
        mesh_diag = (_diagonal(mesh_box) if mesh_box else 0.0) or 1.0
        if bias is None:
            bias = 1e-3 * mesh_diag
        if reach is None:
            scene = _extent([_volume_box(renderer), _volume_box(scene_occluder)])
            reach = 2.0 * _diagonal(_extent([mesh_box, scene])) if scene else 1000.0 * mesh_diag
        self.bias, self.reach = float(bias), float(reach)
        if not (self.bias > 0.0 and math.isfinite(self.bias)):
            raise ValueError("bias must be finite and > 0, got %r" % (bias,))
        if not (self.reach > 0.0 and math.isfinite(self.reach)):
            raise ValueError("reach must be finite and > 0, got %r" % (reach,))

    @torch.no_grad()
    def __call__(self, rays):
        m, light, bvh = self.mixed, self.light, self.bvh
        # MixedRenderer's ztest call, keeping the hit triangles for the normals
        tri, t, rgb_m = m.mesh.layer(rays)
        inner = m.renderer(rays)
        rgb, depth, opacity, mask = ops.mixed_compose("ztest", inner["rgb_fine"], inner["depth_fine"], inner["opacity_fine"], tri, t, rgb_m,
                                                      m.tau, 1.0 if m.white_back else 0.0)
        n, K = rays.shape[0], light.samples
        on_mesh = mask != 0
        s = torch.where(opacity >= m.tau, depth / opacity, torch.full_like(depth, float("inf")))
        rows, cosine = ops.shadow_rays(rays, s, light.kind, light.vector, self.bias, self.reach, K, light.radius, light.rotate,
                                       torch.where(on_mesh, tri, torch.full_like(tri, -1)), bvh.vertices, bvh.triangles)
        hit = ops.mesh_occluded(rows, bvh.tris, bvh.boxes)
        trans = None
        if self.scene_occluder is not None:
            mesh_rows = torch.where(on_mesh.view(n, 1, 1), rows.view(n, K, 8), torch.zeros_like(rows).view(n, K, 8)).view(n * K, 8)
            trans = 1.0 - self.scene_occluder(mesh_rows)["opacity_fine"]
        lit, shadow = ops.light_compose(rgb, mask, cosine, hit, trans, self.ambient, self.strength)
        return {"rgb_fine": lit, "depth_fine": depth, "opacity_fine": opacity, "mesh_mask": mask.to(self.mask_dtype), "shadow": shadow}


class _Background:
    """the scene of a mesh alone: nothing in front of the background"""

    def __init__(self, white_back):
        self.white_back = bool(white_back)

    def __call__(self, rays):
        n = rays.shape[0]
        zero = torch.zeros(n, device=rays.device, dtype=torch.float32)
        return {"rgb_fine": torch.full((n, 3), 1.0 if self.white_back else 0.0, device=rays.device), "depth_fine": zero, "opacity_fine": zero}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Render the poses of a dataset split from a mesh lit by one light, over a background or inside "
                                             "a .vol file's scene, which it shadows and which shadows it (no network involved)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ply", help="the mesh (python -m nerf_pl_amd.mesh, or any file of mesh.write_ply)")
    src.add_argument("--obj", help="a textured mesh (python -m nerf_pl_amd.texture, or any file of texture.write_obj)")
    ap.add_argument("--filter", default="bilinear", choices=["nearest", "bilinear"], help="how --obj's texture is sampled")
    ap.add_argument("--vol", nargs=8, metavar=("FILE", "N", "X0", "X1", "Y0", "Y1", "Z0", "Z1"), default=None,
                    help="a .vol file (python -m nerf_pl_amd.volume), its lattice size and axis ranges: the scene, and its occluder")
    ap.add_argument("--dataset_name", default="blender", choices=["blender", "llff"])
    ap.add_argument("--root_dir", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--img_wh", nargs=2, type=int, default=[800, 800])
    where = ap.add_mutually_exclusive_group(required=True)
    where.add_argument("--light_dir", nargs=3, type=float, help="the direction towards a directional light")
    where.add_argument("--light_pos", nargs=3, type=float, help="the position of a point light")
    ap.add_argument("--samples", type=int, default=1, help="shadow rays per pixel (1 to 64)")
    ap.add_argument("--radius", type=float, default=0.0, help="half-width of the square light; 0: hard shadows")
    ap.add_argument("--ambient", type=float, default=0.3, help="what an unlit part of the mesh keeps")
    ap.add_argument("--strength", type=float, default=0.7, help="how much the mesh's shadow takes from the scene")
    ap.add_argument("--bias", type=float, default=None, help="where a shadow ray starts, in world units (default: 1e-3 mesh diagonals)")
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
    scene, occluder = _Background(white), None
    if a.vol:
        from .baked import BakedRenderer, BakedVolume
        x0, x1, y0, y1, z0, z1 = (float(v) for v in a.vol[2:])
        vol = BakedVolume.from_file(a.vol[0], int(a.vol[1]), ((x0, x1), (y0, y1), (z0, z1)))
        scene, occluder = BakedRenderer(vol, white_back=white), BakedRenderer(vol, white_back=False)
    light = Light(direction=a.light_dir, position=a.light_pos, radius=a.radius, samples=a.samples)
    lit = LitMixedRenderer(scene, bvh, light, white, ambient=a.ambient, strength=a.strength, bias=a.bias, scene_occluder=occluder)
    out = evaluate(dataset, lit, dir_name=a.out, gif_path=a.gif)
    print("%d frames from %s (%d triangles) %s, %s light, %d sample(s), bias %.3g, reach %.3g"
          % (len(out["images"]), a.ply or a.obj, bvh.triangles.shape[0], "in " + a.vol[0] if a.vol else "alone", light.kind, light.samples,
             lit.bias, lit.reach))
    if out["mean_psnr"] is not None:
        print("mean PSNR %.2f dB, mean SSIM %.4f against the split's images" % (out["mean_psnr"], out["mean_ssim"]))


if __name__ == "__main__":
    main()

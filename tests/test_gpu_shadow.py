"""GPU: the shadow kernels (csrc/shadow.hip) and nerf_pl_amd.lighting on the fixtures of tests/mesh_ref.py and
tests/test_shadow_host.py.  The device's any-hit query, shadow rows and compose equal their host twins bit for bit (the same
libm-free routines of csrc/shadow_core.h), so everything tests/test_shadow_host.py establishes for the twins holds for the device by
construction; the analytic shadow is checked on the device's own output as well.  Every launch here is bounded by the traversal's
own loop bound (at most n_nodes visits per ray for any hierarchy), as the mesh caster's tests are."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402
import test_shadow_host as H  # noqa: E402
from test_meshcast_host import built  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 257, 1000)


def to_dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def cpu(tensors):
    return [None if x is None else x.cpu().numpy() for x in tensors]


def same_bits(a, b):
    return H.same_bits(a, b)


# ------------------------------------------------------------------------------------------------------- device == host twin
@pytest.mark.parametrize("name", sorted(R.meshes()))
def test_device_occluded_is_the_host_twin(dev, name):
    from nerf_pl_amd import ops
    _, _, (tris, boxes, _, _) = built(name)
    d_tris, d_boxes = to_dev(dev, tris, boxes)
    sets = dict(R.ray_sets())
    sets.update({"pinhole%d" % n: R.pinhole()[:n] for n in SIZES})
    sets["zero_rows"] = np.zeros((257, 8), np.float32)
    for set_name, rays in sets.items():
        got = ops.mesh_occluded(to_dev(dev, rays)[0], d_tris, d_boxes).cpu().numpy()
        want = ops.mesh_occluded_host(rays, tris, boxes)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, set_name, np.flatnonzero(got != want)[:8])
        if set_name == "zero_rows":
            assert not got.any()


def test_device_rows_are_the_host_twin(dev):
    from nerf_pl_amd import ops
    for name in ("ico2", "flawed"):
        rays, s, tri, v, t = H.primary(name)
        d_v, d_t = to_dev(dev, v, t)
        for n in SIZES:
            d_rays, d_s, d_tri = to_dev(dev, rays[:n], s[:n], tri[:n])
            for (kind, light), (K, radius, rotate) in zip(H.LIGHTS, ((1, 0.0, 1), (4, 0.05, 1), (4, 0.3, 0), (1, 0.05, 0), (4, 0.0, 0), (4, 0.05, 1))):
                got = cpu(ops.shadow_rays(d_rays, d_s, kind, light, H.BIAS, H.REACH, K, radius, rotate, d_tri, d_v, d_t))
                want = ops.shadow_rays_host(rays[:n], s[:n], kind, light, H.BIAS, H.REACH, K, radius, rotate, tri[:n], v, t)
                assert same_bits(got, want), (name, n, kind, light, K, radius, rotate)
                # the null arguments: no mesh layer, no cosine
                got = cpu(ops.shadow_rays(d_rays, d_s, kind, light, H.BIAS, H.REACH, K, radius, rotate))
                assert same_bits([got[0]], [want[0]]) and (got[1] == 1).all()
                rows, none = ops.shadow_rays(d_rays, d_s, kind, light, H.BIAS, H.REACH, K, radius, rotate, d_tri, d_v, d_t, cosine=False)
                assert none is None and same_bits(cpu([rows]), [want[0]])
    # every pixel without a surface: every row zero
    rays = R.pinhole()[:257]
    d_rays, d_s = to_dev(dev, rays, np.full(257, np.inf, np.float32))
    rows = ops.shadow_rays(d_rays, d_s, "point", (3.0, 0.0, 6.0), H.BIAS, H.REACH, 4, 0.05, 1)[0]
    assert rows.shape == (257 * 4, 8) and not bool(rows.view(torch.int32).any())
    rows, cosine = ops.shadow_rays(d_rays[:0], d_s[:0], "point", (3.0, 0.0, 6.0), H.BIAS, H.REACH, 4)
    assert rows.shape == (0, 8) and cosine.shape == (0,)


def test_device_compose_is_the_host_twin(dev):
    from nerf_pl_amd import ops
    for n in SIZES:
        for K in (1, 4):
            inputs = H.compose_inputs(n, K)
            on_dev = to_dev(dev, *inputs)
            for with_trans, ambient, strength in ((True, 0.3, 0.7), (False, 0.3, 0.7), (True, 1.0, 0.0), (True, 0.0, 1.0)):
                a = list(on_dev[:4]) + [on_dev[4] if with_trans else None]
                h = list(inputs[:4]) + [inputs[4] if with_trans else None]
                got = cpu(ops.light_compose(*a, ambient, strength))
                want = ops.light_compose_host(*h, ambient, strength)
                assert same_bits(got, want), (n, K, with_trans, ambient, strength)
                if ambient == 1.0:
                    assert same_bits([got[0]], [inputs[0]])
                out, none = ops.light_compose(*a, ambient, strength, visibility=False)
                assert none is None and same_bits(cpu([out]), [want[0]])


def test_nothing_is_written_past_the_outputs(dev):
    """n = 257 (one full block and one item in a second), K = 4: rows, cosine, hit, rgb_out and visibility of n + pad rows keep the
    pattern behind row n"""
    from nerf_pl_amd import _lib, ops
    lib = _lib.load()
    n, K, pad = 257, 4, 64
    rays, s, tri, v, t = H.primary()
    _, _, (tris, boxes, _, _) = built("ico2")
    d_rays, d_s, d_tri, d_v, d_t, d_tris, d_boxes = to_dev(dev, rays[:n], s[:n], tri[:n], v, t, tris, boxes)
    pattern = -1515870811                                   # 0xa5a5a5a5

    def fresh(rows, tail, dtype):
        return torch.full((rows + pad,) + tail, pattern, device=dev, dtype=torch.int32).view(dtype)

    def untouched(o, rows):
        return bool((o[rows:].contiguous().view(torch.int32) == pattern).all())
    with torch.cuda.device(dev):
        rows, cosine = fresh(n * K, (8,), torch.float32), fresh(n, (), torch.float32)
        _lib.check(lib.nerfhip_shadow_rays(_lib.ptr(d_rays), _lib.ptr(d_s), n, _lib.ptr(d_tri), _lib.ptr(d_v), len(v), _lib.ptr(d_t), len(t), 1,
                                           3.0, 0.0, 6.0, H.BIAS, H.REACH, K, 0.05, 1, _lib.ptr(rows), _lib.ptr(cosine), _lib.stream_ptr()),
                   "nerfhip_shadow_rays")
        want = ops.shadow_rays(d_rays, d_s, "point", (3.0, 0.0, 6.0), H.BIAS, H.REACH, K, 0.05, 1, d_tri, d_v, d_t)
        assert torch.equal(rows[:n * K].view(torch.int32), want[0].view(torch.int32)) and untouched(rows, n * K)
        assert torch.equal(cosine[:n].view(torch.int32), want[1].view(torch.int32)) and untouched(cosine, n)
        hit = torch.full((n * K + pad,), 0xa5, device=dev, dtype=torch.uint8)
        _lib.check(lib.nerfhip_mesh_occluded(_lib.ptr(want[0]), n * K, _lib.ptr(d_tris), _lib.ptr(d_boxes), len(tris), _lib.ptr(hit),
                                             _lib.stream_ptr()), "nerfhip_mesh_occluded")
        assert torch.equal(hit[:n * K], ops.mesh_occluded(want[0], d_tris, d_boxes)) and bool((hit[n * K:] == 0xa5).all())
        rgb, mask, cos_in, _, trans = to_dev(dev, *H.compose_inputs(n, K))
        out, vis = fresh(n, (3,), torch.float32), fresh(n, (), torch.float32)
        _lib.check(lib.nerfhip_light_compose(n, _lib.ptr(rgb), _lib.ptr(mask), _lib.ptr(cos_in), _lib.ptr(hit), _lib.ptr(trans), K, 0.3, 0.7,
                                             _lib.ptr(out), _lib.ptr(vis), _lib.stream_ptr()), "nerfhip_light_compose")
        want = ops.light_compose(rgb, mask, cos_in, hit[:n * K], trans, 0.3, 0.7)
        assert torch.equal(out[:n].view(torch.int32), want[0].view(torch.int32)) and untouched(out, n)
        assert torch.equal(vis[:n].view(torch.int32), want[1].view(torch.int32)) and untouched(vis, n)


def test_analytic_shadow_on_the_device(dev):
    from nerf_pl_amd import ops

    def occluded(rows, tris, boxes):
        return ops.mesh_occluded(*to_dev(dev, rows, tris, boxes)).cpu().numpy()

    def rows_of(rays, s, kind, light, bias, reach, K, radius, rotate):
        return cpu(ops.shadow_rays(*to_dev(dev, rays, s), kind, light, bias, reach, K, radius, rotate))

    def compose(rgb, mask, cosine, hit, trans, ambient, strength):
        return cpu(ops.light_compose(*to_dev(dev, rgb, mask, cosine, hit, trans), ambient, strength))
    H.analytic_check(occluded, rows_of, compose)


# ------------------------------------------------------------------------------------------------------------- the public layer
N_VOL, RANGES = 32, ((-2.0, 4.0), (-2.0, 2.0), (-2.0, 2.0))       # long in +x: rows towards a low light there end in the slab
SLAB_TOP = -0.5
_SMALL = {}


def small_scene(dev):
    """(volume: an opaque slab z in [-1, -0.5] of a 32^3 lattice over RANGES; mesh: the level-2 icosphere of radius 0.5 at
    (0, 0, 0.3), above it; rays: the 32 x 32 pinhole image from above)"""
    from nerf_pl_amd.baked import BakedVolume
    from nerf_pl_amd.meshcast import MeshBVH
    if not _SMALL:
        z = np.linspace(-2.0, 2.0, N_VOL)
        rgba = np.zeros((N_VOL, N_VOL, N_VOL, 4), np.uint8)
        rgba[:, :, (z >= -1.0) & (z <= SLAB_TOP)] = (200, 180, 160, 255)
        vol = BakedVolume.from_dense(torch.from_numpy(rgba).to(dev), RANGES)
        v, t = R.icosphere(2)
        v = (v * np.float32(0.5) + np.array([0.0, 0.0, 0.3], np.float32)).astype(np.float32)
        colors = np.random.default_rng(9).integers(64, 256, (len(v), 3)).astype(np.uint8)
        _SMALL["s"] = (vol, MeshBVH(v, t, colors, device=dev), torch.from_numpy(R.pinhole(near=0.5, far=8.0)).to(dev))
    return _SMALL["s"]


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("white", [False, True])
def test_lit_renderer_is_the_six_steps_by_hand(dev, white):
    from nerf_pl_amd import ops
    from nerf_pl_amd.baked import BakedRenderer
    from nerf_pl_amd.lighting import Light, LitMixedRenderer
    from nerf_pl_amd.meshcast import MeshRenderer, MixedRenderer
    vol, bvh, rays = small_scene(dev)
    inner, occluder = BakedRenderer(vol, white_back=white), BakedRenderer(vol, white_back=False)
    n = rays.shape[0]
    for light, use_occluder in ((Light(direction=(1, 0, 2)), True), (Light(direction=(1, 0, 2), radius=0.1, samples=4), False),
                                (Light(position=(1.5, 0.5, 3.0), radius=0.2, samples=4, rotate=False), True)):
        lit = LitMixedRenderer(inner, bvh, light, white, tau=0.5, ambient=0.25, strength=0.6, scene_occluder=occluder if use_occluder else None)
        out = lit(rays)
        assert list(out) == ["rgb_fine", "depth_fine", "opacity_fine", "mesh_mask", "shadow"]
        assert lit.bias == pytest.approx(1e-3 * float(np.sqrt(3.0)), rel=0.05)              # the sphere's box has edge 1, nearly
        assert lit.reach == pytest.approx(2.0 * float(np.sqrt(36.0 + 16.0 + 16.0)), rel=1e-6)          # the volume's box holds the mesh's
        mixed = MixedRenderer(inner, MeshRenderer(bvh, white, ambient=1.0), white, "ztest", 0.5)(rays)            # 1
        tri = bvh.cast(rays)[0]
        mask = mixed["mesh_mask"]
        s = torch.where(mixed["opacity_fine"] >= 0.5, mixed["depth_fine"] / mixed["opacity_fine"],                 # 2
                        torch.full_like(mixed["depth_fine"], float("inf")))
        rows, cosine = ops.shadow_rays(rays, s, light.kind, light.vector, lit.bias, lit.reach, light.samples, light.radius, light.rotate,   # 3
                                       torch.where(mask != 0, tri, torch.full_like(tri, -1)), bvh.vertices, bvh.triangles)
        hit = ops.mesh_occluded(rows, bvh.tris, bvh.boxes)                                                          # 4
        trans = None
        if use_occluder:                                                                                            # 5
            keep = (mask != 0).repeat_interleave(light.samples)
            trans = 1.0 - occluder(rows * keep[:, None].to(torch.float32))["opacity_fine"]
        rgb, V = ops.light_compose(mixed["rgb_fine"], mask, cosine, hit, trans, 0.25, 0.6)                          # 6
        for key, want in (("rgb_fine", rgb), ("depth_fine", mixed["depth_fine"]), ("opacity_fine", mixed["opacity_fine"]),
                          ("mesh_mask", mask), ("shadow", V)):
            assert bits_equal(out[key], want), (key, light.kind, light.samples)
        assert 50 < int(mask.sum()) < n - 200 and bool((s[mask == 0] < float("inf")).sum() > 200)
        # ambient = 1 and strength = 0: MixedRenderer's pixels, bit for bit
        plain = LitMixedRenderer(inner, bvh, light, white, ambient=1.0, strength=0.0, scene_occluder=occluder if use_occluder else None)(rays)
        for key in ("rgb_fine", "depth_fine", "opacity_fine", "mesh_mask"):
            assert bits_equal(plain[key], mixed[key]), key
        assert bits_equal(plain["shadow"], out["shadow"])


def test_the_mesh_darkens_the_slab_and_the_slab_darkens_the_mesh(dev):
    from nerf_pl_amd.baked import BakedRenderer
    from nerf_pl_amd.lighting import Light, LitMixedRenderer
    vol, bvh, rays = small_scene(dev)
    inner, occluder = BakedRenderer(vol, white_back=True), BakedRenderer(vol, white_back=False)
    alone = inner(rays)["rgb_fine"]
    out = LitMixedRenderer(inner, bvh, Light(direction=(1, 0, 1)), True, scene_occluder=occluder)(rays)
    scene = out["mesh_mask"] == 0
    shadowed = scene & (out["shadow"] < 1)
    # the sphere's shadow falls 0.8 towards -x on the slab's top, most of it beside the sphere's own image
    assert int(shadowed.sum()) > 20 and bool((out["shadow"][scene] == 1).sum() > 400)
    assert bool((out["rgb_fine"][shadowed] < alone[shadowed]).all())                 # darker under the sphere
    assert bool((out["rgb_fine"][scene] <= alone[scene]).all())                      # and no pixel of the slab brighter
    assert bits_equal(out["rgb_fine"][scene & ~shadowed], alone[scene & ~shadowed])
    # the light below the slab, on the +x side: the part of the sphere that faces it sees it only through the slab
    low = Light(direction=(1, 0, -0.5))
    base = LitMixedRenderer(inner, bvh, low, True, ambient=1.0, strength=0.0)(rays)["rgb_fine"]       # the mesh's own colours
    lit_side = None
    for use_occluder in (False, True):
        o = LitMixedRenderer(inner, bvh, low, True, ambient=0.2, scene_occluder=occluder if use_occluder else None)(rays)
        mesh = o["mesh_mask"] != 0
        if lit_side is None:                                                         # without the occluder: lit where it faces the light
            lit_side = mesh & (o["rgb_fine"].sum(1) > 0.2 * 1.001 * base.sum(1)) & (o["shadow"] == 1)
            assert int(lit_side.sum()) > 10
        else:
            # 1 - opacity of a march through 0.5 of opaque slab: opacity is a rounded sum of weights that add up to 1
            assert bool((o["shadow"][lit_side] <= 4 * 2.0 ** -24).all())
            assert bool((o["shadow"][mesh] <= 4 * 2.0 ** -24).all())                 # nothing of the sphere sees this light


class _OneImage:
    img_wh = (32, 32)
    white_back = True

    def __init__(self, rays):
        g = torch.Generator().manual_seed(3)
        self.items = [{"rays": rays, "rgbs": torch.rand(rays.shape[0], 3, generator=g)}]

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.items[i]


def test_lit_renderer_in_evaluate_and_culled(dev):
    from nerf_pl_amd import inference
    from nerf_pl_amd.baked import BakedRenderer
    from nerf_pl_amd.lighting import Light, LitMixedRenderer
    from nerf_pl_amd.occupancy import CulledRenderer, OccupancyGrid
    vol, bvh, rays = small_scene(dev)
    inner, occluder = BakedRenderer(vol, white_back=True), BakedRenderer(vol, white_back=False)
    lit = LitMixedRenderer(inner, bvh, Light(direction=(1, 0, 2)), True, scene_occluder=occluder, mask_dtype=torch.float32)
    out = inference.evaluate(_OneImage(rays), lit)
    assert len(out["images"]) == 1 and out["images"][0].shape == (32, 32, 3) and np.isfinite(out["mean_psnr"])
    want = lit(rays)
    image = (want["rgb_fine"].clamp(0, 1) * 255).to(torch.uint8).cpu().numpy().reshape(32, 32, 3)
    assert np.abs(out["images"][0].astype(int) - image.astype(int)).max() <= 1
    # culled to the half x < 0.4 of the volume: the rays that are rendered keep every bit
    gx, g = torch.linspace(RANGES[0][0], RANGES[0][1], 17, device=dev), torch.linspace(-2.0, 2.0, 17, device=dev)
    y, x, z = torch.meshgrid(g, gx, g, indexing="ij")
    grid = OccupancyGrid.from_sigma((x < 0.4).to(torch.float32).contiguous(), *RANGES, dilate=0)
    culled = CulledRenderer(lit, grid, True, tighten="none")
    got = culled(rays)
    kept = grid.cull(rays)[0] != 0
    assert 0 < culled.stats["rendered"] < culled.stats["rays"] and list(got) == list(want)
    for key in want:
        assert bits_equal(got[key][kept], want[key][kept]), key

"""GPU: the mesh ray caster's kernels (csrc/meshcast.hip) and nerf_pl_amd.meshcast on the fixtures of tests/mesh_ref.py.  The
device build is the host build and numpy's; the device cast, shade and compose equal their host twins bit for bit (the same
libm-free routines of csrc/mesh_core.h), so the float64 caps of tests/test_meshcast_host.py hold for the device by construction, and
are checked on the device's own output as well.  Batching and culling leave every bit where it was."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baked_ref as B  # noqa: E402
import mesh_ref as R  # noqa: E402
import test_meshcast_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

_BVH = {}


def bvh(dev, name):
    """(vertices, triangles, MeshBVH on the device), made once"""
    from nerf_pl_amd.meshcast import MeshBVH
    if name not in _BVH:
        v, t = R.meshes()[name]
        _BVH[name] = (v, t, MeshBVH(v, t, device=dev))
    return _BVH[name]


def cpu(tensors):
    return [x.cpu().numpy() for x in tensors]


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------- format
@pytest.mark.parametrize("name", sorted(R.meshes()))
def test_device_build_is_the_host_build(dev, name):
    v, t, b = bvh(dev, name)
    _, _, (tris, boxes, order, n_bad) = H.built(name)
    want_order, want_boxes, want_bad = R.build(v, t)
    assert b.n_bad == int(n_bad[0]) == want_bad
    got_tris, got_boxes, got_order = cpu([b.tris, b.boxes, b.order])
    assert np.array_equal(got_order, order) and np.array_equal(got_order, want_order)
    assert same_bits([got_tris, got_boxes], [tris, boxes])
    assert np.array_equal(got_boxes, want_boxes)


def test_empty_mesh_on_the_device(dev):
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer
    b = MeshBVH(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), device=dev)
    assert b.boxes.shape == (0, 6) and b.tris.shape == (0, 12) and b.n_bad == 0
    out = MeshRenderer(b, white_back=True)(torch.from_numpy(R.pinhole()).to(dev))
    assert (out["rgb_fine"] == 1).all() and not out["depth_fine"].any() and not out["opacity_fine"].any()


# ------------------------------------------------------------------------------------------------------------------------ cast
@pytest.mark.parametrize("name", sorted(R.meshes()))
def test_device_cast_is_the_host_twin(dev, name):
    from nerf_pl_amd import ops
    v, t, b = bvh(dev, name)
    _, _, (tris, boxes, _, _) = H.built(name)
    bad = np.flatnonzero(R.bad_triangles(v, t))
    for set_name, rays in R.ray_sets().items():
        got = cpu(b.cast(torch.from_numpy(rays).to(dev)))
        want = ops.mesh_cast_host(rays, tris, boxes)
        assert same_bits(got, want), (name, set_name, np.flatnonzero(got[0] != want[0])[:8])
        assert not np.isin(got[0], bad).any()
        if set_name == "pinhole":                            # a ray list in pieces: no bit changes
            half = len(rays) // 2 + 1
            parts = [cpu(b.cast(torch.from_numpy(rays[s]).to(dev))) for s in (slice(0, half), slice(half, None))]
            assert same_bits(got, [np.concatenate(p) for p in zip(*parts)])
        if name != "identical" and set_name in R.JUDGED:
            H.compare64(got, H.ref64(name, set_name), "device %s %s" % (name, set_name))


def test_watertight_on_the_device(dev):
    _, _, b = bvh(dev, "ico2")
    tri = b.cast(torch.from_numpy(R.watertight_rays(2)).to(dev))[0]
    assert tri.shape == (642,) and bool((tri >= 0).all())


def test_marching_cubes_sphere(dev):
    """the mesh extraction's own output as input: a sphere of radius 0.8 on a 17^3 lattice over [-1.2, 1.2]^3"""
    from nerf_pl_amd import mesh, ops
    from nerf_pl_amd.meshcast import MeshBVH
    g = torch.linspace(-1.2, 1.2, 17, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    verts, tris = mesh.marching_cubes((0.8 - torch.sqrt(x * x + y * y + z * z)).contiguous(), 0.0)
    verts = (verts * (2.4 / 16) - 1.2).to(torch.float32)
    b = MeshBVH(verts, tris)
    v, t = verts.cpu().numpy(), tris.cpu().numpy()
    assert len(t) > 500 and b.n_bad == 0
    host = ops.mesh_bvh_build_host(v, t)
    order, boxes, _ = R.build(v, t)
    assert same_bits(cpu([b.tris, b.boxes, b.order]), host[:3]) and np.array_equal(host[2], order) and np.array_equal(host[1], boxes)
    for rays in (R.pinhole(), R.inside_rays(), R.axis_rays(True)):
        got = cpu(b.cast(torch.from_numpy(rays).to(dev)))
        assert same_bits(got, ops.mesh_cast_host(rays, host[0], host[1]))
        assert same_bits(got, ops.mesh_cast_host(rays, host[0], None, brute=True))
    inside = cpu(b.cast(torch.from_numpy(R.inside_rays()).to(dev)))
    assert (inside[0] >= 0).all()                            # a closed surface: no ray from inside gets out
    d = R.inside_rays()[:, 3:6].astype(np.float64)
    # the radius, give or take the origins' offsets (0.087) and the lattice's chord error
    assert np.abs(inside[1] * np.linalg.norm(d, axis=1) - 0.8).max() < 0.1


# ------------------------------------------------------------------------------------------------------------ shade and compose
def test_device_shade_is_the_host_twin(dev):
    from nerf_pl_amd import ops
    for what, rays, tri, b1, b2, v, t, colors, ambient, bg in H.shade_cases():
        args = [torch.from_numpy(a).to(dev) for a in (rays, tri, b1, b2, v, t)]
        got = ops.mesh_shade(*args, None if colors is None else torch.from_numpy(colors).to(dev), ambient, bg).cpu().numpy()
        want = ops.mesh_shade_host(rays, tri, b1, b2, v, t, colors, ambient, bg)
        assert same_bits([got], [want]), what
        e = float(np.abs(got - R.shade64(rays, tri, b1, b2, v, t, colors, ambient, bg)).max())
        print("device shade %s: %.3g (cap %.3g)" % (what, e, H.CAP_SHADE))
        assert e <= H.CAP_SHADE


def test_device_compose_is_the_host_twin(dev):
    from nerf_pl_amd import ops
    inputs = H.compose_inputs()
    on_dev = [torch.from_numpy(a).to(dev) for a in inputs]
    for mode, tau, bg in (("ztest", 0.5, 0.0), ("ztest", 0.25, 1.0), ("clip", 0.5, 0.0), ("clip", 0.5, 1.0)):
        got = cpu(ops.mixed_compose(mode, *on_dev, tau, bg))
        want = ops.mixed_compose_host(mode, *inputs, tau, bg)
        assert got[3].dtype == np.uint8 and same_bits(got, want), mode
        ref = R.compose64(mode, *inputs, tau, bg)
        assert np.array_equal(got[3], ref[3])
        for g, w in zip(got[:3], ref[:3]):
            assert float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max()) <= H.CAP_COMPOSE
    assert got[3][:6].tolist() == [1, 1, 1, 1, 1, 0]           # clip: the mask is "hit"
    assert cpu(ops.mixed_compose("ztest", *on_dev, 0.5, 0.0))[3][:6].tolist() == [0, 1, 1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------------------- the public layer
def colours(n):
    return np.random.default_rng(9).integers(0, 256, (n, 3)).astype(np.uint8)


def test_mesh_renderer_keys_and_values(dev):
    from nerf_pl_amd import ops
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer
    v, t = R.icosphere(2)
    c = colours(len(v))
    b = MeshBVH(v, t, c, device=dev)
    rays = R.pinhole()
    for white, ambient in ((True, 1.0), (False, 0.3)):
        out = MeshRenderer(b, white, ambient)(torch.from_numpy(rays).to(dev))
        assert list(out) == ["rgb_fine", "depth_fine", "opacity_fine"]
        tri, tt, b1, b2 = ops.mesh_cast_host(rays, *H.built("ico2")[2][:2])
        rgb = ops.mesh_shade_host(rays, tri, b1, b2, v, t, c, ambient, float(white))
        assert same_bits(cpu(out.values()), [rgb, tt, (tri >= 0).astype(np.float32)])
        assert set(np.unique(out["opacity_fine"].cpu().numpy())) == {0.0, 1.0}


def test_mesh_bvh_from_ply(dev, tmp_path):
    from nerf_pl_amd import mesh
    from nerf_pl_amd.meshcast import MeshBVH
    v, t = R.icosphere(1)
    c = colours(len(v))
    path = str(tmp_path / "ico.ply")
    mesh.write_ply(path, v, t, c)
    a, b = MeshBVH.from_ply(path, device=dev), MeshBVH(v, t, c, device=dev)
    for x, y in ((a.vertices, b.vertices), (a.triangles, b.triangles), (a.colors, b.colors), (a.tris, b.tris), (a.boxes, b.boxes)):
        assert torch.equal(x, y)


class _TwoImages:
    img_wh = (16, 12)
    white_back = True

    def __init__(self, dev):
        from nerf_pl_amd import rays
        g = torch.Generator().manual_seed(7)
        self.items = []
        for z in (5.0, 4.5):
            c2w = torch.tensor([[1.0, 0, 0, 0.25], [0, 1, 0, 0.1], [0, 0, 1, z]], device=dev)
            self.items.append({"rays": rays.gen_rays(c2w, 12, 16, 30.0, 2.0, 6.0), "rgbs": torch.rand(16 * 12, 3, generator=g)})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_evaluate_takes_a_mesh_renderer(dev):
    from nerf_pl_amd import inference
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer
    v, t = R.icosphere(2)
    out = inference.evaluate(_TwoImages(dev), MeshRenderer(MeshBVH(v, t, colours(len(v)), device=dev), white_back=True))
    assert len(out["psnr"]) == len(out["ssim"]) == len(out["images"]) == 2
    assert np.isfinite(out["mean_psnr"]) and out["mean_psnr"] > 0
    for img in out["images"]:
        assert img.shape == (12, 16, 3) and img.dtype == np.uint8
        assert (img == 255).all(-1).any() and (img != 255).any()      # the white background and the sphere in front of it


@pytest.mark.parametrize("white", [True, False])
def test_culled_renderer_keeps_every_bit(dev, white):
    from nerf_pl_amd.meshcast import MeshRenderer
    from nerf_pl_amd.occupancy import CulledRenderer, OccupancyGrid
    _, _, b = bvh(dev, "ico3")
    g = torch.linspace(-1.2, 1.2, 17, device=dev)
    y, x, z = torch.meshgrid(g, g, g, indexing="ij")
    sigma = (torch.sqrt(x * x + y * y + z * z) <= 1.1).to(torch.float32).contiguous()      # the unit sphere lies inside
    grid = OccupancyGrid.from_sigma(sigma, (-1.2, 1.2), (-1.2, 1.2), (-1.2, 1.2), dilate=1)
    rays = torch.from_numpy(R.pinhole()).to(dev)
    inner = MeshRenderer(b, white, ambient=0.5)
    culled = CulledRenderer(inner, grid, white, tighten="none")
    want, got = inner(rays), culled(rays)
    assert 0 < culled.stats["rendered"] < culled.stats["rays"]
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k


@pytest.mark.parametrize("mode", ["ztest", "clip"])
def test_mixed_renderer_is_compose_by_hand(dev, mode):
    """a sphere behind the one occupied voxel of a 9^3 volume: hidden by it where it is opaque, seen through its thin rim and beside it"""
    from nerf_pl_amd import ops
    from nerf_pl_amd.baked import BakedRenderer, BakedVolume
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer, MixedRenderer
    N = 9
    vol = BakedVolume.from_dense(torch.from_numpy(B.volume("voxel", N)).to(dev), B.RANGES, cell=B.cell_of(N))
    v, t = R.icosphere(1)
    v = (v * np.float32(0.6) + np.array([0.5, 0.1, 0.3], np.float32)).astype(np.float32)
    c = colours(len(v))
    mesh = MeshBVH(v, t, c, device=dev)
    rays = R.pinhole(near=0.5, far=6.0)
    rays_dev = torch.from_numpy(rays).to(dev)
    for white in (False, True):
        inner = BakedRenderer(vol, white_back=white and mode == "ztest")
        mixed = MixedRenderer(inner, MeshRenderer(mesh, white, ambient=0.4), white, mode=mode, tau=0.5)
        out = mixed(rays_dev)
        assert list(out) == ["rgb_fine", "depth_fine", "opacity_fine", "mesh_mask"]
        # by hand, through the host twins
        host = ops.mesh_bvh_build_host(v, t)
        tri, tt, b1, b2 = ops.mesh_cast_host(rays, host[0], host[1])
        rgb_m = ops.mesh_shade_host(rays, tri, b1, b2, v, t, c, 0.4, float(white))
        inner_rays = rays.copy()
        if mode == "clip":
            inner_rays[:, 7] = np.where(tri >= 0, np.minimum(rays[:, 7], tt), rays[:, 7])
        n = inner(torch.from_numpy(inner_rays).to(dev))
        want = ops.mixed_compose_host(mode, *cpu([n["rgb_fine"], n["depth_fine"], n["opacity_fine"]]), tri, tt, rgb_m, 0.5, float(white))
        assert same_bits(cpu(out.values()), want), (mode, white)
        mask = want[3].astype(bool)
        assert mask.any() and (~mask & (tri >= 0)).any() if mode == "ztest" else np.array_equal(mask, tri >= 0)
        assert (n["opacity_fine"].cpu().numpy() > 0.5).any()
    if mode == "clip":
        with pytest.raises(ValueError):
            MixedRenderer(BakedRenderer(vol, white_back=True), mesh, True, mode="clip")


def test_cpu_tensors_raise(dev):
    from nerf_pl_amd._lib import NerfHipError
    _, _, b = bvh(dev, "ico0")
    with pytest.raises(NerfHipError):
        b.cast(torch.from_numpy(R.pinhole()))
    from nerf_pl_amd.meshcast import MeshRenderer
    with pytest.raises(NerfHipError):
        MeshRenderer(b, True)(torch.from_numpy(R.pinhole()))


# --------------------------------------------------------------------------------------------------- optional outputs left out
def test_null_optional_outputs_on_the_device(dev):
    """nerfhip_mesh_cast with t, b1 and b2 null and nerfhip_mixed_compose without a mask, on 257 rays (one full block and one ray
    in a second): what is supplied keeps the bits of the full call, and nothing is written past row n of any output."""
    from nerf_pl_amd import _lib, ops
    lib = _lib.load()
    n, pad = 257, 64
    _, _, b = bvh(dev, "soup5")
    assert b.tris.shape == (5, 12) and b.boxes.shape == (3, 6)
    rays = torch.from_numpy(H.null_output_rays(n)).to(dev)
    full = ops.mesh_cast(rays, b.tris, b.boxes)
    assert bool((full[0] >= 0).any()) and bool((full[0] < 0).any())

    pattern = -1515870811                                   # 0xa5a5a5a5

    def fresh(specs):
        """outputs of n + pad rows filled with the pattern"""
        return [torch.full((n + pad,) + tail, pattern, device=dev, dtype=torch.int32).view(dtype) for tail, dtype in specs]

    def untouched(outs):
        return all(bool((o[n:].view(torch.int32) == pattern).all()) for o in outs)

    with torch.cuda.device(dev):
        for nulls in H.CAST_NULLS:
            out = fresh([((), torch.int32), ((), torch.float32), ((), torch.float32), ((), torch.float32)])
            args = [None if k in nulls else out[k] for k in range(4)]
            _lib.check(lib.nerfhip_mesh_cast(_lib.ptr(rays), n, _lib.ptr(b.tris), _lib.ptr(b.boxes), 5, *[_lib.ptr(a) for a in args],
                                             _lib.stream_ptr()), "nerfhip_mesh_cast")
            assert same_bits(cpu([a[:n] for a in args if a is not None]), cpu([full[k] for k in range(4) if k not in nulls])), nulls
            assert untouched(out), nulls
        inputs = [torch.from_numpy(a).to(dev) for a in H.compose_inputs(n)]
        for mode in ("ztest", "clip"):
            want = ops.mixed_compose(mode, *inputs, tau=0.5, background=1.0)
            out = fresh([((3,), torch.float32), ((), torch.float32), ((), torch.float32)])
            _lib.check(lib.nerfhip_mixed_compose(ops.MIXED_MODES[mode], n, *[_lib.ptr(a) for a in inputs], 0.5, 1.0,
                                                 *[_lib.ptr(a) for a in out], None, _lib.stream_ptr()), "nerfhip_mixed_compose")
            assert same_bits(cpu([a[:n] for a in out]), cpu(want[:3])), mode
            assert untouched(out), mode

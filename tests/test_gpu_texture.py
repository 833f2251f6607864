"""GPU: the texture atlas' kernels (csrc/texture.hip) and nerf_pl_amd.texture on the fixtures of tests/mesh_ref.py.  The device
points, atlas and lookup equal their host twins bit for bit (the same routines of csrc/texture_core.h), so what
tests/test_texture_host.py shows for the twins holds for the device by construction; the renderers, the bake and the export are
checked on top of that."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as M  # noqa: E402
import test_texture_host as TH  # noqa: E402
import texture_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu


def up(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def same_bits(a, b):
    a, b = a.cpu().numpy() if torch.is_tensor(a) else a, b.cpu().numpy() if torch.is_tensor(b) else b
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def hits_of(name):
    """rays and host hits that exercise a mesh: the pinhole image and the rays from inside, plus the crafted rows of the host
    test's kind (tri = -1, tri >= T, b outside the triangle, NaN)"""
    T = len(M.meshes()[name][1])
    parts = [TH.cast(name, s)[2:] for s in ("pinhole", "inside")]
    rays, tri, b1, b2 = (np.concatenate(p) for p in zip(*parts))
    bs = np.array([(0, 0), (1, 0), (0, 1), (1, 1), (-0.25, 0.5), (7, 9), (np.nan, 0.5), (np.inf, -np.inf)], np.float32)
    numbers = np.array([-1, T, 0, T - 1, T // 2], np.int32)
    tri = np.concatenate([tri, np.repeat(numbers, len(bs))]).astype(np.int32)
    b1 = np.concatenate([b1, np.tile(bs[:, 0], len(numbers))])
    b2 = np.concatenate([b2, np.tile(bs[:, 1], len(numbers))])
    rays = np.concatenate([rays, np.tile(rays[:1], (len(numbers) * len(bs), 1))])
    return rays, tri, b1, b2


# ---------------------------------------------------------------------------------------------------------- device = host twin
@pytest.mark.parametrize("name", sorted(M.meshes()))
def test_device_is_the_host_twin(dev, name):
    from nerf_pl_amd import ops, texture
    v, t = M.meshes()[name]
    T = len(t)
    rays, tri, b1, b2 = hits_of(name)
    dv, dt, drays, dtri, db1, db2 = up(dev, v, t, rays, tri, b1, b2)
    for R in TH.RES:
        want_p, want_n = ops.mesh_tex_points_host(v, t, R)
        got_p, got_n = ops.mesh_tex_points(dv, dt, R)
        assert same_bits(got_p, want_p) and same_bits(got_n, want_n)
        only_p, none = ops.mesh_tex_points(dv, dt, R, normals=False)                         # null normals on the device
        assert none is None and same_bits(only_p, want_p)
        rng = np.random.default_rng(R)
        colors = rng.integers(0, 256, (T * X.n_tex(R), 3), dtype=np.uint8)
        for Wa in sorted({texture.default_width(T, R), TH.ceil4(3 * (R + 3) + 1)}):
            if X.height(T, R, Wa) > 16384:
                continue
            want_a = ops.mesh_tex_atlas_host(colors, T, R, Wa)
            got_a = ops.mesh_tex_atlas(up(dev, colors)[0], T, R, Wa)
            assert same_bits(got_a, want_a)
        for filt in ("bilinear", "nearest"):
            for ambient in (1.0, 0.3):
                want = ops.mesh_shade_tex_host(rays, tri, b1, b2, v, t, want_a, R, filt, ambient, 0.25)
                got = ops.mesh_shade_tex(drays, dtri, db1, db2, dv, dt, got_a, R, filt, ambient, 0.25)
                assert same_bits(got, want), (name, R, filt, ambient)


def test_large_soup(dev):
    """10^6 samples and 1.27 M texels: every multi-block path, a ragged last row of blocks, 4096 = 819 blocks and one column over"""
    from nerf_pl_amd import ops
    from nerf_pl_amd.meshcast import MeshBVH
    v, t = M.soup(100000)
    T, R, Wa = len(t), 2, 4096
    assert T * X.n_tex(R) == 10 ** 6 and X.height(T, R, Wa) == 310 and (T + 1) // 2 % (Wa // 5) != 0 and Wa % 5
    dv, dt = up(dev, v, t)
    want_p, want_n = ops.mesh_tex_points_host(v, t, R)
    got_p, got_n = ops.mesh_tex_points(dv, dt, R)
    assert same_bits(got_p, want_p) and same_bits(got_n, want_n)
    colors = np.random.default_rng(11).integers(0, 256, (10 ** 6, 3), dtype=np.uint8)
    dcolors = up(dev, colors)[0]
    want_a = ops.mesh_tex_atlas_host(colors, T, R, Wa)
    got_a = ops.mesh_tex_atlas(dcolors, T, R, Wa)
    assert got_a.shape == (310, 4096, 3) and same_bits(got_a, want_a)
    assert same_bits(ops.mesh_tex_atlas(dcolors, T, R, Wa), got_a)                           # two runs are byte-equal
    assert same_bits(ops.mesh_tex_points(dv, dt, R)[0], got_p)
    drays = up(dev, M.pinhole(wh=64, focal=60.0))[0]
    dtri, _, db1, db2 = MeshBVH(dv, dt).cast(drays)
    assert int((dtri >= 0).sum()) > 2000
    for filt in ("bilinear", "nearest"):
        got = ops.mesh_shade_tex(drays, dtri, db1, db2, dv, dt, got_a, R, filt, 0.5, 1.0)
        want = ops.mesh_shade_tex_host(*(x.cpu().numpy() for x in (drays, dtri, db1, db2)), v, t, want_a, R, filt, 0.5, 1.0)
        assert same_bits(got, want)
        assert same_bits(ops.mesh_shade_tex(drays, dtri, db1, db2, dv, dt, got_a, R, filt, 0.5, 1.0), got)


# ------------------------------------------------------------------------------------------------------------ renderer contract
def field_bytes(points, normals):
    """an analytic colour callable: the claim's field at the sample points, rounded to nearest (host arithmetic, device in and out)"""
    return torch.from_numpy(X.to_bytes(X.field(points.cpu().numpy()))).to(points.device)


def test_renderer_contract(dev):
    from nerf_pl_amd import ops, texture
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer, MixedRenderer
    claim = TH.claim()
    v, t = M.icosphere(2)
    atlas = texture.bake(v, t, 8, field_bytes)
    assert (atlas.res, atlas.n_triangles, atlas.width) == (8, 320, texture.default_width(320, 8)) and atlas.data.is_cuda
    bvh = MeshBVH(v, t, device=dev, texture=atlas)
    drays = up(dev, claim["rays"])[0]
    out = MeshRenderer(bvh, white_back=False)(drays)
    assert sorted(out) == ["depth_fine", "opacity_fine", "rgb_fine"]
    tri, depth, b1, b2 = bvh.cast(drays)
    assert same_bits(out["rgb_fine"], ops.mesh_shade_tex(drays, tri, b1, b2, bvh.vertices, bvh.triangles, atlas.data, 8))
    assert same_bits(out["depth_fine"], depth) and same_bits(out["opacity_fine"], (tri >= 0).to(torch.float32))
    assert same_bits(out["rgb_fine"], claim["rows"][("bilinear", 8)][0])                    # the CPU's picture, bit for bit
    nearest = MeshRenderer(MeshBVH(v, t, device=dev, texture=atlas, filter="nearest"), white_back=False)(drays)["rgb_fine"]
    assert same_bits(nearest, claim["rows"][("nearest", 8)][0])
    # a constant render far behind the mesh: the z-test passes the textured layer through where the mesh is hit
    n = drays.shape[0]

    def inner(rays):
        return {"rgb_fine": torch.full((n, 3), 0.2, device=dev), "depth_fine": torch.full((n,), 50.0, device=dev),
                "opacity_fine": torch.ones(n, device=dev)}
    mixed = MixedRenderer(inner, bvh, white_back=False, mode="ztest")(drays)
    hit = tri >= 0
    assert same_bits(mixed["rgb_fine"][hit], out["rgb_fine"][hit]) and bool((mixed["rgb_fine"][~hit] == 0.2).all())
    assert same_bits(mixed["mesh_mask"], hit.to(torch.uint8)) and same_bits(mixed["depth_fine"][hit], depth[hit])
    with pytest.raises(ValueError):
        MeshBVH(*M.icosphere(1), device=dev, texture=atlas)                                  # another mesh's atlas
    assert bvh.decimated(0.5).texture is None


# -------------------------------------------------------------------------------------------------------------------- bake glue
def _look_at(pos):
    pos = np.asarray(pos, np.float64)
    back = pos / np.linalg.norm(pos)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(back, right), back, pos], 1).astype(np.float32)       # (3, 4) camera-to-world


def holds(atlas, colours):
    """the atlas holds, at every stated address, the colour of that sample"""
    tx = X.texels(atlas.n_triangles, atlas.res, atlas.width).reshape(-1, 2)
    return np.array_equal(atlas.numpy()[tx[:, 1], tx[:, 0]], colours.cpu().numpy())


def test_bake_glue(dev):
    from nerf_pl_amd import mesh, ops, texture
    from nerf_pl_amd.models.nerf import Embedding, NeRF
    torch.manual_seed(3)
    coarse, fine = NeRF(), NeRF()                       # nn.Linear's default initialisation renders black: lift the density head
    with torch.no_grad():
        coarse.sigma.bias.add_(2.0), fine.sigma.bias.add_(2.0)
    coarse, fine = coarse.to(dev).eval(), fine.to(dev).eval()
    emb = [Embedding(3, 10), Embedding(3, 4)]
    v, t = M.icosphere(1)
    dv, dt = up(dev, v, t)
    points, normals = ops.mesh_tex_points(dv, dt, 2)
    assert points.shape == (800, 3)
    near, far = 0.5, 2.5
    along = texture.colours_along_normals(near, far, coarse, fine, emb, N_samples=32, N_importance=32)
    rays = ops.normal_rays(points, normals, np.float32(near), np.float32(far), np.float32(1.0))
    want = ops.rgb_to_u8(mesh._render([coarse, fine], emb, rays, 32, 32, 32 * 1024, False)["rgb_fine"].contiguous())
    whole = texture.bake(dv, dt, 2, along)
    assert len(torch.unique(want)) > 4 and holds(whole, want)
    assert same_bits(texture.bake(dv, dt, 2, along, chunk=256).data, whole.data)            # 25 triangles at a time: no byte changes
    # the training photographs with the occlusion ray
    W, H, focal = 32, 24, 30.0
    poses = np.stack([_look_at(p) for p in ([2.6, 0.9, 0.7], [-1.1, 2.4, -0.6])])
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    images = np.stack([np.stack([127.5 + 100 * np.sin(x / (5.0 + i + c) + c) * np.cos(y / (7.0 + c) - i) for c in range(3)], -1)
                       for i in range(2)]).round().astype(np.uint8)
    dimages = up(dev, images)[0]
    views = texture.colours_from_views(poses, dimages, focal, 1.0, fine, emb, N_samples=32)
    want = mesh.fuse_vertex_colors(points, poses, dimages, focal, 1.0, fine, emb, N_samples=32)
    whole = texture.bake(dv, dt, 2, views)
    assert len(torch.unique(want)) > 4 and holds(whole, want)
    assert same_bits(texture.bake(dv, dt, 2, views, chunk=256).data, whole.data)
    with pytest.raises(ValueError):
        texture.bake(dv, dt, 2, lambda p, n: p)                                             # not (k, 3) uint8


# ----------------------------------------------------------------------------------------------------------------------- export
def test_export_with_the_gpu_encoder(dev, tmp_path):
    from PIL import Image
    from nerf_pl_amd import texture
    from nerf_pl_amd.meshcast import MeshBVH
    v, t = M.icosphere(2)
    atlas = texture.bake(v, t, 4, field_bytes)
    path = str(tmp_path / "ball.obj")
    texture.write_obj(path, v, t, atlas, png_encoder="gpu")
    with Image.open(str(tmp_path / "ball.png")) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), atlas.numpy())
    v2, t2, atlas2, uv2 = texture.read_obj(path, device=dev)
    assert same_bits(v2, v) and same_bits(t2, t) and atlas2.data.is_cuda and same_bits(atlas2.data, atlas.data) and atlas2.res == 4
    assert same_bits(uv2, atlas.uv(normalised=True))
    rays = up(dev, M.pinhole())[0]
    a = MeshBVH.from_obj(path, device=dev)
    b = MeshBVH(v, t, device=dev, texture=atlas)
    tri, _, b1, b2 = b.cast(rays)
    assert same_bits(a.tris, b.tris) and same_bits(a.shade(rays, tri, b1, b2), b.shade(rays, tri, b1, b2)) and int((tri >= 0).sum()) > 250


# -------------------------------------------------------------------------------------------------------------------- no bleeding
@pytest.mark.parametrize("R", TH.RES)
def test_no_bleeding_on_the_device(dev, R):
    from nerf_pl_amd import texture
    from nerf_pl_amd.meshcast import MeshBVH
    v, t = M.icosphere(2)
    flat = TH.flat_colours(len(t))
    dflat = up(dev, flat)[0]
    n_tex = X.n_tex(R)
    atlas = texture.bake(v, t, R, lambda p, n: dflat.repeat_interleave(n_tex, 0))            # constant per triangle
    worst = 0.0
    for rays in (M.watertight_rays(2), M.pinhole()):
        drays = up(dev, rays)[0]
        for filt in ("bilinear", "nearest"):
            bvh = MeshBVH(v, t, device=dev, texture=atlas, filter=filt)
            tri, _, b1, b2 = bvh.cast(drays)
            hit = (tri >= 0).cpu().numpy()
            assert hit.sum() >= 250
            got = bvh.shade(drays, tri, b1, b2).cpu().numpy()[hit].astype(np.float64)
            worst = max(worst, float(np.abs(got - flat[tri.cpu().numpy()[hit]] / 255.0).max()))
    print("R = %d: flat colours off by %.3g on the device (bound %.3g)" % (R, worst, TH.TOL_FLAT))
    assert worst <= TH.TOL_FLAT

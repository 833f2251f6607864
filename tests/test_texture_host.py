"""CPU: the per-triangle texture atlas through its host twins (nerfhip_mesh_tex_points_host, nerfhip_mesh_tex_atlas_host,
nerfhip_mesh_shade_tex_host: the kernels' own routines, csrc/texture_core.h) against tests/texture_ref.py, on the fixtures of
tests/mesh_ref.py.  Fails on a library or a package without the texture entry points.

What is exact is compared exactly: the layout, the points (fp32 restated operation by operation), the OBJ round trip.  The
tolerances are the issue's, derived there from the number formats: normals 4 * 2^-53 per component (a handful of fp64 roundings),
the lookup 1e-6 against float64 (at most 12 fp32 roundings of values <= 1: 7.2e-7), flat colours 4 * 2^-24, a standard sampler
1e-5.  Every test prints the largest error it saw beside its bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as M  # noqa: E402
import texture_ref as X  # noqa: E402

E_BADARG, E_ALIGN = -1, -3
RES = (1, 3, 8)
TOL_NORMAL = 4 * 2.0 ** -53
TOL_LOOKUP = 1e-6
TOL_FLAT = 4 * 2.0 ** -24
TOL_SAMPLER = 1e-5


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def ceil4(x):
    return (x + 3) // 4 * 4


_CAST = {}


def cast(name, rays_name):
    """(vertices, triangles, rays, tri, b1, b2) of the host cast, made once"""
    from nerf_pl_amd import ops
    key = (name, rays_name)
    if key not in _CAST:
        v, t = M.meshes()[name]
        rays = M.watertight_rays(2) if rays_name == "watertight" else M.ray_sets()[rays_name]
        tris, boxes, _, _ = ops.mesh_bvh_build_host(v, t)
        tri, _, b1, b2 = ops.mesh_cast_host(rays, tris, boxes)
        _CAST[key] = (v, t, rays, tri, b1, b2)
    return _CAST[key]


def random_atlas(T, R, Wa, seed):
    """an atlas with seeded bytes in every sample, laid out by the restatement"""
    rng = np.random.default_rng(seed)
    return X.atlas_from(rng.integers(0, 256, (T * X.n_tex(R), 3), dtype=np.uint8), T, R, Wa)


# ---- 1. layout -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_layout(lib, R):
    from nerf_pl_amd import ops, texture
    B = R + 3
    for T in (0, 1, 2, 5, 37):
        # one block per row; several, the width a whole number of blocks; several with columns left over; the default
        for Wa in sorted({ceil4(B), 4 * B, ceil4(3 * B + 1), ceil4(5 * B + 2), texture.default_width(T, R)}):
            Ha = X.height(T, R, Wa)
            assert ops.mesh_tex_height(T, R, Wa) == Ha == lib.nerfhip_mesh_tex_height(T, R, Wa)
            tx = X.texels(T, R, Wa).reshape(-1, 2)
            assert len(np.unique(tx, axis=0)) == len(tx) == T * X.n_tex(R)                  # (t, m) -> texel is injective
            assert not len(tx) or (tx.min() >= 0 and tx[:, 0].max() < Wa and tx[:, 1].max() < Ha)
            kind, q = X.classify(T, R, Wa)
            # the two statements of the layout agree: every sample's texel is classified as that sample
            assert np.array_equal(q[tx[:, 1], tx[:, 0]], np.arange(len(tx)))
            assert ((kind == X.KIND_EVEN) | (kind == X.KIND_ODD)).sum() == len(tx)
            K = T * X.n_tex(R)
            code = np.arange(1, K + 1, dtype=np.int64)                                      # q + 1: no sample is all zero
            colors = np.stack([code & 255, (code >> 8) & 255, (code >> 16) & 255], 1).astype(np.uint8)
            want = X.atlas_from(colors, T, R, Wa)
            assert np.array_equal(ops.mesh_tex_atlas_host(colors, T, R, Wa), want)
            for sentinel in (0xA5, 0x5A):                                                   # every byte is overwritten
                got = ops._np16(np.full((Ha, Wa, 3), sentinel, np.uint8), np.uint8)
                assert lib.nerfhip_mesh_tex_atlas_host(colors.ctypes.data, T, R, Wa, Ha, got.ctypes.data) == 0
                assert T == 0 or np.array_equal(got, want)
    assert texture.default_width(37, R) % 4 == 0 and texture.default_width(37, R) // B >= 5      # ceil(sqrt(19)) = 5 blocks


def test_default_width_and_uv():
    from nerf_pl_amd import texture
    for R in (1, 2, 3, 8, 64):
        for T in (0, 1, 2, 3, 8, 9, 37, 320, 100000):
            Wa = texture.default_width(T, R)
            nb = Wa // (R + 3)
            assert Wa % 4 == 0 and Wa == nb * (R + 3) and nb * nb >= (T + 1) // 2
    for R, T, Wa in ((1, 5, 8), (3, 37, 28), (8, 37, 48)):
        atlas = texture.TextureAtlas(np.zeros((X.height(T, R, Wa), Wa, 3), np.uint8), R, T)
        assert np.array_equal(atlas.uv(), X.uv(T, R, Wa)) and atlas.uv().dtype == np.float32
    with pytest.raises(ValueError):
        texture.TextureAtlas(np.zeros((5, 8, 3), np.uint8), 1, 5)


# ---- 2. points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.meshes()))
def test_points(name):
    from nerf_pl_amd import ops
    v, t = M.meshes()[name]
    worst = 0.0
    for R in RES:
        want_p, want_n, bad = X.points32(v, t, R)
        got_p, got_n = ops.mesh_tex_points_host(v, t, R)
        assert got_p.dtype == np.float32 and got_n.dtype == np.float64 and got_p.shape == got_n.shape == (len(t) * X.n_tex(R), 3)
        assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
        worst = max(worst, float(np.abs(got_n - want_n).max()))
        if bad.any():
            sel = np.repeat(bad, X.n_tex(R))
            assert not got_p[sel].any() and np.array_equal(got_n[sel], np.tile([0.0, 0.0, 1.0], (sel.sum(), 1)))
        only_p, none = ops.mesh_tex_points_host(v, t, R, normals=False)                    # null normals
        assert none is None and np.array_equal(only_p.view(np.uint32), got_p.view(np.uint32))
    print("%s: normals off by %.3g (bound %.3g)" % (name, worst, TOL_NORMAL))
    assert worst <= TOL_NORMAL
    assert name != "flawed" or M.flawed()[2].sum() > 8


# ---- 3. lookup -----------------------------------------------------------------------------------------------------------------
LOOKUP_CASES = [("ico2", "watertight", 3), ("ico2", "pinhole", 8), ("ico1", "inside", 1), ("soup257", "axis", 3), ("plate", "grid", 8),
                ("plate", "pinhole", 1), ("flawed", "pinhole", 3), ("soup33", "nonfinite", 8), ("ico3", "window_near", 1),
                ("soup1000", "window_far", 3)]


@pytest.mark.parametrize("name,rays_name,R", LOOKUP_CASES)
def test_lookup_against_float64(name, rays_name, R):
    from nerf_pl_amd import ops, texture
    v, t, rays, tri, b1, b2 = cast(name, rays_name)
    Wa = texture.default_width(len(t), R)
    atlas = random_atlas(len(t), R, Wa, 7 + R)
    assert (tri >= 0).any() or rays_name == "nonfinite"
    worst = 0.0
    for filt in ("bilinear", "nearest"):
        for ambient in (1.0, 0.3):
            got = ops.mesh_shade_tex_host(rays, tri, b1, b2, v, t, atlas, R, filt, ambient, 0.25)
            want = X.lookup64(rays, tri, b1, b2, v, t, atlas, R, filt, ambient, 0.25)
            assert np.array_equal(got[tri < 0], np.full(((tri < 0).sum(), 3), 0.25, np.float32))
            worst = max(worst, float(np.abs(got - want).max()))
    print("%s / %s at R = %d: %d hits, lookup off by %.3g (bound %.3g)" % (name, rays_name, R, (tri >= 0).sum(), worst, TOL_LOOKUP))
    assert worst <= TOL_LOOKUP


@pytest.mark.parametrize("R", RES)
def test_lookup_crafted_rows(R):
    """rows no cast produces: tri = -1, tri >= T, a triangle with a vertex index outside [0, V), b1 and b2 in {0, 1}, both 1,
    negative, far outside, NaN — the last ones outside any real hit; texture_ref._fetch asserts that every read of the
    restatement stays inside the triangle's own block, and the twin must give the restatement's value."""
    from nerf_pl_amd import ops, texture
    v, t, bad = M.flawed()
    T = len(t)
    assert bad[[17, 200, 201]].all()
    tris = [-1, -7, T, T + 5, 2 ** 31 - 1, 17, 200, 201, 0, 1, 2, 5, T - 2, T - 1]
    bs = [(0, 0), (1, 0), (0, 1), (1, 1), (-0.25, 0.5), (0.5, -0.25), (-3, -3), (7, 9), (0.5, 0.5), (1e30, -1e30), (np.nan, 0.5),
          (0.25, np.nan), (np.inf, -np.inf), (0.999999, 0.000001)]
    tri = np.repeat(np.array(tris, np.int64), len(bs)).astype(np.int32)
    b = np.tile(np.array(bs, np.float32), (len(tris), 1))
    rays = np.tile(M.pinhole()[:1], (len(tri), 1))
    Wa = texture.default_width(T, R)
    atlas = random_atlas(T, R, Wa, 70 + R)
    worst = 0.0
    for filt in ("bilinear", "nearest"):
        for ambient in (1.0, 0.3):
            with np.errstate(all="ignore"):
                want = X.lookup64(rays, tri, b[:, 0], b[:, 1], v, t, atlas, R, filt, ambient, 0.75)
            got = ops.mesh_shade_tex_host(rays, tri, b[:, 0], b[:, 1], v, t, atlas, R, filt, ambient, 0.75)
            back = np.isin(tri, [-1, -7, T, T + 5, 2 ** 31 - 1, 17, 200, 201])
            assert np.array_equal(got[back], np.full((back.sum(), 3), 0.75, np.float32))
            assert np.isfinite(got).all()
            worst = max(worst, float(np.abs(got - want).max()))
    print("R = %d: crafted rows off by %.3g (bound %.3g)" % (R, worst, TOL_LOOKUP))
    assert worst <= TOL_LOOKUP


# ---- 4. no bleeding ------------------------------------------------------------------------------------------------------------
def flat_colours(T):
    """one colour per triangle, all distinct for T <= 65536: red tells k mod 256 (37 is a unit mod 256), green the rest"""
    k = np.arange(T, dtype=np.int64)
    return np.stack([(37 * k + 11) % 256, (101 * k + 91 * (k >> 8) + 3) % 256, (7 * k + 200) % 256], 1).astype(np.uint8)


@pytest.mark.parametrize("R", RES)
def test_no_bleeding(R):
    from nerf_pl_amd import ops, texture
    worst = 0.0
    for rays_name in ("watertight", "pinhole"):
        v, t, rays, tri, b1, b2 = cast("ico2", rays_name)
        T = len(t)
        flat = flat_colours(T)
        assert len(np.unique(flat, axis=0)) == T
        atlas = ops.mesh_tex_atlas_host(np.repeat(flat, X.n_tex(R), 0), T, R, texture.default_width(T, R))
        hit = tri >= 0
        assert hit.sum() >= (642 if rays_name == "watertight" else 250)
        for filt in ("bilinear", "nearest"):
            got = ops.mesh_shade_tex_host(rays, tri, b1, b2, v, t, atlas, R, filt)
            worst = max(worst, float(np.abs(got[hit].astype(np.float64) - flat[tri[hit]] / 255.0).max()))
    print("R = %d: flat colours off by %.3g (bound %.3g)" % (R, worst, TOL_FLAT))
    assert worst <= TOL_FLAT


# ---- 5. a standard sampler sees the same picture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rays_name,R", [("ico2", "pinhole", 8), ("ico2", "watertight", 3), ("ico1", "inside", 1), ("plate", "axis", 2),
                                              ("soup257", "pinhole", 4)])
def test_standard_sampler(name, rays_name, R):
    from nerf_pl_amd import ops, texture
    v, t, rays, tri, b1, b2 = cast(name, rays_name)
    T = len(t)
    Wa = texture.default_width(T, R)
    assert Wa <= 256
    atlas = texture.TextureAtlas(random_atlas(T, R, Wa, 90 + R), R, T)
    hit = tri >= 0
    assert hit.any()
    got = ops.mesh_shade_tex_host(rays, tri, b1, b2, v, t, atlas.data, R, "bilinear")[hit]
    want = X.gl_sample(atlas.data, X.interpolate_uv(atlas.uv(), tri[hit], b1[hit], b2[hit]))
    worst = float(np.abs(got - want).max())
    print("%s / %s at R = %d: a GL sampler differs by %.3g (bound %.3g)" % (name, rays_name, R, worst, TOL_SAMPLER))
    assert worst <= TOL_SAMPLER


# ---- 6. the claim --------------------------------------------------------------------------------------------------------------
_CLAIM = {}


def claim():
    """The resolution claim on icosphere(2), colour field 0.5 + 0.5 sin(12 p + (0, 1, 2)), pinhole(wh=48, focal=60): PSNR over
    the hit pixels against the field at the hit point.  Returns the rays, the hits and, per colouring, (rgb of the host twins,
    PSNR of the host twins, PSNR of the numpy restatement)."""
    from nerf_pl_amd import ops, texture
    if _CLAIM:
        return _CLAIM
    v, t = M.icosphere(2)
    rays = M.pinhole(wh=48, focal=60.0)
    tris, boxes, _, _ = ops.mesh_bvh_build_host(v, t)
    tri, _, b1, b2 = ops.mesh_cast_host(rays, tris, boxes)
    hit = tri >= 0
    truth = X.field(X.hit_points(v, t, tri[hit], b1[hit], b2[hit]))
    vc = X.to_bytes(X.field(v))
    rgb = ops.mesh_shade_host(rays, tri, b1, b2, v, t, vc)
    rows = {"vertex": (rgb, X.psnr(rgb[hit], truth), X.psnr(M.shade64(rays, tri, b1, b2, v, t, vc, 1.0, 0.0)[hit], truth))}
    for R in (1, 2, 4, 8):
        Wa = texture.default_width(len(t), R)
        colours = X.to_bytes(X.field(X.points32(v, t, R)[0]))
        atlas = ops.mesh_tex_atlas_host(X.to_bytes(X.field(ops.mesh_tex_points_host(v, t, R, normals=False)[0])), len(t), R, Wa)
        ref_atlas = X.atlas_from(colours, len(t), R, Wa)
        for filt in ("bilinear", "nearest"):
            rgb = ops.mesh_shade_tex_host(rays, tri, b1, b2, v, t, atlas, R, filt)
            ref = X.lookup64(rays, tri, b1, b2, v, t, ref_atlas, R, filt, 1.0, 0.0)
            rows[(filt, R)] = (rgb, X.psnr(rgb[hit], truth), X.psnr(ref[hit], truth))
    _CLAIM.update(rays=rays, tri=tri, b1=b1, b2=b2, hit=hit, rows=rows)
    return _CLAIM


def test_the_claim():
    """Measured (numpy restatement = host twins to the digits shown): vertex colours 13.8 dB; texture, bilinear, R = 2: 23.0,
    R = 4: 34.4, R = 8: 46.3 dB; nearest filter, R = 8: 28.3 dB.  h^2 scaling predicts + 12 dB per doubling."""
    c = claim()
    rows = c["rows"]
    assert c["hit"].sum() > 500 and len(M.icosphere(2)[1]) == 320
    for key, (_, twin, ref) in rows.items():
        print("%-18s host twins %.2f dB, numpy restatement %.2f dB" % (key, twin, ref))
        assert abs(twin - ref) < 0.01
    psnr = {k: r[1] for k, r in rows.items()}
    assert psnr[("bilinear", 8)] >= psnr["vertex"] + 20.0
    assert psnr[("bilinear", 4)] >= psnr[("bilinear", 2)] + 9.0 and psnr[("bilinear", 8)] >= psnr[("bilinear", 4)] + 9.0
    for R in (2, 4, 8):
        assert psnr[("bilinear", R)] > psnr[("nearest", R)]


# ---- 7. OBJ round trip ---------------------------------------------------------------------------------------------------------
def test_obj_round_trip(tmp_path):
    from nerf_pl_amd import imageio_min, texture
    v, t = M.soup(33)
    v = (v * np.float32(1.234567)).astype(np.float32)
    T, R = len(t), 3
    atlas = texture.TextureAtlas(random_atlas(T, R, texture.default_width(T, R), 5), R, T)
    path = str(tmp_path / "soup.obj")
    texture.write_obj(path, v, t, atlas, png_encoder="host")
    assert sorted(os.listdir(str(tmp_path))) == ["soup.mtl", "soup.obj", "soup.png"]
    assert "map_Kd soup.png" in open(str(tmp_path / "soup.mtl")).read().splitlines()
    text = open(path).read().splitlines()
    assert "mtllib soup.mtl" in text and "usemtl soup" in text
    assert sum(l.startswith("v ") for l in text) == len(v) and sum(l.startswith("vt ") for l in text) == 3 * T
    assert text[-1] == "f %d/%d %d/%d %d/%d" % (t[-1, 0] + 1, 3 * T - 2, t[-1, 1] + 1, 3 * T - 1, t[-1, 2] + 1, 3 * T)
    assert np.array_equal(imageio_min.read_png(str(tmp_path / "soup.png")), atlas.data)
    v2, t2, atlas2, uv2 = texture.read_obj(path)
    assert v2.dtype == np.float32 and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
    assert t2.dtype == np.int32 and np.array_equal(t2, t)
    assert (atlas2.res, atlas2.width, atlas2.height, atlas2.n_triangles) == (R, atlas.width, atlas.height, T)
    assert np.array_equal(atlas2.data, atlas.data)
    px = atlas.uv().astype(np.float64)
    want = np.stack([px[..., 0] / atlas.width, 1.0 - px[..., 1] / atlas.height], -1).astype(np.float32)
    assert uv2.dtype == np.float32 and np.array_equal(uv2.view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        texture.write_obj(path, v, t[:-1], atlas)


# ---- 8. argument checks without a GPU ------------------------------------------------------------------------------------------
def test_sizes(lib):
    from nerf_pl_amd import ops
    for R in (1, 2, 3, 8, 64):
        assert lib.nerfhip_mesh_tex_samples(R) == X.n_tex(R) == ops.mesh_tex_samples(R)
    for R in (0, -1, 65):
        assert lib.nerfhip_mesh_tex_samples(R) == 0
        assert lib.nerfhip_mesh_tex_height(10, R, 64) == 0
        with pytest.raises(ValueError):
            ops.mesh_tex_samples(R)
    assert lib.nerfhip_mesh_tex_height(37, 3, 28) == X.height(37, 3, 28) == 30
    assert lib.nerfhip_mesh_tex_height(0, 3, 28) == 0
    for T, R, Wa in ((-1, 3, 28), (2 ** 28 + 1, 3, 28), (37, 3, 26), (37, 3, 4), (37, 3, 16388), (2 ** 25, 8, 16)):
        assert lib.nerfhip_mesh_tex_height(T, R, Wa) == 0
        with pytest.raises(ValueError):
            ops.mesh_tex_height(T, R, Wa)
    assert lib.nerfhip_mesh_tex_height(2 * 1489 * 1489, 8, 16380) == 11 * 1489          # 16379 rows: the largest atlas at R = 8
    assert lib.nerfhip_mesh_tex_height(2 * 1489 * 1490, 8, 16380) == 0


@pytest.mark.parametrize("device", [False, True])
def test_argument_checks(lib, device):
    """Every refusal happens before anything is launched or dereferenced: null and fake pointers, through the _host and the device
    entry points alike."""
    P, ODD2, ODD4 = 0x10000, 0x10002, 0x10004          # fake: aligned to 16; to 2 only; to 4 only
    tail = (None,) if device else ()

    def points(*a):
        return getattr(lib, "nerfhip_mesh_tex_points" + ("" if device else "_host"))(*a, *tail)

    def atlas(*a):
        return getattr(lib, "nerfhip_mesh_tex_atlas" + ("" if device else "_host"))(*a, *tail)

    def shade(**kw):
        a = dict(rays=P, n=4, tri=P, b1=P, b2=P, vertices=P, V=9, triangles=P, T=5, atlas=P, R=2, Wa=8, Ha=15, filter=1, ambient=1.0,
                 background=0.0, rgb=P)
        a.update(kw)
        return getattr(lib, "nerfhip_mesh_shade_tex" + ("" if device else "_host"))(*a.values(), *tail)

    # points(vertices, V, triangles, T, R, points, normals)
    for R in (0, -3, 65):
        assert points(P, 9, P, 5, R, P, P) == E_BADARG
    for T in (-1, 2 ** 28 + 1, 2 ** 20):                                                  # 2^20 triangles at R = 64: K > 2^30
        assert points(P, 9, P, T, 64, P, P) == E_BADARG
    for V in (-1, 2 ** 31):
        assert points(P, V, P, 5, 2, P, P) == E_BADARG
    assert points(None, 9, P, 5, 2, P, P) == E_BADARG
    assert points(P, 9, None, 5, 2, P, P) == E_BADARG
    assert points(P, 9, P, 5, 2, None, P) == E_BADARG
    assert points(ODD2, 9, P, 5, 2, P, P) == E_ALIGN
    assert points(P, 9, ODD2, 5, 2, P, P) == E_ALIGN
    assert points(P, 9, P, 5, 2, ODD2, P) == E_ALIGN
    assert points(P, 9, P, 5, 2, P, ODD4) == E_ALIGN                                      # normals: 8 bytes
    assert points(None, 0, None, 0, 2, None, None) == 0                                   # T == 0

    # atlas(colors, T, R, Wa, Ha, atlas): 5 triangles at R = 2, width 8 -> one block per row, 15 rows
    assert lib.nerfhip_mesh_tex_height(5, 2, 8) == 15
    for R, Ha in ((0, 15), (65, 15)):
        assert atlas(P, 5, R, 8, Ha, P) == E_BADARG
    for Wa in (0, 4, 6, 10, 16388):                                                       # below B, no multiple of 4, too wide
        assert atlas(P, 5, 2, Wa, 15, P) == E_BADARG
    for Ha in (-15, 0, 10, 14, 16, 20):
        assert atlas(P, 5, 2, 8, Ha, P) == E_BADARG
    for T in (-1, 2 ** 28 + 1, 7, 2 ** 25):                                               # 7 triangles need 20 rows
        assert atlas(P, T, 2, 8, 15, P) == E_BADARG
    assert atlas(None, 5, 2, 8, 15, P) == E_BADARG
    assert atlas(P, 5, 2, 8, 15, None) == E_BADARG
    assert atlas(P, 5, 2, 8, 15, ODD2) == E_ALIGN
    assert atlas(None, 0, 2, 8, 0, None) == 0                                             # T == 0: no rows

    # shade
    assert shade(n=-1) == E_BADARG and shade(n=2 ** 30 + 1) == E_BADARG
    assert shade(V=-1) == E_BADARG and shade(V=2 ** 31) == E_BADARG
    assert shade(T=-1) == E_BADARG and shade(T=7) == E_BADARG and shade(T=2 ** 28 + 1) == E_BADARG
    assert shade(R=0) == E_BADARG and shade(R=65) == E_BADARG and shade(R=3) == E_BADARG  # R = 3: B = 6, another height
    assert shade(Wa=6) == E_BADARG and shade(Wa=4) == E_BADARG and shade(Wa=16388) == E_BADARG
    assert shade(Ha=14) == E_BADARG and shade(Ha=-15) == E_BADARG
    assert shade(filter=2) == E_BADARG and shade(filter=-1) == E_BADARG
    for ambient in (-0.01, 1.01, float("nan")):
        assert shade(ambient=ambient) == E_BADARG
    for background in (float("inf"), float("nan")):
        assert shade(background=background) == E_BADARG
    for name in ("rays", "tri", "b1", "b2", "vertices", "triangles", "atlas", "rgb"):
        assert shade(**{name: None}) == E_BADARG, name
        assert shade(**{name: ODD2}) == E_ALIGN, name
    assert shade(n=0, rays=None, tri=None, b1=None, b2=None, rgb=None) == 0               # n == 0
    assert shade(n=0, T=0, Ha=0, V=0, vertices=None, triangles=None, atlas=None) == 0


def test_empty_mesh_and_no_rays():
    from nerf_pl_amd import ops
    v, t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    p, n = ops.mesh_tex_points_host(v, t, 4)
    assert p.shape == (0, 3) and n.shape == (0, 3)
    atlas = ops.mesh_tex_atlas_host(np.zeros((0, 3), np.uint8), 0, 4, 28)
    assert atlas.shape == (0, 28, 3)
    rays = M.pinhole()[:5]
    zeros = np.zeros(5, np.float32)
    rgb = ops.mesh_shade_tex_host(rays, np.zeros(5, np.int32), zeros, zeros, v, t, atlas, 4, background=0.5)     # T == 0, n > 0
    assert np.array_equal(rgb, np.full((5, 3), 0.5, np.float32))
    v, t = M.icosphere(0)
    atlas = random_atlas(len(t), 2, 16, 3)
    assert ops.mesh_shade_tex_host(rays[:0], np.zeros(0, np.int32), zeros[:0], zeros[:0], v, t, atlas, 2).shape == (0, 3)
    with pytest.raises(ValueError):
        ops.mesh_shade_tex_host(rays, np.zeros(5, np.int32), zeros, zeros, v, t, atlas[:-1], 2)
    with pytest.raises(ValueError):
        ops.mesh_shade_tex_host(rays, np.zeros(5, np.int32), zeros, zeros, v, t, atlas, 2, filter="trilinear")
    with pytest.raises(ValueError):
        ops.mesh_tex_atlas_host(np.zeros((7, 3), np.uint8), len(t), 2, 16)

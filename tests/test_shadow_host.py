"""CPU: the shadow units through their host twins (nerfhip_mesh_occluded_host, nerfhip_shadow_rays_host,
nerfhip_light_compose_host: the kernels' own routines, csrc/shadow_core.h) on the fixtures of tests/mesh_ref.py.  Fails on a library
without these entry points.

What is exact is compared exactly: occlusion against the cast and against brute force; the rows, the cosine and the compose
against the float32 restatement of tests/shadow_ref.py, operation for operation, the integer sample sequence included.

Against the float64 restatement the caps are measured, not derived: the largest deviation of the host twins on these fixtures on
the CPU, times 4.  The arithmetic is libm-free, so the device computes the same bits and adds nothing.  Measured / cap:

    rows (p, d, far), relative to max(1, |value|)      1.54e-07    6.16e-07
    cosine, absolute                                   1.79e-07    7.16e-07
    compose rgb and V, absolute                        6.84e-08    2.74e-07

A pixel is left out of the float64 comparison when its frame hangs on a comparison that the two precisions may decide differently
(shadow_ref's `unsure`); at most 1 % of a case's pixels may be.

The analytic shadow: the level-3 icosphere over a ground plane, where a ground pixel is in shadow iff the sphere's centre is nearer
than its radius to the pixel's shadow ray; every pixel outside the band between the icosphere's inscribed and circumscribed radius
must be right."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402
import shadow_ref as S  # noqa: E402
from test_meshcast_host import aligned, built  # noqa: E402

E_BADARG, E_ALIGN = -1, -3
MEASURED_ROWS, CAP_ROWS = 1.54e-07, 6.16e-07
MEASURED_COSINE, CAP_COSINE = 1.79e-07, 7.16e-07
MEASURED_COMPOSE, CAP_COMPOSE = 6.84e-08, 2.74e-07
MAX_UNSURE = 0.01

LIGHTS = (("directional", (1.0, 0.0, 1.0)), ("directional", (0.3, -2.0, 0.5)), ("directional", (0.0, 0.0, 3.0)),
          ("directional", (-1.0, -1.0, 2.0)), ("point", (3.0, 0.0, 6.0)), ("point", (0.2, 0.1, 1.6)))
BIAS, REACH = 1e-3, 50.0


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same_bits(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------- any hit
@pytest.mark.parametrize("name", sorted(R.meshes()))
def test_occluded_is_the_cast_and_brute_force(name):
    from nerf_pl_amd import ops
    _, _, (tris, boxes, _, _) = built(name)
    for set_name, rays in R.ray_sets().items():
        hit = ops.mesh_occluded_host(rays, tris, boxes)
        brute = ops.mesh_occluded_host(rays, tris, None, brute=True)
        cast = ops.mesh_cast_host(rays, tris, boxes)[0] >= 0
        assert hit.dtype == np.uint8 and set(np.unique(hit)) <= {0, 1}
        assert np.array_equal(hit, brute), (name, set_name, np.flatnonzero(hit != brute)[:8])
        assert np.array_equal(hit.astype(bool), cast), (name, set_name, np.flatnonzero(hit.astype(bool) != cast)[:8])


def test_watertight_rays_are_all_occluded():
    from nerf_pl_amd import ops
    _, _, (tris, boxes, _, _) = built("ico2")
    rays = R.watertight_rays(2)
    assert rays.shape == (642, 8)
    assert ops.mesh_occluded_host(rays, tris, boxes).all() and ops.mesh_occluded_host(rays, tris, None, brute=True).all()


def test_empty_mesh_and_no_rays():
    from nerf_pl_amd import ops
    empty = ops.mesh_bvh_build_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert not ops.mesh_occluded_host(R.pinhole(), empty[0], empty[1]).any()
    _, _, (tris, boxes, _, _) = built("ico1")
    assert ops.mesh_occluded_host(np.zeros((0, 8), np.float32), tris, boxes).shape == (0,)


# ---------------------------------------------------------------------------------------------------------- the sample sequence
@pytest.mark.parametrize("K", [1, 4, 16, 64])
def test_sample_sequence(K):
    n = 300
    for rotate in (0, 1):
        u, v = S.offsets(n, K, rotate)
        assert u.dtype == np.float32 and u.min() >= -1 and u.max() < 1 and v.min() >= -1 and v.max() < 1
        for i in range(n):
            assert len(set(zip(u[i].tolist(), v[i].tolist()))) == K and len(set(u[i].tolist())) == K and len(set(v[i].tolist())) == K
        if rotate:
            assert len({(a, b) for a, b in zip(u[:, 0].tolist(), v[:, 0].tolist())}) == n     # a shift of its own for every pixel
        else:
            assert (u == u[:1]).all() and (v == v[:1]).all() and u[0, 0] == 0 and v[0, 0] == 0    # sample 0 is the centre
    if K == 64:     # low discrepancy: every cell of an 4 x 4 grid over the square holds 2 to 6 of the 64 points
        u, v = S.offsets(1, 64, 0)
        cells = np.bincount((np.floor((u[0] + 1) * 2) * 4 + np.floor((v[0] + 1) * 2)).astype(int), minlength=16)
        assert cells.min() >= 2 and cells.max() <= 6, cells


# ---------------------------------------------------------------------------------------------------- rows, cosine and compose
_CASE = {}


def primary(name="ico2"):
    """(rays, s, tri, vertices, triangles): the pinhole image of a fixture; s is the hit's t on the mesh, a seeded depth on half
    of the other pixels (a scene surface) and +inf on the rest; the first rows are the special cases"""
    from nerf_pl_amd import ops
    if name not in _CASE:
        v, t, (tris, boxes, _, _) = built(name)
        rays = R.pinhole().copy()
        tri, tt, _, _ = ops.mesh_cast_host(rays, tris, boxes)
        rng = np.random.default_rng(21)
        s = np.where(tri >= 0, tt, np.where(rng.random(len(rays)) < 0.5, rng.uniform(3.0, 6.0, len(rays)), np.inf)).astype(np.float32)
        s[:4] = (np.inf, np.nan, 0.0, -1.5)
        rays[4, 1], rays[5, 4], rays[6, 7] = np.nan, np.inf, -np.inf
        s[4:7] = 3.0
        tri = tri.copy()
        tri[7], tri[8], tri[9] = len(t), np.iinfo(np.int32).max, -5                 # out of range; negative: off the mesh
        assert (tri[10:] >= 0).sum() > 100 and (tri[10:] < 0).sum() > 100 and np.isinf(s[10:]).sum() > 100
        _CASE[name] = (rays, s, tri.astype(np.int32), v, t)
    return _CASE[name]


SPECIAL_ZERO = 7         # the first rows of `primary` that have no surface or a non-finite primary row


def row_cases():
    return [(kind, light, K, radius, rotate) for (kind, light), (K, radius, rotate) in
            itertools.product(LIGHTS, ((1, 0.0, 1), (4, 0.0, 0), (1, 0.05, 0), (4, 0.05, 1), (16, 0.3, 1), (16, 0.3, 0)))]


def test_rows_and_cosine_are_the_float32_restatement():
    from nerf_pl_amd import ops
    for name in ("ico2", "flawed"):
        rays, s, tri, v, t = primary(name)
        for kind, light, K, radius, rotate in row_cases():
            rows, cosine = ops.shadow_rays_host(rays, s, kind, light, BIAS, REACH, K, radius, rotate, tri, v, t)
            want_rows, want_cosine, _ = S.shadow_rays(rays, s, kind, light, BIAS, REACH, K, radius, rotate, tri, v, t)
            assert rows.shape == (len(rays) * K, 8) and cosine.shape == (len(rays),)
            assert same_bits([rows, cosine], [want_rows, want_cosine]), (name, kind, light, K, radius, rotate,
                                                                         np.flatnonzero((bits(rows) != bits(want_rows)).reshape(len(rows), -1).any(1))[:8])


def test_rows_and_cosine_against_float64():
    from nerf_pl_amd import ops
    rays, s, tri, v, t = primary("ico2")
    worst_rows = worst_cos = 0.0
    for kind, light, K, radius, rotate in row_cases():
        rows, cosine = ops.shadow_rays_host(rays, s, kind, light, BIAS, REACH, K, radius, rotate, tri, v, t)
        ref_rows, ref_cosine, unsure = S.shadow_rays(rays, s, kind, light, BIAS, REACH, K, radius, rotate, tri, v, t, dt=np.float64)
        assert unsure.mean() <= MAX_UNSURE
        keep = np.repeat(~unsure, K)
        assert np.array_equal((rows[keep] == 0).all(1), (ref_rows[keep] == 0).all(1))
        e_rows = float((np.abs(rows[keep] - ref_rows[keep]) / np.maximum(1.0, np.abs(ref_rows[keep]))).max())
        e_cos = float(np.abs(cosine - ref_cosine)[~unsure].max())
        worst_rows, worst_cos = max(worst_rows, e_rows), max(worst_cos, e_cos)
        d = rows[:, 3:6].astype(np.float64)
        live = ~(rows == 0).all(1)
        assert np.abs(np.linalg.norm(d[live], axis=1) - 1.0).max() < 1e-6                # unit directions
        assert (rows[live, 6] == np.float32(BIAS)).all()
        assert (cosine >= 0).all() and (cosine <= 1).all() and (cosine[tri < 0] == 1).all()
    print("rows %.3g (cap %.3g), cosine %.3g (cap %.3g)" % (worst_rows, CAP_ROWS, worst_cos, CAP_COSINE))
    assert worst_rows <= CAP_ROWS and worst_cos <= CAP_COSINE


def compose_inputs(n=257, K=4):
    rng = np.random.default_rng(33)
    rgb = rng.random((n, 3)).astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    cosine = rng.random(n).astype(np.float32)
    hit = (rng.random(n * K) < 0.4).astype(np.uint8)
    hit[:K], hit[K:2 * K] = 0, 1
    hit[::7] *= 200                                            # any non-zero byte is a hit
    trans = rng.random(n * K).astype(np.float32)
    return rgb, mask, cosine, hit, trans


def test_compose_is_the_restatement_and_passes_rgb_through():
    from nerf_pl_amd import ops
    worst = 0.0
    for K in (1, 4, 16):
        rgb, mask, cosine, hit, trans = compose_inputs(257, K)
        for tr, ambient, strength in ((trans, 0.3, 0.7), (None, 0.3, 0.7), (trans, 0.0, 1.0), (None, 1.0, 0.0), (trans, 1.0, 0.0)):
            out, V = ops.light_compose_host(rgb, mask, cosine, hit, tr, ambient, strength)
            want = S.light_compose(rgb, mask, cosine, hit, tr, ambient, strength)
            assert same_bits([out, V], want), (K, ambient, strength)
            ref = S.light_compose(rgb, mask, cosine, hit, tr, ambient, strength, dt=np.float64)
            worst = max(worst, float(np.abs(out - ref[0]).max()), float(np.abs(V - ref[1]).max()))
            assert (V >= 0).all() and (V <= 1).all()
            if ambient == 1.0 and strength == 0.0:
                assert same_bits([out], [rgb])
            again, none = ops.light_compose_host(rgb, mask, cosine, hit, tr, ambient, strength, visibility=False)
            assert none is None and same_bits([again], [out])
        scene = mask == 0                                       # trans is not read off the mesh
        a = ops.light_compose_host(rgb, mask, cosine, hit, trans, 0.3, 0.7)
        b = ops.light_compose_host(rgb, mask, cosine, hit, None, 0.3, 0.7)
        assert same_bits([a[0][scene], a[1][scene]], [b[0][scene], b[1][scene]]) and not same_bits([a[1][~scene]], [b[1][~scene]])
    print("compose %.3g (cap %.3g)" % (worst, CAP_COMPOSE))
    assert worst <= CAP_COMPOSE


# ------------------------------------------------------------------------------------------------------------------- properties
def test_radius_zero_rows_are_the_single_row():
    from nerf_pl_amd import ops
    rays, s, tri, v, t = primary()
    for kind, light in LIGHTS:
        one = ops.shadow_rays_host(rays, s, kind, light, BIAS, REACH, 1, 0.0, 1)[0]
        for rotate in (0, 1):
            four = ops.shadow_rays_host(rays, s, kind, light, BIAS, REACH, 4, 0.0, rotate)[0].reshape(len(rays), 4, 8)
            for k in range(4):
                assert same_bits([four[:, k]], [one]), (kind, light, k)


def test_zero_rows_and_null_arguments():
    from nerf_pl_amd import ops
    rays, s, tri, v, t = primary()
    _, _, (tris, boxes, _, _) = built("ico2")
    seen = 0
    for kind, light in LIGHTS:
        rows, cosine = ops.shadow_rays_host(rays, s, kind, light, BIAS, REACH, 4, 0.05, 1, tri, v, t)
        rows = rows.reshape(len(rays), 4, 8)
        zero = (bits(rows).reshape(len(rays), -1) == 0).all(1)                     # +0 in every byte
        assert zero[:SPECIAL_ZERO].all() and np.array_equal(zero, ~(np.isfinite(rays).all(1) & np.isfinite(s) & (s > 0)))
        assert (cosine[:SPECIAL_ZERO][tri[:SPECIAL_ZERO] >= 0] == 0).all() and cosine[7] == 0 and cosine[8] == 0 and cosine[9] == 1
        hit = ops.mesh_occluded_host(rows.reshape(-1, 8), tris, boxes).reshape(len(rays), 4)
        assert not hit[zero].any()
        seen += int(hit.sum())
        # tri null: cosine 1 everywhere, the rows unchanged; cosine null: the rows unchanged
        rows_a, cos_a = ops.shadow_rays_host(rays, s, kind, light, BIAS, REACH, 4, 0.05, 1)
        rows_b, cos_b = ops.shadow_rays_host(rays, s, kind, light, BIAS, REACH, 4, 0.05, 1, tri, v, t, cosine=False)
        assert cos_b is None and (cos_a == 1).all() and same_bits([rows_a, rows_b], [rows.reshape(-1, 8)] * 2)
    assert seen > 1000                                         # (the light behind the camera shadows nothing that the camera sees)
    # a pixel on a point light
    on = R.pinhole()[:3].copy()
    rows = ops.shadow_rays_host(on, np.full(3, 2.0, np.float32), "point", tuple((on[1, :3] + 2.0 * on[1, 3:6]).tolist()), BIAS, REACH, 2)[0]
    assert not rows[2:4].any() and rows[:2].any() and rows[4:].any()
    # all rows zero, and no rows at all
    none = ops.shadow_rays_host(rays, np.full(len(rays), np.inf, np.float32), "directional", (0, 0, 1), BIAS, REACH, 4, 0.1)[0]
    assert not bits(none).any() and not ops.mesh_occluded_host(none, tris, boxes).any()
    rows, cosine = ops.shadow_rays_host(np.zeros((0, 8), np.float32), np.zeros(0, np.float32), "directional", (0, 0, 1), BIAS, REACH, 4)
    assert rows.shape == (0, 8) and cosine.shape == (0,)
    out, V = ops.light_compose_host(np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), cosine, np.zeros(0, np.uint8))
    assert out.shape == (0, 3) and V.shape == (0,)


# ----------------------------------------------------------------------------------------------------------- the analytic shadow
_SCENE = {}


def analytic_scene():
    """(vertices, triangles, host hierarchy, primary rays, tri, s) of the sphere over the ground"""
    from nerf_pl_amd import ops
    if not _SCENE:
        v, t = S.sphere_scene(R.icosphere(3))
        h = ops.mesh_bvh_build_host(v, t)
        rays = S.down_rays(48)
        tri, s, _, _ = ops.mesh_cast_host(rays, h[0], h[1])
        assert (tri >= 0).all() and (tri >= len(t) - 2).sum() > 1500       # every row ends on the ground or on the sphere
        _SCENE["s"] = (v, t, h, rays, tri, s)
    return _SCENE["s"]


def analytic_check(occluded_of, rows_of, compose_of):
    """the verdicts of the analytic shadow, through the three given entry points (the host twins here, the device's on the GPU)"""
    v, t, h, rays, tri, s = analytic_scene()
    ground = tri >= len(t) - 2
    p = rays[:, :3].astype(np.float64) + s[:, None].astype(np.float64) * rays[:, 3:6].astype(np.float64)
    n = len(rays)
    scene_px, ones = np.zeros(n, np.uint8), np.ones(n, np.float32)
    white = np.ones((n, 3), np.float32)
    for kind, light in (("directional", (1.0, 0.0, 1.0)), ("point", (3.0, 0.0, 6.0))):
        dist, to_centre = S.distance_to_light_path(p, kind, light)
        judged = ground & ((dist < S.BAND[0]) | (dist > S.BAND[1]))
        assert (ground & ~judged).sum() <= 0.01 * n
        rows, _ = rows_of(rays, s, kind, light, 1e-3, 100.0, 1, 0.0, 1)
        hit = occluded_of(rows, h[0], h[1])
        want = dist < S.BAND[0]
        assert np.array_equal(hit.astype(bool)[judged], want[judged]), (kind, np.flatnonzero(judged & (hit.astype(bool) != want))[:8])
        assert want[judged].sum() > 50 and (~want[judged]).sum() > 1000
        hard = compose_of(white, scene_px, ones, hit, None, 0.3, 1.0)[1]
        assert set(np.unique(hard)) == {0.0, 1.0}
        # a soft light: 16 samples over a square of half-width 0.05.  A sample's direction is within delta = atan(0.05 sqrt 2) of
        # the centre's (directional) — for the point light its position within 0.05 sqrt 2 of the centre's, seen from the ground at
        # least 6 below it: delta = asin(0.05 sqrt 2 / 6) —, so its distance to the sphere's centre is within |p - centre| delta of the
        # central ray's
        radius, K = 0.05, 16
        delta = np.arctan(radius * np.sqrt(2.0)) if kind == "directional" else np.arcsin(radius * np.sqrt(2.0) / 6.0)
        margin = to_centre * delta + 1e-3
        rows, _ = rows_of(rays, s, kind, light, 1e-3, 100.0, K, radius, 1)
        V = compose_of(white, scene_px, ones, occluded_of(rows, h[0], h[1]), None, 0.3, 1.0)[1]
        umbra, lit = ground & (dist < S.BAND[0] - margin), ground & (dist > S.BAND[1] + margin)
        assert umbra.sum() > 10 and lit.sum() > 1000
        assert (V[umbra] == 0).all() and (V[lit] == 1).all(), kind
        assert ((V[ground] > 0) & (V[ground] < 1)).any(), kind


def test_analytic_shadow_of_a_sphere():
    from nerf_pl_amd import ops
    analytic_check(ops.mesh_occluded_host, ops.shadow_rays_host, ops.light_compose_host)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_shadow_entry_points_validate_arguments_without_a_gpu(lib):
    """Every refusal of include/nerfhip.h's shadow section comes back before anything is launched or dereferenced: the pointers
    below are null or fake."""
    null, fake, odd = None, 0x10000, 0x10004
    big = (1 << 28) + 1
    nan, inf = float("nan"), float("inf")
    # any hit
    assert lib.nerfhip_mesh_occluded(fake, -1, fake, fake, 1, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_occluded(fake, (1 << 30) + 1, fake, fake, 1, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_occluded(fake, 4, fake, fake, big, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_occluded(null, 4, fake, fake, 1, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_occluded(fake, 4, null, fake, 1, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_occluded(fake, 4, fake, null, 1, fake, null) == E_BADARG          # no boxes on the device
    assert lib.nerfhip_mesh_occluded(fake, 4, fake, fake, 1, null, null) == E_BADARG
    assert lib.nerfhip_mesh_occluded(odd, 4, fake, fake, 1, fake, null) == E_ALIGN
    assert lib.nerfhip_mesh_occluded(fake, 4, odd, fake, 1, fake, null) == E_ALIGN
    assert lib.nerfhip_mesh_occluded(null, 0, null, null, 0, null, null) == 0
    assert lib.nerfhip_mesh_occluded_host(fake, 4, fake, null, 1, 0, fake) == E_BADARG
    assert lib.nerfhip_mesh_occluded_host(null, 4, fake, null, 1, 1, fake) == E_BADARG

    # rows: (rays, s, n, tri, vertices, V, triangles, T, kind, lx, ly, lz, bias, reach, K, radius, rotate, rows, cosine)
    def rows(rays=fake, s=fake, n=4, tri=null, vertices=null, V=0, triangles=null, T=0, kind=0, l=(1.0, 0.0, 1.0), bias=1e-3, reach=10.0,
             K=1, radius=0.0, rotate=0, out=fake, cosine=null, host=False):
        args = (rays, s, n, tri, vertices, V, triangles, T, kind, l[0], l[1], l[2], bias, reach, K, radius, rotate, out, cosine)
        return lib.nerfhip_shadow_rays_host(*args) if host else lib.nerfhip_shadow_rays(*args, null)
    for host in (False, True):
        assert rows(K=0, host=host) == E_BADARG and rows(K=65, host=host) == E_BADARG and rows(K=-1, host=host) == E_BADARG
        assert rows(bias=0.0, host=host) == E_BADARG and rows(bias=-1.0, host=host) == E_BADARG
        assert rows(bias=nan, host=host) == E_BADARG and rows(bias=inf, host=host) == E_BADARG
        assert rows(reach=inf, host=host) == E_BADARG and rows(reach=nan, host=host) == E_BADARG and rows(reach=0.0, host=host) == E_BADARG
        assert rows(l=(0.0, 0.0, 0.0), host=host) == E_BADARG and rows(l=(0.0, -0.0, 0.0), host=host) == E_BADARG
        assert rows(l=(nan, 0.0, 1.0), host=host) == E_BADARG and rows(l=(1.0, inf, 1.0), kind=1, host=host) == E_BADARG
        assert rows(kind=2, host=host) == E_BADARG and rows(kind=-1, host=host) == E_BADARG
        assert rows(rotate=2, host=host) == E_BADARG
        assert rows(radius=-0.1, host=host) == E_BADARG and rows(radius=inf, host=host) == E_BADARG
        assert rows(n=-1, host=host) == E_BADARG and rows(n=(1 << 30) // 64 + 1, K=64, host=host) == E_BADARG
        assert rows(rays=null, host=host) == E_BADARG and rows(s=null, host=host) == E_BADARG and rows(out=null, host=host) == E_BADARG
        assert rows(tri=fake, T=1, V=3, triangles=null, vertices=fake, host=host) == E_BADARG
        assert rows(tri=fake, T=1, V=3, triangles=fake, vertices=null, host=host) == E_BADARG
        assert rows(tri=fake, T=big, V=3, triangles=fake, vertices=fake, host=host) == E_BADARG
        assert rows(rays=odd, host=host) == E_ALIGN and rows(out=odd, host=host) == E_ALIGN and rows(s=fake + 2, host=host) == E_ALIGN
        assert rows(cosine=fake + 1, host=host) == E_ALIGN and rows(tri=fake + 2, T=1, V=3, triangles=fake, vertices=fake, host=host) == E_ALIGN
        assert rows(n=0, rays=null, s=null, out=null, host=host) == 0
        assert rows(n=0, l=(0.0, 0.0, 0.0), kind=1, rays=null, s=null, out=null, host=host) == 0      # a point light at the origin is a light

    # compose: (n, rgb, mask, cosine, hit, trans, K, ambient, strength, rgb_out, visibility)
    def compose(n=4, rgb=fake, mask=fake, cosine=fake, hit=fake, trans=null, K=1, ambient=0.3, strength=0.7, out=fake, vis=null, host=False):
        args = (n, rgb, mask, cosine, hit, trans, K, ambient, strength, out, vis)
        return lib.nerfhip_light_compose_host(*args) if host else lib.nerfhip_light_compose(*args, null)
    for host in (False, True):
        assert compose(K=0, host=host) == E_BADARG and compose(K=65, host=host) == E_BADARG
        assert compose(ambient=-0.1, host=host) == E_BADARG and compose(ambient=1.5, host=host) == E_BADARG
        assert compose(ambient=nan, host=host) == E_BADARG and compose(strength=nan, host=host) == E_BADARG
        assert compose(strength=-0.1, host=host) == E_BADARG and compose(strength=1.1, host=host) == E_BADARG
        assert compose(n=-1, host=host) == E_BADARG and compose(n=(1 << 30) // 2 + 1, K=2, host=host) == E_BADARG
        for name in ("rgb", "mask", "cosine", "hit", "out"):
            assert compose(host=host, **{name: null}) == E_BADARG, name
        assert compose(rgb=fake + 2, host=host) == E_ALIGN and compose(trans=fake + 1, host=host) == E_ALIGN
        assert compose(out=fake + 2, host=host) == E_ALIGN and compose(vis=fake + 3, host=host) == E_ALIGN
        assert compose(n=0, rgb=null, mask=null, cosine=null, hit=null, out=null, host=host) == 0
    assert lib.nerfhip_abi_version() == 3


def test_python_layer_refuses():
    import torch
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.lighting import Light, LitMixedRenderer
    rays, s, tri, v, t = primary()
    ok = dict(kind="directional", light=(1, 0, 1), bias=1e-3, reach=10.0)

    def rows(**kw):
        a = dict(ok, **kw)
        return ops.shadow_rays_host(a.pop("rays", rays), a.pop("s", s), a.pop("kind"), a.pop("light"), a.pop("bias"), a.pop("reach"), **a)
    for bad in (dict(samples=0), dict(samples=65), dict(samples=2.5), dict(bias=0.0), dict(bias=-1e-3), dict(bias=float("nan")),
                dict(reach=float("inf")), dict(reach=float("nan")), dict(light=(0, 0, 0)), dict(light=(float("nan"), 0, 1)),
                dict(light=(1, float("inf"), 1), kind="point"), dict(light=(1, 2)), dict(kind="spot"), dict(radius=-1.0),
                dict(radius=float("inf")), dict(rays=rays[:, :7]), dict(s=s[:-1]), dict(tri=tri), dict(tri=tri[:-1], vertices=v, triangles=t),
                dict(tri=tri, vertices=v[:, :2], triangles=t)):
        with pytest.raises(ValueError):
            rows(**bad)
    rgb, mask, cosine, hit, trans = compose_inputs(33, 4)
    for bad in (dict(ambient=-0.1), dict(ambient=1.1), dict(strength=-0.1), dict(strength=1.1)):
        with pytest.raises(ValueError):
            ops.light_compose_host(rgb, mask, cosine, hit, trans, **bad)
    for args in ((rgb, mask, cosine, hit[:-1], None), (rgb, mask[:-1], cosine, hit, None), (rgb, mask, cosine, hit, trans[:-1]),
                 (rgb[:, :2], mask, cosine, hit, None), (rgb, mask, cosine, np.zeros(33 * 65, np.uint8), None)):
        with pytest.raises(ValueError):
            ops.light_compose_host(*args)
    _, _, (tris, boxes, _, _) = built("ico2")
    with pytest.raises(ValueError):
        ops.mesh_occluded_host(rays, tris, boxes[:-1])
    with pytest.raises(ValueError):
        ops.mesh_occluded_host(rays[:, :6], tris, boxes)
    # the device wrappers take no CPU tensors
    with pytest.raises(NerfHipError):
        ops.mesh_occluded(torch.from_numpy(rays), torch.from_numpy(tris), torch.from_numpy(boxes))
    with pytest.raises(NerfHipError):
        ops.shadow_rays(torch.from_numpy(rays), torch.from_numpy(s), "directional", (1, 0, 1), 1e-3, 10.0)
    with pytest.raises(NerfHipError):
        ops.light_compose(*[torch.from_numpy(a) for a in (rgb, mask, cosine, hit)])
    # misaligned arrays reach the entry points only from other callers: the twins refuse them
    from nerf_pl_amd import _lib
    lib = _lib.load()
    r16, rows16 = aligned(rays), aligned(np.zeros((len(rays), 8), np.float32))
    off = aligned(np.zeros(len(rays) * 8 + 1, np.float32))[1:]
    assert lib.nerfhip_shadow_rays_host(off.ctypes.data, s.ctypes.data, 4, None, None, 0, None, 0, 0, 1.0, 0.0, 1.0, 1e-3, 10.0, 1, 0.0, 0,
                                        rows16.ctypes.data, None) == E_ALIGN
    assert lib.nerfhip_shadow_rays_host(r16.ctypes.data, s.ctypes.data, 4, None, None, 0, None, 0, 0, 1.0, 0.0, 1.0, 1e-3, 10.0, 1, 0.0, 0,
                                        off.ctypes.data, None) == E_ALIGN
    assert lib.nerfhip_mesh_occluded_host(off.ctypes.data, 4, aligned(tris).ctypes.data, boxes.ctypes.data, len(tris), 0,
                                          np.zeros(4, np.uint8).ctypes.data) == E_ALIGN
    # the light and the renderer
    for kw in (dict(), dict(direction=(1, 0, 1), position=(0, 0, 3)), dict(direction=(0, 0, 0)), dict(direction=(1, float("nan"), 0)),
               dict(position=(float("inf"), 0, 0)), dict(direction=(1, 0)), dict(direction=(1, 0, 1), samples=0),
               dict(direction=(1, 0, 1), samples=65), dict(direction=(1, 0, 1), radius=-1.0)):
        with pytest.raises(ValueError):
            Light(**kw)
    assert Light(position=(0, 0, 0)).kind == "point" and Light(direction=(0, 0, 2)).kind == "directional"
    with pytest.raises(ValueError, match="clip"):
        LitMixedRenderer(None, None, Light(direction=(1, 0, 1)), True, mode="clip")
    for kw in (dict(ambient=1.5), dict(strength=-0.5)):
        with pytest.raises(ValueError):
            LitMixedRenderer(None, None, Light(direction=(1, 0, 1)), True, **kw)

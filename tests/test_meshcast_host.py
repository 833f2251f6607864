"""CPU: the mesh ray caster through its host twins (nerfhip_mesh_*_host, nerfhip_mixed_compose_host: the kernels' own routines,
csrc/mesh_core.h) on the fixtures of tests/mesh_ref.py.  Fails on a library without these entry points.

What is exact is compared exactly: the hierarchy's format against numpy, the hierarchy cast against the brute-force twin (the same
triangle routine and a tie rule that fixes the winner: no tolerance), the watertight rays, the mask of compose.

Against float64 (tests/mesh_ref.py: Moller-Trumbore; shade and compose restated) the caps are measured, not derived: the largest
deviation of the host twins on these fixtures on the CPU, times 4.  The arithmetic is libm-free (+, -, *, IEEE / and sqrt), so the
device computes the same bits and adds nothing.  Measured / cap:

    t, relative to |t|                                             4.75e-06 (soup1000, rays from inside)     1.9e-05
    b1, b2, absolute                                               5.51e-06 (ico3, the pinhole image)        2.2e-05
    shade rgb, absolute                                            1.69e-07                                  6.8e-07
    compose rgb / depth / opacity, relative to max(1, |value|)     1.11e-07                                  4.5e-07

The first two are far above 2^-24 because both fixtures have rays that meet a triangle at a grazing angle (the soup from inside,
the sphere at its silhouette), where t and the barycentrics are ill-conditioned in the fp32 inputs themselves.

Every test prints the largest error it saw beside its cap.  A ray is left out of the float64 comparison when float64 itself cannot
judge it (mesh_ref.cast64's `unsure`); at most 1 % of a fixture's rays may be.  The `identical` fixture — T copies of one
triangle — has every hit "within 1e-5 of the second nearest" by construction; it is checked against the tie rule instead: every
hit names triangle 0 and equals the cast of a single copy bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402

E_BADARG, E_ALIGN = -1, -3
MEASURED_T, CAP_T = 4.75e-06, 1.9e-05
MEASURED_B, CAP_B = 5.51e-06, 2.2e-05
MEASURED_SHADE, CAP_SHADE = 1.69e-07, 6.8e-07
MEASURED_COMPOSE, CAP_COMPOSE = 1.11e-07, 4.5e-07
MAX_UNSURE = 0.01


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


_BUILT, _REF = {}, {}


def built(name):
    """(vertices, triangles, (tris, boxes, order, n_bad) of the host build), made once"""
    from nerf_pl_amd import ops
    if name not in _BUILT:
        v, t = R.meshes()[name]
        _BUILT[name] = (v, t, ops.mesh_bvh_build_host(v, t))
    return _BUILT[name]


def ref64(name, set_name):
    if (name, set_name) not in _REF:
        v, t = R.meshes()[name]
        _REF[name, set_name] = R.cast64(v, t, R.ray_sets()[set_name])
    return _REF[name, set_name]


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def compare64(got, ref, what):
    """hit / miss and the triangle equal on the rays float64 can judge, t, b1, b2 within the caps; returns the largest errors"""
    tri, t, b1, b2 = got
    keep = ~ref["unsure"]
    share = 1.0 - keep.mean()
    assert share <= MAX_UNSURE, (what, share)
    assert np.array_equal(tri[keep], ref["tri"][keep]), (what, np.flatnonzero(tri[keep] != ref["tri"][keep])[:8])
    hit = keep & (tri >= 0)
    e_t = e_b = 0.0
    if hit.any():
        e_t = float((np.abs(t[hit] - ref["t"][hit]) / np.maximum(np.abs(ref["t"][hit]), 1e-30)).max())
        e_b = float(max(np.abs(b1[hit] - ref["b1"][hit]).max(), np.abs(b2[hit] - ref["b2"][hit]).max()))
    print("%s: left out %.2f %%  hits %d  t %.3g (cap %.3g)  b %.3g (cap %.3g)" % (what, 100 * share, hit.sum(), e_t, CAP_T, e_b, CAP_B))
    assert e_t <= CAP_T and e_b <= CAP_B, (what, e_t, e_b)
    return e_t, e_b


# ---------------------------------------------------------------------------------------------------------------------- format
@pytest.mark.parametrize("name", sorted(R.meshes()))
def test_host_build_is_the_format(lib, name):
    from nerf_pl_amd import ops
    v, t, (tris, boxes, order, n_bad) = built(name)
    T = len(t)
    want_order, want_boxes, want_bad = R.build(v, t)
    assert ops.mesh_bvh_levels(T) == R.levels(T)
    assert ops.mesh_bvh_nodes(T) == lib.nerfhip_mesh_bvh_nodes(T) == len(want_boxes) == len(boxes)
    assert int(n_bad[0]) == want_bad
    assert np.array_equal(order, want_order)
    assert np.array_equal(boxes, want_boxes)
    # the packed triangles: the sorted triangles' vertices and numbers, -1 and zeros for a bad one
    bad = R.bad_triangles(v, t)[order]
    assert np.array_equal(tris[:, 3].view(np.int32), np.where(bad, -1, order))
    p = tris.reshape(T, 3, 4)[:, :, :3]
    assert np.array_equal(p[~bad], v[t[order[~bad]]]) and (p[bad] == 0).all() and (tris[:, [7, 11]] == 0).all()


def test_sizes_and_empty_hierarchy(lib):
    from nerf_pl_amd import ops
    assert [ops.mesh_bvh_nodes(T) for T in (0, 1, 4, 5, 32, 33, 257)] == [0, 1, 1, 3, 9, 12, 65 + 9 + 2 + 1]
    assert lib.nerfhip_mesh_bvh_nodes(1 << 28) == sum(1 << k for k in range(26, -1, -3)) + 1 == ops.mesh_bvh_nodes(1 << 28)
    assert len(ops.mesh_bvh_levels(1 << 28)) == 10
    assert lib.nerfhip_mesh_bvh_nodes(-1) == 0 and lib.nerfhip_mesh_bvh_nodes((1 << 28) + 1) == 0
    tris, boxes, order, n_bad = ops.mesh_bvh_build_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert tris.shape == (0, 12) and boxes.shape == (0, 6) and order.shape == (0,) and int(n_bad[0]) == 0
    for brute in (False, True):
        tri, t, b1, b2 = ops.mesh_cast_host(R.pinhole(), tris, boxes, brute=brute)
        assert (tri == -1).all() and not t.any() and not b1.any() and not b2.any()


# ------------------------------------------------------------------------------------------------ hierarchy = brute force
@pytest.mark.parametrize("name", sorted(R.meshes()))
def test_hierarchy_equals_brute_force(name):
    from nerf_pl_amd import ops
    v, t, (tris, boxes, order, _) = built(name)
    bad = np.flatnonzero(R.bad_triangles(v, t))
    for set_name, rays in R.ray_sets().items():
        fast = ops.mesh_cast_host(rays, tris, boxes)
        slow = ops.mesh_cast_host(rays, tris, None, brute=True)
        assert np.array_equal(fast[0], slow[0]) and same_bits(fast[1:], slow[1:]), (name, set_name)
        tri, tt, b1, b2 = fast
        assert ((tri >= -1) & (tri < len(t))).all() and not np.isin(tri, bad).any()
        miss = tri < 0
        assert not tt[miss].any() and not b1[miss].any() and not b2[miss].any()
        assert ((tt[~miss] >= rays[~miss, 6]) & (tt[~miss] <= rays[~miss, 7])).all()
        if set_name == "nonfinite":
            assert miss[:27].all()
        if set_name == "inplane" and name == "plate":
            assert miss[:50].all()                           # a ray in the plane of a triangle does not hit it


def test_identical_triangles_follow_the_tie_rule():
    from nerf_pl_amd import ops
    v, t, (tris, boxes, _, _) = built("identical")
    one = ops.mesh_bvh_build_host(v, t[:1])
    for set_name, rays in R.ray_sets().items():
        got, want = ops.mesh_cast_host(rays, tris, boxes), ops.mesh_cast_host(rays, one[0], one[1])
        assert np.array_equal(got[0], want[0]) and same_bits(got[1:], want[1:]), set_name
        assert set(np.unique(got[0])) <= {-1, 0}
    assert (ops.mesh_cast_host(R.pinhole(), tris, boxes)[0] == 0).any()


# ------------------------------------------------------------------------------------------------------------------ watertight
def test_watertight_through_vertices_and_edges():
    from nerf_pl_amd import ops
    _, _, (tris, boxes, _, _) = built("ico2")
    rays = R.watertight_rays(2)
    assert len(rays) == 642
    for brute in (False, True):
        tri = ops.mesh_cast_host(rays, tris, boxes, brute=brute)[0]
        assert (tri >= 0).all(), np.flatnonzero(tri < 0)
    # what the test separates: float64 Moller-Trumbore with its exact `>= 0` lets some of these rays through
    v, t = R.icosphere(2)
    print("float64 Moller-Trumbore misses %d of 642" % (R.cast64(v, t, rays)["tri"] < 0).sum())


# --------------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("name", sorted(set(R.meshes()) - {"identical"}))
def test_cast_against_float64(name):
    from nerf_pl_amd import ops
    _, _, (tris, boxes, _, _) = built(name)
    worst = (0.0, 0.0)
    for set_name in R.JUDGED:
        got = ops.mesh_cast_host(R.ray_sets()[set_name], tris, boxes)
        e = compare64(got, ref64(name, set_name), "%s %s" % (name, set_name))
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print("%s: worst t %.3g b %.3g" % (name, *worst))


# ------------------------------------------------------------------------------------------------------------ shade and compose
def shade_cases():
    """[(name, rays, tri, b1, b2, vertices, triangles, colors, ambient, background)] from casts of two fixtures"""
    from nerf_pl_amd import ops
    out = []
    for name, set_name, ambient, bg, coloured in (("ico3", "pinhole", 1.0, 1.0, True), ("ico3", "pinhole", 0.25, 0.0, False),
                                                 ("soup257", "inside", 0.0, 0.5, True), ("flawed", "axis", 0.5, 1.0, True)):
        v, t, (tris, boxes, _, _) = built(name)
        rays = R.ray_sets()[set_name]
        tri, _, b1, b2 = ops.mesh_cast_host(rays, tris, boxes)
        colors = np.random.default_rng(3).integers(0, 256, (len(v), 3)).astype(np.uint8) if coloured else None
        out.append(("%s %s a%g" % (name, set_name, ambient), rays, tri, b1, b2, v, t, colors, ambient, bg))
    return out


def test_shade_against_float64():
    from nerf_pl_amd import ops
    worst = 0.0
    for what, rays, tri, b1, b2, v, t, colors, ambient, bg in shade_cases():
        got = ops.mesh_shade_host(rays, tri, b1, b2, v, t, colors, ambient, bg)
        want = R.shade64(rays, tri, b1, b2, v, t, colors, ambient, bg)
        assert (got[tri < 0] == np.float32(bg)).all() and (tri >= 0).any() and (tri < 0).any()
        e = float(np.abs(got - want).max())
        worst = max(worst, e)
        print("shade %s: %.3g (cap %.3g)" % (what, e, CAP_SHADE))
        assert e <= CAP_SHADE, (what, e)
    # a triangle number or a vertex number outside the mesh shades as a miss: nothing is read out of bounds
    what, rays, tri, b1, b2, v, t, colors, ambient, bg = shade_cases()[0]
    wild = tri.copy()
    wild[::3] = len(t)
    got = ops.mesh_shade_host(rays, wild, b1, b2, v, t, colors, ambient, bg)
    assert (got[::3] == np.float32(bg)).all()
    got = ops.mesh_shade_host(rays, tri, b1, b2, v[:5], t, None, ambient, bg)
    assert np.isfinite(got).all()


def compose_inputs(n=600):
    """a seeded render and mesh layer with the special cases in the first rows: opacity exactly tau, just below it, opacity 0,
    a hit with t == s exactly, a miss"""
    rng = np.random.default_rng(11)
    rgb_n, rgb_m = rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32)
    opacity = rng.uniform(0, 1, n).astype(np.float32)
    depth = (opacity * rng.uniform(2, 6, n)).astype(np.float32)
    tri = np.where(rng.uniform(size=n) < 0.7, rng.integers(0, 100, n), -1).astype(np.int32)
    t = np.where(tri >= 0, rng.uniform(2, 6, n), 0.0).astype(np.float32)
    opacity[:6] = (0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.0, 0.75, 0.75, 1.0)
    depth[:6] = (1.5, 1.5, 0.0, 3.0, 3.0, 4.0)
    tri[:6] = (1, 2, 3, 4, 5, -1)
    t[:6] = (3.5, 3.5, 7.0, 4.0, np.nextafter(np.float32(4.0), np.float32(0)), 0.0)
    return rgb_n, depth, opacity, tri, t, rgb_m


def test_compose_against_float64_and_special_cases():
    from nerf_pl_amd import ops
    rgb_n, depth, opacity, tri, t, rgb_m = compose_inputs()
    worst = 0.0
    for mode, tau, bg in (("ztest", 0.5, 0.0), ("ztest", 0.25, 1.0), ("clip", 0.5, 0.0), ("clip", 0.5, 1.0)):
        got = ops.mixed_compose_host(mode, rgb_n, depth, opacity, tri, t, rgb_m, tau, bg)
        want = R.compose64(mode, rgb_n, depth, opacity, tri, t, rgb_m, tau, bg)
        assert got[3].dtype == np.uint8 and np.array_equal(got[3], want[3]), mode
        for g, w in zip(got[:3], want[:3]):
            e = float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max())
            worst = max(worst, e)
            assert e <= CAP_COMPOSE, (mode, e)
        print("compose %s tau %g: %.3g (cap %.3g)" % (mode, tau, worst, CAP_COMPOSE))
    rgb, d, op, mask = ops.mixed_compose_host("ztest", rgb_n, depth, opacity, tri, t, rgb_m, 0.5, 0.0)
    # opacity == tau: s = 1.5 / 0.5 = 3 < t: NeRF; just below tau: s = +inf: mesh; opacity 0: mesh; t == s = 4: NeRF (strict <);
    # t one ulp below s: mesh; a miss: NeRF
    assert mask[:6].tolist() == [0, 1, 1, 0, 1, 0]
    assert same_bits([rgb[mask == 1], rgb[mask == 0]], [rgb_m[mask == 1], rgb_n[mask == 0]])
    assert same_bits([d[mask == 1], d[mask == 0], op[mask == 0]], [t[mask == 1], depth[mask == 0], opacity[mask == 0]])
    assert (op[mask == 1] == 1.0).all()
    rgb, d, op, mask = ops.mixed_compose_host("clip", rgb_n, depth, opacity, tri, t, rgb_m, 0.5, 1.0)
    assert np.array_equal(mask, (tri >= 0).astype(np.uint8)) and (op[tri >= 0] == 1.0).all()
    assert same_bits([d[tri < 0], op[tri < 0]], [depth[tri < 0], opacity[tri < 0]])


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_mesh_entry_points_validate_arguments_without_a_gpu(lib):
    """Every refusal of include/nerfhip.h's mesh section comes back before anything is launched or dereferenced: the pointers
    below are null or fake."""
    null, fake, odd = None, 0x10000, 0x10004
    big = (1 << 28) + 1
    # build
    assert lib.nerfhip_mesh_bvh_keys(fake, 3, fake, -1, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_bvh_keys(fake, 3, fake, big, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_bvh_keys(fake, 1 << 31, fake, 1, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_bvh_keys(fake, 3, null, 1, fake, fake, null) == E_BADARG          # null triangles, T > 0
    assert lib.nerfhip_mesh_bvh_keys(null, 3, fake, 1, fake, fake, null) == E_BADARG          # null vertices, V > 0
    assert lib.nerfhip_mesh_bvh_keys(fake, 3, fake, 1, null, fake, null) == E_BADARG          # null keys
    assert lib.nerfhip_mesh_bvh_keys(fake, 3, fake, 1, fake, null, null) == E_BADARG          # null state
    assert lib.nerfhip_mesh_bvh_keys(fake, 3, fake, 1, odd, fake, null) == E_ALIGN            # keys: 8 bytes
    assert lib.nerfhip_mesh_bvh_keys_host(fake, 3, null, 1, fake, fake) == E_BADARG
    assert lib.nerfhip_mesh_bvh_boxes(fake, 3, fake, big, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_bvh_boxes(fake, 3, fake, 1, null, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_bvh_boxes(fake, 3, fake, 1, fake, null, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_bvh_boxes(fake, 3, fake, 1, fake, fake, null, null) == E_BADARG
    assert lib.nerfhip_mesh_bvh_boxes(fake, 3, fake, 1, fake, odd, fake, null) == E_ALIGN     # tris: 16 bytes
    assert lib.nerfhip_mesh_bvh_boxes(null, 0, null, 0, null, null, null, null) == 0          # T == 0: nothing to do
    assert lib.nerfhip_mesh_bvh_boxes_host(fake, 3, fake, 1, fake, fake, null) == E_BADARG
    # cast
    assert lib.nerfhip_mesh_cast(fake, -1, fake, fake, 1, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_cast(fake, (1 << 30) + 1, fake, fake, 1, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_cast(fake, 4, fake, fake, big, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_cast(null, 4, fake, fake, 1, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_cast(fake, 4, null, fake, 1, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_cast(fake, 4, fake, null, 1, fake, fake, fake, fake, null) == E_BADARG   # no boxes on the device
    assert lib.nerfhip_mesh_cast(fake, 4, fake, fake, 1, null, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_cast(odd, 4, fake, fake, 1, fake, fake, fake, fake, null) == E_ALIGN
    assert lib.nerfhip_mesh_cast(fake, 4, odd, fake, 1, fake, fake, fake, fake, null) == E_ALIGN
    assert lib.nerfhip_mesh_cast(null, 0, null, null, 0, null, null, null, null, null) == 0
    assert lib.nerfhip_mesh_cast_host(fake, 4, fake, null, 1, 0, fake, fake, fake, fake) == E_BADARG
    assert lib.nerfhip_mesh_cast_host(null, 4, fake, null, 1, 1, fake, fake, fake, fake) == E_BADARG
    # shade
    assert lib.nerfhip_mesh_shade(fake, 4, fake, fake, fake, fake, 3, fake, 1, null, 1.5, 0.0, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_shade(fake, 4, fake, fake, fake, fake, 3, fake, 1, null, 0.5, float("nan"), fake, null) == E_BADARG
    assert lib.nerfhip_mesh_shade(fake, 4, null, fake, fake, fake, 3, fake, 1, null, 0.5, 0.0, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_shade(fake, 4, fake, fake, fake, fake, 3, fake, 1, null, 0.5, 0.0, null, null) == E_BADARG
    assert lib.nerfhip_mesh_shade(fake, 4, fake, fake, fake, null, 3, fake, 1, null, 0.5, 0.0, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_shade(fake, 4, fake, fake, fake, fake, 3, fake, 1, null, 0.5, 0.0, fake + 2, null) == E_ALIGN
    assert lib.nerfhip_mesh_shade(null, 0, null, null, null, null, 0, null, 0, null, 0.5, 0.0, null, null) == 0
    assert lib.nerfhip_mesh_shade_host(fake, -2, fake, fake, fake, fake, 3, fake, 1, null, 0.5, 0.0, fake) == E_BADARG
    # compose
    assert lib.nerfhip_mixed_compose(2, 4, fake, fake, fake, fake, fake, fake, 0.5, 0.0, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mixed_compose(0, 4, fake, fake, fake, fake, fake, fake, 0.0, 0.0, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mixed_compose(0, 4, fake, fake, fake, fake, fake, fake, float("inf"), 0.0, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mixed_compose(1, 4, fake, null, fake, fake, fake, fake, 0.5, 0.0, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mixed_compose(1, 4, fake, fake, fake, fake, fake, fake, 0.5, 0.0, fake, fake, null, fake, null) == E_BADARG
    assert lib.nerfhip_mixed_compose(1, 4, fake, fake, fake, fake, fake, fake, 0.5, 0.0, fake, fake + 1, fake, fake, null) == E_ALIGN
    assert lib.nerfhip_mixed_compose(1, 0, null, null, null, null, null, null, 0.5, 0.0, null, null, null, null, null) == 0
    assert lib.nerfhip_mixed_compose_host(0, -1, fake, fake, fake, fake, fake, fake, 0.5, 0.0, fake, fake, fake, fake) == E_BADARG
    assert lib.nerfhip_abi_version() == 3


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer, MixedRenderer
    v, t = R.icosphere(0)
    with pytest.raises(NerfHipError):
        ops.mesh_bvh_build(torch.from_numpy(v), torch.from_numpy(t))
    with pytest.raises(NerfHipError):
        MeshBVH(torch.from_numpy(v), torch.from_numpy(t))
    with pytest.raises(NerfHipError):
        ops.mesh_cast(torch.zeros(4, 8), torch.zeros(20, 12), torch.zeros(6, 6))
    with pytest.raises(NerfHipError):
        ops.mesh_shade(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int32), torch.zeros(4), torch.zeros(4), torch.from_numpy(v),
                       torch.from_numpy(t))
    with pytest.raises(NerfHipError):
        ops.mixed_compose("ztest", torch.zeros(4, 3), torch.zeros(4), torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4),
                          torch.zeros(4, 3))
    with pytest.raises(ValueError):
        ops.mixed_compose_host("blend", *compose_inputs(8))
    with pytest.raises(ValueError):
        ops.mesh_cast_host(R.pinhole(), np.zeros((20, 12), np.float32), np.zeros((5, 6), np.float32))
    with pytest.raises(ValueError):
        MeshRenderer(None, True, ambient=2.0)

    class White:
        white_back = True

        def __call__(self, rays):
            raise AssertionError("never rendered")
    with pytest.raises(ValueError):
        MixedRenderer(White(), None, True, mode="clip")
    with pytest.raises(ValueError):
        MixedRenderer(White(), None, True, mode="blend")


# --------------------------------------------------------------------------------------------------- optional outputs left out
def aligned(a):
    """a copy of `a` whose data is 16-byte aligned, as the entry points want rays and triangles"""
    buf = np.empty(a.nbytes + 16, np.uint8)
    off = (-buf.ctypes.data) & 15
    out = buf[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def null_output_rays(n):
    """n rays from the camera towards seeded points within 0.4 of the centres of soup5's triangles (about half of them hit), the
    last one a NaN row"""
    v, t = R.soup(5)
    rng = np.random.default_rng(29)
    target = v[t].mean(1)[np.arange(n) % 5] + rng.uniform(-0.4, 0.4, (n, 3))
    rays = R._rows(np.array(R.CAMERA)[None], target - np.array(R.CAMERA), 0.0, 100.0)
    rays[-1, 4] = np.nan
    return aligned(rays)


CAST_NULLS = ((1,), (2,), (3,), (1, 2, 3))                 # of (tri, t, b1, b2): each optional output alone, then all three


def test_null_optional_outputs_of_cast_and_compose(lib):
    """t, b1 and b2 of the cast and the mask of compose may be null: what is supplied keeps the bits of the full call.  soup5 is
    the smallest hierarchy with an inner node: two leaves and a root."""
    from nerf_pl_amd import ops
    _, _, (tris, boxes, _, _) = built("soup5")
    assert tris.shape == (5, 12) and boxes.shape == (3, 6)
    rays = null_output_rays(65)
    n = len(rays)
    full = ops.mesh_cast_host(rays, tris, boxes)
    assert (full[0] >= 0).any() and (full[0] < 0).any() and full[0][-1] == -1

    def p(a):
        return None if a is None else a.ctypes.data
    for nulls in CAST_NULLS:
        out = [np.full(n, -7, np.int32)] + [np.full(n, np.nan, np.float32) for _ in range(3)]
        args = [None if k in nulls else out[k] for k in range(4)]
        assert lib.nerfhip_mesh_cast_host(p(rays), n, p(tris), p(boxes), 5, 0, *[p(a) for a in args]) == 0
        assert same_bits([a for a in args if a is not None], [full[k] for k in range(4) if k not in nulls]), nulls
    inputs = compose_inputs(n)
    for mode in ("ztest", "clip"):
        want = ops.mixed_compose_host(mode, *inputs, tau=0.5, background=1.0)
        assert want[3].any() and not want[3].all()
        out = [np.full((n, 3), np.nan, np.float32), np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)]
        assert lib.nerfhip_mixed_compose_host(ops.MIXED_MODES[mode], n, *[p(a) for a in inputs], 0.5, 1.0, *[p(a) for a in out], None) == 0
        assert same_bits(out, want[:3]), mode

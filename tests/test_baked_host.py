"""CPU: the baked-volume march through its host twin (nerfhip_baked_render_host: the kernel's own per-ray routine,
csrc/baked_core.h) against the float64 restatement of tests/baked_ref.py, and the brick layout and the cell-brick bitfield
of nerf_pl_amd.baked against the same file's loops.  Fails on a library without the nerfhip_baked_* entry points.

Tolerance against float64 (a derived cap, not an expected error): each of a ray's K samples carries a lattice coordinate of
magnitude up to N with about four fp32 roundings and a voxel-to-voxel gradient of up to 1, so |rgb| and |opacity| errors are at
most K_max N 2^-22 and the depth error that times the ray's far; K_max is the largest number of segments of a ray of the
fixture.  Every test prints the largest error it saw next to its cap.

One fixture sits on the edge of that cap: N = 9, random lattice, step 8 reaches 0.92 of it (3.9e-6 of 4.3e-6).  K_max is 2
there, one segment spans the lattice, and a rounding of `a` is multiplied by up to e = 8 in the exponent.  A host libm whose exp2f / log2f round differently by an ulp can move this figure; the bound is the
issue's and stays."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baked_ref as R  # noqa: E402

E_BADARG = -1


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


_BRICKED = {}


def bricked(kind, N):
    """(dense, bricked bytes, bitfield words) of a fixture volume, made once."""
    from nerf_pl_amd import baked
    if (kind, N) not in _BRICKED:
        dense = R.volume(kind, N)
        _BRICKED[kind, N] = (dense, baked.bricks_from_dense_host(dense), baked.brick_bits_host(dense))
    return _BRICKED[kind, N]


def host(rays, kind, N, step, skip=True, t_stop=0.0, white_back=False):
    from nerf_pl_amd import ops
    _, data, bits = bricked(kind, N)
    return ops.baked_render_host(rays, data, bits if skip else None, N, R.RANGES, R.cell_of(N), step, t_stop, white_back)


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def check_cap(got, ref, rays, N, what):
    """The module docstring's cap; returns (largest colour / opacity error, cap)."""
    rgb, depth, opacity = got
    cap = float(max(int(ref["K"].max()), 1)) * N * 2.0 ** -22
    e_rgb = np.abs(rgb - ref["rgb"]).max()
    e_op = np.abs(opacity - ref["opacity"]).max()
    far = np.where(np.isfinite(rays[:, 7]), np.abs(rays[:, 7]), 0.0).astype(np.float64)
    e_depth = np.abs(depth - ref["depth"])
    print("%s: K_max %d  rgb %.3g  opacity %.3g  depth/far %.3g  cap %.3g"
          % (what, int(ref["K"].max()), e_rgb, e_op, (e_depth / np.maximum(far, 1e-30))[far > 0].max(), cap))
    assert e_rgb <= cap, (what, e_rgb, cap)
    assert e_op <= cap, (what, e_op, cap)
    assert (e_depth <= cap * far).all(), (what, e_depth.max(), cap)
    return max(e_rgb, e_op), cap


# ------------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("N", [2, 8, 9, 17])
def test_brick_layout_and_bitfield(N):
    from nerf_pl_amd import baked, ops
    for kind in ("random", "voxel", "zero"):
        dense = R.volume(kind, N)
        data = baked.bricks_from_dense_host(dense)
        assert data.dtype == np.uint8 and data.size == ops.baked_bytes(N) == (-(-N // 8)) ** 3 * 2048
        assert np.array_equal(data, R.bricks_from_dense(dense)), (kind, N)
        assert np.array_equal(baked.dense_from_bricks_host(data, N), dense)
        bits = baked.brick_bits_host(dense)
        assert bits.dtype == np.int32 and bits.size == ops.baked_brick_words(N)
        assert np.array_equal(bits, R.brick_bits(dense)), (kind, N)
    assert not baked.brick_bits_host(R.volume("zero", N)).any()


def test_byte_offsets_by_hand(lib):
    from nerf_pl_amd import baked
    N = 9                                                  # NB = 2
    dense = np.zeros((N, N, N, 4), np.uint8)
    dense[3, 1, 4] = (1, 2, 3, 4)                          # brick 0, local (3 * 8 + 1) * 8 + 4 = 204: byte 816
    dense[8, 8, 8] = (5, 6, 7, 8)                          # brick (1 * 2 + 1) * 2 + 1 = 7, local 0: byte 7 * 2048
    dense[0, 8, 1] = (9, 10, 11, 12)                       # brick (0 * 2 + 1) * 2 + 0 = 2, local 1: byte 2 * 2048 + 4
    data = baked.bricks_from_dense_host(dense)
    assert data[816:820].tolist() == [1, 2, 3, 4]
    assert data[14336:14340].tolist() == [5, 6, 7, 8]
    assert data[4100:4104].tolist() == [9, 10, 11, 12]
    assert int(np.count_nonzero(data)) == 12
    assert R.point_offset(9, 3, 1, 4) == 816
    assert lib.nerfhip_baked_bytes(9) == 8 * 2048 and lib.nerfhip_baked_bytes(512) == 512 * 1024 * 1024
    assert lib.nerfhip_baked_bytes(1) == 0 and lib.nerfhip_baked_bytes(1626) == 0
    # the bitfield: N = 17 has 2^3 cell bricks; a voxel on the plane both bricks of an axis touch sets both
    d17 = np.zeros((17, 17, 17, 4), np.uint8)
    d17[8, 0, 16, 3] = 1                                   # iy = 8: by 0 and 1; ix = 0: bx 0; iz = 16: bz 1 -> bricks 1 and 5
    assert baked.brick_bits_host(d17).view(np.uint32).tolist() == [(1 << 1) | (1 << 5)]


# ----------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("step", R.STEPS, ids=["step%g" % s for s in R.STEPS])
@pytest.mark.parametrize("N", R.LATTICES)
def test_march_against_fp64(lib, N, step):
    rays = R.rays(N)
    assert 900 <= len(rays) <= 1100
    worst = 0.0
    for i, kind in enumerate(R.VOLUMES):
        white = bool(i & 1)
        dense = bricked(kind, N)[0]
        ref = R.render(rays, dense, R.RANGES, R.cell_of(N), step, white_back=white)
        assert ref["live"].sum() > len(rays) // 2 and not ref["live"].all()
        got = host(rays, kind, N, step, white_back=white)
        err, cap = check_cap(got, ref, rays, N, "N%d %s step %g" % (N, kind, step))
        worst = max(worst, err / cap)
        # skipping is invisible bit for bit
        assert same_bits(got, host(rays, kind, N, step, skip=False, white_back=white)), (kind, N, step)
        # the NaN row and the zero-direction row are background
        for row in (-1, -2):
            assert got[0][row].tolist() == [float(white)] * 3 and got[1][row] == 0.0 and got[2][row] == 0.0
        if kind == "zero":                                 # exactly the background everywhere
            assert (got[0] == float(white)).all() and (got[1] == 0.0).all() and (got[2] == 0.0).all()
        elif N > 2 or kind != "shell":                     # (the shell has no point on a 2^3 lattice)
            assert got[2].max() > 0.05, (kind, N, step)
    print("largest error / cap: %.3g" % worst)


@pytest.mark.parametrize("N", R.LATTICES)
def test_uniform_volume_closed_form(lib, N):
    """opacity = 1 - (1 - a)^(L |d| / cell) whatever the step and the lattice; tolerance K_max 2^-21."""
    rays = R.rays(N)
    r64 = rays.astype(np.float64)
    L = R.chord_length(rays)
    with np.errstate(invalid="ignore"):
        dn = np.sqrt((r64[:, 3:6] ** 2).sum(1))
    want = np.where(L > 0, 1.0 - (1.0 - 140.0 / 255.0) ** (L * np.where(np.isfinite(dn), dn, 0.0) / R.cell_of(N)), 0.0)
    for step in R.STEPS:
        k_max = np.ceil((L * np.nan_to_num(dn) / (step * R.cell_of(N))).max())
        tol = max(k_max, 1.0) * 2.0 ** -21
        _, _, opacity = host(rays, "uniform", N, step)
        err = np.abs(opacity - want).max()
        print("N%d step %g: closed form error %.3g, tolerance %.3g" % (N, step, err, tol))
        assert err <= tol, (N, step, err, tol)


def test_ranges_that_are_not_fp32_exact(lib):
    """+-1.2 is no float32: the entry point marches the box of the rounded ends, and so does the reference.  Origins exactly on
    a face of that box, with a zero direction component along its axis, are inside (rule 2) for both."""
    from nerf_pl_amd import baked, ops
    N, ranges = 9, ((-1.2, 1.2),) * 3
    cell = R.cell_of(N, ranges)
    dense = R.volume("random", N)
    face = float(np.float32(1.2))
    on_face = np.array([[face, 0.1, -3.0, 0.0, 0.0, 1.0, 0.0, 20.0], [-face, 0.3, 3.0, -0.0, 0.0, -0.7, 0.0, 20.0],
                        [0.2, face, -3.0, 0.0, -0.0, 1.5, 0.0, 20.0], [-3.0, -0.4, -face, 1.0, 0.0, 0.0, 0.0, 20.0]], np.float32)
    rays = np.concatenate([on_face, R.rays(N, n_main=200, ranges=ranges)])
    got = ops.baked_render_host(rays, baked.bricks_from_dense_host(dense), baked.brick_bits_host(dense), N, ranges, cell, 0.5)
    ref = R.render(rays, dense, ranges, cell, 0.5)
    assert ref["live"][:4].all() and (ref["opacity"][:4] > 0.05).all() and (got[2][:4] > 0.05).all()
    check_cap(got, ref, rays, N, "N9 random step 0.5, ranges +-1.2")


# -------------------------------------------------------------------------------------------------------------- exact checks
@pytest.mark.parametrize("N", [9, 33])
def test_batch_equals_its_halves(lib, N):
    rays = R.rays(N)
    h = len(rays) // 2 + 1
    for kind in ("shell", "random"):
        whole = host(rays, kind, N, 0.5, white_back=True)
        a, b = host(rays[:h], kind, N, 0.5, white_back=True), host(rays[h:], kind, N, 0.5, white_back=True)
        assert same_bits(whole, [np.concatenate([x, y]) for x, y in zip(a, b)])


@pytest.mark.parametrize("N", [9, 17, 33])
def test_t_stop(lib, N):
    """Stopping at T < 1e-2 loses at most 1e-2 of weight: the difference to the full march is below that plus the fp32 cap."""
    rays = R.rays(N)
    step = 0.5
    differs = False
    for kind in ("uniform", "shell", "random"):
        ref = R.render(rays, bricked(kind, N)[0], R.RANGES, R.cell_of(N), step)
        cap = float(ref["K"].max()) * N * 2.0 ** -22
        full = host(rays, kind, N, step)
        cut = host(rays, kind, N, step, t_stop=1e-2)
        assert np.abs(cut[0] - full[0]).max() <= 1e-2 + cap
        assert np.abs(cut[2] - full[2]).max() <= 1e-2 + cap
        far = np.nan_to_num(np.abs(rays[:, 7])).astype(np.float64)
        assert (np.abs(cut[1] - full[1]) <= (1e-2 + cap) * far).all()
        assert (cut[2] <= full[2]).all()
        differs = differs or not same_bits(cut, full)
        assert same_bits(cut, host(rays, kind, N, step, t_stop=1e-2, skip=False))
        # and the stopped march is the float64 one stopped by the same rule, up to rays whose T passes within the cap of t_stop
        ref_cut = R.render(rays, bricked(kind, N)[0], R.RANGES, R.cell_of(N), step, t_stop=1e-2)
        assert np.abs(cut[2] - ref_cut["opacity"]).max() <= 1e-2 + cap
    assert differs                                         # the rule did stop some ray early


# ---------------------------------------------------------------------------------------------------------- argument checks
def test_every_refusal_returns_badarg(lib):
    rg = (ctypes.c_float * 6)(-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)

    def call(fn, N=9, ranges=rg, cell=0.25, step=0.5, t_stop=0.0, n=5):
        tail = () if fn is lib.nerfhip_baked_render_host else (None,)
        return fn(None, n, None, None, N, ranges, cell, step, t_stop, 0, None, None, None, *tail)

    for fn in (lib.nerfhip_baked_render_host, lib.nerfhip_baked_render):
        assert call(fn, n=0) == 0                                                       # n == 0 succeeds, null pointers and all
        assert call(fn) == E_BADARG                                                     # null rays / data with n > 0
        assert call(fn, N=1, n=0) == E_BADARG and call(fn, N=0, n=0) == E_BADARG and call(fn, N=-4, n=0) == E_BADARG
        assert call(fn, N=1626, n=0) == E_BADARG and call(fn, N=1625, n=0) == 0         # N^3 >= 2^32
        for bad in ([1.0, -1.0, -1.0, 1.0, -1.0, 1.0], [-1.0, 1.0, 2.0, 2.0, -1.0, 1.0], [-1.0, 1.0, -1.0, 1.0, float("nan"), 1.0],
                    [-1.0, float("inf"), -1.0, 1.0, -1.0, 1.0], [float("-inf"), 1.0, -1.0, 1.0, -1.0, 1.0]):
            assert call(fn, ranges=(ctypes.c_float * 6)(*bad), n=0) == E_BADARG, bad
        assert call(fn, ranges=None, n=0) == E_BADARG
        for cell in (0.0, -0.25, float("nan"), float("inf")):
            assert call(fn, cell=cell, n=0) == E_BADARG, cell
        for step in (0.0, 0.06, -1.0, 8.5, float("nan")):
            assert call(fn, step=step, n=0) == E_BADARG, step
        assert call(fn, step=1.0 / 16, n=0) == 0 and call(fn, step=8.0, n=0) == 0
        for t_stop in (-0.1, 1.0, 2.0, float("nan")):
            assert call(fn, t_stop=t_stop, n=0) == E_BADARG, t_stop
        assert call(fn, cell=1e-9, n=0) == E_BADARG                                     # a march of more than 2^20 segments
        assert call(fn, n=-1) == E_BADARG
    assert lib.nerfhip_baked_scatter(None, 4, 9, None, None, None) == E_BADARG
    assert lib.nerfhip_baked_scatter(None, 0, 1, None, None, None) == E_BADARG
    assert lib.nerfhip_baked_from_dense(None, 9, None, None) == E_BADARG
    assert lib.nerfhip_baked_bricks(None, 9, None, None) == E_BADARG


def test_python_wrappers_check_sizes(lib):
    from nerf_pl_amd import baked, ops
    from nerf_pl_amd._lib import NerfHipError
    import torch
    rays = R.rays(9)[:4]
    _, data, bits = bricked("random", 9)
    with pytest.raises(ValueError):
        ops.baked_render_host(rays, data[:-4], bits, 9, R.RANGES, 0.25)
    with pytest.raises(ValueError):
        ops.baked_render_host(rays, data, bits[:0], 9, R.RANGES, 0.25)
    with pytest.raises(ValueError):
        ops.baked_render_host(rays[:, :7], data, bits, 9, R.RANGES, 0.25)
    with pytest.raises(NerfHipError):                      # CPU tensors are refused, as everywhere
        ops.baked_from_dense(torch.zeros(9, 9, 9, 4, dtype=torch.uint8))
    with pytest.raises(NerfHipError):
        ops.baked_scatter(torch.zeros(3, 2, dtype=torch.int32), 9)
    with pytest.raises(NerfHipError):
        baked.BakedVolume(torch.zeros(ops.baked_bytes(9), dtype=torch.uint8), 9, R.RANGES)
    with pytest.raises(NerfHipError):
        ops.baked_render(torch.zeros(3, 8), torch.zeros(ops.baked_bytes(9), dtype=torch.uint8), None, 9, R.RANGES, 0.25)


# --------------------------------------------------------------------------------------------------- optional outputs left out
def aligned(a):
    """a copy of `a` whose data is 16-byte aligned, as the entry points want rays and the volume"""
    buf = np.empty(a.nbytes + 16, np.uint8)
    off = (-buf.ctypes.data) & 15
    out = buf[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def null_output_case(n):
    """(rays, bricked volume, bitfield words, the C call's scalars after `words`) of the N = 9 random lattice — two bricks per
    axis — and n of its fixture's rays spread over all kinds, the zero-direction row included"""
    N = 9
    rays = R.rays(N)
    rays = aligned(rays[np.linspace(0, len(rays) - 1, n).astype(int)])
    _, data, bits = bricked("random", N)
    rg = (ctypes.c_float * 6)(*[v for r in R.RANGES for v in r])
    return rays, aligned(data), bits, (N, rg, R.cell_of(N), 0.5, 0.0, 1)


def test_null_optional_outputs_of_render(lib):
    """rgb, depth and opacity may each be null: the two that are supplied keep the bits of the full call."""
    from nerf_pl_amd import ops
    rays, data, bits, scalars = null_output_case(65)
    n = len(rays)
    full = ops.baked_render_host(rays, data, bits, 9, R.RANGES, R.cell_of(9), 0.5, 0.0, True)
    assert full[2].max() > 0.05 and (full[2] == 0).any()
    for skip in range(3):
        out = [np.full((n, 3), np.nan, np.float32), np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)]
        ptrs = [None if k == skip else out[k].ctypes.data for k in range(3)]
        assert lib.nerfhip_baked_render_host(rays.ctypes.data, n, data.ctypes.data, bits.ctypes.data, *scalars, *ptrs) == 0
        keep = [k for k in range(3) if k != skip]
        assert same_bits([out[k] for k in keep], [full[k] for k in keep]), skip

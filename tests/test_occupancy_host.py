"""CPU: the occupancy grid's cell rule, dilation and bit layout restated in numpy (tests/cull_ref.py) against the definition, and
the ray cull's host twin (nerfhip_cull_rays_host: the kernel's own per-ray routine, csrc/occupancy_core.h) against the fp64
every-box oracle of tests/cull_ref.py.  Fails on a library without the occupancy entry points.

Per ray, with no exclusions: hit_must => hit; not hit_may => not hit; for hit_must rays
    T0(inflated) - 4 ulp <= t0 <= T0(shrunk) + 4 ulp,   T1(shrunk) - 4 ulp <= t1 <= T1(inflated) + 4 ulp
(near and far folded into every T; ulp = fp32 spacing at the bound); for rays that are hit_may but not hit_must either verdict
stands, and a hit has near <= t0 < t1 <= far.  Such rays are at most 1 % of each generic batch: a condition on the inputs,
checked here."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cull_ref as R  # noqa: E402

E_BADARG, E_ALIGN = -1, -3
SEED = 20240


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


GRIDS = R.grids()


# ------------------------------------------------------------------------------------------------- cell rule, dilation, bits
@pytest.mark.parametrize("N", [2, 6, 34])
def test_cell_rule_and_dilation_restatement(N):
    sigma, thr = R.sigma_fixture(N)
    M = N - 1
    occ = R.cells_from_sigma(sigma, thr)
    # the rule from its words: any of the 8 corners > threshold, NaN counts
    want = np.zeros((M, M, M), bool)
    for iy, ix, iz in np.ndindex(M, M, M):
        c = sigma[iy:iy + 2, ix:ix + 2, iz:iz + 2]
        want[iy, ix, iz] = bool(np.any(c > thr) or np.any(np.isnan(c)))
    assert np.array_equal(occ, want)
    if N == 2:
        assert not occ.any()                               # the one value equal to the threshold does not count
    else:
        c = N // 2
        assert not occ[c - 1:c + 1, 0:2, N - 3:N - 1].any()        # around the value equal to the threshold
        assert occ[0:2, N - 3:N - 1, c - 1:c + 1].all()            # around the NaN
    for r in (0, 1, 2, 40):
        got = R.dilate(occ, r)
        assert np.array_equal(got, R.dilate_brute(occ, r)), r
        if r >= M and occ.any():
            assert got.all()
        assert np.array_equal(R.unpack_bits(R.pack_bits(got), M), got)


def test_bit_layout():
    M = 5
    occ = np.zeros((M, M, M), bool)
    occ[3, 1, 4] = True                                    # c = (3 * 5 + 1) * 5 + 4 = 84: word 2, bit 20
    occ[4, 4, 4] = True                                    # c = 124: word 3, bit 28; bits 29 .. 31 stay zero
    w = R.pack_bits(occ).view(np.uint32)
    assert w.tolist() == [0, 0, 1 << 20, 1 << 28]
    assert R.pack_bits(np.ones((M, M, M), bool)).view(np.uint32)[-1] == (1 << 29) - 1


# --------------------------------------------------------------------------------------------------------------- generic rays
def _cull(grid, rays):
    from nerf_pl_amd import ops
    return ops.cull_rays_host(rays, grid.words, grid.M, grid.ranges)


def check_against_oracle(grid, rays, hit, t0, t1):
    """The per-ray conditions of the module docstring; returns the number of rays that are hit_may but not hit_must."""
    o = R.oracle(grid, rays)
    hit = hit.astype(bool)
    near, far = rays[:, 6].astype(np.float64), rays[:, 7].astype(np.float64)
    t0, t1 = t0.astype(np.float64), t1.astype(np.float64)
    assert not np.isnan(t0).any() and not np.isnan(t1).any()
    must, may = o["hit_must"], o["hit_may"]
    assert not (must & ~may).any()
    bad = np.flatnonzero(must & ~hit)
    assert bad.size == 0, (grid.name, "must-hit rays reported as misses", bad[:5], rays[bad[:5]])
    bad = np.flatnonzero(~may & hit)
    assert bad.size == 0, (grid.name, "rays that pierce no inflated box reported as hits", bad[:5], rays[bad[:5]])
    m = must
    for name, got, lo, hi in (("t0", t0, o["T0_inflated"], o["T0_shrunk"]), ("t1", t1, o["T1_shrunk"], o["T1_inflated"])):
        low = lo[m] - 4 * R.ulp32(lo[m])
        high = hi[m] + 4 * R.ulp32(hi[m])
        bad = np.flatnonzero((got[m] < low) | (got[m] > high))
        assert bad.size == 0, (grid.name, name, got[m][bad[:5]], low[bad[:5]], high[bad[:5]], rays[m][bad[:5]])
    h = hit
    assert (near[h] <= t0[h]).all() and (t0[h] < t1[h]).all() and (t1[h] <= far[h]).all(), grid.name
    return int((may & ~must).sum())


@pytest.mark.parametrize("grid", GRIDS, ids=[g.name for g in GRIDS])
def test_generic_rays(lib, grid):
    rays = R.generic_rays(grid, SEED + grid.M)
    assert 200 <= len(rays) <= 400
    signs = {tuple(np.sign(r[3:6]).astype(int)) for r in rays}
    assert len(signs) == 8                                 # every sign combination of d
    hit, t0, t1 = _cull(grid, rays)
    undecided = check_against_oracle(grid, rays, hit, t0, t1)
    assert undecided <= len(rays) // 100, (grid.name, undecided)     # the condition on the inputs
    if grid.occ.any():
        assert hit.any() and not hit.all(), grid.name       # the batch exercises both verdicts
    else:
        assert not hit.any()


def test_blobs_interval_spans_the_gap(lib):
    """A ray through both blobs along the grid's diagonal: one interval from the first blob's entry to the second one's exit."""
    grid = next(g for g in GRIDS if g.name == "M33-blobs")
    o = np.array([-2.0, -1.75, -2.0])
    d = np.array([1.0, 0.8333333, 1.0])
    rays = np.concatenate([o, d, [0.0, 10.0]])[None].astype(np.float32)
    hit, t0, t1 = _cull(grid, rays)
    res = R.oracle(grid, rays)
    assert res["hit_must"][0] and hit[0]
    assert t1[0] - t0[0] > 1.2                              # the blobs' centres are 1.2 apart in t
    check_against_oracle(grid, rays, hit, t0, t1)


# ----------------------------------------------------------------------------------------------------------- degenerate rays
@pytest.mark.parametrize("grid", GRIDS, ids=[g.name for g in GRIDS])
def test_degenerate_rays(lib, grid):
    rays, nonfinite = R.degenerate_rays(grid)
    hit, t0, t1 = _cull(grid, rays)
    fin = ~nonfinite
    assert not np.isnan(t0[fin]).any() and not np.isnan(t1[fin]).any()
    h = hit.astype(bool) & fin
    assert (rays[h, 6] <= t0[h]).all() and (t1[h] <= rays[h, 7]).all() and (t0[h] < t1[h]).all()
    # non-finite rays come back as hits with their own bounds (bit for bit, NaN included)
    assert hit[nonfinite].all()
    assert np.array_equal(t0[nonfinite].view(np.uint32), rays[nonfinite, 6].view(np.uint32))
    assert np.array_equal(t1[nonfinite].view(np.uint32), rays[nonfinite, 7].view(np.uint32))
    if grid.name.endswith("ones"):
        # axis-parallel rays through the box's interior hit a full grid, whatever the sign of their zeros
        inside = np.array([all(lo < r[a] < hi for a, (lo, hi) in enumerate(grid.ranges) if r[3 + a] == 0) for r in rays])
        axis_parallel = (np.count_nonzero(rays[:, 3:6], axis=1) == 1) & fin
        assert hit[axis_parallel & inside].all()
    if grid.name.endswith("zeros"):
        assert not hit[fin].any()


# ----------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks(lib):
    grid = GRIDS[3]                                        # M = 5
    rays = R.generic_rays(grid, 1)[:7].copy()
    n = len(rays)
    hit, t0, t1 = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32)
    rg = (ctypes.c_float * 6)(*[v for r in grid.ranges for v in r])
    words = grid.words.copy()
    p = lambda a: a.ctypes.data  # noqa: E731
    call = lib.nerfhip_cull_rays_host
    assert call(p(rays), n, p(words), grid.M, rg, p(hit), p(t0), p(t1)) == 0
    assert call(None, 0, p(words), grid.M, rg, None, None, None) == 0                    # n == 0 succeeds
    for args in ((None, n, p(words), grid.M, rg, p(hit), p(t0), p(t1)),
                 (p(rays), n, None, grid.M, rg, p(hit), p(t0), p(t1)),
                 (p(rays), n, p(words), grid.M, None, p(hit), p(t0), p(t1)),
                 (p(rays), n, p(words), grid.M, rg, None, p(t0), p(t1)),
                 (p(rays), n, p(words), grid.M, rg, p(hit), None, p(t1)),
                 (p(rays), n, p(words), grid.M, rg, p(hit), p(t0), None),
                 (p(rays), -1, p(words), grid.M, rg, p(hit), p(t0), p(t1)),
                 (p(rays), n, p(words), 0, rg, p(hit), p(t0), p(t1)),                    # M < 1
                 (p(rays), n, p(words), -3, rg, p(hit), p(t0), p(t1))):
        assert call(*args) == E_BADARG, args
    for bad in ([1.0, -1.0, -1.0, 1.0, -1.0, 1.0], [-1.0, 1.0, 2.0, 2.0, -1.0, 1.0], [-1.0, 1.0, -1.0, 1.0, float("nan"), 1.0],
                [-1.0, float("inf"), -1.0, 1.0, -1.0, 1.0]):                             # inverted, empty, not finite
        assert call(p(rays), n, p(words), grid.M, (ctypes.c_float * 6)(*bad), p(hit), p(t0), p(t1)) == E_BADARG, bad
    # a misaligned words pointer
    raw = np.zeros(words.nbytes + 8, np.uint8)
    base = p(raw) + (-p(raw)) % 4
    assert call(p(rays), n, base + 1, grid.M, rg, p(hit), p(t0), p(t1)) == E_ALIGN
    assert call(p(rays), n, base + 2, grid.M, rg, p(hit), p(t0), p(t1)) == E_ALIGN
    # the device entry point checks the same way before it launches anything (no GPU is touched by a refused call)
    assert lib.nerfhip_cull_rays(p(rays), n, p(words), 0, rg, p(hit), p(t0), p(t1), None) == E_BADARG
    assert lib.nerfhip_cull_rays(p(rays), n, base + 2, grid.M, rg, p(hit), p(t0), p(t1), None) == E_ALIGN
    assert lib.nerfhip_occupancy_workspace_bytes(1) == 0 and lib.nerfhip_occupancy_workspace_bytes(34) >= 2 * 33 ** 3
    assert lib.nerfhip_occupancy_build(None, 6, 1.0, 0, None, None, None) == E_BADARG


def test_python_wrapper_refuses_short_bitfield(lib):
    from nerf_pl_amd import ops
    grid = GRIDS[3]
    with pytest.raises(ValueError):
        ops.cull_rays_host(np.zeros((1, 8), np.float32), grid.words[:-1], grid.M, grid.ranges)

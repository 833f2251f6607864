"""GPU: the Unity volume file — csrc/volume.hip (nerfhip_vol_pack) against the numpy restatement of the notebook
(test_volume_host.vol_ref), the full-network lattice query against the CPU reference network, and export_vol end to end.

The device rounds the fp64 exponential once; numpy's float32 exp may differ from that by an ulp.  Records are therefore compared
byte for byte except at the `fragile` points (test_volume_host.fragile: at most 0.1 % of the sigma > 0 points of every input
used here, asserted there), where membership and the A byte (by 1) may differ."""
import numpy as np
import pytest
import torch

from helpers import O, build_arch_models, build_models
from test_volume_host import (E2E_N, E2E_RANGES, N_CELL, PACK_SIZES, XMAX, XMIN, e2e_reference, fragile, kept_all_input, pack_input,
                              vol_ref)

pytestmark = pytest.mark.gpu
CELL = (XMAX - XMIN) / N_CELL
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def packed_input():
    x = pack_input()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def e2e():
    return e2e_reference()


def u32(records):
    assert records.dtype == torch.int32 and records.dim() == 2 and records.shape[1] == 2
    return records.cpu().numpy().view(np.uint32)


def dense(records, n, first=0):
    """(kept (n,) bool, word (n,) uint32) of (K, 2) uint32 records of the points first .. first+n-1, in strictly increasing order"""
    idx = records[:, 0].astype(np.int64) - first
    assert ((idx >= 0) & (idx < n)).all() and (np.diff(idx) > 0).all()
    kept, word = np.zeros(n, bool), np.zeros(n, np.uint32)
    kept[idx], word[idx] = True, records[:, 1]
    return kept, word


def assert_records_match(got, x, N=N_CELL, xmin=XMIN, xmax=XMAX, first=0):
    n = x.shape[0]
    kg, wg = dense(got, n, first)
    kr, wr = dense(vol_ref(x, N, xmin, xmax, first), n, first)
    frag = fragile(x, N, xmin, xmax)
    assert np.array_equal(kg[~frag], kr[~frag]), "membership differs outside the fragile set"
    both = kg & kr
    assert np.array_equal(wg[both & ~frag], wr[both & ~frag]), "bytes differ outside the fragile set"
    f = both & frag
    assert np.array_equal(wg[f] >> 8, wr[f] >> 8)
    assert (np.abs((wg[f] & 255).astype(np.int64) - (wr[f] & 255).astype(np.int64)) <= 1).all()


def raw_pack(x, first, records, capacity, cursor):
    """One nerfhip_vol_pack call on the caller's own buffers."""
    from nerf_pl_amd import _lib
    lib = _lib.load()
    ws = torch.empty(lib.nerfhip_vol_workspace_bytes(x.shape[0]), device=x.device, dtype=torch.uint8)
    _lib.check(lib.nerfhip_vol_pack(_lib.ptr(x), x.shape[0], first, float(np.float32(-CELL)), _lib.ptr(ws), _lib.ptr(records), capacity,
                                    _lib.ptr(cursor), _lib.stream_ptr()), "nerfhip_vol_pack")
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_matches_the_notebook(dev, packed_input, n):
    from nerf_pl_amd.volume import vol_records
    x = packed_input[:n]
    got = u32(vol_records(torch.from_numpy(x.copy()).to(dev), CELL))
    assert_records_match(got, x)
    if n == PACK_SIZES[-1]:
        assert 0.1 * n < got.shape[0] < 0.3 * n
        shifted = u32(vol_records(torch.from_numpy(x.copy()).to(dev), CELL, first_index=2 ** 32 - n))    # the last indices of a uint32
        assert np.array_equal(shifted[:, 1], got[:, 1])
        assert np.array_equal(shifted[:, 0].astype(np.int64), got[:, 0].astype(np.int64) + 2 ** 32 - n)


def test_special_values(dev):
    """Expected bytes derived by hand, with cell = 2^-8 (c = -2^-8: c * sigma is exact for the densities below).
    exp(t) = 1 + t + t^2/2 - ... rounds to 1 - 2^-24 when it lies below the midpoint 1 - 2^-25, to 1 (ties to even) otherwise:
      sigma = 2^-17             t = -2^-25             exp = 1 - 2^-25 + 2^-51 -> 1        a = 0      dropped
      sigma = 2^-17 (1 + 2^-23) t = -2^-25 (1 + 2^-23) exp = 1 - 2^-25 - 2^-48 + .. -> 1 - 2^-24  a = 2^-24  kept, A = trunc(255 * 2^-24) = 0
    so the second is the smallest density that is kept.  1e-30: t = -3.9e-33, exp = 1, dropped.  -0.0, 0, NaN: dropped.
    +inf and 1e6 (t = -3906.25, exp underflows to 0): a = 1, A = 255.
    Colours: 0 -> 0, 1 -> 255, nextafter(1, 0) = 1 - 2^-24 -> 255 - 255 * 2^-24 rounds to 255 - 2^-16 (the float32 spacing there) ->
    254; k/255 and its neighbours: the correctly rounded float32 product (IEEE multiplication is the same everywhere), truncated."""
    from nerf_pl_amd.volume import vol_records
    f32 = np.float32
    below1 = np.nextafter(f32(1), f32(0))
    sig = [f32(-0.0), f32(0), f32(1e-30), f32(2.0 ** -17), np.nextafter(f32(2.0 ** -17), f32(1)), f32(np.inf), f32(np.nan), f32(1e6)]
    rows = [[0.0, 1.0, below1, s] for s in sig]
    expect = {4: 0 << 24 | 255 << 16 | 254 << 8 | 0, 5: 255 << 16 | 254 << 8 | 255, 7: 255 << 16 | 254 << 8 | 255}
    for k in (1, 127, 128, 254):
        v = f32(k / 255.0)
        trio = [np.nextafter(v, f32(0)), v, np.nextafter(v, f32(1))]
        b = [int(t * f32(255)) for t in trio]                       # float32 product, truncated
        assert all(t_ in (k - 1, k) for t_ in b) and b[0] <= b[1] <= b[2] == k      # the upper neighbour always reaches k
        expect[len(rows)] = b[0] << 24 | b[1] << 16 | b[2] << 8 | 255
        rows.append(trio + [f32(np.inf)])
    x = np.array(rows, np.float32)
    got = u32(vol_records(torch.from_numpy(x).to(dev), 2.0 ** -8))
    assert got.tolist() == [[i, expect[i]] for i in sorted(expect)]


def test_nothing_kept_writes_nothing(dev, packed_input):
    from nerf_pl_amd.volume import vol_records
    x = packed_input[:700].copy()
    x[:, 3] = -np.abs(x[:, 3])
    x[::7, 3] = 0.0
    x[::11, 3] = np.nan
    xd = torch.from_numpy(x).to(dev)
    assert tuple(vol_records(xd, CELL).shape) == (0, 2)
    records = torch.full((700, 2), SENTINEL, device=dev, dtype=torch.int32)
    cursor = torch.full((1,), 5, device=dev, dtype=torch.int64)
    raw_pack(xd, 0, records, 700, cursor)
    assert cursor.item() == 5 and bool((records == SENTINEL).all())


def test_everything_kept(dev):
    from nerf_pl_amd.volume import vol_records
    x = kept_all_input()
    got = u32(vol_records(torch.from_numpy(x).to(dev), CELL, first_index=3))
    assert got.shape[0] == x.shape[0] and got[:, 0].tolist() == list(range(3, 3 + x.shape[0]))
    assert_records_match(got, x, first=3)


def test_cursor_carries_across_calls(dev, packed_input):
    """A lattice packed in three calls (the middle one empty) through one device cursor == one call over the whole."""
    from nerf_pl_amd.volume import vol_records
    xd = torch.from_numpy(packed_input.copy()).to(dev)
    n, cut = xd.shape[0], 100001
    whole = vol_records(xd, CELL)
    records = torch.full((n, 2), SENTINEL, device=dev, dtype=torch.int32)
    cursor = torch.zeros(1, device=dev, dtype=torch.int64)
    raw_pack(xd[:cut], 0, records, n, cursor)
    first = cursor.item()
    raw_pack(xd[cut:cut], cut, records, n, cursor)
    assert cursor.item() == first
    raw_pack(xd[cut:], cut, records, n, cursor)
    K = cursor.item()
    assert 0 < first < K == whole.shape[0]
    assert torch.equal(records[:K], whole) and bool((records[K:] == SENTINEL).all())


def test_capacity_bounds_the_writes(dev, packed_input):
    """A buffer too small for the records: nothing lands at or beyond `capacity` (the guard behind it stays intact), the records
    below it are right, and the cursor reports what was needed."""
    from nerf_pl_amd.volume import vol_records
    xd = torch.from_numpy(packed_input[:5000].copy()).to(dev)
    whole = vol_records(xd, CELL)
    K, cap, guard = whole.shape[0], 300, 512
    assert K > 2 * cap
    buf = torch.full((cap + guard, 2), SENTINEL, device=dev, dtype=torch.int32)
    cursor = torch.zeros(1, device=dev, dtype=torch.int64)
    raw_pack(xd, 0, buf, cap, cursor)
    assert cursor.item() == K
    assert torch.equal(buf[:cap], whole[:cap]) and bool((buf[cap:] == SENTINEL).all())
    # a cursor that already stands beyond the capacity: nothing is written at all
    buf.fill_(SENTINEL)
    cursor.fill_(cap + 7)
    raw_pack(xd, 0, buf, cap, cursor)
    assert cursor.item() == cap + 7 + K and bool((buf == SENTINEL).all())


def _lattice(N, ranges):
    x, y, z = (np.linspace(lo, hi, N) for lo, hi in ranges)
    return torch.FloatTensor(np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3))


def test_rgbsigma_grid_matches_reference_lattice(dev):
    """rgbsigma_grid == the notebook's dense query: np.meshgrid 'xy' order, full network, zero view direction."""
    from nerf_pl_amd.volume import rgbsigma_grid
    p = O.make_params(51, 6.0, 0.3)
    (m,), _ = build_models([p], dev, "fp32")
    N, ranges = 9, ((-1.2, 1.2), (-1.0, 1.3), (-0.7, 1.1))
    xyz = _lattice(N, ranges)
    ref = O.mlp_forward(p, torch.cat([O.posenc(xyz, 10), O.posenc(torch.zeros_like(xyz), 4)], 1))
    got = rgbsigma_grid(m, N, *ranges)
    assert got.is_cuda and got.shape == (N ** 3, 4) and got.dtype == torch.float32
    assert torch.allclose(got.cpu(), ref, rtol=1e-4, atol=1e-5), (got.cpu() - ref).abs().max().item()
    # chunked launches == single launch (ragged last chunk)
    assert torch.equal(rgbsigma_grid(m, N, *ranges, points_per_launch=100), got)
    m.mlp_dtype = "bf16"
    gb = rgbsigma_grid(m, N, *ranges).cpu()
    assert bool(torch.isfinite(gb).all())
    for c in range(4):
        assert (gb[:, c] - ref[:, c]).abs().max().item() <= 3e-2 * max(1.0, ref[:, c].abs().max().item()), c


def test_rgbsigma_grid_non_default_vs_reference_network(dev):
    from nerf_pl_amd.volume import export_vol, rgbsigma_grid
    arch = O.make_arch(D=3, W=64, N_freq_xyz=4, N_freq_dir=1, skips=(2,))
    (m,), embs, (p,) = build_arch_models(arch, [81], dev, "fp32", 3.0, 0.1)
    N, ranges = 9, ((-1, 1), (-1.2, 1.2), (-0.8, 0.8))
    xyz = _lattice(N, ranges)
    ref = O.mlp_forward(p, torch.cat([O.posenc(xyz, 4), O.posenc(torch.zeros_like(xyz), 1)], 1), arch=arch)
    got = rgbsigma_grid(m, N, *ranges, embeddings=embs)
    assert torch.allclose(got.cpu(), ref, rtol=1e-4, atol=1e-5), (got.cpu() - ref).abs().max().item()
    assert torch.equal(rgbsigma_grid(m, N, *ranges, points_per_launch=100, embeddings=embs), got)
    for fn in (rgbsigma_grid, export_vol):
        with pytest.raises(ValueError):
            fn(m, N, *ranges)


def test_export_vol_end_to_end(dev, e2e, tmp_path):
    from nerf_pl_amd.volume import export_vol, read_vol, rgbsigma_grid, vol_records
    p, _, ref = e2e
    (m,), _ = build_models([p], dev, "fp32")
    N, (xr, yr, zr) = E2E_N, E2E_RANGES
    path = str(tmp_path / "scene.vol")
    rec = export_vol(m, N, xr, yr, zr, path=path)
    got = u32(rec)
    # (a) the device's own lattice output through the numpy pack; the chunking does not show
    own = rgbsigma_grid(m, N, xr, yr, zr)
    assert_records_match(got, own.cpu().numpy(), N, *xr)
    assert torch.equal(export_vol(m, N, xr, yr, zr, points_per_launch=100), rec)
    assert torch.equal(vol_records(own, (xr[1] - xr[0]) / N), rec)
    # (b) the CPU reference network through the numpy pack
    kg, wg = dense(got, N ** 3)
    kr, wr = dense(vol_ref(ref, N, *xr), N ** 3)
    assert 0.3 * N ** 3 < kr.sum() < 0.8 * N ** 3
    both = kg & kr
    for shift in (24, 16, 8, 0):
        d = ((wg[both] >> shift) & 255).astype(np.int64) - ((wr[both] >> shift) & 255).astype(np.int64)
        assert np.abs(d).max() <= 1, shift
    s = ref[kg != kr, 3]
    assert (np.abs(s) <= 1e-4 * np.maximum(1, np.abs(s))).all(), s
    # (c) the written file, read back
    with open(path, "rb") as f:
        assert f.read() == got.astype("<u4").tobytes()
    d = read_vol(path, N).reshape(-1, 4)
    assert np.array_equal(d[kg], np.stack([wg[kg] >> 24, (wg[kg] >> 16) & 255, (wg[kg] >> 8) & 255, wg[kg] & 255], -1).astype(np.uint8))
    assert not d[~kg].any()

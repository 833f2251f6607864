"""CPU: the Unity volume file (nerf_pl_amd/volume.py, csrc/volume.hip) — the numpy restatement of the notebook's pack that the GPU
tests compare with (`vol_ref`), the points at which that comparison cannot be exact (`fragile`), the seeded inputs of the GPU
tests with the condition they must satisfy, the file's round trip and refusals, and the argument checks of the C entry points.

extract_mesh.ipynb, cell "Generate .vol file for volume rendering in Unity":
    a = 1-np.exp(-(xmax-xmin)/N*sigma);  rgb = (rgbsigma[:, :3].numpy()*255).astype(np.uint32);  i = np.where(a>0)[0]
    s = rgb[i].dot([1<<24, 1<<16, 1<<8]) + (a[i]*255).astype(np.uint32);  res = np.stack([i, s], -1).astype(np.uint32)
"""
import numpy as np
import pytest
import torch

from helpers import O

# the lattice constants every pack test uses (the notebook's own: N = 512 on [-1.2, 1.2]); the pack itself is per point
N_CELL, XMIN, XMAX = 512, -1.2, 1.2
PACK_SEED = 7
PACK_SIZES = (1, 255, 256, 257, 256 * 1025 + 3)      # the last: ragged, 1026 block totals > one 1024-wide pass of the totals scan
KEPT_ALL_N, KEPT_ALL_SEED = 1000, 11
E2E_N, E2E_RANGES = 12, ((-1.2, 1.2), (-1.0, 1.3), (-0.7, 1.1))
# seeded random weights give an almost flat density (0.006 +- 0.003 for this seed): the gain and bias of the density head spread
# it to about 0.7 +- 5.7, half of the lattice kept, alpha bytes from 0 to above 200
E2E_SEED, E2E_SIGMA_GAIN, E2E_SIGMA_BIAS = 52, 2000.0, -11.0
MAX_FRAGILE_SHARE = 1e-3


def vol_ref(rgbsigma, N, xmin, xmax, first_index=0):
    """The notebook's records (K, 2) uint32 of a float32 (n, 4) array, in float32 numpy as the notebook computes them."""
    rgbsigma = np.asarray(rgbsigma, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sigma = np.maximum(rgbsigma[:, -1], 0)
        a = 1 - np.exp(-(xmax - xmin) / N * sigma)
        assert a.dtype == np.float32
        i = np.where(a > 0)[0]
        rgb = (rgbsigma[i, :3] * 255).astype(np.uint32)
        s = rgb.dot(np.array([1 << 24, 1 << 16, 1 << 8])) + (a[i] * 255).astype(np.uint32)
    return np.stack([i + first_index, s], -1).astype(np.uint32)


def fragile(rgbsigma, N, xmin, xmax):
    """(n,) bool: sigma > 0 and moving exp(t) by up to 2 float32 ulps either way changes the point's membership or its A byte.
    numpy's float32 exp is not correctly rounded, the device rounds the fp64 exponential: they may differ by an ulp."""
    sigma = np.asarray(rgbsigma, dtype=np.float32)[:, -1]
    one, f255 = np.float32(1), np.float32(255)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(-(xmax - xmin) / N) * np.maximum(sigma, 0)
        e0 = np.exp(t.astype(np.float64)).astype(np.float32)

        def outcome(e):
            a = one - e
            return np.where(a > 0, np.trunc(a * f255), -1.0)

        base = outcome(e0)
        differs = np.zeros(sigma.shape, dtype=bool)
        for toward in (np.float32(-np.inf), np.float32(np.inf)):
            e = e0
            for _ in range(2):
                e = np.nextafter(e, toward)
                differs |= outcome(e) != base
    return differs & (sigma > 0)


def fragile_share(rgbsigma, N, xmin, xmax):
    pos = int((np.asarray(rgbsigma)[:, -1] > 0).sum())
    return float(fragile(rgbsigma, N, xmin, xmax).sum()) / max(pos, 1)


def trained_like(n, seed):
    """(n, 4) float32 shaped like a trained field's output: 80 % of the densities negative (empty space), 4 % positive but so
    small that the point is kept with A == 0, 11 % moderate, 5 % large (A == 255); colours are sigmoid outputs."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    sigma = -np.abs(rng.normal(0, 5, n)) - 1e-3
    tiny = 10.0 ** rng.uniform(-3, -1, n)
    moderate = np.exp(rng.normal(3.0, 1.5, n))
    large = rng.uniform(2000, 20000, n)
    sigma = np.where(u < 0.80, sigma, np.where(u < 0.84, tiny, np.where(u < 0.95, moderate, large)))
    rgb = 1 / (1 + np.exp(-rng.normal(0, 2, (n, 3))))
    return np.concatenate([rgb, sigma[:, None]], 1).astype(np.float32)


def pack_input():
    return trained_like(PACK_SIZES[-1], PACK_SEED)


def kept_all_input():
    rng = np.random.default_rng(KEPT_ALL_SEED)
    return np.concatenate([rng.random((KEPT_ALL_N, 3)), rng.uniform(1, 100, (KEPT_ALL_N, 1))], 1).astype(np.float32)


def e2e_reference():
    """(params, lattice points (N^3, 3), the CPU reference network's rgbsigma (N^3, 4) numpy) of the end-to-end test."""
    p = O.make_params(E2E_SEED, E2E_SIGMA_GAIN, E2E_SIGMA_BIAS)
    x, y, z = (np.linspace(lo, hi, E2E_N) for lo, hi in E2E_RANGES)
    xyz = torch.FloatTensor(np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3))
    ref = O.mlp_forward(p, torch.cat([O.posenc(xyz, 10), O.posenc(torch.zeros_like(xyz), 4)], 1))
    return p, xyz, ref.numpy()


def test_vol_ref_on_hand_checked_points():
    # sigma = ln(2) / cell: a = 0.5 -> A = 127; sigma <= 0 dropped; rgb 0.5 -> 127, 1.0 -> 255, 0 -> 0
    cell = (XMAX - XMIN) / N_CELL
    x = np.array([[0.5, 1.0, 0.0, np.log(2) / cell], [0.1, 0.2, 0.3, 0.0], [0.1, 0.2, 0.3, -5.0], [1.0, 1.0, 1.0, 1e9],
                  [0.0, 0.0, 0.0, 0.01]], np.float32)
    rec = vol_ref(x, N_CELL, XMIN, XMAX, first_index=10)
    assert rec.dtype == np.uint32 and rec.tolist() == [[10, 127 << 24 | 255 << 16 | 127], [13, 0xffffffff], [14, 0]]
    assert not fragile(x, N_CELL, XMIN, XMAX)[[1, 2, 3, 4]].any()


def test_fragile_marks_the_membership_and_byte_boundaries():
    cell = (XMAX - XMIN) / N_CELL
    # t about -6e-8: exp rounds to 1 or to 1 - 2^-24 depending on the last ulp -> membership is fragile; far from it: not
    near_one = 6e-8 / cell
    x = np.array([[0, 0, 0, near_one], [0, 0, 0, 0.5], [0, 0, 0, 300.0], [0, 0, 0, -1.0]], np.float32)
    assert fragile(x, N_CELL, XMIN, XMAX).tolist() == [True, False, False, False]
    # a * 255 crosses 128 at sigma = -ln(1 - 128/255) / cell: one float32 step of sigma moves exp(t) by about an ulp, so of the
    # 41 densities around the crossing a handful (and only a handful) are fragile, and A is 127 below them and 128 above
    s = np.float32(-np.log(1 - 128.0 / 255.0) / cell)
    lo = s
    for _ in range(20):
        lo = np.nextafter(lo, np.float32(0))
    sig = [lo]
    for _ in range(40):
        sig.append(np.nextafter(sig[-1], np.float32(np.inf)))
    y = np.zeros((41, 4), np.float32)
    y[:, 3] = sig
    f = fragile(y, N_CELL, XMIN, XMAX)
    assert 1 <= f.sum() <= 12 and not f[0] and not f[-1]
    a = vol_ref(y, N_CELL, XMIN, XMAX)[:, 1] & 255
    assert a[0] == 127 and a[-1] == 128


def test_gpu_test_inputs_are_almost_nowhere_fragile():
    """The condition the GPU comparison rests on: on each of its inputs at most 0.1 % of the sigma > 0 points are fragile."""
    x = pack_input()
    assert 0.10 < (x[:, 3] > 0).mean() < 0.30
    for n in PACK_SIZES:
        assert fragile_share(x[:n], N_CELL, XMIN, XMAX) <= MAX_FRAGILE_SHARE, n
    third = PACK_SIZES[-1] // 3                                   # the slices of the cursor and capacity tests
    for lo, hi in ((0, third), (third, 2 * third), (2 * third, PACK_SIZES[-1]), (0, 5000)):
        assert fragile_share(x[lo:hi], N_CELL, XMIN, XMAX) <= MAX_FRAGILE_SHARE, (lo, hi)
    assert fragile_share(kept_all_input(), N_CELL, XMIN, XMAX) <= MAX_FRAGILE_SHARE
    ref = e2e_reference()[2]
    assert 0.2 < (ref[:, 3] > 0).mean() < 0.95
    assert fragile_share(ref, E2E_N, *E2E_RANGES[0]) <= MAX_FRAGILE_SHARE
    # the input has all three kinds of kept point: A == 0, 0 < A < 255, A == 255
    a = vol_ref(x, N_CELL, XMIN, XMAX)[:, 1] & 255
    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()


def test_write_read_round_trip_and_dense_placement(tmp_path):
    from nerf_pl_amd.volume import read_vol, write_vol
    N = 5
    x = trained_like(N ** 3, 3)
    rec = vol_ref(x, N, XMIN, XMAX)
    assert 0 < rec.shape[0] < N ** 3
    path = tmp_path / "scene.vol"
    assert write_vol(str(path), rec) == 8 * rec.shape[0]
    data = path.read_bytes()
    assert data == rec.astype("<u4").tobytes()                                   # no header, nothing else
    assert write_vol(str(tmp_path / "t.vol"), torch.from_numpy(rec.view(np.int32))) == len(data)   # the device tensor's dtype
    assert (tmp_path / "t.vol").read_bytes() == data
    dense = read_vol(str(path), N)
    assert dense.shape == (N, N, N, 4) and dense.dtype == np.uint8
    assert np.array_equal(dense, read_vol(data, N))
    kept = np.zeros(N ** 3, bool)
    kept[rec[:, 0]] = True
    assert not dense.reshape(-1, 4)[~kept].any()
    for i, s in rec.tolist():
        iy, ix, iz = i // (N * N), (i // N) % N, i % N                          # np.meshgrid 'xy' order
        assert dense[iy, ix, iz].tolist() == [s >> 24, (s >> 16) & 255, (s >> 8) & 255, s & 255]
    assert not read_vol(b"", N).any()


def test_read_vol_refuses_malformed_files():
    from nerf_pl_amd.volume import read_vol
    rec = np.array([[3, 0x01020304], [7, 0x05060708]], "<u4")
    assert read_vol(rec.tobytes(), 2)[0, 1, 1].tolist() == [1, 2, 3, 4]
    with pytest.raises(ValueError, match="8-byte"):
        read_vol(rec.tobytes()[:-3], 2)
    with pytest.raises(ValueError, match="outside"):
        read_vol(np.array([[3, 1], [8, 1]], "<u4").tobytes(), 2)
    with pytest.raises(ValueError, match="increasing"):
        read_vol(np.array([[3, 1], [3, 1]], "<u4").tobytes(), 2)
    with pytest.raises(ValueError, match="increasing"):
        read_vol(np.array([[4, 1], [3, 1]], "<u4").tobytes(), 2)


def test_cpu_tensors_and_oversized_lattices_are_refused():
    from nerf_pl_amd import volume
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.models import NeRF
    with pytest.raises(NerfHipError):
        volume.vol_records(torch.zeros(4, 4), 0.01)
    m = NeRF()
    r = (-1.0, 1.0)
    with pytest.raises(NerfHipError):
        volume.export_vol(m, 4, r, r, r)
    with pytest.raises(NerfHipError):
        volume.rgbsigma_grid(m, 4, r, r, r)
    # 1625^3 < 2^32 <= 1626^3: refused by name before anything is allocated
    assert 1625 ** 3 < 2 ** 32 <= 1626 ** 3
    for fn in (volume.export_vol, volume.rgbsigma_grid):
        with pytest.raises(ValueError, match=r"2\^32"):
            fn(m, 1626, r, r, r)
    with pytest.raises(ValueError, match=r"2\^32"):
        volume.read_vol(b"", 1626)


def test_load_ckpt_takes_the_named_model_of_a_lightning_checkpoint(tmp_path):
    from nerf_pl_amd.models import NeRF
    from nerf_pl_amd.volume import load_ckpt
    fine, coarse = O.make_params(1), O.make_params(2)
    sd = {"nerf_fine." + k: v for k, v in fine.items()}
    sd.update({"nerf_coarse." + k: v for k, v in coarse.items()})
    path = str(tmp_path / "epoch=05.ckpt")
    torch.save({"state_dict": sd, "epoch": 5}, path)
    m = load_ckpt(NeRF(), path, model_name="nerf_fine")
    assert all(torch.equal(v, fine[k]) for k, v in m.state_dict().items())


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def test_vol_entry_points_validate_arguments_without_a_gpu(lib):
    """nerfhip_vol_workspace_bytes / nerfhip_vol_pack: every refusal returns before a pointer is touched or a kernel launched
    (the pointers below are fake)."""
    import ctypes
    ws = lib.nerfhip_vol_workspace_bytes
    assert ws(-1) == 0 and ws(2 ** 32 + 1) == 0
    # 256 B for the call's base + 8 B and 4 B per 256-point block, each array padded to 256 B
    assert ws(1) == 256 + 256 + 256 and ws(256 * 64) == 256 + 512 + 256 and ws(256 * 64 + 1) == 256 + 768 + 512
    assert ws(2 ** 32) == 256 + 8 * 2 ** 24 + 4 * 2 ** 24
    vp = ctypes.c_void_p
    fake = 0x10000
    c = -2.4 / 512

    def pack(rgbsigma=fake, n=5, first=0, ws_=fake, records=fake, capacity=5, cursor=fake):
        return lib.nerfhip_vol_pack(vp(rgbsigma) if rgbsigma else None, n, first, c, vp(ws_) if ws_ else None,
                                    vp(records) if records else None, capacity, vp(cursor) if cursor else None, None)
    assert pack(n=-1) == -1 and pack(capacity=-1) == -1 and pack(first=-1) == -1
    assert pack(n=2, first=2 ** 32 - 1) == -1 and pack(n=2 ** 32 + 1) == -1            # first_index + n > 2^32
    for null in ("rgbsigma", "ws_", "records", "cursor"):
        assert pack(**{null: None}) == -1, null
    assert pack(rgbsigma=None, n=0, ws_=None, records=None, cursor=None) == 0         # n == 0: nothing to do
    assert pack(n=0, first=2 ** 32) == 0
    assert pack(rgbsigma=fake + 4) == -3 and pack(records=fake + 4) == -3 and pack(cursor=fake + 4) == -3    # NERFHIP_E_ALIGN
    assert lib.nerfhip_abi_version() == 3

"""GPU: the baked-volume kernels (csrc/baked.hip) and nerf_pl_amd.baked on the fixtures of tests/baked_ref.py.  The builds and
the bitfield are exact against numpy; the device march is within the cap of tests/test_baked_host.py of the float64
restatement, at every step of the fixtures, and of its host twin (the same baked_core.h: the two differ in exp2f / log2f only);
skipping, batching and culling leave every bit where it was."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baked_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_VOL = {}


def vol(dev, kind, N):
    """(dense numpy lattice, BakedVolume built by the dense path), made once"""
    from nerf_pl_amd.baked import BakedVolume
    if (kind, N) not in _VOL:
        dense = R.volume(kind, N)
        _VOL[kind, N] = (dense, BakedVolume.from_dense(torch.from_numpy(dense).to(dev), R.RANGES, cell=R.cell_of(N)))
    return _VOL[kind, N]


def records_of(dense):
    """the .vol records of a dense lattice: (i, R << 24 | G << 16 | B << 8 | A) of the points with any byte set, ascending"""
    flat = dense.reshape(-1, 4).astype(np.uint32)
    idx = np.flatnonzero(flat.any(1)).astype(np.uint32)
    p = flat[idx]
    return np.stack([idx, (p[:, 0] << 24) | (p[:, 1] << 16) | (p[:, 2] << 8) | p[:, 3]], 1).astype(np.uint32)


def render(dev, v, rays, step, skip=True, t_stop=0.0, white_back=False):
    from nerf_pl_amd.baked import BakedRenderer
    out = BakedRenderer(v, white_back, step=step, t_stop=t_stop, skip=skip)(torch.from_numpy(rays).to(dev))
    assert list(out) == ["rgb_fine", "depth_fine", "opacity_fine"]
    return [out[k].cpu().numpy() for k in out]


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# --------------------------------------------------------------------------------------------------------------------- builds
@pytest.mark.parametrize("N", [2, 8, 9, 17, 33])
def test_builds_and_bitfield(dev, N, tmp_path):
    from nerf_pl_amd import baked, volume
    from nerf_pl_amd.baked import BakedVolume
    for kind in ("random", "voxel", "zero"):
        dense, v = vol(dev, kind, N)
        want = baked.bricks_from_dense_host(dense)
        assert np.array_equal(v.data.cpu().numpy(), want), (kind, N)
        assert np.array_equal(v.bits.cpu().numpy(), baked.brick_bits_host(dense)), (kind, N)
        rec = records_of(dense)
        path = str(tmp_path / ("%s.vol" % kind))
        volume.write_vol(path, rec)
        from_rec = BakedVolume.from_records(torch.from_numpy(rec.view(np.int32)).to(dev), N, R.RANGES)
        from_file = BakedVolume.from_file(path, N, R.RANGES, device=dev)
        for b in (from_rec, from_file):
            assert np.array_equal(b.data.cpu().numpy(), want), (kind, N)
            assert np.array_equal(b.to_dense().cpu().numpy(), volume.read_vol(path, N))
            assert np.array_equal(b.bits.cpu().numpy(), v.bits.cpu().numpy())
            assert b.cell == pytest.approx((R.RANGES[0][1] - R.RANGES[0][0]) / N)
        assert np.array_equal(v.to_dense().cpu().numpy(), dense)


def test_out_of_range_records_raise(dev):
    from nerf_pl_amd.baked import BakedVolume
    rec = np.array([[3, 0x01020304], [9 ** 3, 0x01020304]], np.uint32).view(np.int32)
    with pytest.raises(ValueError):
        BakedVolume.from_records(torch.from_numpy(rec).to(dev), 9, R.RANGES)
    rec[1, 0] = -1                                          # 0xffffffff
    with pytest.raises(ValueError):
        BakedVolume.from_records(torch.from_numpy(rec).to(dev), 9, R.RANGES)
    ok = BakedVolume.from_records(torch.from_numpy(rec[:1].copy()).to(dev), 9, R.RANGES)
    assert ok.to_dense().cpu().numpy()[0, 0, 3].tolist() == [1, 2, 3, 4]
    assert BakedVolume.from_records(torch.zeros(0, 2, dtype=torch.int32, device=dev), 9, R.RANGES).data.sum().item() == 0


# ---------------------------------------------------------------------------------------------------------------------- march
@pytest.mark.parametrize("N", R.LATTICES)
def test_device_march(dev, N):
    from nerf_pl_amd import ops
    rays = R.rays(N)
    half = len(rays) // 2 + 1
    for i, kind in enumerate(R.VOLUMES):
        white = bool(i & 1)
        dense, v = vol(dev, kind, N)
        for step in R.STEPS:
            got = render(dev, v, rays, step, white_back=white)
            # skip on = skip off, a batch = its halves: bit for bit
            assert same_bits(got, render(dev, v, rays, step, skip=False, white_back=white)), (kind, N, step)
            a, b = render(dev, v, rays[:half], step, white_back=white), render(dev, v, rays[half:], step, white_back=white)
            assert same_bits(got, [np.concatenate([x, y]) for x, y in zip(a, b)]), (kind, N, step)
            for row in (-1, -2):                            # the NaN row and the zero-direction row
                assert got[0][row].tolist() == [float(white)] * 3 and got[1][row] == 0.0 and got[2][row] == 0.0
            if kind == "zero":
                assert (got[0] == float(white)).all() and (got[1] == 0.0).all() and (got[2] == 0.0).all()
            # the float64 restatement and the host twin, each within the cap
            want = ops.baked_render_host(rays, v.data.cpu().numpy(), v.bits.cpu().numpy(), N, R.RANGES, v.cell, step, 0.0, white)
            ref = R.render(rays, dense, R.RANGES, v.cell, step, white_back=white)
            refs = [("fp64", ref), ("host", {"rgb": want[0], "depth": want[1], "opacity": want[2]})]
            cap = max(int(ref["K"].max()), 1) * N * 2.0 ** -22
            far = np.nan_to_num(np.abs(rays[:, 7])).astype(np.float64)
            for name, ref in refs:
                e_rgb, e_op = np.abs(got[0] - ref["rgb"]).max(), np.abs(got[2] - ref["opacity"]).max()
                e_depth = np.abs(got[1] - ref["depth"])
                print("N%d %s step %g vs %s: rgb %.3g opacity %.3g depth %.3g cap %.3g" % (N, kind, step, name, e_rgb, e_op, e_depth.max(), cap))
                assert e_rgb <= cap and e_op <= cap and (e_depth <= cap * far).all(), (kind, N, step, name, e_rgb, e_op, cap)


def test_t_stop_on_the_device(dev):
    N = 17
    rays = R.rays(N)
    _, v = vol(dev, "shell", N)
    full, cut = render(dev, v, rays, 0.5), render(dev, v, rays, 0.5, t_stop=1e-2)
    cap = 64 * N * 2.0 ** -22
    assert np.abs(cut[2] - full[2]).max() <= 1e-2 + cap and np.abs(cut[0] - full[0]).max() <= 1e-2 + cap
    assert same_bits(cut, render(dev, v, rays, 0.5, t_stop=1e-2, skip=False))


# ------------------------------------------------------------------------------------------------------- culling and evaluate
@pytest.mark.parametrize("white", [True, False])
def test_culled_renderer_keeps_every_bit(dev, white):
    from nerf_pl_amd.baked import BakedRenderer
    from nerf_pl_amd.occupancy import CulledRenderer
    N = 33
    rays = torch.from_numpy(R.rays(N)[:-2]).to(dev)         # (non-finite rows are the cull's own business: it keeps them)
    for kind in ("shell", "voxel"):
        _, v = vol(dev, kind, N)
        inner = BakedRenderer(v, white)
        culled = CulledRenderer(inner, v.occupancy_grid(dilate=1), white, tighten="none")
        want, got = inner(rays), culled(rays)
        assert 0 < culled.stats["rendered"] < culled.stats["rays"]
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (kind, k)


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


def test_evaluate_takes_a_baked_renderer(dev):
    from nerf_pl_amd import inference
    from nerf_pl_amd.baked import BakedRenderer
    _, v = vol(dev, "shell", 33)
    out = inference.evaluate(_TwoImages(dev), BakedRenderer(v, white_back=True))
    assert len(out["psnr"]) == len(out["ssim"]) == len(out["images"]) == 2
    assert np.isfinite(out["mean_psnr"]) and out["mean_psnr"] > 0
    for img in out["images"]:
        assert img.shape == (12, 16, 3) and img.dtype == np.uint8
        assert (img == 255).all(-1).any() and (img != 255).any()      # the white background and the shell in front of it


def test_from_model_is_export_then_records(dev):
    from nerf_pl_amd import volume
    from nerf_pl_amd.baked import BakedVolume
    from nerf_pl_amd.models import NeRF
    torch.manual_seed(3)
    model = NeRF().to(dev).eval()
    ranges = ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0))
    a = BakedVolume.from_model(model, 9, *ranges)
    rec = volume.export_vol(model, 9, *ranges)
    b = BakedVolume.from_records(rec, 9, ranges)
    assert a.N == b.N == 9 and a.cell == b.cell == pytest.approx(2.0 / 9) and a.ranges == b.ranges
    assert torch.equal(a.data, b.data) and torch.equal(a.bits, b.bits)
    assert np.array_equal(a.to_dense().cpu().numpy(), volume.read_vol(rec.cpu().numpy().view(np.uint32).astype("<u4").tobytes(), 9))


# --------------------------------------------------------------------------------------------------- optional outputs left out
def test_null_optional_outputs_on_the_device(dev):
    """nerfhip_baked_render with rgb, depth and opacity null in turn, on 257 rays (one full block and one ray in a second) through
    the N = 9 lattice: the two that are supplied keep the bits of the full call, and nothing is written past row n of either."""
    import test_baked_host as H
    from nerf_pl_amd import _lib, ops
    lib = _lib.load()
    n, pad, pattern = 257, 64, -1515870811                  # 0xa5a5a5a5
    rays, data, bits, scalars = H.null_output_case(n)
    rays, data, bits = (torch.from_numpy(a).to(dev) for a in (rays, data, bits))
    full = ops.baked_render(rays, data, bits, 9, R.RANGES, R.cell_of(9), 0.5, 0.0, True)
    assert float(full[2].max()) > 0.05 and bool((full[2] == 0).any())
    with torch.cuda.device(dev):
        for skip in range(3):
            out = [torch.full((n + pad,) + tail, pattern, device=dev, dtype=torch.int32).view(torch.float32) for tail in ((3,), (), ())]
            ptrs = [None if k == skip else _lib.ptr(out[k]) for k in range(3)]
            _lib.check(lib.nerfhip_baked_render(_lib.ptr(rays), n, _lib.ptr(data), _lib.ptr(bits), *scalars, *ptrs, _lib.stream_ptr()),
                       "nerfhip_baked_render")
            for k in range(3):
                assert bool((out[k][n:].view(torch.int32) == pattern).all()), (skip, k)
                if k == skip:
                    assert bool((out[k].view(torch.int32) == pattern).all()), skip
                else:
                    assert torch.equal(out[k][:n].view(torch.int32), full[k].view(torch.int32)), (skip, k)

"""GPU: the occupancy kernels (csrc/occupancy.hip) and nerf_pl_amd.occupancy.  Everything here is exact: the bitfield against the
numpy restatement (tests/cull_ref.py), the device cull against its host twin (the same occupancy_core.h), compaction and scatter
against numpy indexing, CulledRenderer against the inner renderer run by hand."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cull_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = R.grids()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------------------------ bitfield
@pytest.mark.parametrize("N", [2, 6, 34])
def test_occupancy_build_is_the_restatement(dev, N):
    from nerf_pl_amd import ops
    sigma, thr = R.sigma_fixture(N)
    assert (sigma == thr).any() and (N == 2 or np.isnan(sigma).sum() == 1)
    occ = R.cells_from_sigma(sigma, thr)
    s = torch.from_numpy(sigma).to(dev)
    for r in (0, 1, 2, 40):
        got = ops.occupancy_build(s, thr, r).cpu().numpy()
        want = R.pack_bits(R.dilate(occ, r))
        assert got.dtype == np.int32 and np.array_equal(got, want), (N, r)
    # `>` and not `>=`: just below the lattice value, the cells around it fill
    below = float(np.nextafter(np.float32(thr), np.float32(0)))
    assert np.array_equal(ops.occupancy_build(s, below, 0).cpu().numpy(), R.pack_bits(R.cells_from_sigma(sigma, below)))
    assert R.cells_from_sigma(sigma, below).sum() > occ.sum()


# ---------------------------------------------------------------------------------------------------------------------- cull
def _device_cull(dev, grid, rays):
    from nerf_pl_amd import ops
    hit, t0, t1 = ops.cull_rays(torch.from_numpy(rays).to(dev), torch.from_numpy(grid.words).to(dev), grid.M, grid.ranges)
    return hit.cpu().numpy(), t0.cpu().numpy(), t1.cpu().numpy()


def _same_as_host(dev, grid, rays):
    from nerf_pl_amd import ops
    want = ops.cull_rays_host(rays, grid.words, grid.M, grid.ranges)
    got = _device_cull(dev, grid, rays)
    for name, g, w in zip(("hit", "t0", "t1"), got, want):
        assert np.array_equal(_bits(g), _bits(w)), (grid.name, name, np.flatnonzero(_bits(g) != _bits(w))[:5])
    return want


@pytest.mark.parametrize("grid", GRIDS, ids=[g.name for g in GRIDS])
def test_cull_device_is_the_host_twin(dev, grid):
    _same_as_host(dev, grid, R.generic_rays(grid, 20240 + grid.M))
    _same_as_host(dev, grid, R.degenerate_rays(grid)[0])


@pytest.fixture(scope="module")
def sphere():
    return next(g for g in GRIDS if g.name == "M33-sphere")


@pytest.fixture(scope="module")
def big_batch(sphere):
    return R.bulk_rays(sphere, 70001, 5)


@pytest.mark.parametrize("n", [1, 63, 257, 70001])
def test_cull_sizes(dev, sphere, big_batch, n):
    hit, _, _ = _same_as_host(dev, sphere, np.ascontiguousarray(big_batch[:n]))
    if n == 70001:
        assert 0.2 < hit.mean() < 0.8
    from nerf_pl_amd import ops
    empty = ops.cull_rays(torch.zeros(0, 8, device=dev), torch.from_numpy(sphere.words).to(dev), sphere.M, sphere.ranges)
    assert [t.shape[0] for t in empty] == [0, 0, 0]


# ----------------------------------------------------------------------------------------------------------------- compaction
def _check_compact(dev, rays, hit, t0, t1):
    from nerf_pl_amd import ops
    n = len(rays)
    slot, index, out, n_hit = ops.cull_compact(torch.from_numpy(hit).to(dev), torch.from_numpy(rays).to(dev), torch.from_numpy(t0).to(dev),
                                               torch.from_numpy(t1).to(dev))
    want = np.flatnonzero(hit)
    k = int(n_hit.item())
    assert n_hit.dtype == torch.int32 and k == len(want)
    assert np.array_equal(index.cpu().numpy()[:k], want.astype(np.int32))
    want_slot = np.full(n, -1, np.int32)
    want_slot[want] = np.arange(k, dtype=np.int32)
    assert np.array_equal(slot.cpu().numpy(), want_slot)
    rows = rays[want].copy()
    rows[:, 6], rows[:, 7] = t0[want], t1[want]
    assert np.array_equal(out.cpu().numpy()[:k].view(np.uint32), rows.view(np.uint32))
    return slot


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "culled"])
def test_compact(dev, sphere, big_batch, pattern):
    from nerf_pl_amd import ops
    rng = np.random.default_rng(3)
    if pattern == "culled":
        rays = big_batch                                   # 274 blocks: the scan of the block totals takes two passes
        hit, t0, t1 = ops.cull_rays_host(rays, sphere.words, sphere.M, sphere.ranges)
    else:
        rays = np.ascontiguousarray(big_batch[:1000])
        t0, t1 = rng.random(1000, dtype=np.float32), rng.random(1000, dtype=np.float32) + 1
        hit = {"all": np.ones(1000, np.uint8), "none": np.zeros(1000, np.uint8),
               "alternating": (np.arange(1000) % 2).astype(np.uint8) * 255}[pattern]     # any non-zero flag is a hit
    _check_compact(dev, rays, hit, t0, t1)


def test_compact_keeps_near_or_far_for_a_null_bound(dev, sphere, big_batch):
    from nerf_pl_amd import ops
    rays = np.ascontiguousarray(big_batch[:3000])
    hit, t0, t1 = ops.cull_rays_host(rays, sphere.words, sphere.M, sphere.ranges)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    want = np.flatnonzero(hit)
    for a0, a1 in ((t0, None), (None, t1), (None, None)):
        _, _, out, n_hit = ops.cull_compact(up(hit), up(rays), up(a0), up(a1))
        rows = rays[want].copy()
        if a0 is not None:
            rows[:, 6] = a0[want]
        if a1 is not None:
            rows[:, 7] = a1[want]
        assert int(n_hit.item()) == len(want)
        assert np.array_equal(out.cpu().numpy()[:len(want)].view(np.uint32), rows.view(np.uint32))


def test_compact_of_no_rays(dev):
    from nerf_pl_amd import ops
    z = torch.zeros(0, device=dev)
    slot, index, out, n_hit = ops.cull_compact(z.to(torch.uint8), torch.zeros(0, 8, device=dev), z, z)
    assert int(n_hit.item()) == 0 and slot.shape == (0,) and out.shape == (0, 8)


# -------------------------------------------------------------------------------------------------------------------- scatter
@pytest.mark.parametrize("white_back", [True, False])
def test_scatter(dev, white_back):
    from nerf_pl_amd import ops
    rng = np.random.default_rng(11)
    n = 1237
    hit = rng.random(n) < 0.4
    k = int(hit.sum())
    slot = np.full(n, -1, np.int32)
    slot[hit] = np.arange(k, dtype=np.int32)
    rgb, depth, oa, ob = rng.random((k, 3), np.float32), rng.random(k, np.float32), rng.random(k, np.float32), rng.random(k, np.float32)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731

    def want(src, bg):
        out = np.full((n,) + src.shape[1:], bg, np.float32)
        out[hit] = src
        return out
    got = ops.cull_scatter(up(slot), white_back, up(rgb), up(depth), up(oa), up(ob))
    for g, (src, bg) in zip(got, ((rgb, 1.0 if white_back else 0.0), (depth, 0.0), (oa, 0.0), (ob, 0.0))):
        assert np.array_equal(g.cpu().numpy(), want(src, bg))
    # null pointers among the outputs
    got = ops.cull_scatter(up(slot), white_back, None, up(depth), None, up(ob))
    assert got[0] is None and got[2] is None
    assert np.array_equal(got[1].cpu().numpy(), want(depth, 0.0)) and np.array_equal(got[3].cpu().numpy(), want(ob, 0.0))
    got = ops.cull_scatter(up(slot), white_back, up(rgb))
    assert np.array_equal(got[0].cpu().numpy(), want(rgb, 1.0 if white_back else 0.0)) and got[1:] == (None, None, None)


# ------------------------------------------------------------------------------------------------------------ CulledRenderer
H, W = 40, 48


@pytest.fixture(scope="module")
def scene(dev):
    """Two randomly initialised default NeRFs behind a GraphRenderer of 512-ray chunks (several chunks and a ragged tail), and a
    48 x 40 image of rays looking at the origin from z = 4."""
    from nerf_pl_amd import inference, rays
    from nerf_pl_amd.models import Embedding, NeRF
    torch.manual_seed(0)
    models = [NeRF().to(dev), NeRF().to(dev)]
    renderer = inference.GraphRenderer(models, [Embedding(3, 10), Embedding(3, 4)], N_samples=64, N_importance=128, white_back=True,
                                       chunk=512)
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]], device=dev)
    r = rays.gen_rays(c2w, H, W, 45.0, 2.0, 6.0)
    assert r.shape == (H * W, 8)
    return renderer, r


def _grid(dev, occ, ranges):
    from nerf_pl_amd.occupancy import OccupancyGrid
    return OccupancyGrid(torch.from_numpy(R.pack_bits(occ)).to(dev), occ.shape[0], ranges)


class _Counting:
    def __init__(self, inner):
        self.inner, self.calls, self.rays = inner, 0, 0

    def __call__(self, rays):
        self.calls += 1
        self.rays += rays.shape[0]
        return self.inner(rays)


def test_culled_renderer_full_grid_is_the_plain_renderer(dev, scene):
    from nerf_pl_amd.occupancy import CulledRenderer
    renderer, rays = scene
    plain = renderer(rays)
    big = ((-16.0, 16.0),) * 3                             # contains every [near, far] segment: no interval changes
    culled = CulledRenderer(renderer, _grid(dev, np.ones((5, 5, 5), bool), big), white_back=True)
    got = culled(rays)
    assert list(got) == list(plain)
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    assert culled.stats["rays"] == H * W and culled.stats["rendered"] == H * W


def test_culled_renderer_empty_grid_never_renders(dev, scene):
    from nerf_pl_amd.occupancy import CulledRenderer
    renderer, rays = scene
    plain = renderer(rays)
    for white_back in (True, False):
        inner = _Counting(renderer)
        got = CulledRenderer(inner, _grid(dev, np.zeros((5, 5, 5), bool), R.CUBE), white_back=white_back)(rays)
        assert inner.calls == 0
        assert sorted(got) == sorted(plain)
        for k, v in got.items():
            assert v.shape == plain[k].shape and v.dtype == torch.float32
            bg = 1.0 if (white_back and k.startswith("rgb")) else 0.0
            assert bool((v == bg).all()), k


def test_culled_renderer_sphere_grid(dev, scene, sphere):
    from nerf_pl_amd import ops
    from nerf_pl_amd.occupancy import CulledRenderer
    renderer, rays = scene
    inner = _Counting(renderer)
    culled = CulledRenderer(inner, _grid(dev, sphere.occ, sphere.ranges), white_back=True)
    got = culled(rays)
    hit, t0, t1 = ops.cull_rays_host(rays.cpu().numpy(), sphere.words, sphere.M, sphere.ranges)
    hit = hit.astype(bool)
    assert 0.03 < hit.mean() < 0.6                         # the sphere covers part of the image
    edited = rays.cpu().numpy()[hit].copy()
    edited[:, 6], edited[:, 7] = t0[hit], t1[hit]
    assert (edited[:, 6] > 2.0).all() and (edited[:, 7] < 6.0).all()
    by_hand = renderer(torch.from_numpy(edited).to(dev))
    mask = torch.from_numpy(hit).to(dev)
    assert list(got) == list(by_hand)
    for k, v in by_hand.items():
        assert torch.equal(got[k][mask], v), k
        bg = 1.0 if k.startswith("rgb") else 0.0
        assert bool((got[k][~mask] == bg).all()), k
    assert inner.calls == 1 and inner.rays == int(hit.sum())
    assert culled.stats == {"rays": H * W, "rendered": int(hit.sum()), "calls": 1}


@pytest.mark.parametrize("tighten", ["near", "none"])
def test_culled_renderer_tighten_modes(dev, scene, sphere, tighten):
    from nerf_pl_amd import ops
    from nerf_pl_amd.occupancy import CulledRenderer
    renderer, rays = scene
    got = CulledRenderer(renderer, _grid(dev, sphere.occ, sphere.ranges), white_back=True, tighten=tighten)(rays)
    hit, t0, _ = ops.cull_rays_host(rays.cpu().numpy(), sphere.words, sphere.M, sphere.ranges)
    hit = hit.astype(bool)
    edited = rays.cpu().numpy()[hit].copy()
    if tighten == "near":
        edited[:, 6] = t0[hit]
    by_hand = renderer(torch.from_numpy(edited).to(dev))
    mask = torch.from_numpy(hit).to(dev)
    for k, v in by_hand.items():
        assert torch.equal(got[k][mask], v), k
        assert bool((got[k][~mask] == (1.0 if k.startswith("rgb") else 0.0)).all()), k
    with pytest.raises(ValueError):
        CulledRenderer(renderer, _grid(dev, sphere.occ, sphere.ranges), white_back=True, tighten="far")


# ------------------------------------------------------------------------------------------------------- evaluate, save / load
class _TwoImages:
    img_wh = (16, 12)
    white_back = True

    def __init__(self, dev):
        from nerf_pl_amd import rays
        g = torch.Generator().manual_seed(7)
        self.items = []
        for z in (4.0, 3.5):
            c2w = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, z]], device=dev)
            self.items.append({"rays": rays.gen_rays(c2w, 12, 16, 30.0, 2.0, 6.0), "rgbs": torch.rand(16 * 12, 3, generator=g)})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_evaluate_takes_a_culled_renderer(dev, sphere):
    from nerf_pl_amd import inference
    from nerf_pl_amd.models import Embedding, NeRF
    from nerf_pl_amd.occupancy import CulledRenderer
    torch.manual_seed(1)
    models, embeddings = [NeRF().to(dev), NeRF().to(dev)], [Embedding(3, 10), Embedding(3, 4)]

    def renderer(rays):
        return inference.batched_inference(models, embeddings, rays, 16, 16, False, 1024, True)
    data = _TwoImages(dev)
    plain = inference.evaluate(data, renderer)
    culled = CulledRenderer(renderer, _grid(dev, sphere.occ, sphere.ranges), white_back=True)
    got = inference.evaluate(data, culled)
    assert sorted(got) == sorted(plain)
    assert len(got["psnr"]) == len(got["ssim"]) == len(got["images"]) == 2
    for a, b in zip(got["images"], plain["images"]):
        assert a.shape == b.shape == (12, 16, 3) and a.dtype == b.dtype
    assert 0 < culled.stats["rendered"] < culled.stats["rays"] == 2 * 16 * 12


def test_grid_save_load_round_trip(dev, sphere, tmp_path):
    from nerf_pl_amd.occupancy import OccupancyGrid
    sigma, thr = R.sigma_fixture(34)
    grid = OccupancyGrid.from_sigma(torch.from_numpy(sigma).to(dev), (-1.5, 1.0), (-1.0, 1.0), (0.25, 2.0), sigma_threshold=thr, dilate=2)
    want = R.dilate(R.cells_from_sigma(sigma, thr), 2)
    assert grid.M == 33 and np.array_equal(grid.bits.cpu().numpy(), R.pack_bits(want))
    assert grid.occupied_fraction() == want.sum() / 33 ** 3
    path = str(tmp_path / "grid.npz")
    grid.save(path)
    assert sorted(np.load(path).files) == ["M", "dilate", "ranges", "sigma_threshold", "words"]
    back = OccupancyGrid.load(path, device=dev)
    assert torch.equal(back.bits, grid.bits) and back.bits.dtype == torch.int32
    assert (back.M, back.ranges, back.sigma_threshold, back.dilate) == (grid.M, grid.ranges, grid.sigma_threshold, grid.dilate)
    rays = torch.from_numpy(R.bulk_rays(sphere, 300, 2)).to(dev)
    for a, b in zip(grid.cull(rays), back.cull(rays)):
        assert torch.equal(a, b)

"""GPU: scene loading (csrc/image.hip, nerf_pl_amd/datasets) against the bytes PIL produced at mint time
(tests/tools/make_golden_blender.py) and against the reference's float formulas on the CPU.  Everything is integer or separately
rounded fp32 arithmetic, so every comparison is exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "blender_mini")


@pytest.fixture(scope="module")
def expected():
    z = np.load(os.path.join(ROOT, "tests", "golden", "blender_mini_expected.npz"))
    return {k: z[k] for k in z.files}


def _blend_cpu(u8):
    """blender.py:56-58 on the CPU from (..., 4) uint8: ToTensor's .div(255), then the blend onto white"""
    img = torch.from_numpy(np.ascontiguousarray(u8)).reshape(-1, 4).to(torch.float32).div(255)
    return img[:, :3] * img[:, -1:] + (1 - img[:, -1:])


# ---- unfilter ------------------------------------------------------------------------------------------------------------------
def test_unfilter_decodes_every_fixture(dev, expected):
    from nerf_pl_amd import ops
    from nerf_pl_amd.imageio_min import png_inflate
    rows = []
    for name in expected["names"]:
        w, h, ch, raw = png_inflate(os.path.join(SCENE, "%s.png" % name))
        assert (w, h, ch) == (48, 48, 4)
        rows.append(np.frombuffer(raw, np.uint8))
    got = ops.decode_png_batch(torch.from_numpy(np.stack(rows)).to(dev), 48, 48, 4).cpu().numpy()
    for k in range(len(rows)):
        assert np.array_equal(got[k], expected["rgba_%d" % k]), expected["names"][k]


def _de_bruijn_pairs():
    """a cyclic order of the filter types 0-4 in which every type follows every type (itself included) exactly once"""
    k, n, a, seq = 5, 2, [0] * 10, []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    assert len(seq) == 25 and len({(seq[i], seq[(i + 1) % 25]) for i in range(25)}) == 25
    return seq


def _forward_filter(raw, filters):
    """(n, H, W, ch) uint8 pixels + (n, H) filter types -> (n, H * (1 + W ch)) PNG scanline streams: filtered = raw - predictor(raw)
    modulo 256, with the predictors formed from the unfiltered image (vectorised: no serial dependency in this direction)"""
    n, H, W, ch = raw.shape
    r = raw.astype(np.int64)
    a = np.zeros_like(r)
    a[:, :, 1:] = r[:, :, :-1]
    b = np.zeros_like(r)
    b[:, 1:] = r[:, :-1]
    c = np.zeros_like(r)
    c[:, 1:, 1:] = r[:, :-1, :-1]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    preds = np.stack([np.zeros_like(r), a, b, (a + b) >> 1, paeth])             # (5, n, H, W, ch)
    f = np.minimum(filters, 4).astype(np.int64)[None, :, :, None, None]
    pred = np.take_along_axis(preds, np.broadcast_to(f, (1,) + r.shape), 0)[0]
    pred = np.where(filters[:, :, None, None] > 4, 0, pred)
    out = np.empty((n, H, 1 + W * ch), np.uint8)
    out[:, :, 0] = filters
    out[:, :, 1:] = ((r - pred) & 255).reshape(n, H, W * ch)
    return out.reshape(n, -1)


UNFILTER_SHAPES = ((1, 1, 4), (1, 37, 3), (37, 1, 1), (5, 3, 4), (33, 70, 4), (70, 33, 3), (1030, 3, 4))


@pytest.mark.parametrize("H,W,ch", UNFILTER_SHAPES)
def test_unfilter_synthetic_streams(dev, H, W, ch):
    """a batch of 3 random images per shape, one forced filter type per row, every type after every other (from 26 rows on);
    1030 rows: more rows than the workgroup has threads, and the first row of the second pass predicts from the row above"""
    from nerf_pl_amd import ops
    rng = np.random.default_rng(H * 1000 + W * 10 + ch)
    seq = np.array(_de_bruijn_pairs())
    raw = rng.integers(0, 256, (3, H, W, ch), dtype=np.uint8)
    raw[1, :, : W // 2] = raw[1, :1, :1]                                         # flat areas too: ties in Paeth's choice
    shift = next(s for s in range(25) if H <= 1024 or seq[(1024 + s) % 25] == 4)
    filters = np.stack([seq[(np.arange(H) + shift + 7 * i) % 25] for i in range(3)]).astype(np.uint8)
    streams = _forward_filter(raw, filters)
    got, flags = ops.decode_png_batch(torch.from_numpy(streams).to(dev), H, W, ch, return_flags=True)
    assert got.shape == (3, H, W, ch) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), raw)
    assert flags.cpu().tolist() == [0, 0, 0]


def test_unfilter_flags_an_unknown_filter_type(dev):
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (3, 9, 6, 4), dtype=np.uint8)
    filters = rng.integers(0, 5, (3, 9)).astype(np.uint8)
    filters[1, 4] = 7
    streams = torch.from_numpy(_forward_filter(raw, filters)).to(dev)
    got, flags = ops.decode_png_batch(streams, 9, 6, 4, return_flags=True)       # returns normally
    assert [bool(f) for f in flags.cpu().tolist()] == [False, True, False]
    got = got.cpu().numpy()
    assert np.array_equal(got[0], raw[0]) and np.array_equal(got[2], raw[2])     # the other images are untouched by it
    with pytest.raises(NerfHipError, match="filter type"):
        ops.decode_png_batch(streams, 9, 6, 4)


# ---- resize --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (48, 20, 31, 80))
def test_resize_equals_pil_on_the_fixtures(dev, expected, size):
    from nerf_pl_amd import ops
    n = len(expected["names"])
    src = np.stack([expected["rgba_%d" % k] for k in range(n)])
    got = ops.resize_rgba_lanczos(torch.from_numpy(src).to(dev), size, size)
    assert got.shape == (n, size, size, 4)
    got = got.cpu().numpy()
    for k in range(n):
        assert np.array_equal(got[k], expected["resized%d_%d" % (size, k)]), (size, k)
    if size == 48:
        assert np.array_equal(got, src)                                          # same size: a copy, no premultiply round trip


def test_resize_non_square_equals_pil_live(dev):
    """64 x 40 -> 23 x 57 (w x h): the horizontal pass shrinks, the vertical one enlarges, with different taps; and each pass alone"""
    Image = pytest.importorskip("PIL.Image")
    from nerf_pl_amd import ops
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (40, 64, 4), dtype=np.uint8)
    img[:10, :, 3] = 0
    img[10:20, :, 3] = 255
    img[20:30, :, 3] = rng.integers(1, 8, (10, 64))                               # small alpha: un-premultiply clips at 255
    src = torch.from_numpy(img).to(dev)
    for (w, h) in ((23, 57), (23, 40), (64, 57)):
        ref = np.asarray(Image.fromarray(img, "RGBA").resize((w, h), Image.LANCZOS))
        got = ops.resize_rgba_lanczos(src, w, h)
        assert got.shape == (h, w, 4)
        assert np.array_equal(got.cpu().numpy(), ref), (w, h)


# ---- blend ---------------------------------------------------------------------------------------------------------------------
def test_blend_every_colour_alpha_pair(dev):
    from nerf_pl_amd import ops
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    u8 = np.stack([c, c[::-1], c.T, a], -1).reshape(-1, 4)                        # (65536, 4): channel 0 runs over every (c, a)
    rgb, mask = ops.rgba_to_rgb_white(torch.from_numpy(u8).to(dev))
    assert rgb.shape == (65536, 3) and mask.dtype == torch.bool
    assert torch.equal(rgb.cpu(), _blend_cpu(u8))
    assert torch.equal(mask.cpu(), torch.from_numpy(u8[:, 3] > 0))
    # into a slice of a larger array, as the dataset assembles a scene
    big = torch.full((3 * 65536, 3), -1.0, device=dev)
    ops.rgba_to_rgb_white(torch.from_numpy(u8).to(dev), out=big[65536:2 * 65536])
    assert torch.equal(big[65536:2 * 65536].cpu(), _blend_cpu(u8)) and bool((big[:65536] == -1).all()) and bool((big[2 * 65536:] == -1).all())


# ---- the dataset ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train20(dev):
    from nerf_pl_amd.datasets import BlenderDataset
    return BlenderDataset(SCENE, "train", (20, 20), device=dev)


def test_train_split(dev, expected, train20):
    from nerf_pl_amd import rays
    ds = train20
    angle = ds.meta["camera_angle_x"]
    assert ds.focal == 0.5 * 800 / np.tan(0.5 * angle) * (20 / 800)
    assert (ds.near, ds.far, ds.white_back) == (2.0, 6.0, True) and ds.bounds.tolist() == [2.0, 6.0]
    assert len(ds.image_paths) == 3 and all(os.path.exists(p) for p in ds.image_paths)
    assert len(ds.poses) == 3 and all(isinstance(p, np.ndarray) and p.shape == (3, 4) for p in ds.poses)
    assert np.array_equal(np.stack(ds.poses), expected["poses_train"])
    assert torch.equal(ds.directions, rays.get_ray_directions(20, 20, ds.focal, device=dev))
    want = torch.cat([_blend_cpu(expected["resized20_%d" % k]) for k in range(3)])
    assert ds.all_rgbs.is_cuda and torch.equal(ds.all_rgbs.cpu(), want)
    poses = torch.from_numpy(expected["poses_train"].astype(np.float32)).to(dev)
    assert torch.equal(ds.all_rays, rays.gen_rays(poses, 20, 20, ds.focal, 2.0, 6.0))
    assert len(ds) == 1200 and ds.all_rays.shape == (1200, 8)
    item = ds[777]
    assert set(item) == {"rays", "rgbs"} and torch.equal(item["rays"], ds.all_rays[777]) and torch.equal(item["rgbs"], ds.all_rgbs[777])
    batch = ds.ray_store().sample(64, return_ids=True)
    ids = batch["ids"]
    assert torch.equal(batch["rgbs"], ds.all_rgbs[ids]) and torch.equal(batch["rays"], ds.all_rays[ids])


def test_train_split_at_the_files_own_size(dev, expected):
    """img_wh equal to the files' size: the pixels pass through untouched (a premultiply round trip would change them)"""
    from nerf_pl_amd.datasets import BlenderDataset
    ds = BlenderDataset(SCENE, "train", (48, 48), device=dev)
    want = torch.cat([_blend_cpu(expected["rgba_%d" % k]) for k in range(3)])
    assert torch.equal(ds.all_rgbs.cpu(), want)


def test_val_and_test_splits(dev, expected):
    from nerf_pl_amd import rays
    from nerf_pl_amd.datasets import BlenderDataset
    ds = BlenderDataset(SCENE, "val", (31, 31), device=dev)
    assert len(ds) == 8
    item = ds[0]
    assert set(item) == {"rays", "rgbs", "c2w", "valid_mask"}
    k = list(expected["names"]).index("val/r_0")
    resized = expected["resized31_%d" % k]
    assert item["valid_mask"].dtype == torch.bool and item["valid_mask"].shape == (31 * 31,)
    assert torch.equal(item["valid_mask"].cpu(), torch.from_numpy(resized[..., 3].reshape(-1) > 0))
    assert torch.equal(item["rgbs"].cpu(), _blend_cpu(resized))
    c2w = torch.FloatTensor(ds.meta["frames"][0]["transform_matrix"])[:3, :4]
    assert item["c2w"].is_cuda and torch.equal(item["c2w"].cpu(), c2w)
    assert torch.equal(item["rays"], rays.gen_rays(c2w.to(dev), 31, 31, ds.focal, 2.0, 6.0)) and item["rays"].shape == (961, 8)
    assert len(BlenderDataset(SCENE, "test", (20, 20), device=dev)) == 1


def test_one_training_step_from_the_dataset(dev, train20):
    from argparse import Namespace
    from nerf_pl_amd.system import NeRFSystem, fit
    hp = Namespace(N_samples=16, N_importance=16, use_disp=False, perturb=1.0, noise_std=0.0, chunk=1024 * 32, loss_type="mse",
                   lr=5e-4, weight_decay=0, decay_step=[100], decay_gamma=0.5)
    system = NeRFSystem(hp, train_dataset=train20).to(dev)
    assert system.white_back is True
    torch.manual_seed(0)
    losses = fit(system, [train20.ray_store().sample(64)])
    assert len(losses) == 1 and bool(torch.isfinite(losses[0]))

"""GPU: JPEG decoding (csrc/jpeg.hip) against the bytes PIL produced at mint time, and nerf_pl_amd.datasets.LLFFDataset against
what the reference's own LLFFDataset produced on the CPU (tests/tools/make_golden_llff.py).  Decoding, resizing and ToTensor are
integer or separately rounded fp32 arithmetic, so those comparisons are exact: no pixel is left out.  The rays are compared at
the tolerance tests/test_rays.py uses for gen_rays (rtol 1e-5, atol 1e-6)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
JPEGS = os.path.join(GOLDEN, "jpeg_mini")
SCENE = os.path.join(GOLDEN, "llff_mini")
SCENE_PNG = os.path.join(GOLDEN, "llff_mini_png")
RAY_STRIDE = 7                         # make_golden_llff.py keeps every ray at width 32 and every 7th at 64 and 80
RAY_TOL = dict(rtol=1e-5, atol=1e-6)
SIZES = ((64, 48), (32, 24), (80, 60))


@pytest.fixture(scope="module")
def jpeg_expected():
    z = np.load(os.path.join(GOLDEN, "jpeg_mini_expected.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def expected():
    z = np.load(os.path.join(GOLDEN, "llff_mini_expected.npz"))
    return {k: z[k] for k in z.files}


def _host_half(name):
    from nerf_pl_amd import ops
    from nerf_pl_amd.imageio_min import jpeg_parse
    parsed = jpeg_parse(os.path.join(JPEGS, name + ".jpg"))
    comps = parsed["components"]
    quant = np.stack([parsed["quant"][c[3]] for c in comps]).astype(np.int16)
    return parsed, ops.jpeg_entropy_decode(parsed), quant


def _decode(dev, items):
    """[(parsed, coefficient arrays, quant)] of one size and sampling -> (n, H, W, 4) uint8 numpy"""
    from nerf_pl_amd import ops
    parsed = items[0][0]
    comps = parsed["components"]
    coefs = [torch.from_numpy(np.stack([it[1][c].reshape(-1, 64) for it in items])).to(dev) for c in range(len(comps))]
    quant = torch.from_numpy(np.stack([it[2] for it in items])).to(dev)
    out = ops.decode_jpeg_batch(coefs, quant, parsed["height"], parsed["width"], comps[0][1], comps[0][2])
    assert out.dtype == torch.uint8 and out.shape == (len(items), parsed["height"], parsed["width"], 4) and out.is_cuda
    return out.cpu().numpy()


def test_decode_equals_pil_on_every_fixture(dev, jpeg_expected):
    names = list(jpeg_expected["names"])
    n = 0
    for k, name in enumerate(names):
        if "progressive" in name:
            continue
        got = _decode(dev, [_host_half(name)])[0]
        want = jpeg_expected["rgb_%d" % k]
        assert np.array_equal(got[..., :3], want), (name, int((got[..., :3] != want).any(-1).sum()))
        assert (got[..., 3] == 255).all(), name
        n += 1
    assert n >= 12


def test_decode_batches_of_equal_size(dev, jpeg_expected):
    """files of one size and sampling but different quantisation tables, Huffman tables and restart intervals, in one batch;
    each image must come out as it does alone"""
    names = list(jpeg_expected["names"])
    for group in (["q90_420_61x45", "q75_420_61x45_optimized", "q85_420_61x45_restart3"], ["q30_420_64x48", "q50_420_64x48_restart1"]):
        got = _decode(dev, [_host_half(n) for n in group])
        for i, name in enumerate(group):
            assert np.array_equal(got[i, ..., :3], jpeg_expected["rgb_%d" % names.index(name)]), name
            assert (got[i, ..., 3] == 255).all()


def test_decode_many_blocks_against_the_single_block_result(dev):
    """more blocks than one workgroup of the inverse-DCT kernel holds (32), spread over several images: a random coefficient block
    must decode to the same 8 x 8 samples wherever it sits (grey, 40 x 72 pixels = 45 blocks, 3 images)"""
    from nerf_pl_amd import ops
    rng = np.random.default_rng(7)
    coef = np.zeros((3, 45, 64), np.int16)
    coef[:, :, 0] = rng.integers(-60, 60, (3, 45))
    coef[:, :, 1:12] = rng.integers(-9, 10, (3, 45, 11))
    quant = rng.integers(1, 20, (3, 1, 64)).astype(np.int16)
    whole = ops.decode_jpeg_batch([torch.from_numpy(coef).to(dev)], torch.from_numpy(quant).to(dev), 72, 40).cpu().numpy()
    single = ops.decode_jpeg_batch([torch.from_numpy(coef.reshape(135, 1, 64)).to(dev)],
                                   torch.from_numpy(np.repeat(quant, 45, 0)).to(dev), 8, 8).cpu().numpy()
    tiles = whole[..., 0].reshape(3, 9, 8, 5, 8).transpose(0, 1, 3, 2, 4).reshape(135, 8, 8)
    assert np.array_equal(tiles, single[..., 0])
    assert len(np.unique(whole[..., 0])) > 50                                              # not a constant image


def test_decode_refuses_wrong_shapes(dev):
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    q = torch.ones(1, 3, 64, dtype=torch.int16, device=dev)
    y = torch.zeros(1, 4, 64, dtype=torch.int16, device=dev)
    c = torch.zeros(1, 1, 64, dtype=torch.int16, device=dev)
    assert ops.decode_jpeg_batch([y, c, c], q, 16, 16, 2, 2).shape == (1, 16, 16, 4)
    with pytest.raises(NerfHipError):
        ops.decode_jpeg_batch([y, c, c], q, 16, 16, 2, 1)                                  # 2x1 needs 2 luma blocks, not 4
    with pytest.raises(NerfHipError):
        ops.decode_jpeg_batch([y, c], q, 16, 16, 2, 2)
    with pytest.raises(NerfHipError):
        ops.decode_jpeg_batch([y, c, c], q, 16, 16, 1, 2)
    with pytest.raises(NerfHipError):
        ops.decode_jpeg_batch([y.to(torch.int32), c, c], q, 16, 16, 2, 2)
    with pytest.raises(NerfHipError):
        ops.decode_jpeg_batch([y, c, c], q[:, :1], 16, 16, 2, 2)


# ---- the dataset ---------------------------------------------------------------------------------------------------------------
def _rgb_float(u8):
    return torch.from_numpy(np.ascontiguousarray(u8)).to(torch.float32).div(255)           # ToTensor


def _kept(rays, w):
    return rays if w == 32 else rays[::RAY_STRIDE]


@pytest.fixture(scope="module")
def train(dev):
    from nerf_pl_amd.datasets import dataset_classes
    return {(mode, w): dataset_classes["llff"](SCENE, "train", (w, h), spheric_poses=(mode == "sph"), device=dev)
            for mode in ("fwd", "sph") for (w, h) in SIZES}


@pytest.mark.parametrize("w,h", SIZES)
def test_train_colours_equal_the_references_bytes(dev, expected, train, w, h):
    for mode in ("fwd", "sph"):
        ds = train[(mode, w)]
        assert ds.all_rgbs.is_cuda and ds.all_rgbs.dtype == torch.float32 and ds.all_rgbs.shape == (4 * h * w, 3)
        assert torch.equal(ds.all_rgbs.cpu(), _rgb_float(expected["rgbs_%d" % w])), (mode, w)
        assert np.array_equal(torch.round(ds.all_rgbs * 255).to(torch.uint8).cpu().numpy(), expected["rgbs_%d" % w])


def test_same_size_is_a_copy_of_the_decoded_bytes(dev, expected, train):
    """img_wh equal to the files' size: Pillow returns a copy, so the colours are the decoder's bytes / 255"""
    from PIL import Image
    val = int(expected["val_idx"].reshape(-1)[0])
    files = [p for i, p in enumerate(sorted(os.listdir(os.path.join(SCENE, "images")))) if i != val]
    want = np.concatenate([np.asarray(Image.open(os.path.join(SCENE, "images", f)).convert("RGB")).reshape(-1, 3) for f in files])
    assert np.array_equal(want, expected["rgbs_64"])
    assert torch.equal(train[("fwd", 64)].all_rgbs.cpu(), _rgb_float(want))


@pytest.mark.parametrize("mode", ("fwd", "sph"))
def test_train_split(dev, expected, train, mode):
    val = int(expected["val_idx"].reshape(-1)[0])
    for (w, h) in SIZES:
        ds = train[(mode, w)]
        assert ds.white_back is False and ds.spheric_poses == (mode == "sph") and ds.img_wh == (w, h)
        np.testing.assert_allclose(ds.poses, expected["poses"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(ds.pose_avg, expected["pose_avg"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(ds.bounds, expected["bounds"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(ds.focal, expected["%s_focal_%d" % (mode, w)], rtol=1e-15)
        assert len(ds.image_paths) == 5 and ds.directions.shape == (h, w, 3)
        assert len(ds) == 4 * h * w and ds.all_rays.shape == (4 * h * w, 8) and ds.all_rays.is_cuda
        np.testing.assert_allclose(_kept(ds.all_rays.cpu().numpy(), w), expected["%s_rays_%d" % (mode, w)], **RAY_TOL)
        near, far = ds.all_rays[:, 6].cpu(), ds.all_rays[:, 7].cpu()
        if mode == "fwd":
            assert bool((near == 0).all()) and bool((far == 1).all())
        else:
            b = expected["bounds"]
            assert bool((near == np.float32(b.min())).all()) and bool((far == np.float32(min(8 * b.min(), b.max()))).all())
    ds = train[(mode, 32)]
    # the val image is the one left out: the training poses are all poses but val_idx, in order
    from nerf_pl_amd import rays
    poses = torch.from_numpy(np.delete(ds.poses, val, 0).astype(np.float32)).to(dev)
    near, far = (0.0, 1.0) if mode == "fwd" else (float(ds.bounds.min()), float(min(8 * ds.bounds.min(), ds.bounds.max())))
    assert torch.equal(ds.all_rays, rays.gen_rays(poses, 24, 32, ds.focal, near, far, use_ndc=(mode == "fwd"), ndc_near_plane=1.0))
    item = ds[777]
    assert set(item) == {"rays", "rgbs"} and torch.equal(item["rays"], ds.all_rays[777]) and torch.equal(item["rgbs"], ds.all_rgbs[777])
    batch = ds.ray_store().sample(64, return_ids=True)
    ids = batch["ids"]
    assert batch["rays"].shape == (64, 8) and batch["rgbs"].shape == (64, 3)
    assert torch.equal(batch["rgbs"], ds.all_rgbs[ids]) and torch.equal(batch["rays"], ds.all_rays[ids])


@pytest.mark.parametrize("mode", ("fwd", "sph"))
def test_val_test_and_test_train_items(dev, expected, mode):
    from nerf_pl_amd.datasets import LLFFDataset
    spheric = mode == "sph"
    val = int(expected["val_idx"].reshape(-1)[0])
    for (w, h) in SIZES:
        ds = LLFFDataset(SCENE, "val", (w, h), spheric_poses=spheric, val_num=3, device=dev)
        assert len(ds) == 3 and ds.image_path_val.endswith("image%03d.jpg" % val)
        np.testing.assert_allclose(ds.c2w_val, expected["poses"][val], rtol=1e-10, atol=1e-12)
        item = ds[0]
        assert set(item) == {"rays", "rgbs", "c2w"}
        assert torch.equal(item["c2w"].cpu(), torch.from_numpy(ds.c2w_val.astype(np.float32))) and item["c2w"].is_cuda
        np.testing.assert_allclose(item["c2w"].cpu().numpy(), expected["poses"][val].astype(np.float32), rtol=1e-6, atol=1e-7)
        assert torch.equal(item["rgbs"].cpu(), _rgb_float(expected["val_rgbs_%d" % w]))
        np.testing.assert_allclose(_kept(item["rays"].cpu().numpy(), w), expected["%s_val_rays_%d" % (mode, w)], **RAY_TOL)
    assert len(LLFFDataset(SCENE, "val", (32, 24), spheric_poses=spheric, val_num=0, device=dev)) == 1
    ds = LLFFDataset(SCENE, "test", (32, 24), spheric_poses=spheric, device=dev)
    assert len(ds) == 120
    np.testing.assert_allclose(ds.poses_test, expected["%s_poses_test" % mode], rtol=1e-10, atol=1e-12)
    item = ds[3]
    assert set(item) == {"rays", "c2w"} and item["rays"].shape == (768, 8)
    assert torch.equal(item["c2w"].cpu(), torch.from_numpy(ds.poses_test[3].astype(np.float32)))
    np.testing.assert_allclose(item["rays"].cpu().numpy(), expected["%s_test_rays_32" % mode], **RAY_TOL)
    ds = LLFFDataset(SCENE, "test_train", (32, 24), spheric_poses=spheric, device=dev)
    assert len(ds) == 5
    np.testing.assert_allclose(ds.poses_test, expected["poses"], rtol=1e-10, atol=1e-12)
    item = ds[val]
    assert torch.equal(item["c2w"].cpu(), torch.from_numpy(ds.poses_test[val].astype(np.float32)))
    np.testing.assert_allclose(item["rays"].cpu().numpy(), expected["%s_val_rays_32" % mode], **RAY_TOL)


@pytest.mark.parametrize("w,h", SIZES)
def test_scene_with_a_png_among_the_jpegs(dev, expected, w, h):
    from nerf_pl_amd.datasets import LLFFDataset
    ds = LLFFDataset(SCENE_PNG, "train", (w, h), device=dev)
    assert sum(p.endswith(".png") for p in ds.image_paths) == 1
    assert torch.equal(ds.all_rgbs.cpu(), _rgb_float(expected["png_rgbs_%d" % w]))


def test_cpu_device_is_refused_and_small_batches_agree(dev, expected, monkeypatch):
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.datasets import LLFFDataset, llff
    with pytest.raises(NerfHipError, match="no CPU fallback"):
        LLFFDataset(SCENE, "train", (32, 24), device="cpu")
    monkeypatch.setattr(llff, "_BATCH_MAX", 2)                                             # the staging bound splits the run of files
    ds = LLFFDataset(SCENE, "train", (32, 24), device=dev)
    assert torch.equal(ds.all_rgbs.cpu(), _rgb_float(expected["rgbs_32"]))


def test_one_training_step_from_the_dataset(dev, train):
    from argparse import Namespace
    from nerf_pl_amd.system import NeRFSystem, fit
    ds = train[("fwd", 32)]
    hp = Namespace(N_samples=16, N_importance=16, use_disp=False, perturb=1.0, noise_std=0.0, chunk=1024 * 32, loss_type="mse",
                   lr=5e-4, weight_decay=0, decay_step=[100], decay_gamma=0.5)
    system = NeRFSystem(hp, train_dataset=ds).to(dev)
    assert system.white_back is False
    torch.manual_seed(0)
    losses = fit(system, [ds.ray_store().sample(64)])
    assert len(losses) == 1 and bool(torch.isfinite(losses[0]))

"""CPU: the COLMAP pose handling of nerf_pl_amd/datasets/llff.py against the arrays the reference's own LLFFDataset produced at
mint time (tests/tools/make_golden_llff.py -> tests/golden/llff_mini_expected.npz).  Everything is float64 numpy on both sides;
the only cause of a difference is operation order on O(1) values through a few dozen operations and one well-conditioned 4 x 4
inverse, hence rtol 1e-10, atol 1e-12."""
import os
import shutil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "llff_mini")
TOL = dict(rtol=1e-10, atol=1e-12)


@pytest.fixture(scope="module")
def expected():
    z = np.load(os.path.join(ROOT, "tests", "golden", "llff_mini_expected.npz"))
    return {k: z[k] for k in z.files}


def _raw_poses():
    pb = np.load(os.path.join(SCENE, "poses_bounds.npy"))
    assert pb.shape == (5, 17) and pb.dtype == np.float64
    p = pb[:, :15].reshape(-1, 3, 5)
    return np.concatenate([p[..., 1:2], -p[..., :1], p[..., 2:4]], -1), pb[:, -2:].copy(), p[0, :, -1]


def test_centering_scaling_and_the_val_index(expected):
    from nerf_pl_amd.datasets import llff
    poses, bounds, (H, W, focal) = _raw_poses()
    assert (H, W) == (48, 64)
    assert np.allclose(llff.normalize(np.array([3.0, 0.0, 4.0])), [0.6, 0.0, 0.8], rtol=1e-15)
    avg = llff.average_poses(poses)
    assert avg.shape == (3, 4)
    assert np.allclose(avg[:, :3].T @ avg[:, :3], np.eye(3), atol=1e-14)                    # an orthonormal frame
    assert np.allclose(avg[:, 3], poses[..., 3].mean(0), rtol=1e-15)
    centered, inv = llff.center_poses(poses)
    assert centered.shape == (5, 3, 4) and inv.shape == (4, 4)
    np.testing.assert_allclose(inv, expected["pose_avg"], **TOL)
    dist = np.linalg.norm(centered[..., 3], axis=1)
    assert int(np.argmin(dist)) == int(expected["val_idx"].reshape(-1)[0])
    assert np.min(np.diff(np.sort(dist))) > 1e-2                                           # ... and not by a coin toss
    scale = bounds.min() * 0.75
    centered[..., 3] /= scale
    np.testing.assert_allclose(centered, expected["poses"], **TOL)
    np.testing.assert_allclose(bounds / scale, expected["bounds"], **TOL)
    assert np.isclose(expected["bounds"].min(), 1 / 0.75, rtol=1e-15)
    for w in (64, 32, 80):
        for mode in ("fwd", "sph"):
            np.testing.assert_allclose(focal * (w / W), expected["%s_focal_%d" % (mode, w)], rtol=1e-15)


def test_spiral_and_spheric_paths(expected):
    from nerf_pl_amd.datasets import llff
    radii = np.percentile(np.abs(expected["poses"][..., 3]), 90, axis=0)
    spiral = llff.create_spiral_poses(radii, 3.5)
    assert spiral.shape == (120, 3, 4)
    np.testing.assert_allclose(spiral, expected["fwd_poses_test"], **TOL)
    circle = llff.create_spheric_poses(1.1 * expected["bounds"].min())
    assert circle.shape == (120, 3, 4)
    np.testing.assert_allclose(circle, expected["sph_poses_test"], **TOL)
    assert llff.create_spiral_poses(radii, 3.5, n_poses=7).shape == (7, 3, 4)
    for mode in ("fwd", "sph"):
        assert np.array_equal(expected["%s_poses_test_train" % mode], expected["poses"])


def test_the_dataset_refuses_a_wrong_aspect_ratio_and_the_cpu():
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.datasets import BlenderDataset, LLFFDataset, dataset_classes
    assert dataset_classes == {"blender": BlenderDataset, "llff": LLFFDataset}
    with pytest.raises(NerfHipError, match="no CPU fallback"):
        LLFFDataset(SCENE, "train", (64, 48), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(NerfHipError, match="no GPU"):
            LLFFDataset(SCENE, "train", (64, 48))
        return
    with pytest.raises(AssertionError, match="aspect ratio"):
        LLFFDataset(SCENE, "test", (64, 40))


def test_aspect_ratio_assertion_fires_before_any_device_work(monkeypatch):
    """read_meta checks img_wh against the poses file's H, W before it touches the device: observable here by letting the
    device check pass and stubbing the one device call that would follow"""
    from nerf_pl_amd import rays
    from nerf_pl_amd.datasets import LLFFDataset
    monkeypatch.setattr(rays, "get_ray_directions", lambda *a, **k: None)
    with pytest.raises(AssertionError, match="aspect ratio"):
        LLFFDataset(SCENE, "test", (64, 40), device="cuda:0")
    ds = LLFFDataset(SCENE, "test", (32, 24), device="cuda:0")                             # the right ratio passes
    assert len(ds) == 120 and ds.white_back is False and ds.focal == 57.5 * 32 / 64


def test_image_count_must_match_the_poses(tmp_path, monkeypatch):
    from nerf_pl_amd import rays
    from nerf_pl_amd.datasets import LLFFDataset
    monkeypatch.setattr(rays, "get_ray_directions", lambda *a, **k: None)
    shutil.copytree(SCENE, tmp_path / "scene")
    os.remove(tmp_path / "scene" / "images" / "image004.jpg")
    with pytest.raises(AssertionError, match="Mismatch"):
        LLFFDataset(str(tmp_path / "scene"), "val", (32, 24), device="cuda:0")

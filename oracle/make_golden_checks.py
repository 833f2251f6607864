"""Mint the fixtures of tests/test_oracle_vs_reference.py and tests/test_image_writers.py by executing the REAL reference
(kwea123/nerf_pl; its location: NERF_PL_REFERENCE, see oracle/ref_shim.py).  TEST INFRASTRUCTURE ONLY.

    python oracle/make_golden_checks.py          # writes tests/golden/reference_checks.npz

What the reference returns on the inputs those tests use, so that they compare this project against the reference without
the reference tree being present:
  * `render_rays` (models/rendering.py, through oracle/ref_shim.py) on three seeded cases that are not in reference_golden.npz;
  * `Embedding.forward` (models/nerf.py) for logscale True / False and F = 10, 4, 6;
  * `get_ray_directions` / `get_rays` / `get_ndc_rays` (datasets/ray_utils.py);
  * the bytes `save_pfm` (datasets/depth_utils.py) writes for four arrays, and what its `read_pfm` reads back from them.
Every check is made here as well before the file is written, against the oracle / nerf_pl_amd.imageio_min, with the
tolerances the tests use.
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import nerf_oracle as O  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_checks.npz")

# (seed, ray kind, N_importance, white_back, test_time, use_disp): rays of 24, 32 coarse samples, perturb = noise_std = 0
RENDER_CASES = [(301, "blender", 64, True, False, False), (302, "ndc", 32, False, True, False), (303, "blender", 0, True, False, True)]
EMB_FREQS = (10, 4, 6)
RAY_GEOM = (13, 17, 15.3, 9)                       # H, W, focal, pose seed


def render_case_key(seed, kind, N_i, white, test_time, disp):
    return "rr_%d_%s_%d_%d_%d_%d" % (seed, kind, N_i, white, test_time, disp)


def depth(h=37, w=53, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w), dtype=np.float32) * 6.0).astype(np.float32)


def pfm_arrays():
    """The arrays test_image_writers.py writes as PFM."""
    return [depth(), depth(8, 8, 3), np.stack([depth(5, 7, 1)] * 3, -1), depth(4, 6, 2)[..., None]]


def main():
    G = {}
    nerf, rend = ref_shim.load_reference()
    for case in RENDER_CASES:
        seed, kind, N_i, white, test_time, disp = case
        params = [O.make_params(seed, 6.0, 0.3), O.make_params(seed + 1, 6.0, 0.3)]
        models = []
        for p in params:
            m = nerf.NeRF()
            m.load_state_dict(p)
            models.append(m)
        rays = O.make_rays(seed, 24, kind)
        with torch.no_grad():
            ref = rend.render_rays(models, [nerf.Embedding(3, 10), nerf.Embedding(3, 4)], rays, 32, disp, 0, 0, N_i, 1024 * 32,
                                   white, test_time=test_time)
            got = O.render_rays(params, rays, 32, disp, 0, 0, N_i, white, test_time)
        assert sorted(ref.keys()) == sorted(got.keys())
        pre = render_case_key(*case)
        G[pre + "/rays"] = rays
        for k, v in ref.items():
            assert torch.allclose(got[k], v, rtol=1e-5, atol=1e-6), (case, k)
            G[pre + "/" + k] = v

    x = torch.randn(57, 3, generator=torch.Generator().manual_seed(5)) * 3
    G["emb_x"] = x
    for logscale in (True, False):
        for F in EMB_FREQS:
            v = nerf.Embedding(3, F, logscale=logscale)(x)
            assert torch.equal(O.posenc(x, F, logscale), v)
            G["emb_%d_%d" % (logscale, F)] = v

    ru = ref_shim.load_reference_ray_utils()
    H, W, focal, pose_seed = RAY_GEOM
    d = ru.get_ray_directions(H, W, focal)
    ro, rd = ru.get_rays(d, O.make_pose(pose_seed))
    no, nd = ru.get_ndc_rays(H, W, focal, 1.0, ro, rd)
    G.update({"ru_dirs": d, "ru_o": ro, "ru_d": rd, "ru_ndc_o": no, "ru_ndc_d": nd})

    spec = importlib.util.spec_from_file_location("ref_depth_utils", os.path.join(ref_shim.REFERENCE_ROOT, "datasets", "depth_utils.py"))
    du = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(du)
    from nerf_pl_amd import imageio_min as io
    with tempfile.TemporaryDirectory() as tmp:
        for i, arr in enumerate(pfm_arrays()):
            a, b = os.path.join(tmp, "a.pfm"), os.path.join(tmp, "b.pfm")
            du.save_pfm(a, arr)
            io.save_pfm(b, arr)
            raw = open(a, "rb").read()
            assert raw == open(b, "rb").read()
            data, scale = du.read_pfm(a)
            G["pfm%d_bytes" % i] = np.frombuffer(raw, dtype=np.uint8)
            G["pfm%d_read" % i] = np.ascontiguousarray(data)
            G["pfm%d_scale" % i] = np.float64(scale)

    out = {k: (v.detach().contiguous().numpy() if torch.is_tensor(v) else v) for k, v in G.items()}
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024), len(out), "arrays")


if __name__ == "__main__":
    main()

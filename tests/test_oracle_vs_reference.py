"""CPU: the oracle restatement against what the REAL reference returns (imported unmodified through oracle/ref_shim.py) on
seeded inputs that are not in reference_golden.npz.  The reference's outputs are stored in tests/golden/reference_checks.npz,
minted by oracle/make_golden_checks.py, which runs the same checks against the live reference before it writes them."""
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from oracle.make_golden_checks import EMB_FREQS, RAY_GEOM, RENDER_CASES, render_case_key

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_checks.npz")


@pytest.fixture(scope="module")
def ref():
    z = np.load(PATH, allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize("seed,kind,N_i,white,test_time,disp", RENDER_CASES)
def test_render_rays_live_reference(ref, seed, kind, N_i, white, test_time, disp):
    params = [O.make_params(seed, 6.0, 0.3), O.make_params(seed + 1, 6.0, 0.3)]
    pre = render_case_key(seed, kind, N_i, white, test_time, disp) + "/"
    rays = O.make_rays(seed, 24, kind)
    assert torch.equal(rays, ref[pre + "rays"])
    want = {k[len(pre):]: v for k, v in ref.items() if k.startswith(pre) and k != pre + "rays"}
    with torch.no_grad():                     # perturb=0, noise_std=0: the reference's randn draws are multiplied by 0
        got = O.render_rays(params, rays, 32, disp, 0, 0, N_i, white, test_time)
    assert sorted(want.keys()) == sorted(got.keys())
    for k in want:
        assert torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-6), (k, (got[k] - want[k]).abs().max().item())


@pytest.mark.parametrize("logscale", [True, False])
def test_embedding_live_reference(ref, logscale):
    """Embedding.forward incl. the `logscale=False` bands torch.linspace(1, 2^(F-1), F) (nerf.py:16-19): bit-equal."""
    x = torch.randn(57, 3, generator=torch.Generator().manual_seed(5)) * 3
    assert torch.equal(x, ref["emb_x"])
    for F in EMB_FREQS:
        assert torch.equal(O.posenc(x, F, logscale), ref["emb_%d_%d" % (logscale, F)])


def test_ray_utils_live_reference(ref):
    H, W, focal, pose_seed = RAY_GEOM
    c2w = O.make_pose(pose_seed)
    d = ref["ru_dirs"]
    assert torch.equal(O.get_ray_directions(H, W, focal), d)
    ro, rd = ref["ru_o"], ref["ru_d"]
    oo, od = O.get_rays(d, c2w)
    assert torch.equal(oo, ro) and torch.allclose(od, rd, rtol=0, atol=1e-7)
    po, pd = O.get_ndc_rays(H, W, focal, 1.0, ro, rd)
    assert torch.equal(po, ref["ru_ndc_o"]) and torch.equal(pd, ref["ru_ndc_d"])

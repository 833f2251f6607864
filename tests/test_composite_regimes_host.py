"""CPU: the trained-scene generator of tests/scenes.py (a) reaches the regimes it is for and (b) is an input on which the fp32
oracle itself stays inside the tolerances tests/test_gpu_composite_regimes.py grants the kernels — a test the reference cannot
pass would be wrong.  Prints the fp32-vs-fp64 oracle distances those tolerances are derived from (pytest -s)."""
import itertools

import pytest
import torch

from oracle import nerf_oracle as O
from tests import scenes as SC

FLT_MIN = 1.1754944e-38        # smallest normal fp32


def _fp32(B, S, kind, noise_std=0.0, white_back=False):
    rays, z, sigma, rgb = SC.trained_scene(B, S, S, kind)
    noise = SC.scene_noise(B, S, S)
    out, _, _ = SC.oracle_composite(rays, z, sigma, rgb, noise, noise_std, white_back, torch.float32)
    return rays, z, sigma, rgb, noise, out


@pytest.mark.parametrize("kind", SC.RAY_KINDS)
@pytest.mark.parametrize("B,S", [bs for bs in SC.SIZES if bs[1] >= 63])
def test_generator_reaches_the_regimes(B, S, kind):
    rays, z, sigma, rgb, noise, out = _fp32(B, S, kind)
    dn = torch.norm(rays[:, 3:6].unsqueeze(1), dim=-1)
    deltas = torch.cat([z[:, 1:] - z[:, :-1], 1e10 * torch.ones(B, 1)], -1) * dn
    alpha = 1 - torch.exp(-deltas * torch.relu(sigma))
    w = out["weights"]
    # >= 5 samples of one ray at alpha == 1.0f exactly, with further samples behind them
    n_opaque_before_last = (alpha[:, :-1] == 1.0).sum(1)
    assert int(n_opaque_before_last.max()) >= 5
    # positive subnormal weights (the fp32 oracle keeps them: 1.4e-45 is the smallest)
    sub = (w > 0) & (w < FLT_MIN)
    assert bool(sub.any())
    # a ray of exactly zero opacity
    assert bool((out["opacity"] == 0).any())
    # an interior zero-length interval
    assert bool((deltas[:, :-1] == 0).any())
    # the knee: alpha rounds to 1 while exp() is still non-zero
    e64 = torch.exp(-deltas.double() * torch.relu(sigma).double())
    assert bool(((alpha == 1.0) & (e64 > 0)).any())
    assert bool(torch.isfinite(w).all()) and bool((w >= 0).all())
    print("regimes %-7s B=%d S=%d: opaque run %d, subnormal weights %d (min %.1e), empty rays %d, zero intervals %d, knee samples %d"
          % (kind, B, S, int(n_opaque_before_last.max()), int(sub.sum()), float(w[sub].min()), int((out["opacity"] == 0).sum()),
             int((deltas[:, :-1] == 0).sum()), int(((alpha == 1.0) & (e64 > 0)).sum())))


def test_scene_kinds_are_what_they_say():
    rays, z, sigma, rgb = SC.trained_scene(48, 64, 5, "blender")
    assert rays.shape == (48, 8) and z.shape == (48, 64) and sigma.shape == (48, 64) and rgb.shape == (48, 64, 3)
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((rgb >= 0).all()) and bool((rgb <= 1).all())
    for r in range(48):
        k, s = SC.SCENE_KINDS[r % 6], sigma[r]
        if k == "empty":
            assert bool((s < 0).all())
        elif k == "solid":
            on = (s > 0).nonzero().flatten()
            assert len(on) >= 1 and bool((s[on[0]:] >= 100).all()) and bool((s[:on[0]] < 0).all())
        elif k == "single":
            assert int((s > 0).sum()) == 1 and float(s.max()) >= 1e4
        elif k == "opaque":
            assert bool((s >= 1e4).all())
        elif k == "knee":
            on = (s > 0).nonzero().flatten()
            n = min(8, 64 - int(on[0]))
            assert torch.equal(s[on[0]:on[0] + n], torch.tensor(SC.KNEE_RAMP[:n])) and bool((s[on[0] + n:] == 1e5).all())
        assert (bool(z[r, 2] == z[r, 1]) and bool(z[r, 63] == z[r, 62])) == (r % 7 == 0)
    # same arguments, same scene; the generators are seeded
    again = SC.trained_scene(48, 64, 5, "blender")
    assert all(torch.equal(a, b) for a, b in zip((rays, z, sigma, rgb), again))


def test_fp32_oracle_noise_is_inside_the_gpu_tolerances():
    """fp32 oracle against the fp64 oracle (same inputs cast to double, autograd for the gradients) on every scene the GPU tests
    use: the per-output maxima are printed, must not exceed tests/scenes.py ORACLE_FP32_NOISE (from which the GPU tolerances are
    formed), and the fp32 oracle must pass the GPU tests' own comparisons."""
    worst = {k: 0.0 for k in SC.ORACLE_FP32_NOISE}
    for (B, S), kind, noise_std, wb in itertools.product(SC.SIZES, SC.RAY_KINDS, (0.0, 1.0), (False, True)):
        rays, z, sigma, rgb = SC.trained_scene(B, S, S, kind)
        noise = SC.scene_noise(B, S, S)
        up = SC.upstream(B, S, S)
        o32, gs32, gc32 = SC.oracle_composite(rays, z, sigma, rgb, noise, noise_std, wb, torch.float32, up)
        o64, gs64, gc64 = SC.oracle_composite(rays, z, sigma, rgb, noise, noise_std, wb, torch.float64, up)
        for name in ("weights", "opacity", "rgb", "depth"):
            assert bool(torch.isfinite(o32[name]).all()), (name, S, kind)
            d = (o32[name].double() - o64[name]).abs()
            worst[name] = max(worst[name], float(d.max()))
            assert bool((d <= SC.fwd_atol(name) + SC.FWD_RTOL * o64[name].abs()).all()), (name, S, kind, noise_std, wb, float(d.max()))
        for name, g32, g64 in (("g_sigma_rel", gs32, gs64), ("g_rgb_rel", gc32, gc64)):
            assert bool(torch.isfinite(g32).all()), (name, S, kind)
            scale = float(g64.abs().max())
            d = float((g32.double() - g64).abs().max())
            assert scale >= 1e-3, (name, S, kind, scale)     # every case has gradients worth comparing
            worst[name] = max(worst[name], d / scale)
            assert d <= SC.bwd_tol(name, scale), (name, S, kind, noise_std, wb, d, scale)
            assert d <= 2e-5 * scale + 1e-7                  # the older test's bound stays an upper bound of this one
        on = SC.gate(sigma, noise, noise_std)
        assert bool((o32["weights"][~on] == 0).all()) and bool((gs32[~on] == 0).all())
    print("fp32 oracle vs fp64 oracle on the trained scenes, maxima: " + ", ".join("%s %.2e" % kv for kv in worst.items()))
    for name, v in worst.items():
        assert v <= SC.ORACLE_FP32_NOISE[name], (name, v)
    for name in SC.ORACLE_FP32_NOISE:
        assert SC.FACTOR * SC.ORACLE_FP32_NOISE[name] <= 2e-5


def test_peaked_rows_take_the_small_denominator_branch():
    """every empty bin of a peaked row has pdf = 1e-5 / (1 + M 1e-5) just below eps, and the fp32 cdf steps in units of 6e-8 or
    1.2e-7 around it: `denom < eps -> 1` (rendering.py:51) is taken by some of a row's bins and not by their neighbours.  torch.sum
    and the restated ATen order agree bit for bit there, so the GPU test's reference (total="aten") is the reference's own."""
    for M in (7, 62, 190, 511):
        w = SC.peaked_rows(M, M)
        bins = torch.sort(torch.rand(w.shape[0], M + 1, generator=torch.Generator().manual_seed(M)) * 4 + 2, -1)[0]
        cdf = O.pdf_to_cdf(w, total="aten")
        assert torch.equal(cdf, O.pdf_to_cdf(w, total="torch"))
        small = (cdf[:, 1:] - cdf[:, :-1]) < 1e-5
        n_peaked = (w.shape[0] - 1) // 2                        # (the subnormal and the all-zero rows come out uniform: 1 / M per bin)
        assert 0.3 < float(small[:n_peaked].float().mean()) < 1.0
        for u in (None, SC.tied_u(cdf, 40, M)):
            a = O.sample_pdf(bins, w, 40, u=u, total="aten")
            assert torch.equal(a, O.sample_pdf(bins, w, 40, u=u, total="torch")) and bool(torch.isfinite(a).all())
        u = SC.tied_u(cdf, 40, M)
        assert int((u[:, :, None] == cdf[:, None, :]).any(-1).sum()) >= u.shape[0] * 40 // 6      # exact ties do occur

"""GPU: the stand-alone compositing and importance-sampling kernels — the root of trust of every single-launch render and
training kernel, which are tested by being bit-identical to them — on inputs shaped like a CONVERGED scene (tests/scenes.py):
empty space, opaque samples in mid-ray with 1e-10 / 1e-20 / subnormal weights behind them, the knee where exp() is tiny but
alpha already rounds to 1, zero-length intervals, NDC rays in the backward, and pdf rows with one bin near 1.

Reference: oracle/nerf_oracle.py `composite` on the inputs cast to fp64 (autograd for the gradients).  Tolerances: 4 x the
distance of the fp32 oracle from that fp64 oracle on the same scenes, measured and asserted by
tests/test_composite_regimes_host.py (maxima over all sizes, both ray kinds, noise_std 0 / 1, both white_back values):

    output     fp32 oracle vs fp64   tolerance here
    weights    8.63e-08              3.48e-07 + 1e-5 |ref|
    opacity    2.63e-07              1.08e-06 + 1e-5 |ref|
    rgb        2.67e-07              1.08e-06 + 1e-5 |ref|
    depth      1.47e-06              6.00e-06 + 1e-5 |ref|      (blender depths 2..6, 2048 terms)
    g_sigma    9.24e-07 max|g|       3.72e-06 max|g| + 1e-7     (below the 2e-5 max|g| + 1e-7 of tests/test_gpu_parity.py)
    g_rgb      2.41e-07 max|g|       1.00e-06 max|g| + 1e-7

The factor 4 pays for the kernel's reduction order (wave butterfly against sequential), not for another arithmetic.  Gates,
emptiness and finiteness are asserted with no tolerance at all; the fused kernels and the sampling are compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import scenes as SC

pytestmark = pytest.mark.gpu

SCENES = [(B, S, kind) for (B, S) in SC.SIZES for kind in SC.RAY_KINDS]
FWD_CFGS = tuple((wb, ns) for wb in (False, True) for ns in (0.0, 1.0))
EXP_IS_ZERO = 105.0        # fp32 exp(-x) is 0 under any rounding for x > 105 (exp(-105) = 2.5e-46, a third of the smallest subnormal)


@functools.lru_cache(maxsize=None)
def _scene(B, S, kind):
    rays, z, sigma, rgb = SC.trained_scene(B, S, S, kind)
    return rays, z, sigma, rgb, SC.scene_noise(B, S, S)


@functools.lru_cache(maxsize=None)
def _ref64(B, S, kind, white_back, noise_std, grads):
    """fp64 oracle outputs (and autograd gradients for the upstream of SC.upstream) of one scene, computed once"""
    rays, z, sigma, rgb, noise = _scene(B, S, kind)
    return SC.oracle_composite(rays, z, sigma, rgb, noise, noise_std, white_back, torch.float64, SC.upstream(B, S, S) if grads else None)


def _on_device(dev, B, S, kind):
    rays, z, sigma, rgb, noise = _scene(B, S, kind)
    raw = torch.cat([rgb, sigma[..., None]], -1).contiguous()
    return raw.to(dev), z.to(dev), rays.to(dev), noise.to(dev)


def _close(got, ref, name, what):
    d = (got.double() - ref).abs()
    tol = SC.fwd_atol(name) + SC.FWD_RTOL * ref.abs()
    print("%s %s: max |kernel - fp64 oracle| %.3e (absolute part of the tolerance %.3e)" % (what, name, float(d.max()), SC.fwd_atol(name)))
    assert bool((d <= tol).all()), (what, name, float(d.max()), float((d - tol).max()))


@pytest.mark.parametrize("B,S,kind", SCENES)
def test_forward_vs_fp64_oracle(dev, B, S, kind):
    from nerf_pl_amd import ops
    rays, z, sigma, rgb, noise = _scene(B, S, kind)
    raw, zd, raysd, noised = _on_device(dev, B, S, kind)
    for wb, ns in FWD_CFGS:
        what = "fwd %s B=%d S=%d wb=%d noise=%g" % (kind, B, S, wb, ns)
        ref, _, _ = _ref64(B, S, kind, wb, ns, False)
        got = dict(zip(("weights", "opacity", "rgb", "depth"), (t.cpu() for t in ops.composite(raw, zd, raysd, noised, ns, wb))))
        for name in ("weights", "opacity", "rgb", "depth"):
            assert bool(torch.isfinite(got[name]).all()), (what, name)
            _close(got[name], ref[name], name, what)
        on = SC.gate(sigma, noise, ns)
        assert bool((got["weights"] >= 0).all()), what
        assert bool((got["weights"][~on] == 0).all()), what
        dark = ~on.any(1)                                   # rays whose every gate is shut
        assert int(dark.sum()) >= 1
        assert bool((got["opacity"][dark] == 0).all()) and bool((got["depth"][dark] == 0).all()), what
        assert bool((got["rgb"][dark] == (1.0 if wb else 0.0)).all()), what
        # the sigma-only path (raw_ch == 1): the same weights and opacity
        w1, op1 = ops.composite(raw[..., 3].contiguous(), zd, raysd, noised, ns, wb)
        _close(w1.cpu(), ref["weights"], "weights", what + " sigma-only")
        _close(op1.cpu(), ref["opacity"], "opacity", what + " sigma-only")
        assert torch.equal(w1.cpu(), got["weights"]) and torch.equal(op1.cpu(), got["opacity"]), what


def _exp_is_zero(rays, z, sigma, noise, ns):
    dn = torch.norm(rays[:, 3:6].unsqueeze(1), dim=-1)
    deltas = torch.cat([z[:, 1:] - z[:, :-1], 1e10 * torch.ones_like(z[:, :1])], -1) * dn
    s = sigma + noise * ns if ns else sigma
    return deltas * torch.relu(s) > EXP_IS_ZERO


@pytest.mark.parametrize("B,S,kind", SCENES)
def test_backward_vs_fp64_autograd(dev, B, S, kind):
    from nerf_pl_amd import ops
    rays, z, sigma, rgb, noise = _scene(B, S, kind)
    raw, zd, raysd, noised = _on_device(dev, B, S, kind)
    grgb, gdep, gop, gw = (t.to(dev) for t in SC.upstream(B, S, S))
    for wb, ns in FWD_CFGS:
        what = "bwd %s B=%d S=%d wb=%d noise=%g" % (kind, B, S, wb, ns)
        _, gs64, gc64 = _ref64(B, S, kind, wb, ns, True)
        r1 = raw.clone().requires_grad_(True)
        w, op, c, depth = ops.composite(r1, zd, raysd, noised, ns, wb)
        ((c * grgb).sum() + (depth * gdep).sum() + (op * gop).sum() + (w * gw).sum()).backward()
        g = r1.grad.cpu()
        assert bool(torch.isfinite(g).all()), what
        for name, got, ref in (("g_sigma_rel", g[..., 3], gs64), ("g_rgb_rel", g[..., :3], gc64)):
            scale = float(ref.abs().max())
            d = (got.double() - ref).abs()
            print("%s %s: max |kernel - fp64 autograd| %.3e = %.3e max|g| (tolerance %.3e)"
                  % (what, name, float(d.max()), float(d.max()) / scale, SC.bwd_tol(name, scale)))
            assert float(d.max()) <= SC.bwd_tol(name, scale), (what, name, float(d.max()), scale, np.unravel_index(int(d.argmax()), d.shape))
            assert SC.bwd_tol(name, scale) <= 2e-5 * scale + 1e-7
        on = SC.gate(sigma, noise, ns)
        assert bool((g[..., 3][~on] == 0).all()), what
        assert bool((g[..., 3][_exp_is_zero(rays, z, sigma, noise, ns)] == 0).all()), what
    # the sigma-only backward (raw_ch == 1): upstream on weights and opacity only
    r1 = raw[..., 3].contiguous().requires_grad_(True)
    w, op = ops.composite(r1, zd, raysd, noised, 1.0, False)
    ((op * gop).sum() + (w * gw).sum()).backward()
    sg = sigma.double().requires_grad_(True)
    ref = O.composite(sg, None, z.double(), rays[:, 3:6].double(), noise.double(), False)
    ((ref["opacity"] * gop.cpu().double()).sum() + (ref["weights"] * gw.cpu().double()).sum()).backward()
    scale = float(sg.grad.abs().max())
    d = (r1.grad.cpu().double() - sg.grad).abs()
    assert bool(torch.isfinite(r1.grad).all()) and float(d.max()) <= SC.bwd_tol("g_sigma_rel", scale), (float(d.max()), scale)
    assert bool((r1.grad.cpu()[~SC.gate(sigma, noise, 1.0)] == 0).all())


def _target(B, S, dev):
    return torch.rand(B, 3, generator=torch.Generator().manual_seed(S + 1)).to(dev)


def _three_launches(ops, raw, z, rays, noise, ns, wb, tgt):
    raw_m = raw.clone().requires_grad_(True)
    w, opac, rgb, depth = ops.composite(raw_m, z, rays, noise, ns, wb)
    loss, _ = ops.mse_psnr(rgb, None, tgt)
    loss.backward()
    return w.detach(), opac.detach(), rgb.detach(), depth.detach(), raw_m.grad


@pytest.mark.parametrize("kind", SC.RAY_KINDS)
@pytest.mark.parametrize("B,S", [(SC.B_SMALL, 63), (SC.B_SMALL, 64), (SC.B_SMALL, 65), (SC.B_SMALL, 192), (SC.B_MAX, SC.S_MAX)])
@pytest.mark.parametrize("white_back,noise_std", [(True, 0.0), (False, 1.0)])
def test_fused_training_kernels_are_bit_identical_on_trained_scenes(dev, B, S, kind, white_back, noise_std):
    """composite_train, composite_train_fine_z and composite_train_loss against composite -> mse_psnr -> composite_bwd (-> fine_z)"""
    from nerf_pl_amd import ops
    raw, z, rays, noise = _on_device(dev, B, S, kind)
    tgt = _target(B, S, dev)
    gs = float(np.float32(2.0) / np.float32(3 * B))
    w, opac, rgb, depth, g_raw = _three_launches(ops, raw, z, rays, noise, noise_std, white_back, tgt)
    assert bool(torch.isfinite(g_raw).all())
    w2, opac2, rgb2, depth2, g_raw2 = ops.composite_train(raw, z, rays, noise, noise_std, white_back, tgt, gs)
    for name, a, b in (("weights", w, w2), ("opacity", opac, opac2), ("rgb", rgb, rgb2), ("depth", depth, depth2), ("g_raw", g_raw, g_raw2)):
        assert torch.equal(a, b), ("composite_train", name)
    rgb_c = torch.rand(B, 3, generator=torch.Generator().manual_seed(S + 2)).to(dev)
    for coarse in (None, rgb_c):
        want = ops.mse_psnr_values(rgb if coarse is None else coarse, None if coarse is None else rgb, tgt)
        opac3, rgb3, depth3, g_raw3, out3 = ops.composite_train_loss(raw, z, rays, noise, noise_std, white_back, tgt, gs, rgb_coarse=coarse)
        for name, a, b in (("opacity", opac, opac3), ("rgb", rgb, rgb3), ("depth", depth, depth3), ("g_raw", g_raw, g_raw3), ("out3", want, out3)):
            assert torch.equal(a, b), ("composite_train_loss", name)
    if S == SC.S_MAX:
        # the stand-alone fine_z launch keeps FOUR rays' tables in 64 KB of LDS and stops short of S = 2048; the fused kernel
        # (two rays per workgroup) goes there, and its depths are the reference's on its own weights
        N = 64
        u = torch.rand(B, N, generator=torch.Generator().manual_seed(N))
        w4, opac4, rgb4, depth4, g_raw4, zf4 = ops.composite_train_fine_z(raw, z, rays, noise, noise_std, white_back, tgt, gs, N, u=u.to(dev),
                                                                          want_weights=True)
        for name, a, b in (("weights", w, w4), ("opacity", opac, opac4), ("rgb", rgb, rgb4), ("depth", depth, depth4), ("g_raw", g_raw, g_raw4)):
            assert torch.equal(a, b), ("composite_train_fine_z", N, name)
        zc = z.cpu()
        zn = O.sample_pdf(0.5 * (zc[:, :-1] + zc[:, 1:]), w.cpu()[:, 1:-1], N, u, total="aten")
        assert torch.equal(zf4.cpu(), torch.sort(torch.cat([zc, zn], -1), -1)[0])
        return
    for N in (64, 128):
        u = torch.rand(B, N, generator=torch.Generator().manual_seed(N)).to(dev)
        for uu in (None, u):
            zf = ops.fine_z(z, w, N, u=uu)
            w4, opac4, rgb4, depth4, g_raw4, zf4 = ops.composite_train_fine_z(raw, z, rays, noise, noise_std, white_back, tgt, gs, N, u=uu,
                                                                              want_weights=True)
            for name, a, b in (("weights", w, w4), ("opacity", opac, opac4), ("rgb", rgb, rgb4), ("depth", depth, depth4),
                               ("g_raw", g_raw, g_raw4), ("z_fine", zf, zf4)):
                assert torch.equal(a, b), ("composite_train_fine_z", N, name)


def _sampling_us(ref_cdf, K, seed):
    return (None, torch.rand(ref_cdf.shape[0], K, generator=torch.Generator().manual_seed(seed)), SC.tied_u(ref_cdf, K, seed + 1))


@pytest.mark.parametrize("M,K", [(7, 16), (62, 64), (62, 128), (190, 64), (511, 40)])
def test_sample_pdf_on_peaked_rows_bit_for_bit(dev, M, K):
    """cdf, searchsorted indices and samples of ops.sample_pdf_u against the oracle with the row total in ATen's order, on rows
    where almost every bin sits on the `denom < eps` knife edge and the cdf is a staircase of near-ties; u deterministic, random,
    and random with every third draw EQUAL to one of the row's cdf values"""
    from nerf_pl_amd import ops
    w = SC.peaked_rows(M, M + K)
    R = w.shape[0]
    bins = torch.sort(torch.rand(R, M + 1, generator=torch.Generator().manual_seed(M)) * 4 + 2, -1)[0]
    prev = ops.set_row_total("aten")
    try:
        for u in _sampling_us(O.pdf_to_cdf(w, total="aten"), K, M * K):
            ref, ref_cdf, _, ref_inds = O.sample_pdf(bins, w, K, u=u, return_aux=True, total="aten")
            smp, cdf, inds = ops.sample_pdf_u(bins.to(dev), w.to(dev), K, u=None if u is None else u.to(dev), return_cdf_inds=True)
            assert bool(torch.isfinite(smp).all())
            assert torch.equal(cdf.cpu(), ref_cdf), (M, K)
            assert torch.equal(inds.cpu(), ref_inds), (M, K, int((inds.cpu() != ref_inds).sum()))
            assert torch.equal(smp.cpu(), ref), (M, K)
    finally:
        ops.set_row_total(prev)


@pytest.mark.parametrize("S,N", [(64, 128), (9, 16), (600, 64)])
def test_fine_z_on_peaked_rows_bit_for_bit(dev, S, N):
    from nerf_pl_amd import ops
    mid_w = SC.peaked_rows(S - 2, S + N)
    R = mid_w.shape[0]
    g = torch.Generator().manual_seed(S)
    wc = torch.cat([torch.rand(R, 1, generator=g), mid_w, torch.rand(R, 1, generator=g)], -1).contiguous()    # the ends are not read
    z = SC.trained_scene(R, S, S + N, "blender")[1]                    # every 7th row with equal neighbours
    mid = 0.5 * (z[:, :-1] + z[:, 1:])
    prev = ops.set_row_total("aten")
    try:
        for u in _sampling_us(O.pdf_to_cdf(mid_w, total="aten"), N, S * N):
            ref, ref_cdf, _, ref_inds = O.sample_pdf(mid, mid_w, N, u=u, return_aux=True, total="aten")
            zf, zn, cdf, inds = ops.fine_z(z.to(dev), wc.to(dev), N, u=None if u is None else u.to(dev), return_new=True, return_cdf_inds=True)
            assert torch.equal(cdf.cpu(), ref_cdf) and torch.equal(inds.cpu(), ref_inds) and torch.equal(zn.cpu(), ref), (S, N)
            assert torch.equal(zf.cpu(), torch.sort(torch.cat([z, ref], -1), -1)[0]), (S, N)
    finally:
        ops.set_row_total(prev)


@pytest.mark.parametrize("kind", SC.RAY_KINDS)
def test_composite_to_sampling_end_to_end(dev, kind):
    """the kernel's OWN coarse weights of a trained scene (subnormals, exact zeros and all) through the fine-depth assembly, with
    no cap on the mismatches: bit for bit the reference's sort(cat(z, sample_pdf(z_mid, w[:, 1:-1])))"""
    from nerf_pl_amd import ops
    B, S, N = SC.B_SMALL, 64, 128
    rays, z, sigma, rgb, noise = _scene(B, S, kind)
    raw, zd, raysd, noised = _on_device(dev, B, S, kind)
    tgt = _target(B, S, dev)
    w = ops.composite(raw, zd, raysd, None, 0.0, True)[0]
    wc = w.cpu()
    assert bool(((wc > 0) & (wc < 1.1754944e-38)).any())             # subnormal weights do reach the sampling
    mid = 0.5 * (z[:, :-1] + z[:, 1:])
    prev = ops.set_row_total("aten")
    try:
        for u in (None, torch.rand(B, N, generator=torch.Generator().manual_seed(3))):
            ud = None if u is None else u.to(dev)
            want = torch.sort(torch.cat([z, O.sample_pdf(mid, wc[:, 1:-1], N, u, total="aten")], -1), -1)[0]
            assert torch.equal(ops.fine_z(zd, w, N, u=ud).cpu(), want)
            zf = ops.composite_train_fine_z(raw, zd, raysd, None, 0.0, True, tgt, 1.0 / B, N, u=ud)[-1]
            assert torch.equal(zf.cpu(), want)
    finally:
        ops.set_row_total(prev)


def test_sample_count_limit_of_the_backward_and_training_kernels(dev):
    """S = 2048 is accepted (the other tests of this file run it), S = 2049 is refused with the library's bad-argument code by
    composite's backward and by the three training entry points"""
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    B, N = 2, 16
    for S, ok in ((2048, True), (2049, False)):
        rays, z, sigma, rgb = SC.trained_scene(B, S, 1, "blender")
        raw = torch.cat([rgb, sigma[..., None]], -1).contiguous().to(dev)
        z, rays, tgt = z.to(dev), rays.to(dev), torch.rand(B, 3).to(dev)

        def bwd():
            r = raw.clone().requires_grad_(True)
            ops.composite(r, z, rays, None, 0.0, True)[2].sum().backward()
            return r.grad
        calls = (bwd,
                 lambda: ops.composite_train(raw, z, rays, None, 0.0, True, tgt, 1.0),
                 lambda: ops.composite_train_fine_z(raw, z, rays, None, 0.0, True, tgt, 1.0, N),
                 lambda: ops.composite_train_loss(raw, z, rays, None, 0.0, True, tgt, 1.0))
        for call in calls:
            if ok:
                out = call()
                assert bool(torch.isfinite(out if torch.is_tensor(out) else out[-1]).all())
            else:
                with pytest.raises(NerfHipError, match=r"code -1\b"):
                    call()

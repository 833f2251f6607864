"""Compositing / importance-sampling inputs shaped like a CONVERGED scene instead of `randn * 3`: long runs of empty space (relu
gate shut), opaque samples in mid-ray (alpha == 1.0f exactly, weights behind them 1e-10, 1e-20, ... down to fp32 subnormals and
to an underflowing fp64 running product), the knee where exp() is tiny but non-zero while alpha already rounds to 1, and
zero-length intervals — plus the pdf rows such rays hand to sample_pdf (one bin near 1, the rest 0 / 1e-10 / subnormal).
Shared by tests/test_composite_regimes_host.py (which proves the regimes are reached and measures the fp32 oracle's own rounding
noise on them) and tests/test_gpu_composite_regimes.py (whose tolerances are that noise times 4)."""
import torch

from oracle import nerf_oracle as O

RAY_KINDS = ("blender", "ndc")
S_SMALL = (2, 3, 63, 64, 65, 129, 192)          # both sides of the 64-sample wave chunks at 64, 128 and 192
B_SMALL = 48
S_MAX, B_MAX = 2048, 3                          # the largest S the backward and the training kernels accept
SIZES = tuple((B_SMALL, S) for S in S_SMALL) + ((B_MAX, S_MAX),)
KNEE_RAMP = (0.5, 5.0, 50.0, 200.0, 500.0, 2e3, 1e4, 1e5)
SCENE_KINDS = ("empty", "knee", "wild", "solid", "single", "opaque")    # ray r is of kind SCENE_KINDS[r % 6]; the first three make B_MAX

# max |fp32 oracle - fp64 oracle| per output over every (B, S) of SIZES, both ray kinds, noise_std 0 / 1 and both white_back
# values: measured, printed and asserted (as an upper bound) by tests/test_composite_regimes_host.py.  The gradients are relative
# to max |gradient| of the case.  The GPU tolerances are FACTOR x these (+ rtol 1e-5 forward, + 1e-7 absolute backward): the
# kernel reduces in another order (wave butterfly against sequential), it is not allowed another arithmetic.
ORACLE_FP32_NOISE = {"weights": 8.7e-8, "opacity": 2.7e-7, "rgb": 2.7e-7, "depth": 1.5e-6, "g_sigma_rel": 9.3e-7, "g_rgb_rel": 2.5e-7}
FACTOR = 4.0
FWD_RTOL = 1e-5
BWD_FLOOR = 1e-7


def fwd_atol(name):
    return FACTOR * ORACLE_FP32_NOISE[name]


def bwd_tol(name, scale):
    return FACTOR * ORACLE_FP32_NOISE[name] * scale + BWD_FLOOR


def trained_scene(B, S, seed, kind):
    """rays (B,8), z (B,S) sorted, sigma (B,S) raw densities, rgb (B,S,3) in [0,1].  Ray r is of kind SCENE_KINDS[r % 6]:
       empty   entirely empty (sigma <= -6: still shut under unit noise)
       knee    empty, KNEE_RAMP from a random index, then 1e5 to the end
       wild    randn * 30
       solid   empty, then from a random index on 10 ** U(2, 5)
       single  exactly one opaque sample (10 ** U(4, 5)), the rest empty
       opaque  10 ** U(4, 5) from sample 0 to the end
    and every 7th ray has z[2] = z[1] and z[S-1] = z[S-2] (S > 3): the zero-length intervals of sort(cat(z, z_new))."""
    g = torch.Generator().manual_seed(seed)
    rays = O.make_rays(seed, B, kind)
    z = O.coarse_z(rays, S, False, 1.0, torch.rand(B, S, generator=g)).clone()
    empty = -(6.0 + 10.0 * torch.rand(B, S, generator=g))
    solid = 10.0 ** (2.0 + 3.0 * torch.rand(B, S, generator=g))
    opaque = 10.0 ** (4.0 + torch.rand(B, S, generator=g))
    wild = 30.0 * torch.randn(B, S, generator=g)
    start = torch.randint(0, max(S - 1, 1), (B,), generator=g)        # a later sample always exists when S > 1
    rgb = torch.rand(B, S, 3, generator=g)
    sigma = empty.clone()
    idx = torch.arange(S)
    for r in range(B):
        k, s0 = SCENE_KINDS[r % len(SCENE_KINDS)], int(start[r])
        if k == "solid":
            sigma[r, s0:] = solid[r, s0:]
        elif k == "single":
            sigma[r, s0] = opaque[r, s0]
        elif k == "opaque":
            sigma[r] = opaque[r]
        elif k == "knee":
            ramp = torch.tensor(KNEE_RAMP)[(idx - s0).clamp(0, len(KNEE_RAMP) - 1)]
            sigma[r, s0:] = ramp[s0:]
        elif k == "wild":
            sigma[r] = wild[r]
        if r % 7 == 0 and S > 3:
            z[r, 2] = z[r, 1]
            z[r, S - 1] = z[r, S - 2]
    return rays, z.contiguous(), sigma.contiguous(), rgb.contiguous()


def scene_noise(B, S, seed):
    """the N(0,1) draws of rendering.py:152 for a scene (multiplied by noise_std by the consumer)"""
    return torch.randn(B, S, generator=torch.Generator().manual_seed(seed + 7919))


def gate(sigma, noise, noise_std):
    """the relu gate as the kernels and the fp32 reference form it: fp32 sigma + noise * noise_std > 0"""
    s = sigma if not noise_std else sigma + noise * noise_std
    return s > 0


def upstream(B, S, seed):
    """random upstream gradients on (rgb, depth, opacity, weights)"""
    g = torch.Generator().manual_seed(seed + 104729)
    return torch.randn(B, 3, generator=g), torch.randn(B, generator=g), torch.randn(B, generator=g), torch.randn(B, S, generator=g)


def oracle_composite(rays, z, sigma, rgb, noise, noise_std, white_back, dtype, grads=None):
    """O.composite in `dtype` (the inputs cast, nothing else changed); with `grads` = upstream(...) also autograd's
    (g_sigma, g_rgb).  Returns (dict of outputs, g_sigma | None, g_rgb | None), detached."""
    sg = sigma.to(dtype).clone().requires_grad_(grads is not None)
    c = None if rgb is None else rgb.to(dtype).clone().requires_grad_(grads is not None)
    nz = (noise * noise_std).to(dtype) if noise_std else None
    out = O.composite(sg, c, z.to(dtype), rays[:, 3:6].to(dtype), nz, white_back)
    if grads is None:
        return {k: v.detach() for k, v in out.items()}, None, None
    grgb, gdep, gop, gw = (t.to(dtype) for t in grads)
    ((out["rgb"] * grgb).sum() + (out["depth"] * gdep).sum() + (out["opacity"] * gop).sum() + (out["weights"] * gw).sum()).backward()
    return {k: v.detach() for k, v in out.items()}, sg.grad, c.grad


# ---------------------------------------------------------------------------------------------------- peaked pdf rows
def peaked_rows(M, seed):
    """(R, M) fp32 pdf rows as weights[:, 1:-1] looks after a surface: one bin at 1.0; two adjacent bins 0.6 / 0.4; the peak in
    the first and in the last bin; each of those again with rand * 1e-10 everywhere; each scaled to ~1e-39 (fp32 subnormals); an
    all-zero row."""
    g = torch.Generator().manual_seed(seed)
    base = []
    for pos in sorted({0, M - 1, M // 2, int(torch.randint(0, M, (1,), generator=g))}):
        row = torch.zeros(M)
        row[pos] = 1.0
        base.append(row)
    if M >= 2:
        for pos in sorted({0, M - 2, (M - 2) // 2}):
            row = torch.zeros(M)
            row[pos], row[pos + 1] = 0.6, 0.4
            base.append(row)
    base = torch.stack(base)
    dusty = base + torch.rand(base.shape, generator=g) * 1e-10
    tiny = torch.cat([base, dusty]) * 1e-39
    return torch.cat([base, dusty, tiny, torch.zeros(1, M)]).float().contiguous()


def tied_u(cdf, K, seed):
    """(R, K) uniforms in [0, 1): random draws, every third of them replaced by one of the row's own cdf values below 1 — the
    exact ties of searchsorted(side='right')"""
    g = torch.Generator().manual_seed(seed)
    R, L = cdf.shape
    u = torch.rand(R, K, generator=g)
    pick = torch.gather(cdf, 1, torch.randint(0, L, (R, K), generator=g))
    use = (torch.arange(K)[None, :] % 3 == 0) & (pick < 1.0)
    return torch.where(use, pick, u).contiguous()

"""The in-kernel ray encodings of the bf16 MLP kernels against fp64: reference, rounding intervals, a restatement of the argument
reduction, and the input families that reach its edges.  Plain numpy / torch, no GPU.

In rays mode the bf16 kernels form their own inputs: x = o + d z (two roundings, rendering.py:206-207) and the 63 + 27 channels of
embedding_xyz(x), embedding_dir(d) (nerf.py:21-38) — encode_slots in nerf_pl_amd/csrc/mlp_fwd_kernel.h, dw_encode_slab in
mlp_bwd_dw.hip.  sin / cos come from the hardware instructions, which take their argument in REVOLUTIONS, so the kernels hand them

    t = fract(rh sc) + rl sc,      vs = x (k even) or 2 x (k odd),  rh = fl(vs HI),  rl = fl(fma(vs, HI, -rh) + fl(vs LO)),  sc = 4^(k >> 1)

with HI + LO = 1 / 2 pi to 2^-57.  What is checked here:
  * enc_reference: sin / cos in fp64 of the EXACT product 2^k x (nerf.py rounds nothing there either: a power of two);
  * enc_interval: a stored bf16 value is right iff it lies between the roundings of ref - E and ref + E, E the absolute error of the
    value BEFORE its bf16 rounding (rounding is monotone); the identity channels have E = 0;
  * reduction_sim: the argument t above, operation for operation in numpy fp32, and four wrong variants of it; sim_encodings rounds
    sin / cos (2 pi t) to bf16 — the value a kernel with a PERFECT sin / cos instruction would store;
  * ray_cases: blender / ndc rays, `far` (|x| <= 64) and `knife`, whose points sit within two ulp of the places where rh sc is an
    integer (fract wraps, t leaves [0, 1)) and where sin or cos cross zero (a bf16 ulp is small there: an argument error shows)."""
import math

import numpy as np
import torch

from oracle import nerf_oracle as O
from oracle.bf16_exact import rne_bf16

K_INV_2PI_HI = np.float32(0.15915494)
K_INV_2PI_LO = np.float32(6.4206297e-9)
FRACT_MAX = np.float32(1.0 - 2.0 ** -24)                 # v_fract_f32 never returns 1.0
VARIANTS = ("no_lo", "fract_first", "no_double", "fma_xyz")
FAMILIES = ("blender", "ndc", "far", "knife")
FAR_NEAR, FAR_MAX = 7.5, 60.0                            # far = min(8 near, max): the spheric LLFF bounds
KNIFE_M_PER_K = 20


# ================================================================================================ points and reference
def ray_points(rays, z, fused=False):
    """(B S, 3) fp32 points o + d z in the kernels' flat order (ray-major), product and sum SEPARATELY rounded — torch CPU on
    rendering.py:206-207, and what nh_mul / nh_add promise.  fused=True: one rounding (the `fma_xyz` wrong kernel), to within a
    double rounding through fp64."""
    rays, z = rays.float(), z.float()
    o, d = rays[:, None, :3], rays[:, None, 3:6]
    if fused:
        return (d.double() * z.double()[:, :, None] + o.double()).float().reshape(-1, 3)
    return (o + d * z[:, :, None]).reshape(-1, 3)


def enc_reference(x, F):
    """fp64 [x, sin(2^0 x), cos(2^0 x), ..., cos(2^(F-1) x)] of the fp32 values x (n, C), channel order of nerf.py:21-38 (=
    O.posenc, which evaluates in fp32).  2^k x is exact in fp64."""
    x = x.float().double()
    out = [x]
    for k in range(F):
        out += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(out, 1)


def channel_freq(C, F):
    """frequency index k of every channel of an (n, C (2F + 1)) encoding; -1 for the identity channels"""
    return torch.tensor([-1] * C + [k for k in range(F) for _ in range(2 * C)])


def enc_interval(ref64, E):
    """(lo, hi) = (rne_bf16(ref - E), rne_bf16(ref + E)); E a number or a tensor that broadcasts (0 for identity channels)"""
    return rne_bf16(ref64 - E), rne_bf16(ref64 + E)


def enc_wrong(stored, ref64, E):
    """mask of the stored bf16 values (n, C (2F + 1)) outside their interval; the identity channels (first 3) under E = 0"""
    Ev = torch.full((ref64.shape[1],), float(E), dtype=torch.float64)
    Ev[:3] = 0.0
    lo, hi = enc_interval(ref64, Ev[None, :])
    s = stored.double()
    return (s < lo) | (s > hi)


def half_ulp_bf16(v):
    """half a bf16 ulp at |v| (fp64); v = 0: the smallest normal's"""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))          # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 1 - 7 - 1)


def needed_error(stored, ref64):
    """per element, the smallest E at which enc_interval(ref, E) holds the stored bf16 value: the distance from ref to the set of
    reals that round to `stored` (0 inside it) — a lower bound of the error the value had before its rounding"""
    s, r = stored.double(), ref64.double()
    a = s.abs()
    m, e = torch.frexp(a)
    up = torch.ldexp(torch.ones_like(a), e - 8) * (a != 0)                    # spacing of bf16 away from zero at |s| ...
    up = up.clamp_min(2.0 ** -133)                                            # (zero and the subnormals: the smallest subnormal)
    dn = torch.where(m == 0.5, up / 2, up).clamp_min(2.0 ** -133)             # ... and towards zero (halved at a power of two)
    r = torch.where(s == 0, r.abs(), r * torch.sign(s))
    return torch.maximum(torch.maximum(a - dn / 2 - r, r - a - up / 2), torch.zeros_like(a))


def per_frequency_table(stored, ref64, F):
    """[(k, share of elements != rne_bf16(ref), largest |stored - ref| in half bf16 ulps of ref, largest needed_error)] for
    k = 0 .. F-1.  A correctly rounded value is within 1.0 half ulp (references under 2^-64, where the fp32 denormal rules decide, are
    left out of that column); an argument error shows as growth of the last column with k."""
    s, kf = stored.double(), channel_freq(3, F)
    diff, units = s != rne_bf16(ref64), (s - ref64).abs() / half_ulp_bf16(ref64) * (ref64.abs() >= 2.0 ** -64)
    need = needed_error(s, ref64)
    return [(k, diff[:, kf == k].double().mean().item(), units[:, kf == k].max().item(), need[:, kf == k].max().item()) for k in range(F)]


# ================================================================================================ the reduction, restated
def hw_fract(a):
    """v_fract_f32: a - floor(a) rounded to fp32, clamped below 1.0"""
    a64 = np.asarray(a, np.float32).astype(np.float64)
    return np.minimum((a64 - np.floor(a64)).astype(np.float32), FRACT_MAX)


def reduction_sim(x, k, variant=None, fused=False):
    """The argument t (fp32, revolutions) that encode_slots hands to v_sin_f32 / v_cos_f32 for frequency k of the fp32 values x.
    fused: the compiler contracted `a b + c` wherever the source has one (rl's sum, the last step) — the last step's product is a
    power-of-two scaling, exact, so there the two roundings coincide.  variant: one of VARIANTS (`fma_xyz` changes x, not the
    reduction: pass points from ray_points(fused=True))."""
    assert variant in (None,) + VARIANTS
    x = np.asarray(x, np.float32)
    h, i = k & 1, k >> 1
    vs = np.float32(2.0) * x if (h and variant != "no_double") else x
    rh = vs * K_INV_2PI_HI
    # fma(vs, HI, -rh): the product's remainder — exact in fp64 (24 x 24 bits), one rounding to fp32
    e = (vs.astype(np.float64) * np.float64(K_INV_2PI_HI) - rh.astype(np.float64)).astype(np.float32)
    if variant == "no_lo":
        rl = np.zeros_like(rh)
    elif fused:
        rl = (vs.astype(np.float64) * np.float64(K_INV_2PI_LO) + e.astype(np.float64)).astype(np.float32)
    else:
        rl = e + vs * K_INV_2PI_LO
    sc = np.float32(4.0 ** i)
    a = hw_fract(rh) * sc if variant == "fract_first" else hw_fract(rh * sc)
    if fused:
        return (a.astype(np.float64) + rl.astype(np.float64) * np.float64(sc)).astype(np.float32)
    return a + rl * sc


def argument_error(x, k, t):
    """circular distance |2 pi t - 2^k x| in radians, fp64 (x, t fp32 arrays)"""
    want = np.asarray(x, np.float32).astype(np.float64) * 2.0 ** k / (2.0 * math.pi)
    d = np.asarray(t, np.float32).astype(np.float64) - want
    return 2.0 * math.pi * np.abs(d - np.round(d))


def sim_encodings(x, F, variant=None, fused=False):
    """(n, 3 (2F + 1)) fp64: the bf16 values a kernel with an exact sin / cos instruction stores for points x (n, 3) fp32"""
    xn = x.float().numpy()
    out = [rne_bf16(x.float().double())]
    for k in range(F):
        a = 2.0 * math.pi * torch.from_numpy(reduction_sim(xn, k, variant, fused).astype(np.float64))
        out += [rne_bf16(torch.sin(a)), rne_bf16(torch.cos(a))]
    return torch.cat(out, 1)


# ================================================================================================ input families
def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def knife_depths():
    """fp32 depths (sorted, unique): the neighbours -2 .. +2 ulp of 2 pi m / 2^k and 2 pi (m + 1/4) / 2^k, k = 0 .. 9, m spread
    geometrically up to |x| ~ 60; and 0, the smallest normal, one subnormal"""
    zs = [0.0, 2.0 ** -126, 2.0 ** -140]
    for k in range(10):
        m_max = int(FAR_MAX * 2 ** k / (2 * math.pi))
        ms = sorted(set(int(round(v)) for v in np.geomspace(1, m_max, KNIFE_M_PER_K)))
        for m in ms:
            for q in (0.0, 0.25):
                c = np.float32(2 * math.pi * (m + q) / 2 ** k)
                lo = hi = c
                zs.append(float(c))
                for _ in range(2):
                    lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
                    zs += [float(lo), float(hi)]
    return np.unique(np.array(zs, dtype=np.float32))


def knife_size():
    return int(knife_depths().size)


def ray_cases(kind, B, S, seed=0):
    """(rays (B, 8) = [o d near far], z (B, S) sorted along S), fp32"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + S)
    u = torch.rand(B, S, generator=g)
    if kind in ("blender", "ndc"):
        rays = O.make_rays(seed + 8, B, kind)
    elif kind == "far":
        o = torch.rand(B, 3, generator=g) * 8 - 4
        d = _unit(torch.randn(B, 3, generator=g))
        rays = torch.cat([o, d, torch.full((B, 1), FAR_NEAR), torch.full((B, 1), FAR_MAX)], 1)
    elif kind == "knife":
        zs = knife_depths()
        assert B * S >= zs.size, (B, S, zs.size)
        z = torch.from_numpy(zs[np.arange(B * S) % zs.size].reshape(S, B).T.copy()).sort(-1)[0]      # ray r: depths r, r + B, ...
        sign = torch.tensor([[1.0 - 2.0 * ((r >> c) & 1) for c in range(3)] for r in range(B)])
        rays = torch.cat([torch.zeros(B, 3), sign, z[:, :1], z[:, -1:]], 1)
        return rays.float().contiguous(), z.float().contiguous()
    else:
        raise ValueError(kind)
    near, far = rays[:, 6:7], rays[:, 7:8]
    z = (near + (far - near) * u).sort(-1)[0]
    return rays.float().contiguous(), z.float().contiguous()

"""CPU: oracle/ray_enc.py — what tests/test_gpu_ray_encodings.py stands on, proven without a GPU:
  * the argument reduction of encode_slots (mlp_fwd_kernel.h), restated in numpy fp32, is within a bound made of its own roundings
    of the exact argument, in either contraction form, over every input family and frequency;
  * the `knife` family reaches the edge it is built for: at every frequency some point makes v_fract wrap against a lo part of the
    opposite sign, so the argument handed to the hardware leaves [0, 1);
  * with a perfect sin / cos the unmodified reduction puts no stored bf16 value outside its fp64 interval at E = 1e-6, while each
    wrong kernel of ray_enc.VARIANTS is flagged at E_CAP — the largest error constant the GPU test may carry;
  * ray_points is the oracle's own xyz in the kernels' point order, enc_reference has posenc's channel order;
  * every GPU test shape goes through the buffer decoders."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import bf16_exact as E
from oracle import f8_exact as F
from oracle import nerf_oracle as O
from oracle import ray_enc as R

SHAPES = [(1, 1), (3, 37), (8, 32), (9, 32), (5, 192), (11, 24)]        # tests/test_gpu_ray_encodings.py
KNIFE_SHAPE = (32, 64)
E_CAP = 2e-5              # a tenth of the smallest argument error among the wrong kernels (fma_xyz: one ulp of x ~ 6: 2.4e-4 rad at k = 9)
_points = {}


def _cases(kind):
    return [KNIFE_SHAPE] if kind == "knife" else SHAPES


def _family_points(kind, fused=False):
    """all points of a family over its shapes, (n, 3) fp32"""
    if (kind, fused) not in _points:
        _points[(kind, fused)] = torch.cat([R.ray_points(*R.ray_cases(kind, B, S), fused=fused) for B, S in _cases(kind)])
    return _points[(kind, fused)]


def _reduction_bound(xmax, k):
    """radians.  fract: exact for an argument >= 0, else one rounding of a value in [0.5, 1) or the clamp under 1.0 — at most the
    spacing there; the last sum: half the spacing of [1, 2) (t may reach 1); the hi + lo pair: the constant's residue, the rounding of
    vs LO and of rl's sum, all scaled by |2^k x|."""
    u = float(np.spacing(np.float32(1.0))) / 2                                      # unit roundoff of fp32
    s = 2.0 ** k * xmax                                                              # |vs| sc
    hi, lo = Fraction(float(R.K_INV_2PI_HI)), Fraction(float(R.K_INV_2PI_LO))
    residue = abs(float(hi + lo - Fraction(1 / (2 * math.pi)))) + 2.0 ** -53         # (+ fp64's own 1 / 2 pi)
    pair = s * (residue + u * float(lo) + u * (u * float(hi) + float(lo)))
    return 2 * math.pi * (float(np.spacing(np.float32(0.5))) + float(np.spacing(np.float32(1.0))) / 2 + pair)


def test_knife_family_fits_its_shape_and_reaches_64():
    n = R.knife_size()
    assert n <= KNIFE_SHAPE[0] * KNIFE_SHAPE[1] <= 4096
    zs = R.knife_depths()
    assert zs[0] == 0.0 and (zs > 0).sum() == n - 1 and zs[1] < 2.0 ** -126 <= zs[2]       # zero, a subnormal, the smallest normal
    x = _family_points("knife")
    rays, z = R.ray_cases("knife", *KNIFE_SHAPE)
    assert torch.equal(x.abs(), z.reshape(-1, 1).expand(-1, 3))                         # x = +- z exactly
    assert set(np.unique(z.numpy())) == set(zs)                                         # every depth of the list is used
    assert 55 <= x.abs().max().item() <= 64 and 55 <= _family_points("far").abs().max().item() <= 64
    for c in range(3):
        assert (x[:, c] < 0).any() and (x[:, c] > 0).any()


def test_reduction_is_within_its_own_roundings_of_the_exact_argument():
    worst = 0.0
    for kind in R.FAMILIES:
        x = _family_points(kind).numpy().reshape(-1)
        for k in range(10):
            bound = _reduction_bound(float(np.abs(x).max()), k)
            assert bound < 1e-6                                                         # (two fp32 roundings near 1: 7.5e-7 rad)
            for fused in (False, True):
                err = R.argument_error(x, k, R.reduction_sim(x, k, None, fused)).max()
                worst = max(worst, err)
                assert err <= bound, (kind, k, fused, err, bound)
    print("  reduction: largest argument error %.4e rad (bound %.4e)" % (worst, bound))


def test_knife_makes_fract_wrap_against_the_lo_part():
    x = _family_points("knife").numpy().reshape(-1)
    for k in range(10):
        t = R.reduction_sim(x, k)
        below, above = int((t < 0).sum()), int((t >= 1).sum())
        print("  knife k=%d: t < 0 at %d points, t >= 1 at %d (min %.3e, max 1 + %.3e)" % (k, below, above, t.min(), float(t.max()) - 1))
        assert below + above > 0, k
    assert below > 0 and above > 0                                                      # both directions at the highest frequency


@pytest.mark.parametrize("kind", R.FAMILIES)
def test_unmodified_reduction_has_no_wrong_element(kind):
    x = _family_points(kind)
    ref = R.enc_reference(x, 10)
    for fused in (False, True):
        st = R.sim_encodings(x, 10, None, fused)
        assert not R.enc_wrong(st, ref, 1e-6).any(), (kind, fused)
        assert torch.equal(st[:, :3], E.rne_bf16(x.double()))
    d = x[:, :3]                                                                          # the dir encoding's four frequencies
    assert not R.enc_wrong(R.sim_encodings(d, 4), R.enc_reference(d, 4), 1e-6).any()


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_kernels_are_flagged_at_the_cap(variant):
    kf = R.channel_freq(3, 10)
    for kind in ("far", "knife"):
        x = _family_points(kind)
        ref = R.enc_reference(x, 10)
        st = R.sim_encodings(_family_points(kind, fused=True), 10) if variant == "fma_xyz" else R.sim_encodings(x, 10, variant)
        wrong = R.enc_wrong(st, ref, E_CAP)
        hi = int(wrong[:, kf >= 6].sum())
        print("  %-12s %-6s flagged at E = %.0e: %d elements at k >= 6 (%d in all)" % (variant, kind, E_CAP, hi, int(wrong.sum())))
        if variant == "fma_xyz" and kind == "knife":
            # o = 0 there: d z + 0 has one rounding either way — the family cannot see this variant, `far` has to
            assert torch.equal(_family_points(kind, fused=True), x) and hi == 0
        else:
            assert hi > 0, (variant, kind)


def test_point_order_and_channel_order():
    for kind in R.FAMILIES:
        for B, S in _cases(kind):
            rays, z = R.ray_cases(kind, B, S)
            assert rays.shape == (B, 8) and z.shape == (B, S) and rays.dtype == z.dtype == torch.float32
            assert bool((z[:, 1:] >= z[:, :-1]).all())
            xyz = rays[:, None, :3] + rays[:, None, 3:6] * z[:, :, None]                # O._infer / test_mlp_rays_vs_oracle
            got = R.ray_points(rays, z)
            assert got.dtype == torch.float32 and torch.equal(got, xyz.reshape(-1, 3))
            assert torch.equal(got.view(B, S, 3)[2 % B, 5 % S], rays[2 % B, :3] + rays[2 % B, 3:6] * z[2 % B, 5 % S])
            rn, zn = rays.numpy(), z.numpy()                                            # numpy fp32: two roundings, point p = ray * S + sample
            want = np.stack([rn[p // S, :3] + rn[p // S, 3:6] * zn[p // S, p % S] for p in range(B * S)])
            assert want.dtype == np.float32 and np.array_equal(got.numpy(), want)
    x = _family_points("blender")
    for Fq in (10, 4):
        ref = R.enc_reference(x, Fq)
        assert ref.dtype == torch.float64 and ref.shape == (x.shape[0], 3 * (2 * Fq + 1))
        # fp32 sin / cos of an argument <= 2^9 * 3: a few ulp of the argument
        assert (ref - O.posenc(x, Fq).double()).abs().max().item() <= 2.0 ** (Fq - 1) * 4 * 2.0 ** -22
        kf = R.channel_freq(3, Fq)
        assert kf.shape == (ref.shape[1],) and torch.equal(ref[:, kf == 1][:, :3], torch.sin(2.0 * x.double()))


def test_interval_and_units():
    ref = torch.tensor([[0.5, 1.0 - 2.0 ** -10, 2.0 ** -9 * 1.5, 0.0]], dtype=torch.float64)
    lo, hi = R.enc_interval(ref, 0.0)
    assert torch.equal(lo, hi) and torch.equal(lo, E.rne_bf16(ref))
    lo, hi = R.enc_interval(ref, 2.0 ** -9)
    assert lo[0, 1] == 1.0 - 2.0 ** -8 and hi[0, 1] == 1.0 and lo[0, 3] == -2.0 ** -9 and hi[0, 3] == 2.0 ** -9
    assert torch.equal(R.half_ulp_bf16(ref[0, :3]), torch.tensor([2.0 ** -9, 2.0 ** -9, 2.0 ** -17], dtype=torch.float64))
    st = E.rne_bf16(ref).expand(2, -1).clone()
    st[1, 3] = 2.0 ** -9
    w = R.enc_wrong(torch.cat([st, st], 1)[:, :7], torch.cat([ref, ref], 1)[:, :7].expand(2, -1), 2.0 ** -9)
    assert w.sum() == 0
    w = R.enc_wrong(torch.cat([st, st], 1)[:, :7], torch.cat([ref, ref], 1)[:, :7].expand(2, -1), 2.0 ** -10)
    assert w.nonzero().tolist() == [[1, 3]]                                             # (column 3 is no identity channel)
    # needed_error is the E at which the interval starts to hold the stored value: checked on a wrong kernel's values
    x = _family_points("knife")
    ref, st = R.enc_reference(x, 10)[:, 3:], R.sim_encodings(x, 10, "no_lo")[:, 3:]
    need = R.needed_error(st, ref)
    assert need.max().item() > 1e-4 and (need == 0).double().mean().item() > 0.5
    inside = lambda Ev: (st >= R.enc_interval(ref, Ev)[0]) & (st <= R.enc_interval(ref, Ev)[1])
    assert bool(inside(need * (1 + 1e-9) + 1e-15).all())                               # (just past a tie, which goes to even)
    pos = need > 1e-12
    assert not inside(need * (1 - 1e-6))[pos].any()
    assert R.needed_error(torch.tensor([0.0, 1.0, 1.0, 0.5]), torch.tensor([1e-45, 1.0 + 2.0 ** -8, 1.0 - 2.0 ** -8, 0.5 - 2.0 ** -9],
                                                                           dtype=torch.float64)).tolist() == [0.0, 0.0, 2.0 ** -9, 2.0 ** -10]


@pytest.mark.parametrize("B,S", SHAPES + [KNIFE_SHAPE])
def test_gpu_shapes_go_through_the_decoders(B, S):
    n = B * S
    tiles = (n + 255) // 256 * 8
    assert 32 * tiles >= n
    kind = "knife" if (B, S) == KNIFE_SHAPE else "far"
    rays, z = R.ray_cases(kind, B, S)
    pad = lambda t: torch.cat([t, t[-1:].expand(32 * tiles - n, -1)])
    ex = pad(R.sim_encodings(R.ray_points(rays, z), 10))
    ed = pad(R.sim_encodings(rays[:, 3:6].repeat_interleave(S, 0), 4))
    acts = {name: torch.zeros(32 * tiles, sec[3], dtype=torch.float64) for name, sec in E.act_sections().items()}
    acts.update(ex=ex, ed=ed, gate_t=torch.zeros(32 * tiles, 128, dtype=torch.bool))
    acts.update({"gate_h%d" % l: torch.zeros(32 * tiles, 256, dtype=torch.bool) for l in range(1, 9)})
    buf = E.encode_acts(acts, tiles)
    assert buf.numel() == tiles * E.act_tile_bytes()
    A = E.decode_acts(buf, tiles)
    assert torch.equal(A["ex"], ex) and torch.equal(A["ed"], ed) and not A["pad_ex"].any() and not A["pad_ed"].any()
    # the fp8 block: the encodings under scale byte 127
    t8 = {}
    for name, sec in E.act_sections().items():
        t8["q_" + name] = torch.from_numpy(F.encode_section(acts[name], np.full(tiles, 127), F.E4M3)) if name in ("ex", "ed") else \
            np.zeros((32 * tiles, sec[3]), dtype=np.int64)
        t8["scale_" + name] = np.full(tiles, 127)
    t8.update({k: v for k, v in acts.items() if k.startswith("gate_")})
    A8 = F.decode_acts_f8(F.encode_acts_f8(t8, tiles), tiles)
    for name in ("ex", "ed"):
        assert np.array_equal(np.asarray(A8["q_" + name]), np.asarray(t8["q_" + name])) and (np.asarray(A8["scale_" + name]) == 127).all()

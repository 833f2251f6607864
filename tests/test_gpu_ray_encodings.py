"""GPU: the encodings the bf16 kernels form THEMSELVES in rays mode — x = o + d z and the 63 + 27 channels of embedding_xyz(x),
embedding_dir(d), encode_slots in csrc/mlp_fwd_kernel.h: hardware v_sin_f32 / v_cos_f32 in revolutions behind a hi + lo reduction —
against fp64, and rays mode against embedded mode bit for bit.  The rounding-exact oracle (tests/test_gpu_bf16_exact.py,
test_gpu_f8_exact.py) runs mlp_fwd_embedded, whose inputs arrive encoded; this file carries its verdict over to the mode the step runs.

  (a) the saved encodings of a saving bf16 rays-mode forward, decoded (oracle/bf16_exact.decode_acts), lie in the interval
      [rne_bf16(ref - E), rne_bf16(ref + E)] of the fp64 sin / cos of the exact 2^k x (oracle/ray_enc.py), x the separately rounded
      o + d z; the identity channels EQUAL rne_bf16(x), rne_bf16(d) — the only place the un-contracted o + d z is pinned; lanes behind
      point n repeat point n - 1, padding slots are zero;
  (b) the decoded encodings fed to mlp_fwd_embedded as fp32 (bf16 values: load_slots rounds them to themselves) give the same `out`,
      the same sigma-only output and the same saved sections and gates, in 'bf16' and in 'bf16_f8'; in 'fp32' rays mode equals
      embedded mode on ops.posenc of the same points (both call sincosf / sinf, cosf on the same exact argument).
  (c) (the other copies of the arithmetic on these inputs: test_gpu_training.py::test_dw_regenerated_encodings_are_the_saved_ones_bf16,
      test_gpu_render_fused.py, their `far` / `knife` cases.)

Families (oracle/ray_enc.ray_cases): blender, ndc, far (|x| <= 64) at (B, S) = (1, 1), (3, 37), (8, 32), (9, 32), (5, 192), (11, 24);
knife — 1298 depths within two ulp of the places where fract wraps or sin / cos cross zero, x = +-z — at (32, 64).

E, the one number: the absolute error of a value before its bf16 rounding.  The instruction's accuracy is documented nowhere in the
project, so E is MEASURED against fp64 on the ladder 5e-7 2^j and fixed at twice the lowest rung with no wrong element; it must stay
<= E_CAP = 2e-5, a tenth of the smallest argument error of the wrong kernels tests/test_ray_enc_host.py shows to be flagged at E_CAP.

Measured (one MI355X run; the file's 76 cases take a few seconds, none more than 0.4 s): no wrong element on the ladder's FIRST rung, 5e-7, in any family -> rung 5e-7, E_ENC =
1e-6.  Per frequency, xyz encoding, all shapes of a family together — share of elements that are not rne_bf16(ref) / largest
|stored - ref| in half bf16 ulps of ref / smallest E whose interval holds every element:
    k   blender                 ndc                     far                     knife
    0   9e-5  1.001  1.4e-7     0     1.000  0          9e-5  1.000  8.3e-9     0.035  409.7  3.735e-7
    1   0     1.000  0          9e-5  1.001  6.8e-8     9e-5  1.003  9.9e-8     0.055  409.7  3.735e-7
    2   9e-5  1.006  2.4e-8     2.7e-4 1.003 2.0e-7     9e-5  1.292  1.4e-7     0.074  409.7  3.735e-7
    3   1.8e-4 1.007 5.1e-8     0     1.000  0          0     1.000  0          0.093  409.7  3.735e-7
    4   2.7e-4 1.031 1.3e-7     0     1.000  0          0     1.000  0          0.113  409.7  3.735e-7
    5   9e-5  1.006  2.3e-8     0     1.000  0          9e-5  1.092  4.4e-8     0.113  409.7  3.735e-7
    6   1.8e-4 1.017 3.9e-8     0     1.000  0          9e-5  1.002  5.4e-8     0.106  409.7  3.735e-7
    7   9e-5  1.002  2.7e-8     0     1.000  0          0     1.000  0          0.106  409.7  3.735e-7
    8   0     1.000  0          0     1.000  0          9e-5  1.003  9.3e-8     0.088  391.8  3.735e-7
    9   0     1.000  0          0     1.000  0          0     1.000  0          0.071  307.3  3.735e-7
and per |x| on knife: 3.735e-7 / 3.575e-7 / 3.346e-7 / 1.866e-7 in [0, 2) / [2, 8) / [8, 32) / [32, 65).  Flat in k, falling with
|x|: no argument error.  3.735e-7 is 2 pi 2^-24, one fp32 spacing of t under 1.0 — the reduction's own rounding where v_fract
wraps (the host test measures 3.745e-7 for the restated reduction alone); the hundreds of half ulps are references of ~1e-9 at a
zero crossing, where that absolute error is all there is.  fp32: rays mode EQUALS embedded mode on every element of every case.
With `rl` dropped from encode_slots alone (a scratch build, never committed): (a) fails in every case but the one-point ones (the
smallest E that fits grows to 2.7e-3 at |x| >= 32) and every case of the regenerated-encodings test fails."""
import pytest
import torch

from oracle import bf16_exact as E
from oracle import f8_exact as F
from oracle import nerf_oracle as O
from oracle import ray_enc as R
from tests.helpers import build_models

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 37), (8, 32), (9, 32), (5, 192), (11, 24)]
KNIFE_SHAPE = (32, 64)
CASES = [(kind, B, S) for kind in ("blender", "ndc", "far") for B, S in SHAPES] + [("knife",) + KNIFE_SHAPE]
E_CAP = 2e-5
E_ENC = 1e-6              # twice the measured rung (5e-7, the ladder's first)
LADDER = [5e-7 * 2 ** j for j in range(8)]
assert E_ENC <= E_CAP

_runs, _model = {}, {}
X_NAMES = ["ex", "ed"] + ["h%d" % l for l in range(1, 9)] + ["t"]
GATES = ["gate_h%d" % l for l in range(1, 9)] + ["gate_t"]


def _run(dev, kind, B, S):
    """every launch the tests compare, once per case, results on the CPU"""
    key = (kind, B, S)
    if key in _runs:
        return _runs[key]
    from nerf_pl_amd import ops
    if "m" not in _model:
        (_model["m"],), _ = build_models([O.make_params(77, 5.0, 0.2)], dev, "bf16")
    m = _model["m"]
    rays, z = R.ray_cases(kind, B, S)
    n, tiles = B * S, (B * S + 255) // 256 * 8
    rd, zd = rays.to(dev), z.to(dev)
    r = dict(kind=kind, n=n, tiles=tiles, rays=rays, z=z, xyz=R.ray_points(rays, z), dirs=rays[:, 3:6].repeat_interleave(S, 0))
    with torch.no_grad():
        # ---- bf16: rays mode, then embedded mode on the encodings rays mode saved
        p16 = m.packed_weights("bf16")
        acts, acts2 = ops.alloc_acts(n, "bf16", dev), ops.alloc_acts(n, "bf16", dev)
        out = ops.mlp_fwd_rays(rd, zd, p16, False, "bf16", save=acts)
        sig = ops.mlp_fwd_rays(rd, zd, p16, True, "bf16")
        torch.cuda.synchronize()
        A = r["A"] = E.decode_acts(acts, tiles)
        x90 = torch.cat([A["ex"][:n], A["ed"][:n]], 1).float().to(dev)
        out2 = ops.mlp_fwd_embedded(x90, p16, False, "bf16", save=acts2)
        sig2 = ops.mlp_fwd_embedded(x90[:, :63].contiguous(), p16, True, "bf16")
        torch.cuda.synchronize()
        r["A2"] = E.decode_acts(acts2, tiles)
        r["bf16"] = (out.cpu().view(n, 4), out2.cpu(), sig.cpu().view(n), sig2.cpu().view(n))
        # ---- bf16_f8: the same two runs; the embedded one is fed the BF16 rays run's encodings
        p8 = m.packed_weights("bf16_f8")
        a8, a82 = ops.alloc_acts(n, "bf16_f8", dev), ops.alloc_acts(n, "bf16_f8", dev)
        o8 = ops.mlp_fwd_rays(rd, zd, p8, False, "bf16_f8", save=a8)
        o82 = ops.mlp_fwd_embedded(x90, p8, False, "bf16_f8", save=a82)
        torch.cuda.synchronize()
        r["A8"], r["A82"] = F.decode_acts_f8(a8, tiles), F.decode_acts_f8(a82, tiles)
        r["f8"] = (o8.cpu().view(n, 4), o82.cpu())
        # ---- fp32: rays mode against embedded mode on the posenc kernel's encodings of the same points
        p32 = m.packed_weights("fp32")
        x32 = torch.cat([ops.posenc(r["xyz"].to(dev), 10), ops.posenc(r["dirs"].to(dev), 4)], 1)
        o32 = ops.mlp_fwd_rays(rd, zd, p32, False, "fp32")
        o322 = ops.mlp_fwd_embedded(x32, p32, False, "fp32")
        torch.cuda.synchronize()
        r["fp32"] = (o32.cpu().view(n, 4), o322.cpu())
    _runs[key] = r
    return r


def _report(r, name, stored, ref, Fq):
    """the ladder and the per-frequency table of one encoding; returns the lowest rung with no wrong element (None: none)"""
    counts = [int(R.enc_wrong(stored, ref, e).sum()) for e in LADDER]
    rung = next((e for e, c in zip(LADDER, counts) if c == 0), None)
    print("  %-7s n=%-4d %s: wrong per rung %s -> rung %s" % (r["kind"], r["n"], name, counts, "%.1e" % rung if rung else "none"))
    for k, share, units, need in R.per_frequency_table(stored, ref, Fq):
        print("      k=%d  != rne_bf16(ref) %.5f   max |stored - ref| %.4f half-ulp   smallest E that fits %.2e" % (k, share, units, need))
    return rung


@pytest.mark.parametrize("kind,B,S", CASES)
def test_saved_encodings_against_fp64(dev, kind, B, S):
    r = _run(dev, kind, B, S)
    n, A = r["n"], r["A"]
    ex, ed = A["ex"][:n], A["ed"][:n]
    refx, refd = R.enc_reference(r["xyz"], 10), R.enc_reference(r["dirs"], 4)
    _report(r, "xyz", ex, refx, 10)
    _report(r, "dir", ed, refd, 4)
    # the identity channels: o + d z with product and sum separately rounded, then ONE rounding to bf16
    assert torch.equal(ex[:, :3], E.rne_bf16(r["xyz"].double())), (ex[:, :3] != E.rne_bf16(r["xyz"].double())).nonzero()[:4].tolist()
    assert torch.equal(ed[:, :3], E.rne_bf16(r["dirs"].double()))
    for name, got, ref in (("xyz", ex, refx), ("dir", ed, refd)):
        wrong = R.enc_wrong(got, ref, E_ENC)
        assert not wrong.any(), (kind, name, int(wrong.sum()), wrong.nonzero()[:4].tolist())
    for name in ("ex", "ed"):
        assert torch.equal(A[name][n:], A[name][n - 1:n].expand(r["tiles"] * 32 - n, -1)), name       # padded lanes compute point n - 1
        assert not A["pad_" + name].any(), name


@pytest.mark.parametrize("kind,B,S", CASES)
def test_rays_mode_is_embedded_mode_bf16(dev, kind, B, S):
    r = _run(dev, kind, B, S)
    out, out2, sig, sig2 = r["bf16"]
    assert torch.isfinite(out).all() and torch.equal(out, out2), (out - out2).abs().max().item()
    assert torch.equal(sig, sig2), (sig - sig2).abs().max().item()
    for name in X_NAMES + GATES:
        assert torch.equal(r["A"][name], r["A2"][name]), name
    assert bool(r["A"]["gate_h8"].any())                                               # (a network that is not dead on these inputs)


@pytest.mark.parametrize("kind,B,S", CASES)
def test_rays_mode_is_embedded_mode_f8(dev, kind, B, S):
    r = _run(dev, kind, B, S)
    out, out2 = r["f8"]
    assert torch.isfinite(out).all() and torch.equal(out, out2), (out - out2).abs().max().item()
    assert torch.equal(out, r["bf16"][0])                                              # (the 8-bit copies do not feed the forward)
    for name in X_NAMES:
        assert torch.equal(torch.as_tensor(r["A8"]["scale_" + name]), torch.as_tensor(r["A82"]["scale_" + name])), name
        assert torch.equal(torch.as_tensor(r["A8"][name]), torch.as_tensor(r["A82"][name])), name
    for name in GATES:
        assert torch.equal(r["A8"][name], r["A82"][name]), name


@pytest.mark.parametrize("kind,B,S", CASES)
def test_rays_mode_is_embedded_mode_fp32(dev, kind, B, S):
    """fp32 kernels: sincosf in rays mode, the posenc kernel's sin / cos in front of embedded mode, the same exact argument 2^k x."""
    r = _run(dev, kind, B, S)
    out, out2 = r["fp32"]
    d = (out - out2).abs()
    print("  %-7s n=%-4d fp32 rays vs embedded: %d of %d differ, max %.3e" % (kind, r["n"], int((d != 0).sum()), d.numel(), d.max().item()))
    assert torch.equal(out, out2)

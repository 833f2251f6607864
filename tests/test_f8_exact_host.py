"""CPU: oracle/f8_exact.py — the 8-bit codecs, block scales and pair-piece decoder of the fp8-storage mode ('bf16_f8') — proven
without a GPU, so that tests/test_gpu_f8_exact.py can trust them:
  * the integer-arithmetic e4m3 / e5m2 codecs equal torch's CPU casts on all 65,536 bf16 patterns at every scale byte that keeps
    the quotient in range, and decode o encode is the identity on every finite code;
  * the layout it restates is the "fp8 storage" section of nerf_pl_amd/csrc/mlp_layout.h, entry by entry (tests/host/f8_maps.cpp);
  * encode -> decode of a tile block is the identity and every byte is claimed exactly once or is documented as never read;
  * the two scale rules keep every stored quotient finite: |q| < 2^8 forward, |q| <= 2^15 in the chain (whose scale comes from the
    fp32 value BEFORE the bf16 rounding, so exactly 2^15 occurs);
  * with the 8-bit rounding switched off (a format wide enough for every scaled bf16) the weight-gradient model is E.dw_job."""
import os
import subprocess

import numpy as np
import torch

from oracle import bf16_exact as E
from oracle import f8_exact as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_BITS = np.arange(65536, dtype=np.int64)


def _all_bf16():
    return torch.from_numpy((ALL_BITS << 16).astype(np.uint32).view(np.float32).copy())


def test_codecs_equal_torch_casts_on_every_bf16_pattern_and_scale():
    x = _all_bf16().double()
    finite = torch.isfinite(x).numpy()
    for fmt, dt, top in ((F.E4M3, torch.float8_e4m3fn, 448.0), (F.E5M2, torch.float8_e5m2, 57344.0)):
        compared = 0
        for Eb in range(1, 255):
            q = x / 2.0 ** (Eb - 127)
            ok = finite & (q.abs() <= top).numpy()            # in range: nothing here may overflow or saturate
            want = q.float().to(dt).view(torch.uint8).numpy().astype(np.int64)
            got = F.encode_bits(ALL_BITS, Eb, fmt)
            assert np.array_equal(F.encode_fast(ALL_BITS, Eb, fmt), got), (fmt.name, Eb)        # the table form, on every pattern
            bad = ok & (got != want)
            assert not bad.any(), (fmt.name, Eb, ALL_BITS[bad][:4], got[bad][:4], want[bad][:4])
            assert F.is_finite_code(got[ok], fmt).all(), (fmt.name, Eb)
            # decode is the exact value of the code: the nearest code cannot be further than half a quantum of the top binade
            back = F.decode_codes(got[ok], Eb, fmt)
            assert (np.abs(back - x.numpy()[ok]) <= np.maximum(np.abs(back), 2.0 ** (Eb - 127 + 1 - fmt.bias)) * 2.0 ** -(fmt.mbits + 1)).all()
            compared += int(ok.sum())
        print("%s: %d (pattern, scale) pairs equal torch's cast" % (fmt.name, compared))
        assert compared > 4_000_000


def test_decode_encode_is_the_identity_on_every_code():
    for fmt in (F.E4M3, F.E5M2):
        codes = np.arange(256, dtype=np.int64)
        live = F.is_finite_code(codes, fmt)
        assert live.sum() == (254 if fmt is F.E4M3 else 248)
        for Eb in (1, 100, 127, 141, 254):
            v = F.decode_codes(codes[live], 127, fmt)                             # every 8-bit value is a bf16 value
            t = torch.from_numpy(v)
            assert torch.equal(t.float().bfloat16().double(), t)
            assert np.array_equal(F.encode_bits(F.bf16_bits(t), 127, fmt), codes[live])
            # the scale is an exact power of two on both sides
            vs = F.decode_codes(codes[live], Eb, fmt)
            assert np.array_equal(vs, np.ldexp(v, Eb - 127))
    # truncation is a different codec (the GPU tests must notice it)
    bits = F.bf16_bits(torch.tensor([1.0625, 1.9375, -3.75, 0.0009765625 * 1.4375]))
    assert (F.encode_bits(bits, 127, F.E4M3) != F.encode_bits(bits, 127, F.E4M3.truncating())).any()
    assert (np.abs(F.decode_codes(F.encode_bits(bits, 127, F.E5M2.truncating()), 127, F.E5M2)) <= np.abs([1.0625, 1.9375, -3.75, 0.0009765625 * 1.4375])).all()


def _header_tables(tmp_path):
    exe = str(tmp_path / "f8_maps")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "nerf_pl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "f8_maps.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}


def test_python_f8_layout_equals_the_header(tmp_path):
    T = _header_tables(tmp_path)
    mine = {
        "consts": [F.kF8ActPairs, F.kF8DyPairs, F.f8_act_gate_off(), F.f8_act_scale_off(), F.f8_act_tile_bytes(), F.f8_dy_scale_off(),
                   F.f8_dy_tile_bytes(), 1, E.kActFeat, E.kDyFeat],           # (the 1: pair pieces are never interleaved)
        "f8_x_section": [F.f8_x_section(s) for s in range(E.kActSlabs)],
        "f8_dy_section": [F.f8_dy_section(s) for s in range(E.kDySlabs)],
        "f8_row_h": [F.f8_row_h(m) for m in range(16)],
        "f8_row_j": [F.f8_row_j(m) for m in range(16)],
        "row_feature": [E.chain_feature(*F.pair_row_place(m)) for m in range(32)],
    }
    assert set(T) == set(mine)
    for name in mine:
        assert T[name] == mine[name], name
    # the 32 operand rows of a pair are its 32 features, each once, and its 1024 bytes, each once
    assert sorted(mine["row_feature"]) == list(range(32))
    assert sorted(F.pair_byte(m, n) for m in range(32) for n in range(32)) == list(range(1024))
    # lane (n, h) holds [slab 2t: 8 B | slab 2t+1: 8 B] in slot order
    for m in range(32):
        s, h, j = F.pair_row_place(m)
        assert F.pair_byte(m, 5) == (32 * h + 5) * 16 + 8 * s + j
    assert max(mine["f8_x_section"]) == F.kXSections - 1 and max(mine["f8_dy_section"]) == F.kDySections - 1
    assert F.f8_x_section(E.kActFeat) == F.kXSectionFeat and F.f8_dy_section(E.kDyFeat) == F.kDySectionFeat
    assert F.kF8ActPairs == 79 and F.kF8DyPairs == 78 and F.f8_act_tile_bytes() == 89 * 1024 and F.f8_dy_tile_bytes() == 79 * 1024


def _random_blocks(tiles, seed):
    rng = np.random.default_rng(seed)

    def codes(shape, fmt):
        q = rng.integers(0, 256, size=shape, dtype=np.int64)
        return np.where(F.is_finite_code(q, fmt), q, q & 0x80)
    acts, dys = {}, {}
    for name, sec in F.x_sections().items():
        acts["q_" + name] = codes((32 * tiles, sec[3]), F.E4M3)
        acts["scale_" + name] = rng.integers(1, 255, size=tiles, dtype=np.int64)
    g = torch.Generator().manual_seed(seed)
    for l in range(1, 9):
        acts["gate_h%d" % l] = torch.rand(32 * tiles, 256, generator=g) < 0.5
    acts["gate_t"] = torch.rand(32 * tiles, 128, generator=g) < 0.5
    for name, sec in F.dy_sections().items():
        dys["q_" + name] = codes((32 * tiles, sec[3]), F.E5M2)
        dys["scale_" + name] = rng.integers(1, 255, size=tiles, dtype=np.int64)
    return acts, dys


def test_f8_encode_decode_identity_and_every_byte_accounted_for():
    tiles = 3
    acts, dys = _random_blocks(tiles, 9)
    for kind, src, enc, dec, nbytes, fmt in (("acts", acts, F.encode_acts_f8, F.decode_acts_f8, F.f8_act_tile_bytes(), F.E4M3),
                                             ("dys", dys, F.encode_dys_f8, F.decode_dys_f8, F.f8_dy_tile_bytes(), F.E5M2)):
        a, b = enc(src, tiles, fill=0x5a), enc(src, tiles, fill=0xa5)
        assert a.numel() == tiles * nbytes
        d = dec(a, tiles)
        for k, v in src.items():
            got = d[k]
            assert (torch.equal(got, v) if torch.is_tensor(v) else np.array_equal(got, v)), (kind, k)
        for name in (F.x_sections() if kind == "acts" else F.dy_sections()):
            want = F.decode_codes(src["q_" + name].reshape(tiles, 32, -1), src["scale_" + name][:, None, None], fmt)
            assert np.array_equal(d[name].numpy().reshape(tiles, 32, -1), want), (kind, name)
            assert (d["pad_" + name] == 0x5a).all()
        assert torch.equal(enc(d, tiles, fill=0x5a), a)
        claims, written, why = F.byte_claims(kind)
        assert claims.shape == (nbytes,) and claims.max() == 1
        # the two encodings differ in exactly the bytes no value claims: every claimed byte is written from the tensors
        same = (a.numpy() == b.numpy()).reshape(tiles, nbytes)
        assert np.array_equal(same, np.broadcast_to(claims == 1, same.shape)), kind
        assert not (claims[~written] != 0).any()
        # unclaimed AND written: the padding slots inside a written pair piece, nothing else
        pad = written & (claims == 0)
        assert pad.sum() == 32 * sum(int((sec[2] < 0).sum()) for sec in (F.x_sections() if kind == "acts" else F.dy_sections()).values())
    ca, wa, ya = F.byte_claims("acts")
    cd, wd, yd = F.byte_claims("dys")
    assert ca.sum() == 32 * (63 + 27 + 8 * 256 + 128) + 32 * (8 * 256 + 128) // 8 + 4 * 11
    assert cd.sum() == 32 * (3 + 1 + 128 + 8 * 256) + 4 * 11
    count = lambda y, label: int((y == label).sum())
    assert count(ya, "feat") == 8 * 1024 and count(yd, "feat") == 8 * 1024                     # pairs 67..74 / 5..12
    assert set(np.flatnonzero(ya == "feat") // 1024) == set(range(67, 75)) and set(np.flatnonzero(yd == "feat") // 1024) == set(range(5, 13))
    assert count(ya, "scale-feat") == 4 and count(yd, "scale-feat") == 4
    assert count(ya, "scale-rest") == 1024 - 48 and count(yd, "scale-rest") == 1024 - 48
    assert count(ya, "gate") == 64 * 8                  # the 128-wide dir layer has four of eight output tiles: two of four gate words
    assert int((~wa).sum()) == 8 * 1024 + 4 + 976 + 512 and int((~wd).sum()) == 8 * 1024 + 4 + 976


def test_scale_rules_keep_every_quotient_finite():
    g = torch.Generator().manual_seed(3)
    tiles = 64
    # forward rule on random blocks over the whole exponent range, and on the adversarial maximum 1.9921875 2^k
    mag = torch.randint(-130, 120, (tiles, 1, 1), generator=g).double()
    x = E.rne_bf16(torch.randn(tiles, 32, 64, generator=g).double() * 2.0 ** mag).reshape(32 * tiles, 64)
    x[::97, 3] = 0.0
    for k, tl in zip(range(-126, 127, 4), range(tiles)):
        x[32 * tl + 7, 11] = 1.9921875 * 2.0 ** k
    q, Eb, v = F.store_x(x, tiles)
    assert all(1 <= e <= 254 for e in Eb)
    assert F.is_finite_code(q, F.E4M3).all()
    # the quotient the conversion is handed is < 2^8; the e4m3 rounding is monotone and 2^8 is a code, so the stored code is <= 2^8
    quo = (x.reshape(tiles, -1) / 2.0 ** (torch.tensor(Eb).double()[:, None] - 127)).abs()
    assert quo.max().item() < 2.0 ** 8 and quo.max().item() >= 2.0 ** 7
    code = np.abs(F.decode_codes(q, 127, F.E4M3))
    assert code.max() == 2.0 ** 8                      # (1.9921875 2^k rounds up to it: still far below 448)
    assert Eb == [max(F.biased_exponent(m) - 7, 1) for m in F.tile_max(x, tiles)]
    # chain rule: the scale comes from the ungated fp32 value, the stored value is its bf16 rounding under the gate
    s = (torch.randn(tiles, 32, 64, generator=g).double() * 2.0 ** mag.clamp(-100, 100)).float().double().reshape(32 * tiles, 64)
    for tl in range(0, tiles, 2):                   # just under a power of two: rounds UP to it in bf16
        s[32 * tl + 3, 5] = float(torch.tensor(2.0 ** (tl - 20) * (1 - 2.0 ** -20)).float())
        s[32 * tl:32 * tl + 32] = s[32 * tl:32 * tl + 32].clamp(-2.0 ** (tl - 20), 2.0 ** (tl - 20) * (1 - 2.0 ** -20))
    gate = (torch.rand(32 * tiles, 64, generator=g) < 0.5).double()
    gate[3::64, 5] = 1.0
    stored = E.rne_bf16(s * gate)
    q, Eb, v = F.store_dy(stored, s, tiles)
    assert F.is_finite_code(q, F.E5M2).all()
    quo = np.abs(F.decode_codes(q, 127, F.E5M2))
    assert quo.max() == 2.0 ** 15                      # reached, never passed: "<= 2^15", not "< 2^15"
    tight = [F.bf8_scale_byte(m) for m in F.tile_max(stored, tiles)]
    assert all(e >= t - 1 for e, t in zip(Eb, tight)) and any(e == t - 1 for e, t in zip(Eb, tight))
    # a closed gate on the largest value: the scale sits ABOVE the tight one, the codes stay finite and lose range, not correctness
    gate[:] = 1.0
    gate[3::64, 5] = 0.0
    s2 = s.clone()
    s2[3::64, 5] *= 2.0 ** 6
    q2, Eb2, _ = F.store_dy(E.rne_bf16(s2 * gate), s2, tiles)
    assert F.is_finite_code(q2, F.E5M2).all()
    assert any(e > F.bf8_scale_byte(m) for e, m in zip(Eb2, F.tile_max(E.rne_bf16(s2 * gate), tiles)))


def test_without_8_bit_rounding_the_dw_model_is_the_bf16_one():
    g = torch.Generator().manual_seed(4)
    tiles = 5
    dy = E.rne_bf16(torch.randn(32 * tiles, 48, generator=g).double() * 1e-3)
    X = E.rne_bf16(torch.randn(32 * tiles, 80, generator=g).double().abs())
    Edy, EX = F.chain_scales(dy, tiles), F.forward_scales(X, tiles)
    wide = F.dw_job_f8(F.encode_section(dy, Edy, F.WIDE), Edy, F.encode_section(X, EX, F.WIDE), EX, F.WIDE, F.WIDE)
    for a, b in zip(wide, E.dw_job(dy, X)):
        assert torch.equal(a, b)
    real = F.dw_job_f8(F.encode_section(dy, Edy, F.E5M2), Edy, F.encode_section(X, EX, F.E4M3), EX)
    rel = ((real[0] - wide[0]).norm() / wide[0].norm()).item()
    print("dW of e5m2 x e4m3 operands against the bf16 operands: relative L2 %.4f" % rel)
    assert 1e-3 < rel < 0.15
    # a wrong decoder is far outside that: dY read as e4m3, one tile under its neighbour's scale
    as_e4m3 = F.dw_job_f8(F.encode_section(dy, Edy, F.E5M2), Edy, F.encode_section(X, EX, F.E4M3), EX, fdy=F.E4M3)
    assert not torch.isfinite(as_e4m3[0]).all() or ((as_e4m3[0] - wide[0]).norm() / wide[0].norm()).item() > 0.5


def test_f8_model_sits_in_the_band_recorded_for_the_kernels():
    """tests/test_gpu_training.py gates the bf16_f8 gradients at relative L2 <= 0.15 of the bf16 gradients: the model of the mode
    has to be as far from the bf16 model, and it has to differ from it (it does round)."""
    p, x, g_out = E.embedded_case(256)
    net = E.Net(p)
    f, grads = F.model_gradients(net, x, g_out)
    ref = E.backward(net, E.forward(net, x), g_out)["grads"]
    rels = {k: ((grads[k] - ref[k]).norm() / ref[k].norm()).item() for k in ref}
    print("f8 model vs bf16 model, relative L2 per tensor: %.4f .. %.4f" % (min(rels.values()), max(rels.values())))
    assert max(rels.values()) <= 0.15 and min(rels.values()) >= 1e-4, rels

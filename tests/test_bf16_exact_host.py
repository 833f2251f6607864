"""CPU: oracle/bf16_exact.py — the rounding-exact model of the bf16 MLP kernels and the decoder of their saved buffers — proven
without a GPU, so that tests/test_gpu_bf16_exact.py can trust both:
  * with every rounding off the model IS NeRF.forward and its backward (fp64 autograd through the oracle): the fold algebra, the
    skip and dir concatenations and the chain are right;
  * the index maps it restates are those of nerf_pl_amd/csrc/mlp_layout.h, entry by entry (tests/host/bf16_maps.cpp prints them);
  * encode -> decode is the identity and every byte of a tile block is read by exactly one decoded value or is documented padding;
  * with rounding on, its distance to the fp32 oracle is the one this project recorded for the kernels (a mis-stated rounding model
    would leave that band);
  * the share of elements a teacher-forced layer check has to excuse (fp32 accumulation order against fp64) stays under the cap
    the GPU test allows, measured where no GPU is needed."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import bf16_exact as E
from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXCUSED_CAP = 1e-3        # tests/test_gpu_bf16_exact.py: at most this share of a layer's elements may need the rounding-boundary excuse


def test_without_rounding_the_model_is_fp64_autograd():
    p, x, g_out = E.embedded_case(33)
    pr = {k: v.double().requires_grad_(True) for k, v in p.items()}
    xr = x.double().requires_grad_(True)
    out = O.mlp_forward(pr, xr)
    (out * g_out.double()).sum().backward()
    net = E.Net(p, E.Rounding(on=False))
    f = E.forward(net, x.double())
    b = E.backward(net, f, g_out)
    rel = lambda a, r: ((a - r).norm() / r.norm()).item()
    assert rel(f["out"], out.detach()) <= 1e-12
    assert set(b["grads"]) == set(pr) and len(pr) == 24
    for k in pr:
        assert b["grads"][k].shape == pr[k].grad.shape and rel(b["grads"][k], pr[k].grad) <= 1e-12, k
    assert rel(b["dx"], xr.grad) <= 1e-12


def _header_tables(tmp_path):
    exe = str(tmp_path / "bf16_maps")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "nerf_pl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "bf16_maps.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}


def test_python_index_maps_equal_the_header(tmp_path):
    T = _header_tables(tmp_path)
    slots = lambda slabs, fn: [fn(ks, h, j) for ks in range(slabs) for h in range(2) for j in range(8)]
    mine = {
        "consts": [E.kXyzCh, E.kDirCh, E.kW, E.kXyzSlabs, E.kDirSlabs, E.kPieceBytes, E.kActEncX, E.kActEncD, E.kActH0, E.kActFeat, E.kActT,
                   E.kActSlabs, E.kMaskPieces, E.kMaskPieceT, E.kDyRgb, E.kDyDir, E.kDyFeat, E.kDySigma, E.kDyH0, E.kDySlabs,
                   E.act_mask_off(), E.act_tile_bytes(), E.dy_tile_bytes(), 1, E.kNumLayers, E.kSigmaLayer, E.kDirLayer,
                   E.bias_block_start(), E.bias_block_pieces()],          # (the 1: the decoder's default il is the header's kActIl)
        "act_h": [E.act_h(l) for l in range(1, 9)],
        "dy_h": [E.dy_h(l) for l in range(1, 9)],
        "mask_piece_h": [l - 1 for l in range(1, 9)],
        "chain_feature": slots(16, E.chain_feature),
        "xyz_slot_channel": slots(E.kXyzSlabs, E.xyz_slot_channel),
        "dir_slot_channel": slots(E.kDirSlabs, E.dir_slot_channel),
        "gate_word": [E.gate_word(i) for i in range(128)],
        "gate_bit": [E.gate_bit(i) for i in range(128)],
        "tile_block_off": [E.tile_block_off(t, E.act_tile_bytes(), il) for il in (1, 8) for t in range(20)],
        "layers": [v for L in range(E.kNumLayers) for v in list(E.kLayers[L]) + [E.layer_start(L)]],
        "layer_in_col": [E.layer_in_col(L, ks, h, j) for L in range(E.kNumLayers) for ks in range(E.layer_slabs(L)) for h in range(2)
                         for j in range(8)],
        "dw_jobs": [v for jb in E.kDwJobs for v in jb],
    }
    assert set(T) == set(mine)
    for name in mine:
        assert len(T[name]) == len(mine[name]), name
        bad = [i for i, (a, b) in enumerate(zip(T[name], mine[name])) if a != b]
        assert not bad, (name, bad[:8])


def _random_saved_tensors(tiles, seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda *s: E.rne_bf16(torch.randn(*s, generator=g).double())
    acts = {name: bf(32 * tiles, sec[3]) for name, sec in E.act_sections().items()}
    for l in range(1, 9):
        acts["gate_h%d" % l] = torch.rand(32 * tiles, 256, generator=g) < 0.5
    acts["gate_t"] = torch.rand(32 * tiles, 128, generator=g) < 0.5
    dys = {name: bf(32 * tiles, sec[3]) for name, sec in E.dy_sections().items()}
    return acts, dys


def test_encode_decode_identity_and_every_byte_accounted_for():
    tiles = 3
    acts, dys = _random_saved_tensors(tiles, 5)
    ba, bd = E.encode_acts(acts, tiles), E.encode_dys(dys, tiles)
    assert ba.numel() == tiles * E.act_tile_bytes() and bd.numel() == tiles * E.dy_tile_bytes()
    da, dd = E.decode_acts(ba, tiles), E.decode_dys(bd, tiles)
    for k, v in acts.items():
        assert torch.equal(da[k], v), k
    for k, v in dys.items():
        assert torch.equal(dd[k], v), k
    # a second encoding of what was decoded is the same bytes (the maps are bijections onto the claimed bytes)
    assert torch.equal(E.encode_acts(da, tiles), ba) and torch.equal(E.encode_dys(dd, tiles), bd)
    # the interleaved block addressing (kActIl = 8) holds the same pieces elsewhere
    il, per = 8, E.act_tile_bytes() // E.kPieceBytes
    src = E.encode_acts({k: torch.cat([v] * 3)[:32 * 8] for k, v in acts.items()}, 8).numpy().reshape(8, per, E.kPieceBytes)
    inter = np.zeros(8 * E.act_tile_bytes(), dtype=np.uint8)
    for t in range(8):
        for p in range(per):
            o = E.tile_block_off(t, E.act_tile_bytes(), il) + p * il * E.kPieceBytes
            inter[o:o + E.kPieceBytes] = src[t, p]
    d8 = E.decode_acts(torch.from_numpy(inter), 8, il=8)
    assert torch.equal(d8["h5"], torch.cat([acts["h5"]] * 3)[:256]) and torch.equal(d8["gate_t"], torch.cat([acts["gate_t"]] * 3)[:256])
    for kind, nbytes in (("acts", E.act_tile_bytes()), ("dys", E.dy_tile_bytes())):
        claims, padding = E.byte_claims(kind)
        assert claims.shape == (nbytes,) and claims.max() == 1
        assert np.array_equal(claims == 1, ~padding)          # claimed once XOR documented padding, no byte left over
    # what is claimed: 63 + 27 + 8 * 256 + 128 values + 9 gate sets / 3 + 1 + 128 + 8 * 256 values
    assert E.byte_claims("acts")[0].sum() == 2 * 32 * (63 + 27 + 8 * 256 + 128) + 32 * (8 * 256 + 128) // 8
    assert E.byte_claims("dys")[0].sum() == 2 * 32 * (3 + 1 + 128 + 8 * 256)


def test_rounding_helpers():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.3, 0.0, 1e-30], dtype=torch.float64)
    want = x.float().bfloat16().double()
    want[3] = 1.0 + 2.0 ** -7                       # just above a tie: one rounding goes up (fp64 -> fp32 -> bf16 would tie to even)
    assert torch.equal(E.rne_bf16(x), want)
    assert torch.equal(E.rne_bf16(x)[[1, 2]], torch.tensor([1.0, 1.0 + 2.0 ** -6], dtype=torch.float64))     # ties to even
    t = E.trunc_bf16(x)
    assert bool((t.abs() <= x.abs()).all()) and torch.equal(t.float().bfloat16().double(), t)


@pytest.fixture(scope="module")
def case1000():
    p, x, g_out = E.embedded_case(1000)
    net = E.Net(p)
    f = E.forward(net, x)
    return p, x, g_out, net, f, E.backward(net, f, g_out)


def test_rounded_model_sits_in_the_band_recorded_for_the_kernels(case1000):
    """tests/test_gpu_bf16.py records a relative L2 error of 0.111-0.117 (gate 0.15) between the bf16 kernels' gradients and the fp32
    oracle's at n = 1000 / 4096: a model of those kernels has to be as far from the fp32 oracle, no further."""
    p, x, g_out, net, f, b = case1000
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = O.mlp_forward(pr, x)
    (out * g_out).sum().backward()
    rels = {k: ((b["grads"][k] - pr[k].grad.double()).norm() / pr[k].grad.double().norm()).item() for k in pr}
    print("rounded model vs fp32 oracle, relative L2 per tensor: %.4f .. %.4f" % (min(rels.values()), max(rels.values())))
    assert max(rels.values()) <= 0.15, rels
    assert max(rels.values()) >= 0.02            # ... and it does round: the fp32 oracle itself would sit at ~1e-6
    assert (f["out"] - out.detach().double()).abs().max().item() <= 3e-2


def test_excused_share_of_a_teacher_forced_layer_stays_under_the_cap():
    """The GPU test compares a layer's stored output with bf16(relu(fp64 sum)) and excuses an element only where the fp64
    pre-activation is within K 2^-24 sum|terms| of a rounding boundary (or of zero).  Here the 'kernel' is the model itself with
    fp32 accumulation, in two summation orders, at n = 512: every element is exact or excused (the bound is a worst case), and the
    excused share stays far below the cap — so the cap can only be reached by a kernel that is wrong."""
    p, x, g_out = E.embedded_case(512)
    net = E.Net(p)
    f = E.forward(net, x)
    b = E.backward(net, f, g_out)
    worst = 0.0
    for mode in ("f32", "f32perm"):
        acc = E.Accumulate(mode, seed=7)
        for l in range(1, 9):
            pre, terms = E.pre_trunk(net, l, f["X"][l])
            got = E.activation(net, E.pre_trunk(net, l, f["X"][l], acc)[0])
            K = f["X"][l].shape[1] + 1
            exact, excused, wrong = E.judge(net, got, pre, terms, K, relu=True)
            assert not wrong.any(), (mode, l, int(wrong.sum()))
            assert ((E.pre_trunk(net, l, f["X"][l], acc)[0] - pre).abs() <= K * E.U32 * terms).all()
            worst = max(worst, excused.double().mean().item())
        for l in range(7, 0, -1):
            gate = (f["h"][l] > 0).double()
            _, s, terms = E.chain_trunk(net, l, b["dY"][l + 1], gate)
            got = E.chain_trunk(net, l, b["dY"][l + 1], gate, acc)[0]
            exact, excused, wrong = E.judge(net, got, s, terms, 256, gate=gate)
            assert not wrong.any(), (mode, "chain", l)
            worst = max(worst, excused.double().mean().item())
    print("largest excused share of a layer (fp32 accumulation, two orders, against fp64): %.2e" % worst)
    assert worst <= EXCUSED_CAP / 4
    # one swapped pair of columns: no excuse covers it (an element outside its interval fails the GPU check outright, whatever
    # its share: with these weights most of a column is zero on both sides of the swap)
    got = f["h"][3].clone()
    got[:, [17, 18]] = f["h"][3][:, [18, 17]]
    pre, terms = E.pre_trunk(net, 3, f["X"][3])
    exact, excused, wrong = E.judge(net, got, pre, terms, 257, relu=True)
    assert wrong.any() and wrong.double().mean().item() > worst

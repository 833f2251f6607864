"""GPU: the fp8-storage mode ('bf16_f8') — the SV == 2 saving forward, the F8 backward chain, mlp_bwd_dw_f8_kernel, the F8 reduce
and the fold — against oracle/f8_exact.py (codecs, scale rules, pair / scale decoder: proven on the CPU in
tests/test_f8_exact_host.py), stage by stage on the operands each stage actually consumed.

One cached run per size does the saving forward, the chain (phases = 1) and dW + reduce + fold (phases = 6) in 'bf16' AND in
'bf16_f8' on the same E.embedded_case(n) inputs; the f8 forward and chain run twice, over buffers filled with 0x5a and with 0xa5.
Both modes issue the same bf16 MFMAs in the same order (mlp_fwd_kernel.h run_layer_pipe; mlp_bwd_chain.hip run_bwd_layer_tm:
tile-major, slabs ascending, zero-initialised accumulator, with kChainDepth = 0 as with 2 — the depth only moves the LDS reads), so
the bf16 run's saved activations and dY ARE the f8 run's registers before the 8-bit store.  The checks:
  (a) anchors, exact: `out` of both modes equal; the nine gate pieces byte-identical; the encodings under scale byte 127; every byte
      the layout does not claim still the fill byte, every byte it writes equal in both fills; every scale dword in 1..254 with zero
      upper bytes; no NaN / Inf code; behind point n every dY code +-0 and X the codes of point n - 1;
  (b) forward storage, bit-exact: scale byte = f8_scale_byte(largest bf16 magnitude of the section over the whole tile), every code
      = encode_e4m3(bf16 activation, that scale); no element excused;
  (c) chain storage: every code = encode_e5m2(bf16 dY, stored scale byte), no element excused; the scale byte bracketed by
      bf8_scale_byte(max |ungated fp64 sum| -+ K 2^-24 sum|terms|) — the kernel takes it from its ungated fp32 accumulators — and
      at least the tight scale of the stored gated values, less one where their maximum is an exact power of two (a value just under
      2^k rounds UP to it in bf16 after the scale was taken: the stored quotient is then exactly 2^15, finite in e5m2); seeds: tight;
  (d) the 24 gradients within (B ceil(n / 64) + c) 2^-24 sum_p |dY X| of the fp64 sum over the DECODED f8 operands (F.dw_job_f8),
      c = 8 + splits, carried through the fold as in the bf16 file; B = 4 x the measured worst error of ONE scaled fp8 MFMA per
      64-point block (MFMA_BLOCK_UNITS below) — the fp32-sum form (n + c) does not hold for this instruction: the kernel sits at
      0.008 / 43.6 / 20.8 / 3.7 / 4.0 / 0.86 / 0.12 of it at the seven sizes, the instruction alone at up to 85; accumulate = 1 at n = 33;
  (e) two models of different sizes and parameters in one mlp_bwd_multi launch: (d) per model on its own operands;
  (f) end to end against the model's own bf16 tensors stored and decoded by the two scale rules, bound built as in the bf16 file.
Sizes: 1 (one live lane of T0, T1 of the pair all padding), 33 (both K blocks of one MFMA), 64 (one tile pair), 256, 288, 1000 and
the smallest n at which the BF16_F8 plan gives a job two point splits.  Measured ratios of one run: DESIGN.md section 6."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import bf16_exact as E
from oracle import f8_exact as F
from tests.helpers import build_models
from tests.test_gpu_bf16_exact import _dw_checks, _ratio, _rel

pytestmark = pytest.mark.gpu

SIZES = [1, 33, 64, 256, 288, 1000, "split"]
FILLS = (0x5a, 0xa5)
U = E.U32
_runs = {}
X_NAMES = ["ex", "ed"] + ["h%d" % l for l in range(1, 9)] + ["t"]
DY_NAMES = ["rgb", "sigma", "dir"] + ["dy%d" % l for l in range(8, 0, -1)]


def _splits(ns):
    from nerf_pl_amd import _lib
    out = (ctypes.c_int * (12 * len(ns)))()
    total = _lib.load().nerfhip_mlp_dw_plan((ctypes.c_int64 * len(ns))(*ns), len(ns), _lib.BF16_F8, out, None)
    assert total > 0
    return list(out)


def _split_size():
    """smallest n whose BF16_F8 plan has a job with >= 2 point splits (the plan depends on n through its whole forward workgroups)"""
    for k in range(1, 80):
        n = 256 * (k - 1) + 1
        if max(_splits([n])) >= 2:
            return n
    return None


def _f8_forward_and_chain(ops, m, xd, gd, n, dev):
    """the f8 saving forward and chain, once per fill byte: [(out, acts, dys)] on the CPU, + the device handles of the last run"""
    packed, packed_bwd = m.packed_weights_train("bf16_f8")
    acts = ops.alloc_acts(n, "bf16_f8", dev)
    ws, got = {}, []
    for fill in FILLS:
        acts.fill_(fill)
        out = ops.mlp_fwd_embedded(xd, packed, False, "bf16_f8", save=acts)
        if "dys" not in ws:
            ops.mlp_bwd(gd, out, packed_bwd, acts, "bf16_f8", phases=1, workspace=ws)          # (allocates the dY buffer)
        ws["dys"].fill_(fill)
        ops.mlp_bwd(gd, out, packed_bwd, acts, "bf16_f8", phases=1, workspace=ws)
        torch.cuda.synchronize()
        got.append((out.cpu(), acts.cpu(), ws["dys"].cpu()))
    return got, (packed_bwd, acts, ws, out)


def _run(dev, n, seed=21):
    if n == "split":
        n = _split_size()
        # (the f8 plan counts tile PAIRS: about twice the bf16 plan's 2817)
        assert n is not None and n <= 20000, n
    if (n, seed) in _runs:
        return _runs[(n, seed)]
    from nerf_pl_amd import ops
    from oracle import nerf_oracle as O
    p, x, g_out = E.embedded_case(n)
    if seed != 21:
        p = O.make_params(seed, 3.0, 0.1)
    (m,), _ = build_models([p], dev, "bf16")
    xd, gd = x.to(dev), g_out.to(dev)
    tiles = (n + 255) // 256 * 8
    # ---- bf16
    packed, packed_bwd = m.packed_weights_train("bf16")
    acts = ops.alloc_acts(n, "bf16", dev)
    out = ops.mlp_fwd_embedded(xd, packed, False, "bf16", save=acts)
    ws = {}
    ops.mlp_bwd(gd, out, packed_bwd, acts, "bf16", phases=1, workspace=ws)
    torch.cuda.synchronize()
    r = dict(n=n, tiles=tiles, p=p, x=x, g_out=g_out, out16=out.cpu(), acts16=acts.cpu(), A16=E.decode_acts(acts, tiles),
             D16=E.decode_dys(ws["dys"], tiles), splits=_splits([n]))
    Ws, Bs = E.decode_packed_fwd(packed)
    r["net"] = E.Net(p, wc=Ws[E.kDirLayer][:, :256], bc=Bs[E.kDirLayer][:128])
    # ---- bf16_f8
    fills, (pb8, acts8, ws8, out8) = _f8_forward_and_chain(ops, m, xd, gd, n, dev)
    gw, gb, flat = ops.mlp_bwd(gd, out8, pb8, acts8, "bf16_f8", phases=6, workspace=ws8)
    torch.cuda.synchronize()
    assert fills[0][1].numel() == tiles * F.f8_act_tile_bytes() and fills[0][2].numel() == tiles * F.f8_dy_tile_bytes()
    r["fills"] = fills
    r["out"] = fills[-1][0]
    r["A"], r["D"] = F.decode_acts_f8(fills[-1][1], tiles), F.decode_dys_f8(fills[-1][2], tiles)
    r["grads"] = {}
    for i, name in enumerate(E.PARAM_ORDER):
        r["grads"][name + ".weight"], r["grads"][name + ".bias"] = gw[i].cpu().double(), gb[i].cpu().double()
    r["dev_handles"] = (m, pb8, acts8, ws8, gd, out8, gw, gb, xd)
    _runs[(n, seed)] = r
    return r


def _tile_blocks(buf, tiles, nbytes):
    return buf.numpy().reshape(tiles, nbytes)


@pytest.mark.parametrize("n", SIZES)
def test_anchors(dev, n):
    r = _run(dev, n)
    n, tiles, A, D, A16 = r["n"], r["tiles"], r["A"], r["D"], r["A16"]
    assert torch.equal(r["out"], r["out16"]) and torch.equal(r["fills"][0][0], r["out16"])
    for kind, idx, nbytes in (("acts", 1, F.f8_act_tile_bytes()), ("dys", 2, F.f8_dy_tile_bytes())):
        claims, written, why = F.byte_claims(kind)
        a, b = _tile_blocks(r["fills"][0][idx], tiles, nbytes), _tile_blocks(r["fills"][1][idx], tiles, nbytes)
        for label in sorted(set(why[~written])):
            sel = why == label
            assert (a[:, sel] == FILLS[0]).all() and (b[:, sel] == FILLS[1]).all(), (kind, label)      # never written
        # every byte the layout writes was written in both runs (the kernels are deterministic; a byte left alone differs)
        diff = (a != b)[:, written]
        assert not diff.any(), (kind, int(diff.sum()), sorted(set(np.flatnonzero(written)[np.nonzero(diff)[1]] // 1024))[:8])
    # gates: byte-identical to the bf16 run's (claimed bytes; the others are not written by either)
    gclaim = E.byte_claims("acts")[0][E.kActSlabs * E.kPieceBytes:] > 0
    g16 = r["acts16"].numpy().reshape(tiles, E.act_tile_bytes())[:, E.kActSlabs * E.kPieceBytes:]
    g8 = _tile_blocks(r["fills"][1][1], tiles, F.f8_act_tile_bytes())[:, F.f8_act_gate_off():F.f8_act_scale_off()]
    assert np.array_equal(g16[:, gclaim], g8[:, gclaim])
    for name in ["h%d" % l for l in range(1, 9)] + ["t"]:
        assert torch.equal(A["gate_" + name], A16["gate_" + name]), name
    # encodings: the fixed scale 2^0, the e4m3 codes of bf16(x)
    for name, cols in (("ex", slice(0, 63)), ("ed", slice(63, 90))):
        assert (A["scale_" + name] == 127).all(), name
        want = F.encode_bits(F.bf16_bits(E.rne_bf16(r["x"][:, cols].double())), 127, F.E4M3)
        assert np.array_equal(A["q_" + name][:n], want), name
    for S, names, fmt in ((A, X_NAMES, F.E4M3), (D, DY_NAMES, F.E5M2)):
        for name in names:
            sc = S["scale_" + name]
            assert ((sc >= 1) & (sc <= 254)).all(), (name, [hex(int(v)) for v in sc[(sc < 1) | (sc > 254)][:4]])
            assert F.is_finite_code(S["q_" + name], fmt).all() and F.is_finite_code(S["pad_" + name], fmt).all(), name
            assert not S["pad_" + name].any(), name                                   # padding slots: +0
    live_end = min(32 * ((n + 31) // 32), 32 * tiles)
    for name in DY_NAMES:
        assert not (D["q_" + name][n:] & 0x7f).any(), name                            # behind point n: +-0, contributes nothing
    for name in X_NAMES:
        q = A["q_" + name]
        assert (q[n:live_end] == q[n - 1]).all(), name                                # same tile, same scale: point n - 1 again
        if live_end < 32 * tiles:                                                     # whole padding tiles: point n - 1 under their own scale
            rest = F.encode_section(A16[name][live_end:], A["scale_" + name][live_end // 32:] & 0xff, F.E4M3)
            assert np.array_equal(q[live_end:], rest), name
            assert torch.equal(A16[name][live_end:], A16[name][n - 1:n].expand(32 * tiles - live_end, -1)), name


@pytest.mark.parametrize("n", SIZES)
def test_forward_storage_is_bit_exact(dev, n):
    r = _run(dev, n)
    tiles, A, A16 = r["tiles"], r["A"], r["A16"]
    for name in X_NAMES[2:]:
        want_scale = np.array(F.forward_scales(A16[name], tiles))
        got_scale = A["scale_" + name]
        assert np.array_equal(got_scale, want_scale), (name, np.flatnonzero(got_scale != want_scale)[:8].tolist())
        want = F.encode_section(A16[name], want_scale, F.E4M3)
        bad = A["q_" + name] != want
        assert not bad.any(), (r["n"], name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    for name in X_NAMES[:2]:
        assert np.array_equal(A["q_" + name], F.encode_section(A16[name], [127] * tiles, F.E4M3)), name
    print("  n=%d forward storage: %d codes and %d scale bytes equal" % (r["n"], sum(A["q_" + k].size for k in X_NAMES), 11 * tiles))


def _ungated(r):
    """{dY section: (ungated fp64 sum, fp32 bound)} of the chain layers on the bf16 run's decoded operands, first n points"""
    n, net, A, D = r["n"], r["net"], r["A16"], r["D16"]
    one = lambda name: torch.ones_like(A["gate_" + name][:n], dtype=torch.float64)
    out = {}
    _, s, terms = E.chain_dir(net, D["rgb"][:n], one("t"))
    out["dir"] = (s, 3 * U * terms)
    _, s, terms = E.chain_h8(net, D["dir"][:n], D["sigma"][:n], one("h8"))
    out["dy8"] = (s, 129 * U * terms)
    for l in range(7, 0, -1):
        _, s, terms = E.chain_trunk(net, l, D["dy%d" % (l + 1)][:n], one("h%d" % l))
        out["dy%d" % l] = (s, 256 * U * terms)
    return out


def _pad_rows(t, rows):
    return torch.cat([t, torch.zeros(rows - t.shape[0], t.shape[1], dtype=t.dtype)], 0)


@pytest.mark.parametrize("n", SIZES)
def test_chain_storage(dev, n):
    r = _run(dev, n)
    tiles, D, D16 = r["tiles"], r["D"], r["D16"]
    differ = 0
    for name in DY_NAMES:
        want = F.encode_section(D16[name], D["scale_" + name] & 0xff, F.E5M2)
        bad = D["q_" + name] != want
        differ += int(bad.sum())
        assert not bad.any(), (r["n"], name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    # seeds: stored as slabs, their scale is the tight one
    for name in ("rgb", "sigma"):
        assert np.array_equal(D["scale_" + name], np.array([F.bf8_scale_byte(v) for v in F.tile_max(D16[name], tiles)])), name
    above, pow2 = [], 0
    for name, (s, bound) in _ungated(r).items():
        got = D["scale_" + name]
        hi = [F.bf8_scale_byte(v) for v in F.tile_max(_pad_rows(s.abs() + bound, 32 * tiles), tiles)]
        lo = [F.bf8_scale_byte(v) for v in F.tile_max(_pad_rows((s.abs() - bound).clamp_min(0), 32 * tiles), tiles)]
        stored_max = F.tile_max(D16[name], tiles)
        tight = [F.bf8_scale_byte(v) for v in stored_max]
        for tl in range(tiles):
            assert lo[tl] <= got[tl] <= hi[tl], (r["n"], name, tl, lo[tl], int(got[tl]), hi[tl])
            p2 = stored_max[tl] > 0 and np.frexp(stored_max[tl])[0] == 0.5            # an exact power of two: may have rounded up to it
            assert got[tl] >= tight[tl] - (1 if p2 else 0), (r["n"], name, tl, int(got[tl]), tight[tl])
            pow2 += int(got[tl] < tight[tl])
            above.append(int(got[tl]) - tight[tl])
        quo = np.abs(F.decode_codes(D["q_" + name], 127, F.E5M2))
        assert quo.max() <= 2.0 ** 15, name
    above = np.array(above)
    print("  n=%d chain storage: codes differing from encode_e5m2(bf16 dY) %d; scale above the tight one by 0 / 1 / 2+ units in %d / %d / %d "
          "of %d blocks (largest %d), below it (maximum rounded up to a power of two) in %d" %
          (r["n"], differ, int((above == 0).sum()), int((above == 1).sum()), int((above >= 2).sum()), above.size, int(above.max()), pow2))


def _f8_view(r):
    """the run as tests.test_gpu_bf16_exact._dw_checks reads it: A / D are the DECODED f8 operands (fp64)"""
    return dict(n=r["n"], net=r["net"], A=r["A"], D=r["D"], grads=r["grads"])


# v_mfma_scale_f32_32x32x64_f8f6f4 does not add its 64 products like an fp32 sum: measured on an MI355X with
# tools/probes/probe_fp8_accum.hip (one MFMA per trial, random finite e5m2 x e4m3 codes and block scales, 524,288 results per
# distribution, against fp64), its worst error is 4989 (C = 0) / 5431 (C != 0) units of 2^-24 (sum |products| + |C|) when the
# operands span their whole range — the products are aligned to the largest and lose their low bits — and 1.3 - 2.0 units when they
# lie within four binades.  The bound therefore carries 4 x the larger figure per 64-point block in the place of the 64 fp32 units
# of that block; the fp32 form (n + c), which the kernel misses at most sizes, is printed next to it.
MFMA_BLOCK_UNITS = 4 * 5432


def _c_eff(n, c):
    """c' with n + c' = MFMA_BLOCK_UNITS ceil(n / 64) + c: _dw_checks forms its bound as (n + c') 2^-24 sum|dY X|"""
    return MFMA_BLOCK_UNITS * ((n + 63) // 64) + c - n


def _check_dw(r, c, tag=""):
    worst, worst32 = 0.0, 0.0
    as_fp32 = {name: _ratio(got, ref, bound) for name, got, ref, bound in _dw_checks(_f8_view(r), c)}
    for name, got, ref, bound in _dw_checks(_f8_view(r), _c_eff(r["n"], c)):
        assert got.shape == ref.shape, name
        assert torch.isfinite(got).all(), name
        q = _ratio(got, ref, bound)
        worst, worst32 = max(worst, q), max(worst32, as_fp32[name])
        print("  n=%d%s %-28s error / bound %.4f (of the fp32-sum form: %.3f)" % (r["n"], tag, name, q, as_fp32[name]))
        assert q <= 1.0, (r["n"], name, q)
    print("  n=%d%s worst dW error / bound %.4f (of the fp32-sum form: %.3f)" % (r["n"], tag, worst, worst32))
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_weight_gradients_teacher_forced(dev, n):
    r = _run(dev, n)
    c = 8 + max(r["splits"])
    print("  n=%d: splits per job %s" % (r["n"], r["splits"]))
    if n == "split":
        assert max(r["splits"]) >= 2
    # _dw_checks forms E.dw_job of the decoded operands: that IS F.dw_job_f8 of the codes and scale bytes
    nn, A, D = r["n"], r["A"], r["D"]
    tl = (nn + 31) // 32
    a = F.dw_job_f8(D["q_dy3"][:32 * tl], D["scale_dy3"][:tl] & 0xff, A["q_h2"][:32 * tl], A["scale_h2"][:tl] & 0xff)
    b = E.dw_job(D["dy3"][:32 * tl], A["h2"][:32 * tl])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _check_dw(r, c)


def test_accumulate_adds_a_second_backward(dev):
    from nerf_pl_amd import _lib
    r = _run(dev, 33)
    m, pb8, acts8, ws8, gd, out8, gw, gb, _ = r["dev_handles"]
    gwp = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in gw])
    gbp = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in gb])
    with torch.cuda.device(out8.device):
        _lib.check(_lib.load().nerfhip_mlp_bwd_phases(_lib.ptr(gd), _lib.ptr(out8), 33, _lib.ptr(pb8), _lib.ptr(acts8), _lib.ptr(ws8["dys"]),
                                                      _lib.ptr(ws8["ws"]), gwp, gbp, 1, _lib.BF16_F8, 7, _lib.stream_ptr()), "nerfhip_mlp_bwd_phases")
        torch.cuda.synchronize()
    c = 8 + max(r["splits"])
    i = {name: j for j, name in enumerate(E.PARAM_ORDER)}
    for name, _, ref, bound in _dw_checks(_f8_view(r), _c_eff(33, c + 2)):
        base, kind = name.rsplit(".", 1)
        got = (gw if kind == "weight" else gb)[i[base]].cpu().double()
        q = _ratio(got, 2 * ref, 2 * bound)
        assert q <= 1.0, (name, q)
    # (the cached first-call gradients were copied to the CPU before this call: the other tests are unaffected)


def test_two_models_in_one_launch(dev):
    """mlp_bwd_multi with two entries of different sizes and parameters: the per-model indexing of the sigma fold
    (fold_of[(jid / kNumDwJobs) * kNumDwJobs + kDwJobSigma]) and the per-job buffer pointers"""
    from nerf_pl_amd import ops
    ra, rb = _run(dev, 33), _run(dev, 288, seed=22)
    entries = []
    for r in (ra, rb):
        m, pb8, acts8, ws8, gd, out8, _, _, xd = r["dev_handles"]
        entries.append((gd, out8, pb8, acts8))
    wsm = {}
    grads = ops.mlp_bwd_multi(entries, "bf16_f8", workspace=wsm)
    torch.cuda.synchronize()
    (dys, _), = wsm.values()
    splits = _splits([33, 288])
    c = 8 + max(splits)
    for k, r in enumerate((ra, rb)):
        # the chain ran again on the same inputs: the same dY blocks, byte for byte, where the layout writes
        _, written, _ = F.byte_claims("dys")
        got = dys[k].cpu().numpy().reshape(r["tiles"], -1)[:, written]
        assert np.array_equal(got, _tile_blocks(r["fills"][1][2], r["tiles"], F.f8_dy_tile_bytes())[:, written]), k
        view = _f8_view(r)
        view["grads"] = {}
        for i, name in enumerate(E.PARAM_ORDER):
            view["grads"][name + ".weight"], view["grads"][name + ".bias"] = grads[k][0][i].cpu().double(), grads[k][1][i].cpu().double()
        _check_dw(view, c, tag=" (model %d of 2)" % k)
    # the two models' gradients are not each other's
    assert not torch.equal(grads[0][2], grads[1][2])


@pytest.mark.parametrize("n", SIZES)
def test_end_to_end_against_the_model(dev, n):
    """The f8 model run on its own bf16 tensors (F.model_gradients: no teacher forcing) against the kernels' 24 gradients; bound as in
    tests/test_gpu_bf16_exact.py: 8 x the model's own sensitivity to the order of its fp32 sums (two orders against fp64, which here
    includes the 8-bit codes and block scales that flip on a one-digit bf16 difference) + the loosest bound of (d).  A tensor whose
    bound is not below 1 (100 % of the tensor) says nothing: it is printed, not asserted — with the MFMA's measured error in (d) that
    is every tensor from n = 1000 on (measured there: <= 2.9e-3 at n = 1000, <= 6.4e-3 at n = 5889; asserted at n <= 288)."""
    r = _run(dev, n)
    net, x, g_out = r["net"], r["x"], r["g_out"]
    _, g64 = F.model_gradients(net, x, g_out)
    c = 8 + max(r["splits"])
    loosest = max((bound.norm() / ref.norm().clamp_min(1e-300)).item() for _, _, ref, bound in _dw_checks(_f8_view(r), _c_eff(r["n"], c)))
    sens = {k: 0.0 for k in g64}
    if loosest < 1.0:                                # (otherwise no tensor has a usable bound: the sensitivity runs would decide nothing)
        for mode in ("f32", "f32perm"):
            _, g = F.model_gradients(net, x, g_out, acc=E.Accumulate(mode, seed=11))
            for k in sens:
                sens[k] = max(sens[k], _rel(g[k], g64[k]))
    fails = []
    for k in sens:
        bound, got = 8 * sens[k] + loosest, _rel(r["grads"][k], g64[k])
        usable = bound < 1.0
        print("  n=%d %-28s relative L2 %.3e, %s" % (r["n"], k, got, "bound %.3e (model's own %.3e)" % (bound, sens[k]) if usable else
                                                     "NOT ASSERTED: the bound of (d) alone is %.2e of the tensor" % loosest))
        if usable and got > bound:
            fails.append((k, got, bound))
    assert not fails, (r["n"], fails)

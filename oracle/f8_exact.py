"""The fp8-storage half (dtype 'bf16_f8') of the rounding-exact model: the 8-bit codecs, the block scales and a decoder of the pair
pieces and scale dwords the activation-saving forward and the backward chain leave for mlp_bwd_dw_f8_kernel.  Plain numpy / torch,
integer arithmetic for the codecs, fp64 accumulation, no GPU.  oracle/bf16_exact.py (E below) holds the bf16 arithmetic this mode
shares with the bf16 mode: both issue the same bf16 MFMAs, so every activation and dY is the same bf16 value BEFORE it is stored.

What only this mode does, as the code has it (nerf_pl_amd/csrc/f8_store.h, mlp_fwd_kernel.h SV == 2, mlp_bwd_chain.hip F8):
  * a slab PAIR (2t, 2t+1) — 32 features x 32 points — is one 1 KiB piece: lane (h, n) = 32 h + n holds 16 code bytes,
    [slab 2t: slots j = 0..7 | slab 2t+1: slots j = 0..7]; ds_read_b64_tr_b8 hands the MFMA operand row m = slab 2t + (m >> 4),
    half f8_row_h(m & 15), slot f8_row_j(m & 15);
  * X (activations, encodings) is OCP e4m3 (fn: no infinities, 0x7f NaN), dY is OCP e5m2; a stored code is
    round-to-nearest-even(x / 2^(E-127)) with subnormals, E the e8m0 scale byte of the (32-point tile, section);
  * forward rule: E = max(Emax - 7, 1), Emax the biased exponent of the largest STORED bf16 magnitude of the section over the whole
    tile (padded lanes included), so |q| < 2^8 <= 448; the encodings use E = 127;
  * chain rule: E = max(Emax - 14, 1), Emax the biased exponent of the largest UNGATED fp32 accumulator of the section — taken
    before the bf16 rounding and before the ReLU gate — so a stored value may round up to exactly 2^15 (< 57344, an e5m2 normal) and
    the scale may sit above the tight one; the rgb / sigma seeds take it from their bf16 slabs (tight);
  * each scale is one dword (the byte, zero-extended) at index f8_x_section / f8_dy_section of the tile block's last KiB;
  * the dW kernel multiplies decode(dY) decode(X) on v_mfma_scale_f32_32x32x64_f8f6f4 — exact products, fp32 accumulation — two
    tiles (K = 64 points) per MFMA, the reduce kernel maps operand rows back with f8_row_h / f8_row_j.
The layout constants restate the "fp8 storage" section of mlp_layout.h; tests/test_f8_exact_host.py compares them with the header
entry by entry (tests/host/f8_maps.cpp)."""
import math

import numpy as np
import torch

from oracle import bf16_exact as E

# ================================================================================================ mlp_layout.h "fp8 storage", restated
kF8ActPairs = E.kActSlabs // 2
kF8DyPairs = E.kDySlabs // 2
kXSections, kDySections = 12, 12                      # scale dwords of a tile block (one of each belongs to the unsaved `feat`)
kXSectionFeat, kDySectionFeat = 10, 2


def f8_act_gate_off():
    return kF8ActPairs * E.kPieceBytes


def f8_act_scale_off():
    return f8_act_gate_off() + E.kMaskPieces * E.kPieceBytes


def f8_act_tile_bytes():
    return f8_act_scale_off() + E.kPieceBytes


def f8_dy_scale_off():
    return kF8DyPairs * E.kPieceBytes


def f8_dy_tile_bytes():
    return f8_dy_scale_off() + E.kPieceBytes


def f8_x_section(slab):
    if slab < E.kActEncD:
        return 0
    if slab < E.kActH0:
        return 1
    if slab < E.kActFeat:
        return 2 + (slab - E.kActH0) // 16
    return 10 if slab < E.kActT else 11


def f8_dy_section(slab):
    if slab < E.kDyDir:
        return 0
    if slab < E.kDyFeat:
        return 1
    if slab < E.kDySigma:
        return 2
    return 3 if slab < E.kDyH0 else 4 + (slab - E.kDyH0) // 16


def f8_row_h(m):
    return (m >> 3) & 1


def f8_row_j(m):
    return m & 7


def pair_row_place(m):
    """operand row m (0..31) of a pair piece -> (slab of the pair 0 / 1, half h, slot j): where ds_read_b64_tr_b8 takes it from"""
    return m >> 4, f8_row_h(m & 15), f8_row_j(m & 15)


def pair_byte(m, n):
    """byte offset inside a pair piece of operand row m, point n: lane (h, n) = 32 h + n, 16 B per lane, [slab 2t | slab 2t+1]"""
    s, h, j = pair_row_place(m)
    return (32 * h + n) * 16 + 8 * s + j


# ================================================================================================ codecs
class Format:
    """a sign / exponent / mantissa float of at most 31 bits as integer codes.  nan_from: the smallest magnitude code that is not a
    finite number (e4m3fn: 0x7f, the single NaN; e5m2: 0x7c, infinity)."""

    def __init__(self, name, ebits, mbits, bias, nan_from, nearest=True):
        self.name, self.ebits, self.mbits, self.bias, self.nan_from, self.nearest = name, ebits, mbits, bias, nan_from, nearest
        self.sign = 1 << (ebits + mbits)

    def truncating(self):
        """round toward zero (NOT what v_cvt_scalef32_pk_* does: tests use it to show that they notice)"""
        return Format(self.name + "-trunc", self.ebits, self.mbits, self.bias, self.nan_from, nearest=False)


E4M3 = Format("e4m3", 4, 3, 7, 0x7f)
E5M2 = Format("e5m2", 5, 2, 15, 0x7c)
# wide enough to hold every scaled bf16 exactly: with it the 8-bit rounding is switched off and only the plumbing is left
WIDE = Format("wide", 11, 7, 1023, 0x7ff << 7)


def bf16_bits(t):
    """bf16-valued tensor (any float dtype) -> int64 numpy array of the 16-bit patterns"""
    a = t.detach().cpu().float().contiguous().numpy().view(np.uint32)
    assert not (a & 0xffff).any(), "not bf16 values"
    return (a >> 16).astype(np.int64)


def encode_bits(bits, Eb, fmt):
    """bf16 bit patterns (int64 array) and scale byte(s) Eb (broadcastable) -> codes of round(x / 2^(Eb - 127)) in `fmt` (int64).
    Integer arithmetic throughout: x = M 2^ex with an 8-bit integer M; the code's quantum is 2^qe; the quotient M 2^(ex' - qe) is
    rounded to nearest, ties to even.  A magnitude that rounds past the largest finite number gives fmt.nan_from (the hardware
    conversions do not saturate either)."""
    bits = np.asarray(bits, dtype=np.int64)
    Eb = np.broadcast_to(np.asarray(Eb, dtype=np.int64), bits.shape)
    s, e, m = (bits >> 15) & 1, (bits >> 7) & 0xff, bits & 0x7f
    M = np.where(e > 0, m | 0x80, m)
    ex = np.where(e > 0, e, 1) - 127 - 7 - (Eb - 127)                 # x / scale = M 2^ex
    msb = np.zeros_like(M)
    for k in range(1, 8):
        msb = np.where(M >> k > 0, k, msb)
    te = msb + ex                                                      # exponent of the leading bit
    emin = 1 - fmt.bias
    normal = te >= emin
    qe = np.maximum(te, emin) - fmt.mbits
    sh = qe - ex                                                       # right shift of M to units of the quantum (< 0: left)
    left = np.clip(-sh, 0, 40)
    right = np.clip(sh, 0, 40)
    Ml = M << left
    if fmt.nearest:
        half = np.where(right > 0, np.int64(1) << np.maximum(right - 1, 0), 0)
        R = np.where(right > 0, (Ml + half - 1 + ((Ml >> right) & 1)) >> right, Ml)
    else:
        R = Ml >> right
    one = 1 << fmt.mbits
    mag = np.where(normal, ((te + fmt.bias) << fmt.mbits) + R - one, R)  # (a carry to 2 * one moves into the exponent field by itself)
    mag = np.where(M == 0, 0, mag)
    bad = (e == 0xff) | (mag >= fmt.nan_from)
    mag = np.where(bad, fmt.nan_from, mag)
    return mag | (s * fmt.sign)


def decode_codes(q, Eb, fmt):
    """codes (int array) under scale byte(s) Eb -> fp64 numpy array q 2^(Eb - 127); non-finite codes give NaN"""
    q = np.asarray(q, dtype=np.int64)
    mag = q & (fmt.sign - 1)
    ef, mf = mag >> fmt.mbits, mag & ((1 << fmt.mbits) - 1)
    v = np.where(ef == 0, mf, mf | (1 << fmt.mbits)).astype(np.float64)
    v = np.ldexp(v, (np.where(ef == 0, 1, ef) - fmt.bias - fmt.mbits).astype(np.int64))
    v = np.ldexp(v, np.broadcast_to(np.asarray(Eb, dtype=np.int64) - 127, q.shape))
    v = np.where(q & fmt.sign, -v, v)
    return np.where(mag >= fmt.nan_from, np.nan, v)


def is_finite_code(q, fmt):
    return (np.asarray(q, dtype=np.int64) & (fmt.sign - 1)) < fmt.nan_from


def biased_exponent(v):
    """the fp32 / bf16 biased exponent field of |v| (a Python float or 0-d tensor): 0 for zero and the subnormal range"""
    v = abs(float(v))
    if v == 0.0 or v < 2.0 ** -126:
        return 0
    return min(math.frexp(v)[1] - 1 + 127, 255)


def f8_scale_byte(vmax):
    """forward rule, from the largest stored magnitude"""
    return max(biased_exponent(vmax) - 7, 1)


def bf8_scale_byte(vmax):
    """chain rule, from the largest (ungated fp32) magnitude"""
    return max(biased_exponent(vmax) - 14, 1)


def tile_max(t, tiles):
    """(32 tiles, F) -> per-tile max |value| as a Python list"""
    return t.abs().reshape(tiles, -1).max(1).values.tolist()


_tables = {}


def _table(fmt):
    """codes of the NORMAL bf16 magnitudes by (exponent field - scale byte, mantissa): a power-of-two scale only shifts the
    exponent, so encode_bits on one (e, Eb) pair per difference d = e - Eb in -253..253 is the whole function"""
    key = (fmt.name, fmt.nearest)
    if key not in _tables:
        d = np.arange(-253, 254, dtype=np.int64)[:, None]
        e = np.maximum(1, 1 + d)
        _tables[key] = encode_bits((e << 7) | np.arange(128, dtype=np.int64)[None, :], e - d, fmt).reshape(-1)
    return _tables[key]


def encode_fast(bits, Eb, fmt):
    """encode_bits through the table above (zero, subnormal and non-finite inputs take encode_bits itself): the same codes, proven
    on every pattern in tests/test_f8_exact_host.py, at a tenth of the time"""
    bits = np.asarray(bits, dtype=np.int64)
    Eb = np.broadcast_to(np.asarray(Eb, dtype=np.int64), bits.shape)
    e = (bits >> 7) & 0xff
    out = _table(fmt)[(np.clip(e - Eb, -253, 253) + 253) * 128 + (bits & 0x7f)] | ((bits >> 15) * fmt.sign)
    odd = (e == 0) | (e == 0xff)
    if odd.any():
        out[odd] = encode_bits(bits[odd], Eb[odd], fmt)
    return out


def encode_section(t, Eb, fmt):
    """(32 tiles, F) bf16 values, per-tile scale bytes (tiles,) -> codes (32 tiles, F) int64"""
    tiles = len(Eb)
    bits = bf16_bits(t).reshape(tiles, 32, -1)
    return encode_fast(bits, np.asarray(Eb, dtype=np.int64)[:, None, None], fmt).reshape(32 * tiles, -1)


def decode_section(q, Eb, fmt):
    """codes (32 tiles, F), per-tile scale bytes -> fp64 tensor (32 tiles, F)"""
    tiles = len(Eb)
    v = decode_codes(np.asarray(q).reshape(tiles, 32, -1), np.asarray(Eb, dtype=np.int64)[:, None, None], fmt)
    return torch.from_numpy(v.reshape(32 * tiles, -1).copy())


# ================================================================================================ saved buffers <-> tensors
def x_sections():
    """name -> (first slab, slabs, slot table, features, scale index): E.act_sections() + the section's scale dword"""
    return {k: v + (f8_x_section(v[0]),) for k, v in E.act_sections().items()}


def dy_sections():
    return {k: v + (f8_dy_section(v[0]),) for k, v in E.dy_sections().items()}


def _blocks(buf, tiles, tile_bytes):
    b = buf.detach().cpu().contiguous().numpy().view(np.uint8)
    return b[:tiles * tile_bytes].reshape(tiles, tile_bytes // E.kPieceBytes, E.kPieceBytes)


def _row_tables():
    """per operand row m of a pair: (byte offsets of its 32 points inside the piece (32,), slab of the pair, h, j)"""
    return [(np.array([pair_byte(m, n) for n in range(32)]),) + pair_row_place(m) for m in range(32)]


def _decode_pairs(blocks, sec, fmt, scale_piece):
    first, slabs, table, feats, sidx = sec
    tiles = blocks.shape[0]
    codes = np.zeros((tiles, 32, feats), dtype=np.int64)
    pad = []
    rows = _row_tables()
    for p in range(slabs // 2):
        piece = blocks[:, first // 2 + p]                                           # [T][1024]
        for offs, s, h, j in rows:
            f = table[2 * p + s, h, j]
            if f >= 0:
                codes[:, :, f] = piece[:, offs]
            else:
                pad.append(piece[:, offs])
    dwords = blocks[:, scale_piece].copy().view(np.uint32)                          # [T][256]
    sc = dwords[:, sidx].astype(np.int64)
    padding = np.stack(pad, -1).reshape(tiles * 32, -1) if pad else np.zeros((tiles * 32, 0), dtype=np.uint8)
    q = codes.reshape(tiles * 32, feats)
    return q, sc, decode_section(q, sc & 0xff, fmt), padding


def decode_acts_f8(buf, tiles):
    """X tile blocks of the 'bf16_f8' saving forward -> {q_<name>: codes (32 tiles, F) int64, scale_<name>: the section's scale
    DWORD per tile (tiles,), <name>: decoded fp64 (32 tiles, F), pad_<name>: the code bytes of the padding slots, gate_*: bool, as
    E.decode_acts} for name in ex, ed, h1..h8, t"""
    bl = _blocks(buf, tiles, f8_act_tile_bytes())
    out = {}
    for name, sec in x_sections().items():
        out["q_" + name], out["scale_" + name], out[name], out["pad_" + name] = _decode_pairs(bl, sec, E4M3, kF8ActPairs + E.kMaskPieces)
    words = bl[:, kF8ActPairs:kF8ActPairs + E.kMaskPieces].copy().view(np.uint32).reshape(tiles, E.kMaskPieces, 2, 32, 4)
    for name, piece, slabs in [("gate_h%d" % l, l - 1, 16) for l in range(1, 9)] + [("gate_t", E.kMaskPieceT, 8)]:
        g = np.zeros((tiles, 32, 16 * slabs), dtype=bool)
        for ks in range(slabs):
            for h in range(2):
                for j in range(8):
                    idx = 8 * ks + j
                    g[:, :, E.chain_feature(ks, h, j)] = (words[:, piece, h, :, E.gate_word(idx)] >> E.gate_bit(idx)) & 1
        out[name] = torch.from_numpy(g.reshape(tiles * 32, -1))
    return out


def decode_dys_f8(buf, tiles):
    """dY tile blocks of the 'bf16_f8' chain -> {q_*, scale_*, decoded, pad_*} for rgb, sigma, dir, dy1..dy8"""
    bl = _blocks(buf, tiles, f8_dy_tile_bytes())
    out = {}
    for name, sec in dy_sections().items():
        out["q_" + name], out["scale_" + name], out[name], out["pad_" + name] = _decode_pairs(bl, sec, E5M2, kF8DyPairs)
    return out


def _encode_pairs(blocks, q, sc, sec, scale_piece):
    first, slabs, table, feats, sidx = sec
    tiles = blocks.shape[0]
    codes = np.asarray(q).reshape(tiles, 32, feats).astype(np.uint8)
    for p in range(slabs // 2):
        piece = blocks[:, first // 2 + p]
        for offs, s, h, j in _row_tables():
            f = table[2 * p + s, h, j]
            if f >= 0:
                piece[:, offs] = codes[:, :, f]
    dw = blocks[:, scale_piece].view(np.uint32)
    dw[:, sidx] = np.asarray(sc, dtype=np.uint32)


def encode_acts_f8(tensors, tiles, fill=0):
    """the inverse of decode_acts_f8 from q_*, scale_*, gate_*: every byte no value claims holds `fill`"""
    bl = np.full((tiles, f8_act_tile_bytes() // E.kPieceBytes, E.kPieceBytes), fill, dtype=np.uint8)
    for name, sec in x_sections().items():
        _encode_pairs(bl, tensors["q_" + name], tensors["scale_" + name], sec, kF8ActPairs + E.kMaskPieces)
    gates = E.encode_acts({**{k: torch.zeros(32 * tiles, sec[3], dtype=torch.float64) for k, sec in E.act_sections().items()},
                           **{k: v for k, v in tensors.items() if k.startswith("gate_")}}, tiles).numpy()
    gates = gates.reshape(tiles, E.act_tile_bytes() // E.kPieceBytes, E.kPieceBytes)[:, E.kActSlabs:]
    claimed = byte_claims("acts")[0].reshape(-1, E.kPieceBytes)[kF8ActPairs:kF8ActPairs + E.kMaskPieces] > 0
    g = bl[:, kF8ActPairs:kF8ActPairs + E.kMaskPieces]
    g[:, claimed] = gates[:, claimed]
    return torch.from_numpy(bl.reshape(-1))


def encode_dys_f8(tensors, tiles, fill=0):
    bl = np.full((tiles, f8_dy_tile_bytes() // E.kPieceBytes, E.kPieceBytes), fill, dtype=np.uint8)
    for name, sec in dy_sections().items():
        _encode_pairs(bl, tensors["q_" + name], tensors["scale_" + name], sec, kF8DyPairs)
    return torch.from_numpy(bl.reshape(-1))


def byte_claims(kind):
    """(claims, written, why) per byte of ONE tile block.  claims: how many decoded values (codes, gate bits by the byte, scale
    dwords) read the byte; written: whether the kernels store to it — a claimed byte, or a padding slot INSIDE a written pair piece
    (an encoding's empty slots, the unused features of the rgb / sigma pairs: stored as zero codes); why: a label for the bytes
    nobody writes — 'feat' (pair pieces 67..74 of X / 5..12 of dY, the folded final layer: mlp_layout.h kActFeat / kDyFeat), 'gate'
    (gate words of output tiles a 128-wide layer does not have), 'scale-feat' (the feat section's scale dword), 'scale-rest'
    (the remainder of the scale piece); '' where written."""
    acts = kind == "acts"
    sections = x_sections() if acts else dy_sections()
    nbytes = f8_act_tile_bytes() if acts else f8_dy_tile_bytes()
    pairs = kF8ActPairs if acts else kF8DyPairs
    claims = np.zeros(nbytes, dtype=np.int64)
    written = np.zeros(nbytes, dtype=bool)
    why = np.full(nbytes, "", dtype=object)
    rows = _row_tables()
    for first, slabs, table, feats, sidx in sections.values():
        for p in range(slabs // 2):
            base = (first // 2 + p) * E.kPieceBytes
            written[base:base + E.kPieceBytes] = True
            for offs, s, h, j in rows:
                if table[2 * p + s, h, j] >= 0:
                    claims[base + offs] += 1
    feat0 = (E.kActFeat if acts else E.kDyFeat) // 2
    assert not written[feat0 * E.kPieceBytes:(feat0 + 8) * E.kPieceBytes].any()
    why[feat0 * E.kPieceBytes:(feat0 + 8) * E.kPieceBytes] = "feat"
    scale0 = pairs * E.kPieceBytes
    if acts:
        bf = E.byte_claims("acts")[0][E.kActSlabs * E.kPieceBytes:]               # the nine gate pieces: as in the bf16 block
        g0 = f8_act_gate_off()
        claims[g0:g0 + bf.size] = bf
        written[g0:g0 + bf.size] = bf > 0
        why[g0:g0 + bf.size][bf == 0] = "gate"
        scale0 = f8_act_scale_off()
    why[scale0:scale0 + E.kPieceBytes] = "scale-rest"
    for k in range(kXSections if acts else kDySections):
        o = scale0 + 4 * k
        if k == (kXSectionFeat if acts else kDySectionFeat):
            why[o:o + 4] = "scale-feat"
        else:
            claims[o:o + 4] += 1
            written[o:o + 4] = True
            why[o:o + 4] = ""
    assert not (why[written] != "").any() and (why[~written] != "").all()
    return claims, written, why


# ================================================================================================ the model
def dw_job_f8(qdY, EdY, qX, EX, fdy=E5M2, fx=E4M3):
    """(dW, db, |terms| of dW, |terms| of db) of one weight-gradient job from the STORED operands: codes (N, features) and per-tile
    scale bytes (N / 32,).  decode(dY) decode(X) is a product of two <= 4-bit significands and a power of two: exact in fp64."""
    return E.dw_job(decode_section(qdY, EdY, fdy), decode_section(qX, EX, fx))


def forward_scales(t, tiles):
    """forward rule: per-tile scale bytes of a (32 tiles, F) section of stored bf16 values"""
    return [f8_scale_byte(v) for v in tile_max(t, tiles)]


def chain_scales(s_ungated, tiles):
    """chain rule: per-tile scale bytes from the ungated sums (fp64 here, rounded to fp32 as the accumulators are)"""
    return [bf8_scale_byte(v) for v in tile_max(s_ungated.float().double(), tiles)]


def store_x(t, tiles, Eb=None, fmt=E4M3):
    """what the forward leaves of a section: (codes, scale bytes, decoded values)"""
    Eb = forward_scales(t, tiles) if Eb is None else Eb
    q = encode_section(t, Eb, fmt)
    return q, Eb, decode_section(q, Eb, fmt)


def store_dy(t, s_ungated, tiles, fmt=E5M2):
    """what the chain leaves of a section whose ungated sums are s_ungated (None: a seed, scale from the stored values)"""
    Eb = chain_scales(t if s_ungated is None else s_ungated, tiles)
    q = encode_section(t, Eb, fmt)
    return q, Eb, decode_section(q, Eb, fmt)


def _pad(t, rows, repeat_last):
    """(n, F) -> (rows, F): lanes behind point n repeat point n - 1 (X) or are zero (dY)"""
    n = t.shape[0]
    tail = t[n - 1:n].expand(rows - n, -1) if repeat_last else torch.zeros(rows - n, t.shape[1], dtype=t.dtype)
    return torch.cat([t, tail], 0)


def model_gradients(net, x, g_out, acc=None, fx=E4M3, fdy=E5M2):
    """The 'bf16_f8' backward on the model's OWN bf16 tensors (no teacher forcing): bf16 forward and chain of E, every dW operand
    stored by the two rules above and decoded again, the 24 gradients in fp64 (E.gradients)."""
    n = x.shape[0]
    tiles = (n + 255) // 256 * 8
    R = 32 * tiles
    f = E.forward(net, x, acc)
    sx = lambda t: store_x(_pad(t, R, True), tiles, fmt=fx)[2][:n]
    ex = store_x(_pad(f["ex"], R, True), tiles, [127] * tiles, fx)[2][:n]
    ed = store_x(_pad(f["ed"], R, True), tiles, [127] * tiles, fx)[2][:n]
    h = {l: sx(f["h"][l]) for l in range(1, 9)}
    t = sx(f["t"])
    sd = lambda v, s: store_dy(_pad(v, R, False), None if s is None else _pad(s, R, False), tiles, fdy)[2][:n]
    dy_rgb, dy_sigma = E.seed(net, g_out, f["out"])
    dy_dir, s, _ = E.chain_dir(net, dy_rgb, (f["t"] > 0).double(), acc)
    dY, S = {}, {}
    dY[8], S[8], _ = E.chain_h8(net, dy_dir, dy_sigma, (f["h"][8] > 0).double(), acc)
    for l in range(7, 0, -1):
        dY[l], S[l], _ = E.chain_trunk(net, l, dY[l + 1], (f["h"][l] > 0).double(), acc)
    X = {l: E.layer_operand(l, ex, h.get(l - 1)) for l in range(1, 9)}
    return f, E.gradients(net, X, {l: sd(dY[l], S[l]) for l in range(1, 9)}, ed, h[8], t, sd(dy_rgb, None), sd(dy_sigma, None),
                          sd(dy_dir, s), acc)

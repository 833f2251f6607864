"""A rounding-exact model of the bf16 MLP kernels, and a decoder of the buffers they save.  Plain torch, fp64 accumulation, no GPU.

The bf16 kernels (nerf_pl_amd/csrc/mlp_fwd_kernel.h, mlp_bwd_chain.hip, mlp_bwd_dw.hip, mlp_bwd_reduce.hip, mlp_dx.hip) multiply
bf16 operands exactly and accumulate in fp32.  Their results therefore differ from the fp32 oracle (oracle/nerf_oracle.py) by the
bf16 ROUNDING of the operands — 2-13 % relative L2 on a gradient tensor — which is legitimate, and from a model that rounds at the
same places only by the ORDER of an fp32 sum, which is tiny and has a worst-case bound.  This module is that model.

Rounding points, as the code has them:
  * x, every weight (mlp_pack_pieces.h: `(__bf16)v`), every post-ReLU activation (epi_piece: v_cvt_pk_bf16_f32, then max with 0 —
    rounding and ReLU commute) and every dY (chain epilogue: convert, then AND with the gate mask) are rounded to nearest even;
  * the bias is the fp32 INITIAL value of the accumulator (pipe_bias), never rounded;
  * the dir layer runs on h8 with the product W_c = W_dir[:, :256] W_final and b_c = W_dir[:, :256] b_final + b_dir, formed in fp32
    from the fp32 masters and rounded ONCE (pack_fold_tile); forward and chain read the same bf16 W_c;
  * sigma = fp32 accumulator of the head, rgb = 1 / (1 + expf(-acc)) in fp32: neither is rounded to bf16;
  * the chain's seed is fp32 arithmetic on the kernel's OWN fp32 output: g_rgb * rgb * (1 - rgb), g_sigma; then rounded;
  * the ReLU gate the chain applies is [stored bf16 activation > 0];
  * dW = sum over points of exact products of the stored bf16 dY and X, fp32 accumulation; the reduce kernel adds the splits;
  * the final layer's and the dir layer's h8-side gradients are finished in fp32 from G = dY_dir^T h8 and s = sum dY_dir with the
    fp32 MASTER weights (mlp_bwd_fold_kernel): dW_dir[:, :256] = G W_f^T + s b_f^T, dW_final = W_dx^T G, db_final = W_dx^T s;
  * mlp_dx_embedded multiplies the stored bf16 dY_1, dY_5, dY_dir by the fp32 MASTER weights.

Every stage is a function of GIVEN inputs, so a test can feed a kernel's stage the values the previous kernel stage actually
stored ("teacher forcing") and is left with nothing but the summation order between model and kernel.

The second half restates the index maps of nerf_pl_amd/csrc/mlp_layout.h in Python (tests/test_bf16_exact_host.py compares them
entry by entry with tables printed from the header) and maps the saved buffers to plain (points, features) tensors and back.
"""
import numpy as np
import torch

PARAM_ORDER = ["xyz_encoding_1.0", "xyz_encoding_2.0", "xyz_encoding_3.0", "xyz_encoding_4.0", "xyz_encoding_5.0", "xyz_encoding_6.0",
               "xyz_encoding_7.0", "xyz_encoding_8.0", "xyz_encoding_final", "dir_encoding.0", "sigma", "rgb.0"]
U32 = 2.0 ** -24          # unit roundoff of fp32


# ================================================================================================ rounding
def rne_bf16(t):
    """fp64 -> nearest-even bf16 value (as fp64), in ONE rounding (fp64 -> fp32 -> bf16 would round twice)."""
    t = t.double()
    bits = t.contiguous().view(torch.int64)
    low = (1 << 45) - 1                                    # fp64 keeps 52 mantissa bits, bf16 7
    r = (bits + (low >> 1) + ((bits >> 45) & 1)) & ~low
    out = r.view(torch.float64)
    tiny = t.abs() < 2.0 ** -120                           # bf16 subnormal range: let the hardware formats decide
    return torch.where(tiny, t.float().bfloat16().double(), out)


def trunc_bf16(t):
    """round toward zero (NOT what the kernels do: tests use it to show that they notice)"""
    bits = t.double().contiguous().view(torch.int64)
    return (bits & ~((1 << 45) - 1)).view(torch.float64)


class Rounding:
    """the rounding model: `on=False` turns every rounding off (the algebra alone: equals fp64 autograd)"""

    def __init__(self, on=True, fn=None):
        self.on = on
        self.fn = fn or rne_bf16

    def __call__(self, t):
        return self.fn(t) if self.on else t.double()


# ================================================================================================ accumulation
class Accumulate:
    """how a sum of products is formed: 'f64' (the model), 'f32' / 'f32perm' (fp32 accumulation in two different orders — what
    separates a kernel from the model: used to derive bounds from the model alone)."""

    def __init__(self, mode="f64", seed=0):
        assert mode in ("f64", "f32", "f32perm")
        self.mode, self.seed = mode, seed

    def mm(self, a, b):
        """a (m, K) @ b (K, n), both holding bf16 (or fp32) values"""
        if self.mode == "f64":
            return a.double() @ b.double()
        if self.mode == "f32":
            return (a.float() @ b.float()).double()
        K = a.shape[1]
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(self.seed + K))
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
        for lo in range(0, K, 8):                          # blocks of 8 in a shuffled order, added to a running fp32 sum
            idx = perm[lo:lo + 8]
            acc = acc + a[:, idx].float() @ b[idx].float()
        return acc.double()

    def add(self, a, b):
        if self.mode == "f64":
            return a.double() + b.double()
        return (a.float() + b.float()).double()


# ================================================================================================ the network
class Net:
    """bf16 images of a state dict (values held as fp64) + the fp32 masters the fold and dx kernels read.
    wc / bc: the folded dir-layer weights as the pack kernel formed them (decoded from a packed image); default: the fp64 product
    rounded to fp32, then to bf16 — the kernel's fp32 fmaf chains may differ from that in the last bf16 digit of a few elements."""

    def __init__(self, params, rounding=None, wc=None, bc=None):
        r = self.r = rounding or Rounding()
        p = {k: v.detach().double() for k, v in params.items()}
        self.W = [p[n + ".weight"] for n in PARAM_ORDER]                      # fp32 masters (as fp64)
        self.B = [p[n + ".bias"] for n in PARAM_ORDER]
        self.Wb = [r(w) for w in self.W]                                      # what the MFMA kernels multiply by
        Wdir, Wf, bf = self.W[9], self.W[8], self.B[8]
        self.Wdx, self.Wdd = Wdir[:, :256], Wdir[:, 256:]
        if r.on:
            self.Wc = r((self.Wdx @ Wf).float().double()) if wc is None else wc.double()
            self.bc = ((self.Wdx @ bf + self.B[9]).float().double()) if bc is None else bc.double()
        else:
            self.Wc, self.bc = self.Wdx @ Wf, self.Wdx @ bf + self.B[9]
        self.Wddb = r(self.Wdd)


def layer_operand(l, ex, h_prev):
    """the B operand of trunk layer l (1..8) = the X operand of its weight-gradient job"""
    return ex if l == 1 else (torch.cat([ex, h_prev], 1) if l == 5 else h_prev)


def pre_trunk(net, l, X, acc=None):
    """pre-activation of trunk layer l on operand X, and the sum of |terms| (the scale of its fp32 rounding error)"""
    acc = acc or Accumulate()
    Wb, b = net.Wb[l - 1], net.B[l - 1]
    return acc.add(acc.mm(X, Wb.t()), b), X.abs().double() @ Wb.abs().t() + b.abs()


def pre_dir(net, h8, ed, acc=None):
    acc = acc or Accumulate()
    X, Wb = torch.cat([ed, h8], 1), torch.cat([net.Wddb, net.Wc], 1)          # (the kernel consumes the dir slabs first)
    return acc.add(acc.mm(X, Wb.t()), net.bc), X.abs().double() @ Wb.abs().t() + net.bc.abs()


def pre_sigma(net, h8, acc=None):
    acc = acc or Accumulate()
    return acc.add(acc.mm(h8, net.Wb[10].t()), net.B[10]), h8.abs().double() @ net.Wb[10].abs().t() + net.B[10].abs()


def pre_rgb(net, t, acc=None):
    acc = acc or Accumulate()
    return acc.add(acc.mm(t, net.Wb[11].t()), net.B[11]), t.abs().double() @ net.Wb[11].abs().t() + net.B[11].abs()


def activation(net, pre):
    return net.r(torch.relu(pre))


def forward(net, x, acc=None):
    """NeRF.forward on pre-embedded x (n, 90).  Returns every intermediate: ex, ed, X[l], pre[l], h[l] (l = 1..8), pre_dir, t,
    pre_rgb, pre_sigma, out (n, 4)."""
    f = dict(ex=net.r(x[:, :63]), ed=net.r(x[:, 63:90]), X={}, pre={}, h={})
    h = None
    for l in range(1, 9):
        f["X"][l] = layer_operand(l, f["ex"], h)
        f["pre"][l], _ = pre_trunk(net, l, f["X"][l], acc)
        h = f["h"][l] = activation(net, f["pre"][l])
    f["pre_sigma"], _ = pre_sigma(net, h, acc)
    f["pre_dir"], _ = pre_dir(net, h, f["ed"], acc)
    f["t"] = activation(net, f["pre_dir"])
    f["pre_rgb"], _ = pre_rgb(net, f["t"], acc)
    f["out"] = torch.cat([torch.sigmoid(f["pre_rgb"]), f["pre_sigma"]], 1)
    return f


def seed(net, g_out, out):
    """(dY_rgb (n, 3), dY_sigma (n, 1)) as the chain kernel packs them: fp32 arithmetic on its fp32 inputs, then one rounding"""
    if not net.r.on:
        g, o = g_out.double(), out.double()
        return g[:, :3] * o[:, :3] * (1 - o[:, :3]), g[:, 3:4]
    g, o = g_out.float(), out.float()
    return net.r(((g[:, :3] * o[:, :3]) * (1.0 - o[:, :3])).double()), net.r(g[:, 3:4].double())


def chain_dir(net, dy_rgb, gate_t, acc=None):
    """dY_dir = bf16(gate_t * W_rgb^T dY_rgb); also the ungated fp64 sum and its |terms|"""
    acc = acc or Accumulate()
    s = acc.mm(dy_rgb, net.Wb[11])
    return net.r(s * gate_t), s, dy_rgb.abs().double() @ net.Wb[11].abs()


def chain_h8(net, dy_dir, dy_sigma, gate, acc=None):
    """dY_8 through the folded layer [W_c^T | W_sigma^T]"""
    acc = acc or Accumulate()
    X, Wb = torch.cat([dy_dir, dy_sigma], 1), torch.cat([net.Wc, net.Wb[10]], 0)
    s = acc.mm(X, Wb)
    return net.r(s * gate), s, X.abs().double() @ Wb.abs()


def chain_trunk(net, l, dy_next, gate, acc=None):
    """dY_l = bf16(gate_l * W_{l+1}^T dY_{l+1}), l = 1..7 (the skip layer's hidden columns 63..318 only)"""
    acc = acc or Accumulate()
    Wb = net.Wb[l][:, 63:] if l == 4 else net.Wb[l]
    s = acc.mm(dy_next, Wb)
    return net.r(s * gate), s, dy_next.abs().double() @ Wb.abs()


def dw_job(dy, X, acc=None):
    """(dW, db, |terms| of dW, |terms| of db) of one weight-gradient job: exact products of the stored operands, summed over points"""
    acc = acc or Accumulate()
    return (acc.mm(dy.t().contiguous(), X), acc.mm(dy.t().contiguous(), torch.ones(dy.shape[0], 1, dtype=dy.dtype))[:, 0],
            dy.abs().double().t() @ X.abs().double(), dy.abs().double().sum(0))


def fold(net, G, s):
    """mlp_bwd_fold_kernel: (dW_dir[:, :256], dW_final, db_final) from G = dY_dir^T h8, s = sum dY_dir and the fp32 masters"""
    Wf, bf = net.W[8], net.B[8]
    return G @ Wf.t() + s[:, None] * bf[None, :], net.Wdx.t() @ G, net.Wdx.t() @ s


def dx(net, dy1, dy5, dy_dir):
    """mlp_dx_embedded: dL/dx (n, 90) from the stored dY and the fp32 masters; also |terms|"""
    W1, W5x, Wdd = net.W[0], net.W[4][:, :63], net.Wdd
    g = torch.cat([dy1.double() @ W1 + dy5.double() @ W5x, dy_dir.double() @ Wdd], 1)
    a = torch.cat([dy1.abs().double() @ W1.abs() + dy5.abs().double() @ W5x.abs(), dy_dir.abs().double() @ Wdd.abs()], 1)
    return g, a


def gradients(net, X, dY, ed, h8, t, dy_rgb, dy_sigma, dy_dir, acc=None):
    """the 24 gradients {name.weight / name.bias} from the jobs' operands: X[l], dY[l] (l = 1..8) and the heads'"""
    G = {}
    for l in range(1, 9):
        G[PARAM_ORDER[l - 1] + ".weight"], G[PARAM_ORDER[l - 1] + ".bias"], _, _ = dw_job(dY[l], X[l], acc)
    G["rgb.0.weight"], G["rgb.0.bias"], _, _ = dw_job(dy_rgb, t, acc)
    G["sigma.weight"], G["sigma.bias"], _, _ = dw_job(dy_sigma, h8, acc)
    Gd, s, _, _ = dw_job(dy_dir, torch.cat([ed, h8], 1), acc)
    dWdx, dWf, dbf = fold(net, Gd[:, 27:], s)
    G["dir_encoding.0.weight"], G["dir_encoding.0.bias"] = torch.cat([dWdx, Gd[:, :27]], 1), s
    G["xyz_encoding_final.weight"], G["xyz_encoding_final.bias"] = dWf, dbf
    return G


def backward(net, f, g_out, out=None, acc=None):
    """The backward of forward()'s record f for dL/d(out) = g_out; out: the output the seed is formed from (default f['out']).
    Returns dict(dy_rgb, dy_sigma, dy_dir, dY[l], grads, dx)."""
    out = f["out"] if out is None else out
    b = dict(dY={})
    b["dy_rgb"], b["dy_sigma"] = seed(net, g_out, out)
    b["dy_dir"], _, _ = chain_dir(net, b["dy_rgb"], (f["t"] > 0).double(), acc)
    b["dY"][8], _, _ = chain_h8(net, b["dy_dir"], b["dy_sigma"], (f["h"][8] > 0).double(), acc)
    for l in range(7, 0, -1):
        b["dY"][l], _, _ = chain_trunk(net, l, b["dY"][l + 1], (f["h"][l] > 0).double(), acc)
    b["grads"] = gradients(net, f["X"], b["dY"], f["ed"], f["h"][8], f["t"], b["dy_rgb"], b["dy_sigma"], b["dy_dir"], acc)
    b["dx"], _ = dx(net, b["dY"][1], b["dY"][5], b["dy_dir"])
    return b


def rounding_interval(net, pre, tol, gate=None, relu=False):
    """[lo, hi]: the bf16 values a kernel may legitimately store for an fp64 result `pre` whose fp32 evaluation can be off by `tol`
    (rounding is monotone: every value between the roundings of pre - tol and pre + tol, nothing else)."""
    lo, hi = pre - tol, pre + tol
    if relu:
        lo, hi = torch.relu(lo), torch.relu(hi)
    if gate is not None:
        lo, hi = lo * gate, hi * gate
    return net.r(lo), net.r(hi)


def judge(net, got, pre, terms, K, gate=None, relu=False):
    """(exact, excused, wrong) element masks for a stored bf16 tensor `got` against the fp64 result `pre` of a length-K fp32 sum"""
    want = pre * gate if gate is not None else pre
    want = net.r(torch.relu(want) if relu else want)
    lo, hi = rounding_interval(net, pre, K * U32 * terms, gate, relu)
    got = got.double()
    exact = got == want
    inside = (got >= lo) & (got <= hi)
    return exact, inside & ~exact, ~inside


# ================================================================================================ mlp_layout.h, restated
kXyzCh, kDirCh, kW = 63, 27, 256
kXyzSlabs, kDirSlabs = 4, 2
kPieceBytes, kChunkPieces, kSlots = 1024, 32, 3
kActEncX, kActEncD, kActH0 = 0, 4, 6
kActFeat = kActH0 + 128
kActT = kActFeat + 16
kActSlabs = kActT + 8
kMaskPieces, kMaskPieceT = 9, 8
kDyRgb, kDyDir, kDyFeat, kDySigma, kDyH0 = 0, 2, 10, 26, 28
kDySlabs = kDyH0 + 128
kNumLayers, kSigmaLayer, kDirLayer, kLoopFirst, kLoopSecond = 11, 8, 9, 1, 5
IN_XYZ, IN_CHAIN, IN_XYZ_CHAIN, IN_DIR_CHAIN = 0, 1, 2, 3
# (param, nt, n_out, kind, enc_slabs, chain_slabs) in the kernels' execution order
kLayers = [(0, 8, 256, IN_XYZ, 4, 0), (1, 8, 256, IN_CHAIN, 0, 16), (2, 8, 256, IN_CHAIN, 0, 16), (3, 8, 256, IN_CHAIN, 0, 16),
           (4, 8, 256, IN_XYZ_CHAIN, 4, 16), (5, 8, 256, IN_CHAIN, 0, 16), (6, 8, 256, IN_CHAIN, 0, 16), (7, 8, 256, IN_CHAIN, 0, 16),
           (10, 1, 1, IN_CHAIN, 0, 16), (9, 4, 128, IN_DIR_CHAIN, 2, 16), (11, 1, 3, IN_CHAIN, 0, 8)]
# (param, dy_off, dy_slabs, x1_off, x1_slabs, x1_col0, x1_enc, x2_off, x2_slabs, x2_col0, x2_enc)
kDwEncFold = 3


def act_h(l):
    return kActH0 + 16 * (l - 1)


def dy_h(l):
    return kDyH0 + 16 * (8 - l)


kDwJobs = [(0, dy_h(1), 16, kActEncX, 4, 0, 1, 0, 0, 0, 0)] + \
          [(l - 1, dy_h(l), 16, act_h(l - 1), 16, 0, 0, 0, 0, 0, 0) for l in (2, 3, 4)] + \
          [(4, dy_h(5), 16, kActEncX, 4, 0, 1, act_h(4), 16, 63, 0)] + \
          [(l - 1, dy_h(l), 16, act_h(l - 1), 16, 0, 0, 0, 0, 0, 0) for l in (6, 7, 8)] + \
          [(8, kDyFeat, 16, act_h(8), 16, 0, 0, 0, 0, 0, 0), (9, kDyDir, 8, kActEncD, 2, 256, 2, act_h(8), 16, 0, kDwEncFold),
           (10, kDySigma, 2, act_h(8), 16, 0, 0, 0, 0, 0, 0), (11, kDyRgb, 2, kActT, 8, 0, 0, 0, 0, 0, 0)]


def enc_slot_channel(F, slabs, ks, h, j):
    idx, npair = 8 * ks + j, 3 * (F // 2)
    if idx < 2 * npair:
        p = idx >> 1
        i, c = p // 3, p % 3
        return 3 + 6 * (2 * i + h) + c + 3 * (idx & 1)
    tail = idx - 2 * npair
    if h == 0:
        return tail if tail < 2 else -1
    return 2 if tail == 0 else -1


def xyz_slot_channel(ks, h, j):
    return enc_slot_channel(10, kXyzSlabs, ks, h, j)


def dir_slot_channel(ks, h, j):
    return enc_slot_channel(4, kDirSlabs, ks, h, j)


def chain_feature(ks, h, j):
    return 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)


def gate_word(idx):
    return idx >> 5


def gate_bit(idx):
    return 16 * (idx & 1) + 15 - ((idx & 31) >> 1)


def act_mask_off():
    return kActSlabs * kPieceBytes


def act_tile_bytes():
    return act_mask_off() + kMaskPieces * kPieceBytes


def dy_tile_bytes():
    return kDySlabs * kPieceBytes


def tile_block_off(tile, tile_bytes, il=1):
    return (tile // il) * il * tile_bytes + (tile % il) * kPieceBytes


def layer_slabs(L):
    return kLayers[L][4] + kLayers[L][5]


def layer_pieces(L):                                       # bf16: one piece per (tile, slab) fragment
    return layer_slabs(L) * kLayers[L][1]


def raw_start(L):
    return sum(layer_pieces(i) for i in range(L))


def bias_block_pieces():
    chunks = (kNumLayers + kChunkPieces - 1) // kChunkPieces
    while ((raw_start(kLoopSecond) - raw_start(kLoopFirst)) // kChunkPieces + chunks) % kSlots != 0:
        chunks += 1
    return chunks * kChunkPieces


def bias_block_start():
    return raw_start(kLoopSecond)


def layer_start(L):
    return raw_start(L) + (bias_block_pieces() if L >= kLoopSecond else 0)


def layer_in_col(L, ks, h, j):
    _, _, _, kind, enc, _ = kLayers[L]
    if ks < enc:
        if kind == IN_DIR_CHAIN:
            c = dir_slot_channel(ks, h, j)
            return -1 if c < 0 else kW + c
        return xyz_slot_channel(ks, h, j)
    f = chain_feature(ks - enc, h, j)
    return kXyzCh + f if kind == IN_XYZ_CHAIN else f


# ================================================================================================ saved buffers <-> tensors
# A bf16 slab is one 1 KiB piece: lane (h, n) = h * 32 + n holds 8 bf16 (slot j) of point n of the tile: [2][32][8] bf16.
def _slot_table(slabs, fn):
    """feature of slot (ks, h, j) as an int array [slabs][2][8] (-1: padding)"""
    return np.array([[[fn(ks, h, j) for j in range(8)] for h in range(2)] for ks in range(slabs)], dtype=np.int64)


def act_sections():
    """name -> (first slab, slabs, slot table, features) of the activation tile block"""
    s = {"ex": (kActEncX, kXyzSlabs, _slot_table(kXyzSlabs, xyz_slot_channel), kXyzCh),
         "ed": (kActEncD, kDirSlabs, _slot_table(kDirSlabs, dir_slot_channel), kDirCh),
         "t": (kActT, 8, _slot_table(8, chain_feature), 128)}
    for l in range(1, 9):
        s["h%d" % l] = (act_h(l), 16, _slot_table(16, chain_feature), 256)
    return s


def dy_sections():
    rgb = _slot_table(2, chain_feature)
    sig = rgb.copy()
    rgb[rgb >= 3] = -1                                     # 3 real features (h = 0, j < 3), the rest of the two slabs is zero
    sig[sig >= 1] = -1
    s = {"rgb": (kDyRgb, 2, rgb, 3), "sigma": (kDySigma, 2, sig, 1), "dir": (kDyDir, 8, _slot_table(8, chain_feature), 128)}
    for l in range(1, 9):
        s["dy%d" % l] = (dy_h(l), 16, _slot_table(16, chain_feature), 256)
    return s


def _pieces(buf, tiles, tile_bytes, il):
    """uint8 buffer -> int16 view [tile][piece][512] of the first `tiles` tile blocks (bf16 bit patterns)"""
    b = buf.detach().cpu().contiguous().numpy().view(np.uint8)
    per = tile_bytes // kPieceBytes
    if il == 1:
        return b[:tiles * tile_bytes].reshape(tiles, per, kPieceBytes).view(np.int16)
    out = np.empty((tiles, per, kPieceBytes), dtype=np.uint8)
    for t in range(tiles):
        o = tile_block_off(t, tile_bytes, il)
        for p in range(per):
            out[t, p] = b[o + p * il * kPieceBytes: o + p * il * kPieceBytes + kPieceBytes]
    return out.view(np.int16)


def _bf16_bits_to_f64(a):
    return torch.from_numpy((a.astype(np.int32) << 16).view(np.float32).astype(np.float64))


def _decode_section(pieces, sec):
    first, slabs, table, feats = sec
    tiles = pieces.shape[0]
    v = pieces[:, first:first + slabs].reshape(tiles, slabs, 2, 32, 8)             # [T][ks][h][n][j]
    out = np.zeros((tiles, 32, feats), dtype=np.int16)
    pad = []
    for ks in range(slabs):
        for h in range(2):
            for j in range(8):
                f = table[ks, h, j]
                if f >= 0:
                    out[:, :, f] = v[:, ks, h, :, j]
                else:
                    pad.append(v[:, ks, h, :, j])
    padding = np.stack(pad, -1).reshape(tiles * 32, -1) if pad else np.zeros((tiles * 32, 0), dtype=np.int16)
    return _bf16_bits_to_f64(out.reshape(tiles * 32, feats)), padding


def decode_acts(buf, tiles, il=1):
    """activation tile blocks (ops.alloc_acts / save=) -> {ex, ed, h1..h8, t: (32 tiles, features) fp64; gate_h1..gate_h8, gate_t:
    bool; pad_<name>: the raw bits of the section's padding slots}"""
    pc = _pieces(buf, tiles, act_tile_bytes(), il)
    out = {}
    for name, sec in act_sections().items():
        out[name], out["pad_" + name] = _decode_section(pc, sec)
    words = pc[:, kActSlabs:kActSlabs + kMaskPieces].copy().view(np.uint32).reshape(tiles, kMaskPieces, 2, 32, 4)   # [T][piece][h][n][w]
    for name, piece, slabs in [("gate_h%d" % l, l - 1, 16) for l in range(1, 9)] + [("gate_t", kMaskPieceT, 8)]:
        g = np.zeros((tiles, 32, 16 * slabs), dtype=bool)
        for ks in range(slabs):
            for h in range(2):
                for j in range(8):
                    idx = 8 * ks + j
                    g[:, :, chain_feature(ks, h, j)] = (words[:, piece, h, :, gate_word(idx)] >> gate_bit(idx)) & 1
        out[name] = torch.from_numpy(g.reshape(tiles * 32, -1))
    return out


def decode_dys(buf, tiles, il=1):
    """dY tile blocks (ops.mlp_bwd(..., phases=1, workspace=ws) leaves them in ws['dys']) -> {rgb, sigma, dir, dy1..dy8, pad_*}"""
    pc = _pieces(buf, tiles, dy_tile_bytes(), il)
    out = {}
    for name, sec in dy_sections().items():
        out[name], out["pad_" + name] = _decode_section(pc, sec)
    return out


def _f64_to_bf16_bits(t):
    return (t.float().contiguous().numpy().view(np.int32) >> 16).astype(np.int16)     # (values already bf16: exact)


def _encode(tensors, sections, tiles, tile_bytes):
    pc = np.zeros((tiles, tile_bytes // kPieceBytes, 512), dtype=np.int16)
    for name, (first, slabs, table, feats) in sections.items():
        bits = _f64_to_bf16_bits(tensors[name]).reshape(tiles, 32, feats)
        v = pc[:, first:first + slabs].reshape(tiles, slabs, 2, 32, 8)
        for ks in range(slabs):
            for h in range(2):
                for j in range(8):
                    if table[ks, h, j] >= 0:
                        v[:, ks, h, :, j] = bits[:, :, table[ks, h, j]]
    return pc


def encode_acts(tensors, tiles):
    """the inverse of decode_acts (il = 1): padding slots and the unsaved `final` section are zero, gate bits from gate_*"""
    pc = _encode(tensors, act_sections(), tiles, act_tile_bytes())
    words = np.zeros((tiles, kMaskPieces, 2, 32, 4), dtype=np.uint32)
    for name, piece, slabs in [("gate_h%d" % l, l - 1, 16) for l in range(1, 9)] + [("gate_t", kMaskPieceT, 8)]:
        g = tensors[name].numpy().reshape(tiles, 32, 16 * slabs)
        for ks in range(slabs):
            for h in range(2):
                for j in range(8):
                    idx = 8 * ks + j
                    words[:, piece, h, :, gate_word(idx)] |= g[:, :, chain_feature(ks, h, j)].astype(np.uint32) << np.uint32(gate_bit(idx))
    pc[:, kActSlabs:] = words.reshape(tiles, kMaskPieces, 256).view(np.int16)
    return torch.from_numpy(pc.view(np.uint8).reshape(-1))


def encode_dys(tensors, tiles):
    return torch.from_numpy(_encode(tensors, dy_sections(), tiles, dy_tile_bytes()).view(np.uint8).reshape(-1))


def byte_claims(kind):
    """(claims, padding) per byte of ONE tile block: how many decoded values read the byte, and whether the layout documents it as
    padding — an encoding's empty slots, the rgb / sigma slabs' unused features, the `final` sections that are no longer stored
    (mlp_layout.h kActFeat / kDyFeat), the gate words of output tiles a 128-wide layer does not have."""
    sections, tile_bytes = (act_sections(), act_tile_bytes()) if kind == "acts" else (dy_sections(), dy_tile_bytes())
    claims = np.zeros(tile_bytes // 2, dtype=np.int64).reshape(-1, 2, 32, 8)            # per bf16 value: [piece][h][n][j]
    padding = np.zeros_like(claims, dtype=bool)
    for first, slabs, table, _ in sections.values():
        claims[first:first + slabs] += (table >= 0)[:, :, None, :]
        padding[first:first + slabs] |= (table < 0)[:, :, None, :]
    unsaved = kActFeat if kind == "acts" else kDyFeat
    padding[unsaved:unsaved + 16] = True
    claims, padding = np.repeat(claims.reshape(-1), 2), np.repeat(padding.reshape(-1), 2)
    if kind == "acts":
        bits = np.zeros((kMaskPieces, 2, 32, 4, 32), dtype=np.int64)                    # per gate BIT
        for piece, slabs in [(l - 1, 16) for l in range(1, 9)] + [(kMaskPieceT, 8)]:
            for ks in range(slabs):
                for j in range(8):
                    bits[piece, :, :, gate_word(8 * ks + j), gate_bit(8 * ks + j)] += 1
        assert bits.max() <= 1
        full = bits.reshape(-1, 4, 8).sum(-1)                                           # per byte: 8 claimed bits or none
        assert set(np.unique(full)) <= {0, 8}
        claims[kActSlabs * kPieceBytes:] = full.reshape(-1) // 8
        padding[kActSlabs * kPieceBytes:] = full.reshape(-1) == 0
    return claims, padding


def decode_packed_fwd(buf):
    """the packed forward image (NeRF.packed_weights('bf16')) -> ([W of kLayers[L] as (32 nt, in_features) fp64], [bias (256,)]):
    the bf16 weights and fp32 biases the forward kernel actually multiplies by / starts from.  Layer kDirLayer: [W_c | W_dd] in
    W_dir's column order (columns 0..255 = the product matrix), bias b_c."""
    b = buf.detach().cpu().contiguous().numpy().view(np.uint8)
    Ws, Bs = [], []
    in_features = [63, 256, 256, 256, 319, 256, 256, 256, 256, 283, 256, 128]
    for L, (param, nt, _, _, _, _) in enumerate(kLayers):
        nks, g0 = layer_slabs(L), layer_start(L)
        fr = b[g0 * kPieceBytes:(g0 + nt * nks) * kPieceBytes].view(np.int16).reshape(nt, nks, 2, 32, 8)     # [t][ks][h][m][j]
        W = np.zeros((32 * nt, in_features[param]), dtype=np.int16)
        for ks in range(nks):
            for h in range(2):
                for j in range(8):
                    c = layer_in_col(L, ks, h, j)
                    if c >= 0:
                        W[:, c] = fr[:, ks, h, :, j].reshape(-1)
        Ws.append(_bf16_bits_to_f64(W))
        o = (bias_block_start() + L) * kPieceBytes
        Bs.append(torch.from_numpy(b[o:o + kPieceBytes].copy().view(np.float32).astype(np.float64)))
    return Ws, Bs


# ================================================================================================ the tests' inputs
def embedded_case(n):
    """(params, x (n, 90), g_out (n, 4)): the inputs of tests/test_gpu_training.py::test_mlp_backward_embedded_vs_autograd"""
    from oracle import nerf_oracle as O
    g = torch.Generator().manual_seed(n)
    p = O.make_params(21, 3.0, 0.1)
    pts = torch.rand(n, 3, generator=g) * 4 - 2
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    x = torch.cat([O.posenc(pts, 10), O.posenc(dirs, 4)], 1)
    g_out = torch.randn(n, 4, generator=g)
    return p, x, g_out

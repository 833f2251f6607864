"""CPU side of the elementwise check of csrc/linear.hip (tests/test_linear_ref_host.py proves it, tests/test_gpu_linear_exact.py
applies it to the kernels): the case table, the guarded buffers every logical matrix lives in, the fp64 reference of the three GEMMs
of a layer ON THE OPERANDS THE KERNEL MULTIPLIES, and componentwise bounds.  No GPU import.

Operands: fp32 mode as given; bf16 mode `oracle.bf16_exact.rne_bf16` of each.  The gated operand of both gradients is g = gy act'(y),
formed in float32 in the kernel's order (ReLU: y > 0 ? gy : 0; Sigmoid: (gy (1 - y)) y, three separately rounded operations) and, in
bf16 mode, rounded once more.  y is an INPUT of the two gradient entry points, so reference and kernel gate on the same values.

Bounds, u = 2^-24, S = the reference's sum over absolute values (|bias| and |old value| included where they are added):
    forward pre-activation   (n_in + 4) u S         none: |y - pre|, ReLU: |y - max(pre, 0)| and y >= 0, Sigmoid: 0.25 bound + 8 u
    input gradient           (n_out + 4) u S
    weight / bias gradient   (n + ceil(n / 512) + 4) u S        (bias: S = sum |g| + |old|)
A length-K fp32 sum contributes K, each product's rounding 1, the bias / accumulate / split additions one each; ceil(n / 512) is
dw_plan's own ceiling on the number of point splits; 8 u is the expf / add / divide epilogue's, as in tests/test_gpu_bf16_exact.py.
Where S == 0 the result must be an exact zero.  None of the constants is measured on the kernel."""
import math

import torch

from oracle.bf16_exact import rne_bf16, trunc_bf16  # noqa: F401  (trunc_bf16: the host test's mutation)

U = 2.0 ** -24
ACT = {"none": 0, "relu": 1, "sigmoid": 2}
MODES = ("fp32", "bf16")

# (n, n_in, n_out): the smallest shapes at which each path of the kernel can go wrong
SHAPES = [
    (1, 1, 1),          # one live lane, K = 1
    (129, 33, 3),       # a second row tile holding one row; one full 32-step stage plus one element; K % 4 = 1
    (127, 32, 128),     # exactly one stage; a full 128-column tile with one dead row
    (128, 36, 129),     # the 256-column tile chosen with one live column beyond 128; a K tail of exactly one 4-element unit
    (130, 260, 257),    # two 256-column tiles in the forward, two column tiles in the input gradient; eight stages plus four
    (300, 6, 300),      # three row tiles of the weight gradient (Ip = 384); a narrow n_in that is no multiple of 4
    (513, 64, 64),      # the smallest n with two point splits (the second: 7 stages plus one point)
    (4097, 40, 5),      # nine splits
]
ALL_ACTS = {(129, 33, 3), (130, 260, 257)}
CASES = [(s, a) for s in SHAPES for a in (("none", "relu", "sigmoid") if s in ALL_ACTS else ("relu",))]


def case_id(case):
    (n, n_in, n_out), act = case
    return "%dx%dx%d-%s" % (n, n_in, n_out, act)


# ------------------------------------------------------------------------------------------------ the plan of the weight gradient
def tile_j(J):
    return 256 if J > 128 else 128


def cdiv(a, b):
    return -(-a // b)


def dw_plan(n, n_in, n_out):
    """restatement of linear.hip's dw_plan (the host test holds it to nerfhip_linear_bwd_weight_workspace_bytes)"""
    TJ = tile_j(n_in)
    ti, tj = cdiv(n_out, 128), cdiv(n_in, TJ)
    want = max(1, min(cdiv(1024, ti * tj * (TJ // 128)), cdiv(n, 512)))
    per = max(32, cdiv(cdiv(n, want), 32) * 32)
    return dict(TJ=TJ, Ip=ti * 128, Jp=tj * TJ, per=per, splits=max(1, cdiv(n, per)))


def workspace_bytes(n, n_in, n_out):
    p = dw_plan(n, n_in, n_out)
    return p["splits"] * p["Ip"] * (p["Jp"] + 1) * 4


def last_stage(n, n_in, n_out):
    """(first, end) of the points of the last 32-point stage of the last split"""
    p = dw_plan(n, n_in, n_out)
    beg = (p["splits"] - 1) * p["per"]
    return beg + (n - beg - 1) // 32 * 32, n


# ------------------------------------------------------------------------------------------------ data
_data = {}


def data(case):
    """float32 CPU tensors of one case, drawn once: uniform in [-1, 1], weights scaled by 1 / sqrt(K) (no product is subnormal).
    `y` is the layer output handed to the gradient entry points: exact zeros for the ReLU gate, exact 0.0 / 1.0 for the sigmoid."""
    if case in _data:
        return _data[case]
    (n, n_in, n_out), act = case
    g = torch.Generator().manual_seed(1000003 * n + 1009 * n_in + n_out + 7 * ACT[act])
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    d = dict(x=r(n, n_in), w=r(n_out, n_in) / math.sqrt(n_in), b=r(n_out), y_old=r(n, n_out), gy=r(n, n_out),
             gx_old=r(n, n_in), gw_old=r(n_out, n_in), gb_old=r(n_out))
    y = r(n, n_out)
    if act == "sigmoid":
        y = y.abs()
        flat = y.view(-1)
        flat[0::7] = 0.0
        flat[3::11] = 1.0
    else:
        y = y.clamp_min(0.0)                                   # half of them exactly 0
        y.view(-1)[1::13] = -0.0
    d["y"] = y
    _data[case] = d
    return d


def operand(t, mode, rnd=rne_bf16):
    """the value the MFMA multiplies, as fp64"""
    return t.double() if mode == "fp32" else rnd(t.double())


def gated(gy, y, act):
    """g = gy act'(y) in float32, the kernel's order of operations (act_grad in linear.hip)"""
    if act == "relu":
        return torch.where(y > 0, gy, torch.zeros_like(gy))
    if act == "sigmoid":
        return (gy * (1.0 - y)) * y
    return gy


# ------------------------------------------------------------------------------------------------ references (fp64) and bounds
def fwd_ref(x, w, b, y_old, mode, rnd=rne_bf16):
    """(pre, S) of the forward's pre-activation; b / y_old None when they are not added"""
    X, W = operand(x, mode, rnd), operand(w, mode, rnd)
    pre, S = X @ W.t(), X.abs() @ W.abs().t()
    if y_old is not None:
        pre, S = pre + y_old.double(), S + y_old.double().abs()
    if b is not None:
        pre, S = pre + b.double(), S + b.double().abs()
    return pre, S


def gx_ref(gy, y, act, w, old, mode, rnd=rne_bf16):
    G, W = operand(gated(gy, y, act), mode, rnd), operand(w, mode, rnd)
    ref, S = G @ W, G.abs() @ W.abs()
    if old is not None:
        ref, S = ref + old.double(), S + old.double().abs()
    return ref, S


def gw_ref(gy, y, act, x, gw_old, gb_old, mode, rnd=rne_bf16, rows=None, rnd_bias=None):
    """(gw, Sw, gb, Sb); rows: the points summed (default all); the bias gradient sums the same rounded g"""
    G, X = operand(gated(gy, y, act), mode, rnd), operand(x, mode, rnd)
    Gb = G if rnd_bias is None else operand(gated(gy, y, act), mode, rnd_bias)
    if rows is not None:
        G, X, Gb = G[rows], X[rows], Gb[rows]
    gw, Sw, gb, Sb = G.t() @ X, G.abs().t() @ X.abs(), Gb.sum(0), Gb.abs().sum(0)
    if gw_old is not None:
        gw, Sw = gw + gw_old.double(), Sw + gw_old.double().abs()
    if gb_old is not None:
        gb, Sb = gb + gb_old.double(), Sb + gb_old.double().abs()
    return gw, Sw, gb, Sb


def bound_fwd(n_in, S, extra=0):
    """extra: one addition per further column segment of ops.linear_act"""
    return (n_in + 4 + extra) * U * S


def bound_gx(n_out, S):
    return (n_out + 4) * U * S


def bound_dw(n, S):
    return (n + cdiv(n, 512) + 4) * U * S


def ratio(got, ref, tol):
    """worst |got - ref| / tol; inf if anything is not finite, or differs at all where the tolerance is 0 (no terms: an exact zero)"""
    got = got.double()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    if bool((err[tol == 0] != 0).any()):
        return math.inf
    if err.numel() == 0:
        return 0.0
    return (err / tol.clamp_min(1e-300)).max().item()


def fwd_ratio(y, pre, bound, act):
    if act == "relu":
        return math.inf if bool((y < 0).any()) else ratio(y, pre.clamp_min(0.0), bound)
    if act == "sigmoid":
        return ratio(y, torch.sigmoid(pre), 0.25 * bound + 8 * U)       # sigmoid' <= 1/4; expf, the addition, the division
    return ratio(y, pre, bound)


# ------------------------------------------------------------------------------------------------ guarded buffers and layouts
PATTERN = 0x5A5AA5A5                     # what output guards hold (a finite float, 1.5e16)
LEAD, TRAIL = 2, 3                       # extra rows in front of and behind every matrix


def pattern_value():
    return torch.tensor([PATTERN], dtype=torch.int32).view(torch.float32).item()


class Placed:
    """a (rows, width) matrix inside a larger flat float32 buffer: element (r, c) at start + r ld + c"""

    def __init__(self, mat, off, ld, fill):
        rows, width = mat.shape
        assert ld >= width and off >= 0
        self.rows, self.width, self.ld = rows, width, ld
        self.start = LEAD * ld + off
        self.buf = torch.full(((LEAD + rows + TRAIL) * ld + off + 8,), fill, dtype=torch.float32)
        self.view(self.buf).copy_(mat)

    def view(self, buf):
        return torch.as_strided(buf, (self.rows, self.width), (self.ld, 1), self.start)

    def guards(self, buf):
        """the bits of everything outside the matrix"""
        m = torch.ones(buf.numel(), dtype=torch.bool)
        self.view(m).fill_(False)
        return buf.view(torch.int32)[m]

    def byte_offset(self):
        return 4 * self.start

    def loadable16(self, base_alignment=256):
        """whether vec_ok of linear.hip holds, the allocation itself aligned to base_alignment bytes"""
        assert base_alignment % 16 == 0
        return self.byte_offset() % 16 == 0 and self.ld % 4 == 0


def up4(v):
    return (v + 3) // 4 * 4


# how one operand is placed: (offset in floats, stride) as functions of the width.  "vec": 16-byte aligned, stride a multiple of 4;
# "shift": pointer one float past such an address; "odd": an odd stride.
PLACE = {
    "vec": lambda w: (4, up4(w) + 4),
    "vec2": lambda w: (8, up4(w) + 8),
    "shift": lambda w: (5, up4(w) + 4),
    "odd": lambda w: (4, up4(w) + 5),
}
# A = the first GEMM operand (x in the forward, gy in both gradients), Ay = the y that gates it, B = the second (w, w, x)
LAYOUTS = {
    "a": dict(A="vec", Ay="vec2", B="vec"),       # the template VEC kernel
    "b": dict(A="vec2", Ay="vec", B="odd"),       # only A in 16 bytes (run-time O.vec)
    "c": dict(A="shift", Ay="vec", B="vec2"),     # only B (gy is not loadable, so the gated operand is not, whatever y is)
    "d": dict(A="odd", Ay="shift", B="shift"),    # neither
    "e": dict(A="vec", Ay="odd", B="vec2"),       # gy loadable, y not: only the gated operand of the gradients loses its 16-byte path
}
OUT = lambda w: (3, w + 5)                        # every output: ld > width, no alignment


def place(mat, how, fill):
    off, ld = (OUT if how == "out" else PLACE[how])(mat.shape[1])
    return Placed(mat, off, ld, fill)


def loads16(layout, gated_operand):
    """(A, B) loadable in 16 bytes under `layout`, as linear.hip's vec_ok decides it"""
    L = LAYOUTS[layout]
    ok = lambda how: place(torch.zeros(3, 5), how, 0.0).loadable16()
    return ok(L["A"]) and (not gated_operand or ok(L["Ay"])), ok(L["B"])

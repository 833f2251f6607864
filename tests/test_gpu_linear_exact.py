"""GPU: csrc/linear.hip (linear_gemm_kernel, linear_dw_reduce_kernel) element by element against the fp64 sum of the operands it
actually multiplies (tests/linear_ref.py: cases, guarded buffers, references, bounds; proven on the CPU in
tests/test_linear_ref_host.py).  The three C entry points are called directly, so leading dimensions, pointer offsets, `accumulate`
and `gb` are the test's: every matrix lies inside a larger buffer (input guards NaN, output guards and the workspace tail a fixed
bit pattern), in five layouts that pick the template VEC kernel, the run-time 16-byte path of either operand alone, the scalar
path, and a gated operand whose gy is 16-byte loadable while its y is not.  Only layout (a) is held to the bounds; the others must reproduce its bits (the load width differs, the LDS image and the MFMA
order do not).  Bounds: linear_ref's docstring; nothing but the order of an fp32 sum lies between kernel and reference.
Measured ratios of one run: DESIGN.md section 6."""
import ctypes

import pytest
import torch

import linear_ref as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(c) for c in R.CASES]
NAN = float("nan")
_cache = {}


def _code(mode):
    from nerf_pl_amd import _lib
    return {"fp32": _lib.F32, "bf16": _lib.BF16, "bf16_f8": _lib.BF16_F8}[mode]


class _Dev:
    """a Placed matrix on the device; `done()` brings the buffer back, checks that nothing outside the matrix changed, returns it"""

    def __init__(self, dev, mat, how, fill):
        self.p = R.place(mat, how, fill)
        self.t = self.p.buf.to(dev)
        self.ptr = ctypes.c_void_p(self.t.data_ptr() + self.p.byte_offset())
        self.ld = self.p.ld
        assert self.t.data_ptr() % 256 == 0                          # what the layouts' alignment stands on

    def done(self, what):
        after = self.t.cpu()
        assert torch.equal(self.p.guards(after), self.p.guards(self.p.buf)), "%s: a guard element changed" % what
        return self.p.view(after).clone()


def _out(dev, shape_or_old):
    """an output matrix: the old values under accumulate = 1, the guard pattern otherwise (accumulate = 0 must not read it)"""
    pat = R.pattern_value()
    mat = torch.full(shape_or_old, pat) if isinstance(shape_or_old, tuple) else shape_or_old
    return _Dev(dev, mat, "out", pat)


def _call(name, *args):
    from nerf_pl_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*args, _lib.stream_ptr()), name)
    torch.cuda.synchronize()


def run_fwd(dev, d, shape, act, mode, lay="a", guard=NAN, bias=True, y_old=None, x=None):
    n, n_in, n_out = shape
    L = R.LAYOUTS[lay]
    x_ = _Dev(dev, d["x"] if x is None else x, L["A"], guard)
    w_ = _Dev(dev, d["w"], L["B"], guard)
    b_ = _Dev(dev, d["b"][None, :], "shift", guard) if bias else None
    y_ = _out(dev, (n, n_out) if y_old is None else y_old)
    _call("nerfhip_linear_fwd", x_.ptr, x_.ld, w_.ptr, w_.ld, b_.ptr if bias else None, y_.ptr, y_.ld, n, n_in, n_out, R.ACT[act],
          int(y_old is not None), _code(mode))
    return y_.done("forward y")


def run_gx(dev, d, shape, act, mode, lay="a", guard=NAN, gx_old=None, gy=None):
    n, n_in, n_out = shape
    L = R.LAYOUTS[lay]
    gy_ = _Dev(dev, d["gy"] if gy is None else gy, L["A"], guard)
    yy_ = _Dev(dev, d["y"], L["Ay"], guard)
    w_ = _Dev(dev, d["w"], L["B"], guard)
    gx_ = _out(dev, (n, n_in) if gx_old is None else gx_old)
    _call("nerfhip_linear_bwd_input", gy_.ptr, gy_.ld, yy_.ptr, yy_.ld, R.ACT[act], w_.ptr, w_.ld, gx_.ptr, gx_.ld, n, n_in, n_out,
          int(gx_old is not None), _code(mode))
    return gx_.done("input gradient")


def run_gw(dev, d, shape, act, mode, lay="a", guard=NAN, gw_old=None, gb_old=None, with_gb=True):
    """(gw, gb); with_gb False: gb == NULL, and the gb buffer (guarded like the others) must come back untouched"""
    from nerf_pl_amd import _lib
    n, n_in, n_out = shape
    L = R.LAYOUTS[lay]
    gy_ = _Dev(dev, d["gy"], L["A"], guard)
    yy_ = _Dev(dev, d["y"], L["Ay"], guard)
    x_ = _Dev(dev, d["x"], L["B"], guard)
    gw_ = _out(dev, (n_out, n_in) if gw_old is None else gw_old)
    gb_ = _out(dev, (1, n_out) if gb_old is None else gb_old[None, :])
    nbytes = _lib.load().nerfhip_linear_bwd_weight_workspace_bytes(n, n_in, n_out)
    assert nbytes == R.workspace_bytes(n, n_in, n_out) and nbytes % 4 == 0
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev)          # NaNs: nothing may be read before it is written
    _call("nerfhip_linear_bwd_weight", gy_.ptr, gy_.ld, yy_.ptr, yy_.ld, R.ACT[act], x_.ptr, x_.ld, gw_.ptr, gw_.ld,
          gb_.ptr if with_gb else None, _lib.ptr(ws), n, n_in, n_out, int(gw_old is not None), _code(mode))
    assert bool((ws[nbytes:] == 0xFF).all()), "the tail behind the workspace changed"
    gw, gb = gw_.done("weight gradient"), gb_.done("bias gradient")[0]
    if not with_gb:
        want = torch.full_like(gb, R.pattern_value()) if gb_old is None else gb_old
        assert torch.equal(_bits(gb), _bits(want)), "gb == NULL, yet the bias gradient's buffer changed"
    return gw, gb


def _all(dev, case, mode, lay="a", guard=NAN):
    """forward, input gradient, weight + bias gradient of one case, once per (case, mode, layout, guard)"""
    key = (case, mode, lay, guard != guard)
    if key not in _cache:
        shape, act = case
        d = R.data(case)
        gw, gb = run_gw(dev, d, shape, act, mode, lay, guard)
        _cache[key] = dict(y=run_fwd(dev, d, shape, act, mode, lay, guard), gx=run_gx(dev, d, shape, act, mode, lay, guard), gw=gw, gb=gb)
    return _cache[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ratios(case, mode, got, y_old=None, gx_old=None, gw_old=None, gb_old=None, bias=True):
    """error / bound of the four results against the fp64 reference (those present in `got`)"""
    (n, n_in, n_out), act = case
    d = R.data(case)
    q = {}
    if "y" in got:
        pre, S = R.fwd_ref(d["x"], d["w"], d["b"] if bias else None, y_old, mode)
        q["fwd"] = R.fwd_ratio(got["y"], pre, R.bound_fwd(n_in, S), act)
    if "gx" in got:
        ref, S = R.gx_ref(d["gy"], d["y"], act, d["w"], gx_old, mode)
        q["gx"] = R.ratio(got["gx"], ref, R.bound_gx(n_out, S))
    if "gw" in got or "gb" in got:
        gw, Sw, gb, Sb = R.gw_ref(d["gy"], d["y"], act, d["x"], gw_old, gb_old, mode)
        q["gw"] = R.ratio(got["gw"], gw, R.bound_dw(n, Sw))
        if "gb" in got:
            q["gb"] = R.ratio(got["gb"], gb, R.bound_dw(n, Sb))
    return q


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_against_fp64_within_the_bounds(dev, case, mode):
    q = _ratios(case, mode, _all(dev, case, mode))
    print("  %s %s: error / bound %s" % (R.case_id(case), mode, "  ".join("%s %.4f" % kv for kv in q.items())))
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_layouts_and_guards_leave_the_bits_alone(dev, case, mode):
    """layouts (b), (c), (d), (e) — other load paths — and zero in the place of NaN guards: the bits of layout (a)"""
    base = _all(dev, case, mode)
    for lay, guard in (("b", NAN), ("c", NAN), ("d", NAN), ("e", NAN), ("a", 0.0), ("d", 0.0)):
        got = _all(dev, case, mode, lay, guard)
        for k in base:
            assert torch.equal(_bits(got[k]), _bits(base[k])), (lay, guard, k, (got[k] - base[k]).abs().max().item())


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", [(129, 33, 3), (130, 260, 257)])
def test_non_finite_rows_stay_in_their_rows(dev, shape, mode):
    """a NaN row and one +inf element (in the K tail) of x / gy: exactly those two rows are non-finite, every other row of the same
    128-row tile and of the next keeps its bits.  No activation: ReLU and the sigmoid turn -inf into a finite value."""
    case = (shape, "none")
    d = R.data(case)
    n, n_in, n_out = shape
    r_nan, r_inf = 5, 70
    for run, key, clean in ((run_fwd, "x", _all(dev, case, mode)["y"]), (run_gx, "gy", _all(dev, case, mode)["gx"])):
        for lay in ("a", "d"):
            bad = d[key].clone()
            bad[r_nan] = NAN
            bad[r_inf, -1] = float("inf")
            got = run(dev, d, shape, "none", mode, lay, **{key: bad})
            finite = torch.isfinite(got)
            assert not finite[r_nan].any() and not finite[r_inf].any(), (key, lay)
            keep = torch.ones(n, dtype=torch.bool)
            keep[[r_nan, r_inf]] = False
            assert torch.equal(_bits(got[keep]), _bits(clean[keep])), (key, lay)


ACC_CASES = [((129, 33, 3), "sigmoid"), ((130, 260, 257), "relu"), ((513, 64, 64), "relu"), ((4097, 40, 5), "relu")]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", ACC_CASES, ids=[R.case_id(c) for c in ACC_CASES])
def test_accumulate_and_null_bias_gradient(dev, case, mode):
    """accumulate = 1 at all three entry points (the forward as ops.linear_act issues its second segment, with and without the bias)
    within the bounds with |old| included; gb == NULL leaves the bias gradient's buffer alone and the weight gradient's bits as they are"""
    shape, act = case
    d = R.data(case)
    q = {}
    for bias in (True, False):
        y = run_fwd(dev, d, shape, act, mode, bias=bias, y_old=d["y_old"])
        q["fwd" + ("" if bias else " no bias")] = _ratios(case, mode, dict(y=y), y_old=d["y_old"], bias=bias)["fwd"]
    q["fwd no bias, fresh"] = _ratios(case, mode, dict(y=run_fwd(dev, d, shape, act, mode, bias=False)), bias=False)["fwd"]
    q["gx"] = _ratios(case, mode, dict(gx=run_gx(dev, d, shape, act, mode, gx_old=d["gx_old"])), gx_old=d["gx_old"])["gx"]
    gw, gb = run_gw(dev, d, shape, act, mode, gw_old=d["gw_old"], gb_old=d["gb_old"])
    q.update({"acc " + k: v for k, v in _ratios(case, mode, dict(gw=gw, gb=gb), gw_old=d["gw_old"], gb_old=d["gb_old"]).items()})
    gw2, _ = run_gw(dev, d, shape, act, mode, gw_old=d["gw_old"], gb_old=d["gb_old"], with_gb=False)
    assert torch.equal(_bits(gw2), _bits(gw))
    gw3, _ = run_gw(dev, d, shape, act, mode, with_gb=False)
    assert torch.equal(_bits(gw3), _bits(_all(dev, case, mode)["gw"]))
    print("  %s %s accumulate: error / bound %s" % (R.case_id(case), mode, "  ".join("%s %.4f" % kv for kv in q.items())))
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("case", [((129, 33, 3), "sigmoid"), ((130, 260, 257), "relu"), ((4097, 40, 5), "relu")], ids=R.case_id)
def test_bf16_f8_code_and_determinism(dev, case):
    """NERFHIP_BF16_F8 is NERFHIP_BF16 in this file's kernels; a second run of either mode gives the first one's bits (the split sums
    are added in a fixed order)"""
    shape, act = case
    d = R.data(case)
    for mode in R.MODES:
        first = _all(dev, case, mode)
        gw, gb = run_gw(dev, d, shape, act, mode)
        again = dict(y=run_fwd(dev, d, shape, act, mode), gx=run_gx(dev, d, shape, act, mode), gw=gw, gb=gb)
        for k in first:
            assert torch.equal(_bits(again[k]), _bits(first[k])), (mode, k)
    first = _all(dev, case, "bf16")
    gw, gb = run_gw(dev, d, shape, act, "bf16_f8")
    f8 = dict(y=run_fwd(dev, d, shape, act, "bf16_f8"), gx=run_gx(dev, d, shape, act, "bf16_f8"), gw=gw, gb=gb)
    for k in first:
        assert torch.equal(_bits(f8[k]), _bits(first[k])), k


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case,segs", [(((129, 33, 3), "sigmoid"), (6, 27)), (((130, 260, 257), "relu"), (100, 160)),
                                       (((130, 260, 257), "sigmoid"), (33, 127, 100)), (((513, 64, 64), "relu"), (61, 3))],
                         ids=lambda v: R.case_id(v) if isinstance(v[0], tuple) else "+".join(map(str, v)))
def test_ops_linear_act_segments(dev, case, segs, mode):
    """ops.linear_act on two and three column segments against the fp64 reference of the concatenation: K is the total width, plus
    one addition per extra segment.  The gradients gate on the y the forward returned, as the reference here does."""
    from nerf_pl_amd import ops
    (n, n_in, n_out), act = case
    assert sum(segs) == n_in
    d = R.data(case)
    wide = torch.full((n, n_in + 9), NAN)
    wide[:, 4:4 + n_in] = d["x"]
    wide = wide.to(dev)
    xs, col = [], 4
    for c in segs:
        xs.append(wide[:, col:col + c].detach().requires_grad_(True))
        col += c
    w, b = d["w"].to(dev).requires_grad_(True), d["b"].to(dev).requires_grad_(True)
    y = ops.linear_act(xs, w, b, R.ACT[act], mode)
    (y * d["gy"].to(dev)).sum().backward()
    yc = y.detach().cpu()
    pre, S = R.fwd_ref(d["x"], d["w"], d["b"], None, mode)
    q = {"fwd": R.fwd_ratio(yc, pre, R.bound_fwd(n_in, S, extra=len(segs) - 1), act)}
    ref, S = R.gx_ref(d["gy"], yc, act, d["w"], None, mode)
    q["gx"] = R.ratio(torch.cat([x.grad for x in xs], 1).cpu(), ref, R.bound_gx(n_out, S))
    gw, Sw, gb, Sb = R.gw_ref(d["gy"], yc, act, d["x"], None, None, mode)
    q["gw"], q["gb"] = R.ratio(w.grad.cpu(), gw, R.bound_dw(n, Sw)), R.ratio(b.grad.cpu(), gb, R.bound_dw(n, Sb))
    print("  %s %s segments %s: error / bound %s" % (R.case_id(case), mode, segs, "  ".join("%s %.4f" % kv for kv in q.items())))
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("mode", R.MODES)
def test_ops_linear_act_input_forms(dev, mode):
    """a transposed, an expanded (stride 0) and a float64 input give the bits of the contiguous float32 call, forward and gradients"""
    from nerf_pl_amd import ops
    case = ((129, 33, 3), "relu")
    (n, n_in, n_out), act = case
    d = R.data(case)

    def run(x):
        x = x.requires_grad_(True)
        w, b = d["w"].to(dev).requires_grad_(True), d["b"].to(dev).requires_grad_(True)
        y = ops.linear_act([x], w, b, R.ACT[act], mode)
        (y * d["gy"].to(dev)).sum().backward()
        return [_bits(t.detach().float().cpu()) for t in (y, w.grad, b.grad, x.grad)]

    x = d["x"].to(dev)
    base = run(x.clone())
    pre, S = R.fwd_ref(d["x"], d["w"], d["b"], None, mode)
    assert R.fwd_ratio(base[0].view(torch.float32), pre, R.bound_fwd(n_in, S), act) <= 1.0
    for name, form in (("transposed", x.t().contiguous().t()), ("float64", x.double())):
        assert not form.is_contiguous() or form.dtype != torch.float32
        for a, r in zip(run(form.detach()), base):
            assert torch.equal(a, r), name
    row = x[7:8]
    flat = run(row.expand(n, n_in).contiguous())
    leaf = row.clone().requires_grad_(True)
    w, b = d["w"].to(dev).requires_grad_(True), d["b"].to(dev).requires_grad_(True)
    y = ops.linear_act([leaf.expand(n, n_in)], w, b, R.ACT[act], mode)
    assert leaf.expand(n, n_in).stride(0) == 0
    (y * d["gy"].to(dev)).sum().backward()
    for a, r in zip([_bits(t.detach().cpu()) for t in (y, w.grad, b.grad)], flat[:3]):
        assert torch.equal(a, r), "expanded"
    # the expanded call's input gradient is autograd's fp32 sum over the n rows of the contiguous call's: n u sum|rows|
    rows = flat[3].view(torch.float32).double()
    assert leaf.grad.shape == (1, n_in)
    assert R.ratio(leaf.grad.cpu(), rows.sum(0, keepdim=True), n * R.U * rows.abs().sum(0, keepdim=True)) <= 1.0

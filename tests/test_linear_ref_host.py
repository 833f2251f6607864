"""CPU: the checker of tests/linear_ref.py, proven before any kernel meets it.  (1) the reference computed with fp32 accumulation in
two orders stays within the bounds; (2) subtly wrong results are rejected; (3) the case table reaches the tiles, splits, tails and
layouts it claims, from the shapes alone and from nerfhip_linear_bwd_weight_workspace_bytes (a host function)."""
import math

import pytest
import torch

import linear_ref as R

IDS = [R.case_id(c) for c in R.CASES]


def _acc32(A, B, order, extra=()):
    """sum_k A[:, k] B[:, k]^T with every product and every partial sum rounded to float32, k in `order`; then the `extra` terms"""
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    for k in order:
        acc = acc + (A[:, k, None] * B[None, :, k]).float()
    for e in extra:
        if e is not None:
            acc = acc + e
    return acc


def _orders(K, seed):
    return [list(range(K)), torch.randperm(K, generator=torch.Generator().manual_seed(seed)).tolist()]


def _refs(case, mode, rnd=R.rne_bf16, acc=False, rnd_bias=None):
    """the three references of a case: {name: (ref, S, K-bound function applied)} with or without the old values"""
    (n, n_in, n_out), act = case
    d = R.data(case)
    old = (lambda k: d[k]) if acc else (lambda k: None)
    pre, S = R.fwd_ref(d["x"], d["w"], d["b"], old("y_old"), mode, rnd)
    gx, Sx = R.gx_ref(d["gy"], d["y"], act, d["w"], old("gx_old"), mode, rnd)
    gw, Sw, gb, Sb = R.gw_ref(d["gy"], d["y"], act, d["x"], old("gw_old"), old("gb_old"), mode, rnd, rnd_bias=rnd_bias)
    return dict(pre=(pre, R.bound_fwd(n_in, S)), gx=(gx, R.bound_gx(n_out, Sx)), gw=(gw, R.bound_dw(n, Sw)), gb=(gb, R.bound_dw(n, Sb)))


def _fwd_out(pre, act):
    return {"none": pre, "relu": pre.clamp_min(0.0), "sigmoid": torch.sigmoid(pre)}[act]


def _accepts(case, name, got, refs):
    ref, bound = refs[name]
    if name == "pre":
        return R.fwd_ratio(got, ref, bound, case[1]) <= 1.0
    return R.ratio(got, ref, bound) <= 1.0


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_reference_in_fp32_stays_within_the_bounds(case, mode):
    (n, n_in, n_out), act = case
    d = R.data(case)
    op = lambda t: R.operand(t, mode)
    g = R.gated(d["gy"], d["y"], act)
    worst = {}
    for acc in (False, True):
        refs = _refs(case, mode, acc=acc)
        old = (lambda k: d[k]) if acc else (lambda k: None)
        for order in _orders(n_in, 5):
            y = _acc32(op(d["x"]), op(d["w"]), order, (old("y_old"), d["b"]))
            y = {"none": y, "relu": y.clamp_min(0.0), "sigmoid": torch.sigmoid(y)}[act]
            worst["fwd"] = max(worst.get("fwd", 0.0), R.fwd_ratio(y, *refs["pre"], act))
        for order in _orders(n_out, 6):
            gx = _acc32(op(g), op(d["w"]).t(), order, (old("gx_old"),))
            worst["gx"] = max(worst.get("gx", 0.0), R.ratio(gx, *refs["gx"]))
        for order in _orders(n, 7):
            gw = _acc32(op(g).t(), op(d["x"]).t(), order, (old("gw_old"),))
            gb = _acc32(op(g).t(), torch.ones(1, n, dtype=torch.float64), order, (old("gb_old")[:, None] if acc else None,))[:, 0]
            worst["gw"] = max(worst.get("gw", 0.0), R.ratio(gw, *refs["gw"]))
            worst["gb"] = max(worst.get("gb", 0.0), R.ratio(gb, *refs["gb"]))
    print("  %s %s: worst error / bound %s" % (R.case_id(case), mode, {k: round(v, 4) for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


def _mutations(case, mode):
    """[(what, name, mutated result)]: each a reference result that is wrong in one small way"""
    (n, n_in, n_out), act = case
    d = R.data(case)
    op = lambda t: R.operand(t, mode)
    g = R.gated(d["gy"], d["y"], act)
    X, W, G = op(d["x"]), op(d["w"]), op(g)
    pre, _ = R.fwd_ref(d["x"], d["w"], d["b"], None, mode)
    gx, _ = R.gx_ref(d["gy"], d["y"], act, d["w"], None, mode)
    gw, _, gb, _ = R.gw_ref(d["gy"], d["y"], act, d["x"], None, None, mode)
    out = []

    def drop_one(name, res, terms, i, j):
        """element (i, j) loses the largest term of its own sum"""
        m = res.clone()
        t = terms(i, j)
        m[i, j] -= t[t.abs().argmax()]
        out.append(("one term dropped", name, m))

    i, j = n - 1, n_out - 1
    drop_one("pre", pre, lambda i, j: X[i] * W[j], i, j)
    drop_one("gx", gx, lambda i, c: G[i] * W[:, c], n - 1, n_in - 1)
    drop_one("gw", gw, lambda f, c: G[:, f] * X[:, c], n_out - 1, n_in - 1)
    m = gb.clone()
    m[n_out - 1] -= G[:, n_out - 1][G[:, n_out - 1].abs().argmax()]
    out.append(("one term dropped", "gb", m))

    first, end = R.last_stage(n, n_in, n_out)
    keep = torch.ones(n, dtype=torch.bool)
    keep[first:end] = False
    mw, _, mb, _ = R.gw_ref(d["gy"], d["y"], act, d["x"], None, None, mode, rows=keep)
    out += [("last stage of the last split dropped", "gw", mw), ("last stage of the last split dropped", "gb", mb)]
    if first - 32 >= (R.dw_plan(n, n_in, n_out)["splits"] - 1) * R.dw_plan(n, n_in, n_out)["per"]:
        keep = torch.ones(n, dtype=torch.bool)
        keep[first - 32:first] = False                                     # the last FULL 32-point stage of that split
        mw, _, mb, _ = R.gw_ref(d["gy"], d["y"], act, d["x"], None, None, mode, rows=keep)
        out += [("last full stage of the last split dropped", "gw", mw), ("last full stage of the last split dropped", "gb", mb)]

    out.append(("bias added twice", "pre", pre + d["b"].double()))
    out.append(("bias not added", "pre", pre - d["b"].double()))
    if mode == "bf16":
        t = _refs(case, mode, rnd=R.trunc_bf16)
        # Rejected at all four results of every case, with ONE exception: the bias gradient at n = 4097.  Truncation differs from
        # rounding to nearest on about half of the g, by one bf16 spacing (2^-8 .. 2^-7 of |g|) toward zero; over n points that is
        # a drift of ~2^-9 |sum g| plus a random walk of ~n^1/2 2^-8 rms(g), against a bound of (n + 13) 2^-24 sum|g| ~ n^2 2^-24
        # mean|g|.  At n = 513 the walk (~0.03) is 7 x the bound (0.004); the two cross near n ~ 2000; at n = 4097 drift + walk are
        # ~0.05 + 0.07 against a bound of 0.22 (on this case's data: errors of the 5 features up to 0.124, bounds 0.22 - 0.23).  The weight gradient of the same case
        # has 200 elements with both operands truncated and is rejected.  The exception's outcome is printed.
        for k in ("pre", "gx", "gw", "gb"):
            excepted = k == "gb" and n == 4097
            out.append((("(reported) " if excepted else "") + "operands truncated to bf16", k, t[k][0]))
        if n <= 130:
            out.append(("bias gradient of the fp32 g", "gb", _refs(case, mode, rnd_bias=lambda v: v)["gb"][0]))
    nan = float("nan")
    for name, res in (("pre", pre), ("gx", gx), ("gw", gw), ("gb", gb)):
        m = res.clone()
        m.view(-1)[-1] += nan
        out.append(("a NaN guard element in one sum", name, m))
    return out


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_checker_rejects_subtly_wrong_results(case, mode):
    (n, n_in, n_out), act = case
    refs = _refs(case, mode)
    for name in refs:
        assert _accepts(case, name, _fwd_out(refs[name][0], act) if name == "pre" else refs[name][0], refs), name
    changed = 0
    for what, name, mut in _mutations(case, mode):
        ref = refs[name][0]
        got, want = (_fwd_out(mut, act), _fwd_out(ref, act)) if name == "pre" else (mut, ref)
        if torch.equal(got, want):
            continue                                   # e.g. every g of the dropped points gated to zero, or a value bf16 holds exactly
        if what.startswith("(reported)"):
            print("  %s %s: %s, %s: %s" % (R.case_id(case), mode, what, name, "accepted" if _accepts(case, name, got, refs) else "rejected"))
            continue
        changed += 1
        assert not _accepts(case, name, got, refs), (what, name)
    # y_old ignored under accumulate = 1: the result without the old values, judged by the reference with them
    with_old = _refs(case, mode, acc=True)
    for name in refs:
        got = _fwd_out(refs[name][0], act) if name == "pre" else refs[name][0]
        want = _fwd_out(with_old[name][0], act) if name == "pre" else with_old[name][0]
        if not torch.equal(got, want):
            changed += 1
            assert not _accepts(case, name, got, with_old), ("old value ignored", name)
    print("  %s %s: %d mutations rejected" % (R.case_id(case), mode, changed))
    assert changed >= (8 if n > 1 else 4), changed      # the table is not vacuous: nearly every mutation bites on every case


def test_the_restated_plan_is_the_librarys():
    """nerfhip_linear_bwd_weight_workspace_bytes is a host function: the plan test_the_table_reaches_what_it_claims reasons with
    gives the library's sizes, and the size grows where the second split appears"""
    from nerf_pl_amd import _lib
    lib = _lib.load()
    for s in R.SHAPES + [(512, 64, 64), (1, 129, 129), (5000, 400, 400)]:
        assert lib.nerfhip_linear_bwd_weight_workspace_bytes(*s) == R.workspace_bytes(*s), s
    assert lib.nerfhip_linear_bwd_weight_workspace_bytes(513, 64, 64) > lib.nerfhip_linear_bwd_weight_workspace_bytes(512, 64, 64)


def test_the_table_reaches_what_it_claims():
    shapes = R.SHAPES
    for s in shapes:
        assert max(s[0] * s[1], s[0] * s[2]) <= 5000 * 400
    assert R.dw_plan(512, 64, 64)["splits"] == 1 and R.dw_plan(513, 64, 64)["splits"] == 2
    # both tile widths, in each of the three GEMMs (forward: columns = n_out; input gradient and weight gradient: columns = n_in)
    for width in (lambda s: s[2], lambda s: s[1]):
        assert {R.tile_j(width(s)) for s in shapes} == {128, 256}
    # more than one tile along the rows (points; out features in the weight gradient) and along the columns
    assert any(R.cdiv(s[0], 128) > 1 for s in shapes)
    assert max(R.dw_plan(*s)["Ip"] for s in shapes) >= 384
    assert any(R.cdiv(s[2], R.tile_j(s[2])) > 1 for s in shapes), "forward column tiles"
    assert any(R.cdiv(s[1], R.tile_j(s[1])) > 1 for s in shapes), "gradient column tiles"
    splits = {R.dw_plan(*s)["splits"] for s in shapes}
    assert 1 in splits and 2 in splits and max(splits) >= 3, splits
    assert R.dw_plan(4097, 40, 5)["splits"] == 9
    assert R.last_stage(513, 64, 64) == (512, 513) and R.dw_plan(513, 64, 64)["per"] == 288      # 7 stages plus one point
    # K tails, for each GEMM's reduction length
    for K in (lambda s: s[1], lambda s: s[2], lambda s: s[0]):
        assert any(K(s) % 4 for s in shapes) and any(K(s) % 32 and K(s) > 32 for s in shapes)
    assert (127, 32, 128) in shapes and 36 % 32 == 4                                             # one stage exactly; one 4-element unit
    # the layouts (a) - (d): (A, B) loadable in 16 bytes, with and without a gating y; every output stride exceeds its width
    for gatedop in (False, True):
        assert R.loads16("a", gatedop) == (True, True)
        assert R.loads16("b", gatedop) == (True, False)
        assert R.loads16("c", gatedop) == (False, True)
        assert R.loads16("d", gatedop) == (False, False)
    # (e): gy loadable, the y that gates it not — the `!y || ...` half of vec_ok alone turns the gated operand's 16-byte path off
    assert R.loads16("e", False) == (True, True) and R.loads16("e", True) == (False, True)
    assert R.place(torch.zeros(3, 5), R.LAYOUTS["e"]["A"], 0.0).loadable16()
    kinds = {how for L in R.LAYOUTS.values() for how in L.values()}
    assert {"shift", "odd"} <= kinds                                    # a pointer off by one float, and an odd stride
    for w in (1, 3, 33, 257):
        p = R.place(torch.zeros(2, w), "out", 0.0)
        assert p.ld > w
        for how in R.PLACE:
            q = R.place(torch.zeros(2, w), how, 0.0)
            # a 16-byte load that starts inside the matrix ends inside the buffer
            assert q.ld > w and q.start + (q.rows - 1) * q.ld + R.up4(w) <= q.buf.numel()
    # the data holds the gate's edge values
    for case in R.CASES:
        y = R.data(case)["y"]
        if case[1] == "sigmoid":
            assert bool((y == 0).any()) and bool((y == 1).any())
        elif y.numel() > 1:
            assert bool((y == 0).any())


def test_placed_buffers():
    m = torch.arange(12, dtype=torch.float32).view(3, 4)
    p = R.place(m, "shift", float("nan"))
    assert torch.equal(p.view(p.buf), m) and p.buf.isnan().sum().item() == p.buf.numel() - 12
    q = R.place(m, "out", R.pattern_value())
    g = q.guards(q.buf)
    assert g.numel() == q.buf.numel() - 12 and bool((g == R.PATTERN).all()) and math.isfinite(R.pattern_value())
    q.buf[q.start + 4] = 0.0                                                # the first element behind row 0
    assert not torch.equal(q.guards(q.buf), g)

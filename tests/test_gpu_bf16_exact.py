"""GPU: the bf16 MLP kernels — mlp_fwd_kernel<bf16> (activation-saving), mlp_bwd_chain_kernel, mlp_bwd_dw_kernel + reduce + fold,
mlp_dx_embedded — against the rounding-exact model oracle/bf16_exact.py, ONE KERNEL STAGE AT A TIME ON THE VALUES IT ACTUALLY CONSUMED
("teacher forcing"): the saved activation and dY buffers are decoded to plain tensors, each layer / chain layer / weight-gradient
job is recomputed in fp64 from the decoded operands of that very stage, and nothing but the order of an fp32 sum is left between
kernel and model.  The fp32 oracle cannot do this: the legitimate bf16 rounding is 10 % of a gradient tensor (tests/test_gpu_bf16.py),
while a dropped 32-point tile, one wrong feature column or a padded lane leaking into a sum is far less.

Bounds (none of them measured on the kernels; model and decoder are proven on the CPU in tests/test_bf16_exact_host.py):
  * a stored bf16 value (activation, dY) EQUALS bf16(fp64 result), or lies between the roundings of (result -+ K 2^-24 sum|terms|), K
    the reduction length: the worst-case error of a length-K fp32 sum.  Such excused elements are at most EXCUSED_CAP of a layer (the
    model alone, fp32 accumulation in two orders against fp64, needs 6.1e-5: host test);
  * a weight gradient is within (n + c) 2^-24 sum_p |dY X| of the fp64 sum of the exact products of the decoded operands, c the fixed
    depth of the split / lane-half / fold sums; the tensors finished by mlp_bwd_fold_kernel carry that bound through |G| |W_f|^T etc.;
  * end to end (model not teacher-forced): 8 x the model's own fp32-order sensitivity, computed in the test, + the loosest fp32 bound.

Sizes: 1 (one live lane), 33 (a tile + a point), 256 (exactly one forward workgroup), 288 (a workgroup + a tile), 1000 (ragged) and
the smallest n at which the weight-gradient plan gives a job two point splits (asked of nerfhip_mlp_dw_plan, "split" below).
Measured ratios of one run: DESIGN.md section 6."""
import ctypes

import pytest
import torch

from oracle import bf16_exact as E
from tests.helpers import build_models

pytestmark = pytest.mark.gpu

EXCUSED_CAP = 1e-3
SIZES = [1, 33, 256, 288, 1000, "split"]
U = E.U32
_runs = {}


def _splits(n):
    from nerf_pl_amd import _lib
    out = (ctypes.c_int * 12)()
    total = _lib.load().nerfhip_mlp_dw_plan((ctypes.c_int64 * 1)(n), 1, _lib.BF16, out, None)
    assert total > 0
    return list(out)


def _split_size():
    """smallest n whose plan has a job with >= 2 point splits (the plan depends on n through its whole forward workgroups)"""
    for k in range(1, 80):
        n = 256 * (k - 1) + 1
        if max(_splits(n)) >= 2:
            return n
    return None


def _run(dev, n):
    """one forward (saving), chain, dW + reduce + fold and dx at n points: everything the tests compare, on the CPU, computed once"""
    if n == "split":
        n = _split_size()
        # (the plan wants >= 48 ring iterations per workgroup: 2817 points — well under the 20,000 at which this case would be
        # replaced by the largest of the others)
        assert n is not None and n <= 20000, n
    if n in _runs:
        return _runs[n]
    from nerf_pl_amd import ops
    p, x, g_out = E.embedded_case(n)
    (m,), _ = build_models([p], dev, "bf16")
    packed, packed_bwd = m.packed_weights_train("bf16")
    acts = ops.alloc_acts(n, "bf16", dev)
    xd, gd = x.to(dev), g_out.to(dev)
    out = ops.mlp_fwd_embedded(xd, packed, False, "bf16", save=acts)
    ws = {}
    ops.mlp_bwd(gd, out, packed_bwd, acts, "bf16", phases=1, workspace=ws)
    gw, gb, flat = ops.mlp_bwd(gd, out, packed_bwd, acts, "bf16", phases=6, workspace=ws)
    gx = ops.mlp_dx_embedded(ws["dys"], n, m.xyz_encoding_1[0].weight, m.xyz_encoding_5[0].weight, m.dir_encoding[0].weight, "bf16")
    torch.cuda.synchronize()
    tiles = (n + 255) // 256 * 8
    r = dict(n=n, tiles=tiles, p=p, x=x, g_out=g_out, out=out.cpu(), gx=gx.cpu().double(),
             A=E.decode_acts(acts, tiles), D=E.decode_dys(ws["dys"], tiles), splits=_splits(n),
             grads={})
    for i, name in enumerate(E.PARAM_ORDER):
        r["grads"][name + ".weight"], r["grads"][name + ".bias"] = gw[i].cpu().double(), gb[i].cpu().double()
    Ws, Bs = E.decode_packed_fwd(packed)
    r["Ws"], r["Bs"] = Ws, Bs
    # the model with the folded dir-layer weights the pack kernel actually formed (its fp32 chains are not the model's fp64 product)
    r["net"] = E.Net(p, wc=Ws[E.kDirLayer][:, :256], bc=Bs[E.kDirLayer][:128])
    r["dev_handles"] = (m, packed_bwd, acts, ws, gd, out, gw, gb)
    _runs[n] = r
    return r


def _share(mask):
    return mask.double().mean().item()


def _judge(r, what, got, pre, terms, K, gate=None, relu=False):
    exact, excused, wrong = E.judge(r["net"], got, pre, terms, K, gate=gate, relu=relu)
    print("  n=%d %-10s exact %.6f  excused %d of %d (%.2e)  wrong %d" % (r["n"], what, _share(exact), int(excused.sum()), excused.numel(),
                                                                        _share(excused), int(wrong.sum())))
    assert not wrong.any(), (r["n"], what, int(wrong.sum()), wrong.nonzero()[:4].tolist())
    assert int(excused.sum()) <= EXCUSED_CAP * excused.numel(), (r["n"], what, int(excused.sum()), excused.numel())
    return _share(excused)


@pytest.mark.parametrize("n", SIZES)
def test_packed_weights_and_anchors(dev, n):
    """What the other checks stand on, all exact: the bf16 weights the kernels multiply by are the roundings of the masters (the
    folded W_c: within its fp32 product's bound); the saved encodings are bf16(x); the chain's seed is fp32 arithmetic on the kernel's
    own output; a gate bit is [stored activation > 0]; behind point n the activations repeat point n - 1, every dY is zero (so
    whatever a weight-gradient job reads there contributes nothing) and every padding slot is zero."""
    r = _run(dev, n)
    n, net, A, D = r["n"], r["net"], r["A"], r["D"]
    ref = E.Net(r["p"])
    for L, (param, nt, n_out, _, _, _) in enumerate(E.kLayers):
        W, b = r["Ws"][L], r["Bs"][L]
        assert not W[n_out:].any() and not b[n_out:].any(), L                      # rows of the padded output tile
        if L == E.kDirLayer:
            assert torch.equal(W[:, 256:], ref.Wddb) and torch.equal(net.Wddb, ref.Wddb)
            exact, excused, wrong = E.judge(ref, W[:, :256], ref.Wdx @ ref.W[8], ref.Wdx.abs() @ ref.W[8].abs(), 256)
            print("  W_c: exact %.5f of the model's fp64 product, wrong %d" % (_share(exact), int(wrong.sum())))
            assert not wrong.any()
            bc64 = ref.Wdx @ ref.B[8] + ref.B[9]
            assert ((b[:128] - bc64).abs() <= 258 * U * (ref.Wdx.abs() @ ref.B[8].abs() + ref.B[9].abs())).all()
        else:
            assert torch.equal(W[:n_out], ref.Wb[param]), L
            assert torch.equal(b[:n_out], ref.B[param]), L
    assert torch.equal(A["ex"][:n], E.rne_bf16(r["x"][:, :63].double())) and torch.equal(A["ed"][:n], E.rne_bf16(r["x"][:, 63:].double()))
    dy_rgb, dy_sigma = E.seed(net, r["g_out"], r["out"])
    assert torch.equal(D["rgb"][:n], dy_rgb) and torch.equal(D["sigma"][:n], dy_sigma)
    for name in ["h%d" % l for l in range(1, 9)] + ["t"]:
        assert torch.equal(A["gate_" + name], A[name] > 0), name
        assert bool((A[name] >= 0).all()), name
    for name in E.act_sections():
        assert torch.equal(A[name][n:], A[name][n - 1:n].expand(r["tiles"] * 32 - n, -1)), name      # padded lanes compute point n - 1
        assert not A["pad_" + name].any(), name
    for name in E.dy_sections():
        assert not D[name][n:].any(), name                                         # ... and contribute nothing
        assert not D["pad_" + name].any(), name


@pytest.mark.parametrize("n", SIZES)
def test_forward_layers_teacher_forced(dev, n):
    r = _run(dev, n)
    n, net, A = r["n"], r["net"], r["A"]
    h = None
    for l in range(1, 9):
        X = E.layer_operand(l, A["ex"][:n], h)
        pre, terms = E.pre_trunk(net, l, X)
        h = A["h%d" % l][:n]
        _judge(r, "h%d" % l, h, pre, terms, X.shape[1] + 1, relu=True)
    pre, terms = E.pre_dir(net, h, A["ed"][:n])
    _judge(r, "t", A["t"][:n], pre, terms, 27 + 256 + 1, relu=True)
    out = r["out"].double()
    pre, terms = E.pre_sigma(net, h)
    err = ((out[:, 3:4] - pre).abs() / (257 * U * terms)).max().item()
    print("  n=%d sigma: error / bound %.3f" % (n, err))
    assert err <= 1.0
    pre, terms = E.pre_rgb(net, A["t"][:n])
    # sigmoid' <= 1/4; expf, the addition and the division in fp32 on a result <= 1: 8 units in all
    err = ((out[:, :3] - torch.sigmoid(pre)).abs() / (0.25 * 129 * U * terms + 8 * U)).max().item()
    print("  n=%d rgb: error / bound %.3f" % (n, err))
    assert err <= 1.0


@pytest.mark.parametrize("n", SIZES)
def test_chain_layers_teacher_forced(dev, n):
    r = _run(dev, n)
    n, net, A, D = r["n"], r["net"], r["A"], r["D"]
    gate = lambda name: A["gate_" + name][:n].double()
    _, s, terms = E.chain_dir(net, D["rgb"][:n], gate("t"))
    _judge(r, "dY_dir", D["dir"][:n], s, terms, 3, gate=gate("t"))
    _, s, terms = E.chain_h8(net, D["dir"][:n], D["sigma"][:n], gate("h8"))
    _judge(r, "dY_8", D["dy8"][:n], s, terms, 129, gate=gate("h8"))
    for l in range(7, 0, -1):
        _, s, terms = E.chain_trunk(net, l, D["dy%d" % (l + 1)][:n], gate("h%d" % l))
        _judge(r, "dY_%d" % l, D["dy%d" % l][:n], s, terms, 256, gate=gate("h%d" % l))


def _dw_checks(r, c):
    """[(name, got, ref, bound)] of the 24 gradient tensors from the decoded operands of their jobs (first n points, fp64)"""
    n, net, A, D, g = r["n"], r["net"], r["A"], r["D"], r["grads"]
    k = (n + c) * U
    rows = []
    h = lambda l: A["h%d" % l][:n]
    for l in range(1, 9):
        X = E.layer_operand(l, A["ex"][:n], h(l - 1) if l > 1 else None)
        dW, db, aW, ab = E.dw_job(D["dy%d" % l][:n], X)
        rows += [(E.PARAM_ORDER[l - 1] + ".weight", dW, k * aW), (E.PARAM_ORDER[l - 1] + ".bias", db, k * ab)]
    dW, db, aW, ab = E.dw_job(D["rgb"][:n], A["t"][:n])
    rows += [("rgb.0.weight", dW, k * aW), ("rgb.0.bias", db, k * ab)]
    dW, db, aW, ab = E.dw_job(D["sigma"][:n], h(8))
    rows += [("sigma.weight", dW, k * aW), ("sigma.bias", db, k * ab)]
    Gd, s, aG, a_s = E.dw_job(D["dir"][:n], torch.cat([A["ed"][:n], h(8)], 1))
    G, eG, es = Gd[:, 27:], k * aG[:, 27:], k * a_s
    dWdx, dWf, dbf = E.fold(net, G, s)
    Wf, bf, Wdx = net.W[8].abs(), net.B[8].abs(), net.Wdx.abs()
    # mlp_bwd_fold_kernel: fp32 sums of 256 (+ the s b_f term) / 128 products of the fp32 G, s it is handed
    b_dx = eG @ Wf.t() + es[:, None] * bf[None, :] + 260 * U * (G.abs() @ Wf.t() + s.abs()[:, None] * bf[None, :])
    b_f = Wdx.t() @ eG + 132 * U * (Wdx.t() @ G.abs())
    b_bf = Wdx.t() @ es + 132 * U * (Wdx.t() @ s.abs())
    rows += [("dir_encoding.0.weight", torch.cat([dWdx, Gd[:, :27]], 1), torch.cat([b_dx, k * aG[:, :27]], 1)),
             ("dir_encoding.0.bias", s, es), ("xyz_encoding_final.weight", dWf, b_f), ("xyz_encoding_final.bias", dbf, b_bf)]
    return [(name, g[name], ref, bound) for name, ref, bound in rows]


def _ratio(got, ref, bound):
    err = (got - ref).abs()
    assert bool((err[bound == 0] == 0).all())                                     # no terms at all: the sum is an exact zero
    return (err / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("n", SIZES)
def test_weight_gradients_teacher_forced(dev, n):
    r = _run(dev, n)
    c = 8 + max(r["splits"])             # the splits' sum, the two bias chains, the lane halves, the fold's four partial tiles
    print("  n=%d: splits per job %s" % (r["n"], r["splits"]))
    if n == "split":
        assert max(r["splits"]) >= 2
    worst = 0.0
    for name, got, ref, bound in _dw_checks(r, c):
        assert got.shape == ref.shape, name
        q = _ratio(got, ref, bound)
        worst = max(worst, q)
        print("  n=%d %-28s error / bound %.4f" % (r["n"], name, q))
        assert q <= 1.0, (r["n"], name, q)
    print("  n=%d worst dW error / bound %.4f" % (r["n"], worst))


@pytest.mark.parametrize("n", SIZES)
def test_dx_teacher_forced(dev, n):
    r = _run(dev, n)
    n, D = r["n"], r["D"]
    ref, a = E.dx(r["net"], D["dy1"][:n], D["dy5"][:n], D["dir"][:n])
    K = torch.cat([torch.full((63,), 512.0 + 2), torch.full((27,), 128.0 + 2)]).double()     # fmaf chains of a lane half + the halves' sum
    q = _ratio(r["gx"], ref, K[None, :] * U * a)
    print("  n=%d dx: error / bound %.4f" % (n, q))
    assert q <= 1.0


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("n", SIZES)
def test_end_to_end_against_the_model(dev, n):
    """The model run on its own (no teacher forcing) against the kernels: out and the 24 gradients.  Rare one-digit differences of a
    stored bf16 value and ReLU gates that flip on them propagate, so this is blunter than the per-stage checks; its bound is the
    model's own sensitivity to the order of its fp32 sums — fp32 accumulation in two orders against fp64, here, on these inputs —
    times 8 (the MFMA's block order is none of the two), plus the loosest fp32 bound of the per-stage checks."""
    r = _run(dev, n)
    net, x, g_out = r["net"], r["x"], r["g_out"]
    f64 = E.forward(net, x)
    b64 = E.backward(net, f64, g_out)
    sens_out, sens = 0.0, {k: 0.0 for k in b64["grads"]}
    for mode in ("f32", "f32perm"):
        acc = E.Accumulate(mode, seed=11)
        f = E.forward(net, x, acc)
        b = E.backward(net, f, g_out, acc=acc)
        sens_out = max(sens_out, (f["out"] - f64["out"]).abs().max().item())
        for k in sens:
            sens[k] = max(sens[k], _rel(b["grads"][k], b64["grads"][k]))
    c = 8 + max(r["splits"])
    loosest = max((bound.norm() / ref.norm().clamp_min(1e-300)).item() for _, _, ref, bound in _dw_checks(r, c))
    out_tol = 8 * sens_out + 257 * U * E.pre_sigma(net, f64["h"][8])[1].max().item()
    out_err = (r["out"].double() - f64["out"]).abs().max().item()
    print("  n=%d out: max abs difference %.3e, bound %.3e" % (r["n"], out_err, out_tol))
    fails = []
    for k in sens:
        bound, got = 8 * sens[k] + loosest, _rel(r["grads"][k], b64["grads"][k])
        print("  n=%d %-28s relative L2 %.3e, bound %.3e (model's own %.3e)" % (r["n"], k, got, bound, sens[k]))
        if got > bound:
            fails.append((k, got, bound))
    assert out_err <= out_tol and not fails, (r["n"], out_err, out_tol, fails)


def test_accumulate_adds_a_second_backward(dev):
    """accumulate = 1 on the gradients of a first call: twice the first call's sums, within the bound of the doubled sum (+ the one
    addition); G and s of the fold are this call's alone, its three tensors accumulate like the others."""
    from nerf_pl_amd import _lib, ops
    r = _run(dev, 33)
    m, packed_bwd, acts, ws, gd, out, gw, gb = r["dev_handles"]
    gwp = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in gw])
    gbp = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in gb])
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().nerfhip_mlp_bwd_phases(_lib.ptr(gd), _lib.ptr(out), 33, _lib.ptr(packed_bwd), _lib.ptr(acts), _lib.ptr(ws["dys"]),
                                                      _lib.ptr(ws["ws"]), gwp, gbp, 1, _lib.BF16, 7, _lib.stream_ptr()), "nerfhip_mlp_bwd_phases")
        torch.cuda.synchronize()
    c = 8 + max(r["splits"])
    i = {name: j for j, name in enumerate(E.PARAM_ORDER)}
    for name, _, ref, bound in _dw_checks(r, c + 2):
        base, kind = name.rsplit(".", 1)
        got = (gw if kind == "weight" else gb)[i[base]].cpu().double()
        q = _ratio(got, 2 * ref, 2 * bound)
        assert q <= 1.0, (name, q)
    # (the cached first-call gradients were copied to the CPU before this call: the other tests are unaffected)

"""GPU: TWO ranks of the real training step on ONE MI355X (both on cuda:0, gloo on device tensors, file rendezvous), every result
checked against a single-process computation on the same inputs: what one process gets by computing both ranks' gradients and
averaging them by hand.  At world 1 (tests/test_gpu_training.py) the average of one rank is that rank; here a missing or doubled
division, an all-reduce ordered before the reduce kernel finished, a replay that reduces a stale buffer or Adam applied inside the
reduce on LOCAL gradients all show as numbers.

The module-scoped fixture starts the two ranks ONCE (tests/world2_launch.py -> tests/world2_rank.py, each under `timeout`), then
computes the references in this process; every test below only compares stored tensors.  Three processes have the GPU open.

Not covered here, on purpose: RCCL between devices (needs two), and the one-graph form with the collective captured (gloo cannot
be captured; every stepper here is built with sync_in_graph=False).

Time limits: one clean run of the pair (all twelve scenarios, start of the children to their exit) measured 5.0 s on an MI355X
(MEASURED_PAIR_SECONDS; 4.8 and 5.4 s in two further runs, the last one among the other GPU tests); each child's `timeout` is three
times that rounded up to 10 s = 20 s (CHILD_LIMIT), the gloo collective timeout half of the child's limit = 10 s
(COLLECTIVE_TIMEOUT).  A child ended at its limit counts as a hang."""
import pytest
import torch

from tests import world2_launch as L
from tests import world2_rank as W

pytestmark = pytest.mark.gpu

MEASURED_PAIR_SECONDS = 5.0             # one clean run of the pair, all scenarios, on an MI355X
CHILD_LIMIT, COLLECTIVE_TIMEOUT = 20, 10          # 3 x 5.0 s rounded up to 10 s; half of that


def _plain_backward(system, batch, i):
    out = system.training_step(batch, i)
    system.optimizer.zero_grad(set_to_none=True)
    out["loss"].backward()


def _reference_grads(dev):
    """per rank: the gradient of batch 0 (scenario a) and the accumulated gradient of batches 0 + 1 (scenario b), plain backwards"""
    system = W.make_system(dev)
    system.configure_optimizers()
    one, acc = [], []
    for r in range(2):
        _plain_backward(system, W.make_batch(r, 0, dev), 0)
        one.append(W.flat_grads(system))
        system.training_step(W.make_batch(r, 1, dev), 1)["loss"].backward()        # on top of batch 0's: p.grad accumulates
        acc.append(W.flat_grads(system))
    return one, acc


def _reference_trajectory(dev, dtype):
    """STEPS steps of FlatAdam on the hand average: both ranks' gradients computed one after the other, averaged into the flat
    buffers the optimizer reads"""
    from nerf_pl_amd.models.mlp_autograd import flat_grad
    from nerf_pl_amd.parallel import GradSync
    system = W.make_system(dev, dtype)
    (opt,), _ = system.configure_optimizers()
    for i in range(W.STEPS):
        gs = []
        for r in range(2):
            _plain_backward(system, W.make_batch(r, i, dev), i)
            gs.append([flat_grad(m).clone() for m in system.models])
        for k, m in enumerate(system.models):
            assert GradSync._aliases(list(m.parameters()), flat_grad(m))            # p.grad IS the buffer the average goes into
            flat_grad(m).copy_((gs[0][k] + gs[1][k]) / 2)
        opt.step()
    return W.train_state(system, opt)


def _reference_ddp(dev):
    system = W.make_system(dev, flat_optimizer=False)
    gs = []
    for r in range(2):
        b = W.make_batch(r, 1, dev)                                                 # the batch of the ranks' SECOND backward
        system.zero_grad(set_to_none=True)
        system.loss(system(b["rays"]), b["rgbs"]).backward()
        gs.append(W.named_grads(system))
    return gs


@pytest.fixture(scope="module")
def world2(dev, tmp_path_factory):
    ranks, seconds = L.run_pair(W.GPU_SCENARIOS, tmp_path_factory.mktemp("world2"), CHILD_LIMIT, COLLECTIVE_TIMEOUT)
    print("world-2 pair: %.1f s (child limit %d s, collective timeout %d s)" % (seconds, CHILD_LIMIT, COLLECTIVE_TIMEOUT))
    one, acc = _reference_grads(dev)
    ref = {"one": one, "acc": acc, "ddp": _reference_ddp(dev),
           "traj": {"fp32": _reference_trajectory(dev, "fp32"), "bf16": _reference_trajectory(dev, "bf16")}}
    with torch.no_grad():
        ref["shard"] = {k: v.cpu() for k, v in W.render_fn(W.make_system(dev))(W.shard_rays(dev)).items()}
    torch.cuda.synchronize()
    return {"ranks": ranks, "ref": ref, "seconds": seconds}


def _bit_equal_up_to_denormal_halving(got, g0, g1):
    """got == (g0 + g1) / 2 bit for bit: two fp32 addends sum the same in either order and halving is exact — except where
    |g0 + g1| < 2^-125, whose half may fall between denormals: one denormal step (2^-149) there.  Returns the largest difference."""
    want = (g0 + g1) / 2
    assert torch.isfinite(got).all()
    diff = (got.double() - want.double()).abs()
    bad = got != want
    if bool(bad.any()):
        allowed = ((g0.double() + g1.double()).abs() < 2.0 ** -125) & (diff <= 2.0 ** -149)
        assert bool((~bad | allowed).all()), (int((bad & ~allowed).sum()), float(diff[bad & ~allowed].max()))
    return float(diff.max())


@pytest.mark.parametrize("form,overlap", W.GRAD_CASES)
def test_one_averaged_gradient(world2, form, overlap):
    """a. training_step, zero_grad(set_to_none=True), backward, sync(): both ranks hold the same flat gradient, bit-equal to the
    hand average of two plain backwards; with overlap the collective was issued from the backward's hook, without it by sync()"""
    r0, r1 = (rk[W.grad_case_name(form, overlap)] for rk in world2["ranks"])
    g0, g1 = world2["ref"]["one"]
    worst = 0.0
    for n in W.MODEL_NAMES:
        assert float(g0[n].abs().max()) > 0 and not torch.equal(g0[n], g1[n])       # an average that is neither rank's own
        assert torch.equal(r0[n], r1[n]), (form, overlap, n)
        worst = max(worst, _bit_equal_up_to_denormal_halving(r0[n], g0[n], g1[n]))
    print("one averaged gradient, %s overlap=%s: ranks identical, max |g - (g0 + g1) / 2| = %.3e" % (form, overlap, worst))
    for r in (r0, r1):
        assert r["adopted"]                                                          # p.grad are views of the reduced buffer
        if not overlap:
            assert r["issue_log"] == [] and r["started_early"] == 0
        elif form == "merged":
            assert r["issue_log"] == [["joint", "2"]] and r["started_early"] == 1
        else:
            assert sorted(r["issue_log"]) == [["model", "coarse"], ["model", "fine"]] and r["started_early"] == 2
            assert r["issue_log"][0] == ["model", "fine"]                            # autograd order: the fine model's travels first


def test_accumulated_gradient(world2):
    """b. two backwards on two batches before one sync() (the hook's "p.grad is not None" branch): the mean over the ranks of the
    per-rank sums; the bound of test_stock_ddp_world1_on_flat_buffer_grads"""
    r0, r1 = (rk["accum"] for rk in world2["ranks"])
    s0, s1 = world2["ref"]["acc"]
    one = world2["ref"]["one"]
    worst = 0.0
    for n in W.MODEL_NAMES:
        want = (s0[n] + s1[n]) / 2
        assert not torch.equal(s0[n], one[0][n])                                     # the second batch did add something
        assert torch.equal(r0[n], r1[n]), n
        worst = max(worst, float((r0[n] - want).abs().max()))
        assert torch.allclose(r0[n], want, rtol=1e-5, atol=1e-9), (n, float((r0[n] - want).abs().max()))
    print("accumulated gradient: ranks identical, max |g - mean of sums| = %.3e" % worst)
    assert r0["started_early"] == r1["started_early"] == 1                           # the first backward's; the second issued nothing


@pytest.mark.parametrize("form", W.TRAJ_FORMS)
def test_trajectory(world2, form):
    """c. six FlatAdam steps — eager fit(), the two-graph GraphedTrainStep, the same in bf16 with system.fuse_adam = True (hooks on,
    and with GradSync(overlap=False): no hook, so only NeRFSystem._fused_adam_ok keeps Adam out of the reduce kernel): replicas
    identical, and equal to six single-process steps on the hand-averaged gradients within the bound of
    test_graphed_train_step_equals_eager.  A fused update on local gradients separates the ranks after step 1."""
    r0, r1 = (rk["traj_" + form] for rk in world2["ranks"])
    ref = world2["ref"]["traj"]["bf16" if "bf16" in form else "fp32"]
    init = W.make_system(torch.device("cpu"))
    worst = 0.0
    for n, m in zip(W.MODEL_NAMES, init.models):
        for what in ("param_", "exp_avg_", "exp_avg_sq_"):
            k = what + n
            assert torch.equal(r0[k], r1[k]), (form, k, float((r0[k] - r1[k]).abs().max()))
            worst = max(worst, float((r0[k] - ref[k]).abs().max()))
            assert torch.allclose(r0[k], ref[k], rtol=1e-5, atol=1e-7), (form, k, float((r0[k] - ref[k]).abs().max()))
        start = torch.cat([p.detach().reshape(-1) for p in m.flat_params()])
        assert float((r0["param_" + n] - start).abs().max()) > 1e-4                 # six steps of lr 5e-4 did move the weights
    print("trajectory %s: ranks identical, max |x - single-process| over params and moments = %.3e; last step's all-reduces: %s"
          % (form, worst, r0.get("last_step_all_reduce_numels")))
    for r in (r0, r1):
        assert r["optimizer"] == "FlatAdam" and r["step"] == 6.0
        assert all(torch.isfinite(torch.tensor(r["losses"]))) and len(r["losses"]) == W.STEPS
        if form != "eager":
            assert r["graph"] and r["graph_opt"] and r["hooks_enabled"] and r["capture_fallback"] == "None"
            # between the two graphs sync() sends the step's gradients as ONE message: the joint buffer of both models
            assert r["last_step_all_reduce_numels"] == [r["param_coarse"].numel() + r["param_fine"].numel()]
    assert ref["step"] == 6.0


def test_stock_ddp_world2(world2):
    """d. DistributedDataParallel(system, device_ids=[0]) over the same gloo group, two backwards with set_to_none between them"""
    r0, r1 = (rk["ddp"]["grad"] for rk in world2["ranks"])
    g0, g1 = world2["ref"]["ddp"]
    want = (g0 + g1) / 2
    assert float(want.abs().max()) > 0 and not torch.equal(g0, g1)
    assert torch.equal(r0, r1)
    print("stock DDP: ranks identical, max |g - hand average| = %.3e" % float((r0 - want).abs().max()))
    assert torch.allclose(r0, want, rtol=1e-5, atol=1e-9), float((r0 - want).abs().max())


def test_sharded_inference(world2):
    """e. render_sharded over 1001 rays (501 / 500): the gathered image is the same on both ranks and bit-equal to one unsharded
    call — rays are independent, so a difference would mean the render depends on a ray's position in its batch"""
    r0, r1 = (rk["shard"] for rk in world2["ranks"])
    ref = world2["ref"]["shard"]
    assert r0["host_gather"] == r1["host_gather"]
    print("sharded inference: gather on the %s%s" % ("HOST (gloo refused the device tensor: %s)" % r0["gather_error"]
                                                       if r0["host_gather"] else "device", ""))
    for k, shape in (("rgb_fine", (W.SHARD_RAYS, 3)), ("depth_fine", (W.SHARD_RAYS,)), ("opacity_fine", (W.SHARD_RAYS,))):
        assert tuple(r0[k].shape) == shape and float(ref[k].abs().max()) > 0
        assert torch.equal(r0[k], r1[k]), k
        assert torch.equal(r0[k], ref[k]), (k, float((r0[k] - ref[k]).abs().max()), int((r0[k] != ref[k]).sum()))
    for r in (r0, r1):
        assert r["one_key_names"] == ["rgb_fine"] and torch.equal(r["one_key_rgb_fine"], ref["rgb_fine"])


def test_ranks_agree(world2):
    """f. GradSync.agree_any: true on every rank if true on any"""
    for rk in world2["ranks"]:
        assert rk["agree"]["one_rank_true"] is True and rk["agree"]["all_false"] is False

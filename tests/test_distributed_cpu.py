"""N>1 path on CPU: world_size-2 `gloo` processes exercise the ray sharding + gather of
`parallel.render_sharded` and the gradient averaging of `parallel.GradSync` (both the flat-buffer
branch the HIP backward produces and the generic branch) — the host logic that `bench.py --gpus N`
and the 8-GPU configs use with backend nccl (= RCCL).  No HIP compute is called here."""
import contextlib
import os
import socket
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nerf_pl_amd import parallel
from nerf_pl_amd.models.mlp_autograd import flat_grad, grad_hooks, grads_ready


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_render(rays):
    # a deterministic per-ray function, so that sharded == unsharded can be checked exactly
    return {"rgb_fine": torch.stack([rays[:, 0] * 2, rays[:, 1] + 1, rays[:, 2] ** 2], 1),
            "depth_fine": rays[:, 6] + rays[:, 7], "opacity_fine": rays.sum(1)}


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Linear(7, 3)


class _RecordingBackend:
    """Stand-in for system._HipGraphBackend on CPU.  Like a stream capture, `capture` does NOT execute the work (it only
    records the callable); every `replay` executes it and refreshes the static output holder in place — the same
    contract (static inputs, static outputs, nothing runs at capture time) without a device."""

    class _G:
        def __init__(self, fn, holder):
            self.fn, self.holder, self.replays = fn, holder, 0

        def replay(self):
            self.replays += 1
            r = self.fn()
            if isinstance(r, dict):
                self.holder.clear()
                self.holder.update(r)

    def __init__(self):
        self.captures = 0

    def on_side_stream(self, fn, *args):
        return fn(*args)

    def capture(self, fn, share_pool_with=None):
        self.captures += 1
        holder = {}
        return self._G(fn, holder), holder


class _TinySystem(torch.nn.Module):
    """training_step contract of NeRFSystem (train.py:103-117) on a toy model whose backward announces its flat gradient
    buffer exactly like the fused HIP backward does (models/mlp_autograd._param_grads)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.net = _Tiny()
        self.models = [self.net]

    def training_step(self, batch, nb):
        y = self.net.b(torch.relu(self.net.a(batch["x"])))
        return {"loss": ((y - batch["y"]) ** 2).mean()}


class _Checks:
    """Every condition a rank checks, by name; none short-circuits another (the parent test prints the names that failed)."""

    def __init__(self):
        self.results = {}

    def __call__(self, name, cond):
        assert name not in self.results, name
        self.results[name] = bool(cond)


_SIZES = [p.numel() for p in _Tiny().parameters()]
_N = sum(_SIZES)


def _base():
    return torch.arange(_N, dtype=torch.float32)


def _adopt(model, flat):
    """what autograd does with the views the backward returns: they become p.grad"""
    off = 0
    for p, sz in zip(model.parameters(), _SIZES):
        p.grad = flat[off:off + sz].view_as(p)
        off += sz


def _accumulate(model, flat):
    """what autograd does with them when p.grad exists"""
    off = 0
    for p, sz in zip(model.parameters(), _SIZES):
        p.grad += flat[off:off + sz].view_as(p)
        off += sz


def _grads(model):
    return torch.cat([p.grad.reshape(-1) for p in model.parameters()])


def _clear(model):
    for p in model.parameters():
        p.grad = None


@contextlib.contextmanager
def _patched(name, make):
    """dist.<name> replaced by make(real) inside the block; yields the list of the calls' first arguments"""
    real, seen = getattr(dist, name), []
    setattr(dist, name, make(real, seen))
    try:
        yield seen
    finally:
        setattr(dist, name, real)


def _counting(real, seen):
    def f(*a, **kw):
        seen.append(a[0] if a else None)
        return real(*a, **kw)
    return f


def _raising(exc):
    def make(real, seen):
        def f(*a, **kw):
            raise exc
        return f
    return make


def _graphed_step_host_logic(check, rank, world):
    """The N>1 training step's host logic (system.GraphedTrainStep): eager warm-up steps, capture of [forward+backward] and
    [optimizer] as two graphs with the collective issued eagerly in between, replays, re-capture on a learning-rate change —
    with a recording stand-in for the hipGraph backend."""
    from nerf_pl_amd.system import GraphedTrainStep
    g = torch.Generator().manual_seed(100 + rank)           # every rank draws its own batch (weak scaling)
    batches = [{"x": torch.randn(16, 5, generator=g), "y": torch.randn(16, 3, generator=g)} for _ in range(7)]
    sysm = _TinySystem()
    opt = torch.optim.SGD(sysm.parameters(), lr=0.1)
    sync = parallel.GradSync(sysm.models)
    be = _RecordingBackend()
    stepper = GraphedTrainStep(sysm, opt, grad_sync=sync, warmup=2, backend=be, sync_in_graph=False)    # the two-graph form
    for b in batches[:5]:
        stepper(b)
    check("step/two_graphs_captured", be.captures == 2 and stepper.graph is not None and stepper.graph_opt is not None)
    check("step/two_graphs_replayed", stepper.graph.replays == 3 and stepper.graph_opt.replays == 3)     # calls 3,4,5 replayed
    check("step/hooks_back_on_after_capture", sync.hooks_enabled)
    for grp in opt.param_groups:                            # scheduler step: lr is a captured argument
        grp["lr"] = 0.05
    for b in batches[5:]:
        stepper(b)
    check("step/recaptured_on_lr_change", be.captures == 4 and stepper.captured_lr == 0.05)
    # replicas stay identical (same init, averaged gradients) and equal a single-process run on the averaged gradient
    flat = torch.cat([p.detach().reshape(-1) for p in sysm.parameters()])
    gathered = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    check("step/replicas_identical", all(torch.equal(gathered[0], t) for t in gathered))
    ref = _TinySystem()
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1)
    gens = [torch.Generator().manual_seed(100 + r) for r in range(world)]
    allb = [[{"x": torch.randn(16, 5, generator=gg), "y": torch.randn(16, 3, generator=gg)} for _ in range(7)] for gg in gens]
    for i in range(7):
        if i == 5:
            for grp in ropt.param_groups:
                grp["lr"] = 0.05
        ropt.zero_grad()
        for r in range(world):
            (ref.training_step(allb[r][i], i)["loss"] / world).backward()
        ropt.step()
    rflat = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
    check("step/two_graphs_follow_reference", torch.allclose(flat, rflat, rtol=1e-5, atol=1e-6))
    # the default IS the one-graph form (round 6; the two-graph form is the agreed fallback and an explicit choice)
    check("step/default_is_one_graph", not GraphedTrainStep(sysm, opt, grad_sync=sync, backend=_RecordingBackend())._two_graphs())

    def run(step, optimizer):
        for i, b in enumerate(batches):
            if i == 5:
                for grp in optimizer.param_groups:
                    grp["lr"] = 0.05
            step(b)

    # the default N > 1 form: ONE graph with the collectives inside (issued by sync() during the captured step) — same replicas
    sys1 = _TinySystem()
    opt1 = torch.optim.SGD(sys1.parameters(), lr=0.1)
    be1 = _RecordingBackend()
    step1 = GraphedTrainStep(sys1, opt1, grad_sync=parallel.GradSync(sys1.models), warmup=2, backend=be1)
    run(step1, opt1)
    flat1 = torch.cat([p.detach().reshape(-1) for p in sys1.parameters()])
    check("step/one_graph_per_capture", be1.captures == 2 and step1.graph_opt is None and step1.graph.replays == 2)
    check("step/one_graph_follows_reference", torch.allclose(flat1, rflat, rtol=1e-5, atol=1e-6))
    # a stack that cannot capture the collective: the one-graph capture raises, the stepper falls back to two graphs on every
    # rank alike and the replicas still follow the reference run
    sys2 = _TinySystem()
    opt2 = torch.optim.SGD(sys2.parameters(), lr=0.1)

    class _NoCollectiveInGraph(_RecordingBackend):
        def capture(self, fn, share_pool_with=None):
            if getattr(fn, "__name__", "") == "<lambda>" and "_eager" in fn.__code__.co_names:
                raise RuntimeError("collective not capturable")
            return super().capture(fn, share_pool_with)

    be2 = _NoCollectiveInGraph()
    step2 = GraphedTrainStep(sys2, opt2, grad_sync=parallel.GradSync(sys2.models), warmup=2, backend=be2, sync_in_graph=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run(step2, opt2)
    flat2 = torch.cat([p.detach().reshape(-1) for p in sys2.parameters()])
    check("step/uncapturable_falls_back_to_two_graphs",
          step2.capture_fallback is not None and step2._two_graphs() and step2.graph_opt is not None)
    check("step/uncapturable_follows_reference", torch.allclose(flat2, rflat, rtol=1e-5, atol=1e-6))
    # ... and a capture that fails on ONE rank only (rank 1), with its peer waiting in the collective the ranks use to agree on the
    # branch (GradSync.agree_any): BOTH ranks must fall back — a rank replaying a captured all-reduce against a rank issuing an
    # eager one would deadlock — and the replicas still follow the reference run
    sys3 = _TinySystem()
    opt3 = torch.optim.SGD(sys3.parameters(), lr=0.1)

    class _Rank1CannotCapture(_RecordingBackend):
        def capture(self, fn, share_pool_with=None):
            if rank == 1 and getattr(fn, "__name__", "") == "<lambda>" and "_eager" in fn.__code__.co_names:
                raise ValueError("capture failed on this rank only (not a RuntimeError: the peer must still not be left waiting)")
            return super().capture(fn, share_pool_with)

    step3 = GraphedTrainStep(sys3, opt3, grad_sync=parallel.GradSync(sys3.models), warmup=2, backend=_Rank1CannotCapture(), sync_in_graph=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run(step3, opt3)
    flat3 = torch.cat([p.detach().reshape(-1) for p in sys3.parameters()])
    check("step/one_rank_fails_both_fall_back", step3.capture_fallback is not None and step3._two_graphs() and step3.graph_opt is not None)
    check("step/one_rank_fails_peer_is_told", ("another rank" in step3.capture_fallback) == (rank != 1))
    check("step/one_rank_fails_follows_reference", torch.allclose(flat3, rflat, rtol=1e-5, atol=1e-6))


def _fused_backward_issue_order(check, rank, world):
    """The fused training node's backward (models/train_step._TrainRender.backward) under the two GradSync forms, with the HIP
    launch (ops.mlp_bwd_multi) replaced by a recorder: WHAT is launched and WHEN the collectives are issued relative to it.
      form="per_model": fine chain/dW/reduce -> the fine model's all-reduce is ISSUED -> only then the coarse model's launches;
      form="merged" (default): ONE launch for both models -> ONE all-reduce over the joint buffer."""
    from types import SimpleNamespace

    from nerf_pl_amd import ops
    from nerf_pl_amd.models import NeRF
    from nerf_pl_amd.models import train_step as TS
    real_multi, real_ar = ops.mlp_bwd_multi, dist.all_reduce
    for form in ("per_model", "merged"):
        torch.manual_seed(3)
        coarse, fine = NeRF(), NeRF()
        gs = parallel.GradSync([coarse, fine], form=form)
        for m_ in (coarse, fine):
            m_.images_packed()                              # what the forward this backward belongs to did
        log = []

        def fake_multi(entries, dtype, adam=None, phases=7, workspace=None, g_scale=None):
            log.append(("launch", tuple(e[0] for e in entries)))
            joint = torch.empty(len(entries) * ops.FLAT_GRAD_FLOATS)
            out = []
            for k, e in enumerate(entries):
                fl = joint[k * ops.FLAT_GRAD_FLOATS:(k + 1) * ops.FLAT_GRAD_FLOATS]
                fl.fill_(float(rank + 1) * (1.0 if e[0] == "fine" else 3.0))
                out.append(ops.flat_grad_views(1, "cpu", out=fl))
            return out

        def logging_ar(t, *a_, **kw_):
            log.append(("all_reduce", t.numel()))
            return real_ar(t, *a_, **kw_)
        ops.mlp_bwd_multi, dist.all_reduce = fake_multi, logging_ar
        try:
            ctx = SimpleNamespace(n_params=[24, 24], entries=[("fine", None, None, None), ("coarse", None, None, None)], dtype="bf16",
                                  adam=None, models=[fine, coarse], serials=[fine.pack_serial(), coarse.pack_serial()])
            grads = TS._TrainRender.backward(ctx, torch.ones(()))
            # autograd adopts the returned views as p.grad (parameter order of forward(): coarse, then fine)
            for p_, g_ in zip(coarse.flat_params() + fine.flat_params(), grads[3:]):
                p_.grad = g_
            issued = list(log)
            gs.sync()
        finally:
            ops.mlp_bwd_multi, dist.all_reduce = real_multi, real_ar
        n = ops.FLAT_GRAD_FLOATS
        if form == "per_model":
            check("fused_backward/per_model/launch_and_collective_order",
                  issued == [("launch", ("fine",)), ("all_reduce", n), ("launch", ("coarse",)), ("all_reduce", n)])
            check("fused_backward/per_model/issue_log", gs.issue_log[:2] == [("model", id(fine)), ("model", id(coarse))])
        else:
            check("fused_backward/merged/launch_and_collective_order", issued == [("launch", ("fine", "coarse")), ("all_reduce", 2 * n)])
            check("fused_backward/merged/issue_log", gs.issue_log[:1] == [("joint", 2)])
        check("fused_backward/%s/sync_only_waited" % form, len(log) == len(issued))                # no further collective
        want = (world + 1) / 2.0
        check("fused_backward/%s/fine_averaged" % form, all(torch.allclose(p_.grad, torch.full_like(p_, want)) for p_ in fine.parameters()))
        check("fused_backward/%s/coarse_averaged" % form,
              all(torch.allclose(p_.grad, torch.full_like(p_, 3.0 * want)) for p_ in coarse.parameters()))
        gs.detach()


def _sharded_render(check, rank, world, n_rays):
    g = torch.Generator().manual_seed(7)
    rays = torch.rand(n_rays, 8, generator=g)
    with _patched("all_gather_into_tensor", _counting) as gathers:
        out = parallel.render_sharded(_fake_render, rays)
    ref = _fake_render(rays)
    # every key comes back whole, through ONE collective per image (rgb + depth + opacity packed as the columns of one buffer)
    check("render/every_key_whole", all(torch.equal(out[k], ref[k]) for k in ref))
    check("render/one_gather_per_image", len(gathers) == 1)


def _generic(check, rank, world):
    """generic branch: per-rank grads r+1 -> mean (world+1)/2"""
    m = _Tiny()
    for p in m.parameters():
        p.grad = torch.full_like(p, float(rank + 1))
    parallel.GradSync([m]).sync()
    want = (world + 1) / 2.0
    check("generic/averaged", all(torch.allclose(p.grad, torch.full_like(p, want)) for p in m.parameters()))


def _flat_and_alias(check, rank, world):
    """flat branch: grads are views of one flat buffer (what ops.mlp_bwd hands autograd)"""
    m = _Tiny()
    flat = _base() * (rank + 1)
    _adopt(m, flat)
    grads_ready([m], [flat])                                # (no hook attached yet: records the buffer)
    parallel.GradSync([m]).sync()
    check("flat/averaged_in_place", torch.allclose(flat, _base() * (world + 1) / 2.0))
    # and the parameters' .grad still alias the averaged buffer
    check("flat/grads_still_alias", all(p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for p in m.parameters()))


def _overlap(check, rank, world, m, gs):
    """the fused backward announces a finished flat buffer through the grad-ready hook; the all-reduce is issued THEN (while
    "the rest of backward" still runs) and sync() only waits and averages"""
    want = (world + 1) / 2.0
    flat = _base() * (rank + 1) + 1.0
    check("overlap/hook_attached", grad_hooks([m])[0])
    grads_ready([m], [flat])                                # what models/mlp_autograd._param_grads does (p.grad still None)
    _adopt(m, flat)
    started = gs.started_early
    gs.sync()
    check("overlap/issued_from_hook", started == 1)
    check("overlap/nothing_left_in_flight", not gs._inflight)
    check("overlap/averaged", torch.allclose(flat, _base() * want + 1.0))


def _hooks_off(check, rank, world, m, gs):
    """hooks switched off (two-graph capture): nothing is issued early, sync() does the whole job"""
    want = (world + 1) / 2.0
    gs.hooks_enabled = False
    _clear(m)
    flat = flat_grad(m)
    flat.copy_(_base() * (rank + 1))
    before = gs.started_early
    grads_ready([m], [flat])
    _adopt(m, flat)
    check("hooks_off/issues_nothing", gs.started_early == before == 1)
    gs.sync()
    check("hooks_off/averaged", torch.allclose(flat, _base() * want))
    gs.hooks_enabled = True


def _accumulation(check, rank, world, m, gs):
    """gradient accumulation: p.grad exists when the backward announces its buffer -> autograd ACCUMULATES the
    views into p.grad, so no early collective may touch the buffer; sync() averages the accumulated p.grad"""
    want = (world + 1) / 2.0
    for p in m.parameters():
        p.grad = torch.full_like(p, 10.0 * (rank + 1))
    flat = _base() * (rank + 1)
    before = gs.started_early
    grads_ready([m], [flat])
    _accumulate(m, flat)
    gs.sync()
    check("accumulation/issues_nothing", gs.started_early == before)
    check("accumulation/averaged", torch.allclose(_grads(m), _base() * want + 10.0 * want))


def _two_backwards(check, rank, world, m, gs):
    """two backwards before one sync(): the first buffer is all-reduced early, the second backward accumulates on top of it"""
    want = (world + 1) / 2.0
    _clear(m)
    first = _base() * (rank + 1)
    grads_ready([m], [first])
    _adopt(m, first)
    second = _base() * (rank + 1) * 2.0
    grads_ready([m], [second])                              # waits for + finishes the first collective, issues nothing
    _accumulate(m, second)
    gs.sync()
    check("two_backwards/averaged", torch.allclose(_grads(m), _base() * want * 3.0))


def _copied_views_refused(check, rank, world, m, gs):
    """autograd COPIED the announced views instead of adopting them: refused, never silently un-averaged"""
    _clear(m)
    flat = _base() * (rank + 1)
    grads_ready([m], [flat])
    _adopt(m, flat.clone())
    try:
        gs.sync()
        raised = False
    except RuntimeError:
        raised = True
    check("copied_views/refused", raised)


def _two_models(rank):
    ms, flats = [], []
    for k in range(2):
        m = _Tiny()
        fl = _base() * (rank + 1) * (k + 1)
        _adopt(m, fl)
        grads_ready([m], [fl])
        ms.append(m)
        flats.append(fl)
    gs = parallel.GradSync(ms)
    gs.hooks_enabled = False
    gs._coalesce_backends = ("nccl", "gloo")
    return gs, flats


def _grouped(check, rank, world):
    """round 5: the two-graph step's sync() issues the models' all-reduces as ONE grouped launch (RCCL: ncclGroupStart / End
    through torch's coalescing manager).  Same branch driven over gloo here: one manager entry for both buffers, the values
    of two separate calls; and when the grouped form raises, sync() falls back to one call per model for good."""
    want = (world + 1) / 2.0
    gs, flats = _two_models(rank)
    with _patched("_coalescing_manager", _counting) as entered:
        gs.sync()
    check("grouped/ok/one_manager_entry", len(entered) == 1)
    check("grouped/ok/stays_on", gs._coalesce)
    check("grouped/ok/averaged", all(torch.allclose(f, _base() * want * (k + 1)) for k, f in enumerate(flats)))
    # a stack WITHOUT the grouped form: the only reason to fall back
    gs, flats = _two_models(rank)
    with _patched("_coalescing_manager", _raising(NotImplementedError("no grouped collectives on this stack"))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gs.sync()
    check("grouped/unavailable/switched_off", not gs._coalesce)
    check("grouped/unavailable/averaged", all(torch.allclose(f, _base() * want * (k + 1)) for k, f in enumerate(flats)))
    #  any OTHER error — a communicator error, a failure after a partial enqueue — is re-raised, never papered over by
    # re-issuing the collectives one by one (they could run twice, or mismatch across the ranks): every rank raises alike here
    gs, flats = _two_models(rank)
    with _patched("_coalescing_manager", _raising(RuntimeError("communicator error"))):
        try:
            gs.sync()
            raised = False
        except RuntimeError:
            raised = True
    check("grouped/error/raised", raised)
    check("grouped/error/stays_on", gs._coalesce)
    check("grouped/error/nothing_reissued", all(torch.allclose(f, _base() * (rank + 1) * (k + 1)) for k, f in enumerate(flats)))


def _joint_models(rank, scale):
    ms = [_Tiny(), _Tiny()]
    joint = torch.empty(2 * _N)
    flats = [joint[k * _N:(k + 1) * _N] for k in range(2)]
    for k, fl in enumerate(flats):
        fl.copy_(_base() * (rank + 1) * (k + 1) * scale)
        grads_ready([ms[k]], [fl])
    return ms, flats


def _joint(check, rank, world):
    """round 6: the fused step's backward writes both models' flat buffers as consecutive slices of ONE allocation
    (ops.mlp_bwd_multi) and announces them together; GradSync(form="merged") — the default — issues ONE all-reduce over the
    joint buffer from that hook, and sync() only waits.  With the hooks off (the two-graph fallback) sync() itself sends the
    joint range as one message: no coalescing manager involved."""
    want = (world + 1) / 2.0
    ms, flats = _joint_models(rank, 1.0)
    gs = parallel.GradSync(ms)
    check("joint/hook/merged_is_default", gs.form == "merged")
    check("joint/hook/one_hook_for_all_models", grad_hooks(ms)[1] is not None)
    with _patched("all_reduce", _counting) as sent:
        grads_ready(ms, flats)                              # what models/train_step._TrainRender.backward does (p.grad still None)
        check("joint/hook/one_message_over_joint_range", [t.numel() for t in sent] == [2 * _N])
        check("joint/hook/issue_log", gs.issue_log == [("joint", 2)])
        for m, fl in zip(ms, flats):
            _adopt(m, fl)
        gs.sync()
        check("joint/hook/sync_only_waited", len(sent) == 1)
    check("joint/hook/nothing_left_in_flight", not gs._inflight)
    check("joint/hook/averaged", all(torch.allclose(f, _base() * want * (k + 1)) for k, f in enumerate(flats)))
    # hooks off: sync() sends the joint range itself, as ONE message
    ms, flats = _joint_models(rank, 2.0)
    gs = parallel.GradSync(ms)
    gs.hooks_enabled = False
    gs._coalesce_backends = ("nccl", "gloo")
    with _patched("all_reduce", _counting) as sent, _patched("_coalescing_manager", _counting) as entered:
        grads_ready(ms, flats)
        for m, fl in zip(ms, flats):
            _adopt(m, fl)
        gs.sync()
    check("joint/hooks_off/one_message_over_joint_range", [t.numel() for t in sent] == [2 * _N])
    check("joint/hooks_off/no_coalescing_manager", len(entered) == 0)
    check("joint/hooks_off/averaged", all(torch.allclose(f, _base() * want * (k + 1) * 2.0) for k, f in enumerate(flats)))
    # ... whatever the order the models are listed in: the real backward lays the FINE model's buffer first while NeRFSystem
    # lists the coarse model first (on the GPU: tests/test_gpu_world2.py) — still ONE message over the joint range
    ms, flats = _joint_models(rank, 3.0)
    gs = parallel.GradSync(ms[::-1])
    gs.hooks_enabled = False
    with _patched("all_reduce", _counting) as sent:
        for m, fl in zip(ms, flats):
            _adopt(m, fl)
        gs.sync()
    check("joint/reversed/one_message_over_joint_range", [t.numel() for t in sent] == [2 * _N])
    check("joint/reversed/averaged", all(torch.allclose(f, _base() * want * (k + 1) * 3.0) for k, f in enumerate(flats)))
    # gradient accumulation under the joint hook: nothing is issued early, sync() averages the accumulated p.grad
    ms, flats = _joint_models(rank, 1.0)
    gs = parallel.GradSync(ms)
    for m in ms:
        for p in m.parameters():
            p.grad = torch.full_like(p, 10.0 * (rank + 1))
    with _patched("all_reduce", _counting) as sent:
        grads_ready(ms, flats)
    check("joint/accumulation/issues_nothing", len(sent) == 0)
    for m, fl in zip(ms, flats):
        _accumulate(m, fl)
    gs.sync()
    check("joint/accumulation/averaged",
          all(torch.allclose(_grads(m), _base() * want * (k + 1) + 10.0 * want) for k, m in enumerate(ms)))


def _worker(rank, world, port, n_rays, q):
    """Every scenario runs on every rank, in this order (the same sequence of collectives on both: a rank that skipped one
    would leave its peer waiting in gloo)."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        check = _Checks()
        _sharded_render(check, rank, world, n_rays)
        _generic(check, rank, world)
        _flat_and_alias(check, rank, world)
        m = _Tiny()                                         # one model and one GradSync through the hook scenarios, as a training
        gs = parallel.GradSync([m])                         # loop has: each starts from what the one before left behind
        for scenario in (_overlap, _hooks_off, _accumulation, _two_backwards, _copied_views_refused):
            scenario(check, rank, world, m, gs)
        _grouped(check, rank, world)
        _joint(check, rank, world)
        _fused_backward_issue_order(check, rank, world)
        _graphed_step_host_logic(check, rank, world)
        q.put((rank, check.results))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_rays", [10, 7, 1])      # even split, ragged split, fewer rays than ranks
def test_world2_gloo_sharding_and_gradsync(n_rays):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_rays, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    failed = sorted("rank %d: %s" % (rank, name) for rank, results in res for name, ok in results.items() if not ok)
    print("\n".join(failed))
    assert not failed, failed
    assert all(len(results) == len(res[0][1]) > 40 for _, results in res)      # every rank ran every check


def test_shard_bounds_cover_exactly():
    for n in (0, 1, 7, 8, 640000, 190512):
        for world in (1, 2, 3, 8):
            spans = [parallel.shard_bounds(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            for (a, b), (c, d) in zip(spans, spans[1:]):
                assert b == c and a <= b
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    # BASELINE configs[4]: 800x800 image over 8 GPUs = 80,000 rays each
    assert parallel.shard_bounds(640000, 3, 8) == (240000, 320000)


def test_single_process_passthrough():
    rays = torch.rand(5, 8)
    out = parallel.render_sharded(_fake_render, rays, keys=("rgb_fine",))
    assert torch.equal(out["rgb_fine"], _fake_render(rays)["rgb_fine"])
    parallel.GradSync([_Tiny()]).sync()     # no process group: no-op


def test_graphed_step_batch_source_host_logic():
    """GraphedTrainStep(batch_source=...): the source is called inside every eager step and inside every replay (i.e. inside
    the captured region), never at capture time, and mixing it with an explicit batch is refused."""
    from nerf_pl_amd.system import GraphedTrainStep
    sysm = _TinySystem()
    opt = torch.optim.SGD(sysm.parameters(), lr=0.1)
    g = torch.Generator().manual_seed(3)
    calls = []

    def source():
        calls.append(len(calls))
        return {"x": torch.randn(16, 5, generator=g), "y": torch.randn(16, 3, generator=g)}
    be = _RecordingBackend()
    stepper = GraphedTrainStep(sysm, opt, warmup=2, backend=be, batch_source=source)
    before = torch.cat([p.detach().reshape(-1).clone() for p in sysm.parameters()])
    for _ in range(5):
        stepper()
    assert be.captures == 1 and stepper.graph.replays == 3
    assert len(calls) == 5                                  # 2 eager + 3 replays; the capture itself ran nothing
    after = torch.cat([p.detach().reshape(-1) for p in sysm.parameters()])
    assert not torch.equal(before, after)
    with pytest.raises(ValueError):
        stepper({"x": torch.zeros(16, 5), "y": torch.zeros(16, 3)})
    with pytest.raises(ValueError):
        GraphedTrainStep(sysm, opt, warmup=2, backend=_RecordingBackend())()


def _torchrun(nproc, script_args, timeout=180):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "tests", "host", "bench_rank_logic.py")] + script_args
    return subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout, cwd=root)


def test_bench_rank_logic_world2_gloo_end_to_end():
    """bench.py's own launch-contract functions under the launcher the driver uses (torch.distributed.run, 2 processes, gloo):
    init_world sees a 2-rank communicator, timed_region reports the SLOWER rank's time (rank 1 sleeps twice as long), the
    sharded image equals the unsharded one, and exactly one JSON line comes out (rank 0's)."""
    import json
    r = _torchrun(2, ["2"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_nranks"] == 2 and d["sharded_equal"] and d["span"] == [0, 501]
    assert 5 * 0.04 * 0.95 <= d["dt"] <= 5 * 0.04 * 3, d["dt"]          # 5 steps of rank 1's 40 ms, not rank 0's 20 ms


def test_bench_rank_logic_refuses_a_world_that_is_not_gpus():
    """2 processes launched, --gpus 4 requested: every rank exits 2 before any group is formed, no line."""
    r = _torchrun(2, ["4"])
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert "WORLD_SIZE=2 but --gpus 4" in r.stderr

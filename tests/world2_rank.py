"""The program ONE rank of the world-2 tests runs (not a test module; started by tests/world2_launch.py):

    python tests/world2_rank.py RANK WORLD RENDEZVOUS_FILE OUT SCENARIO[,SCENARIO...] [--timeout SECONDS]

Both ranks sit on the same device (cuda:0) and talk over gloo with a file rendezvous (no `device_id`: RCCL refuses two ranks on
one device; no TCP store).  The scenarios run in order; the named tensors of each are saved, on the CPU, to OUT.rank<r>.pt.  On
any Python exception the rank saves what it has plus the traceback and exits 1: no retry, nothing after a failed scenario.

The model, the batches and the read-out helpers below are also what the parent test uses for its single-process references
(tests/test_gpu_world2.py), so both sides compute on the same inputs by construction."""
import argparse
import datetime
import os
import sys
import traceback
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

N_RAYS, S_COARSE, S_FINE = 128, 64, 64          # the smallest shape of the fused-step tests
STEPS = 6                                        # trajectory length
SHARD_RAYS, SHARD_SEED = 1001, 77                # sharded inference: 501 / 500 rays
GRAD_CASES = [(form, overlap) for form in ("merged", "per_model") for overlap in (True, False)]
TRAJ_FORMS = ("eager", "graphed", "graphed_bf16_fuse", "graphed_bf16_fuse_nohook")
MODEL_NAMES = ("coarse", "fine")


def grad_case_name(form, overlap):
    return "grad_%s_%s" % (form, "overlap" if overlap else "nooverlap")


# ---- shared with the parent ---------------------------------------------------------------------------------------------------
def make_system(dev, dtype="fp32", **hp_extra):
    """NeRFSystem with the seeded weights of the world-1 tests; perturb = 0, noise_std = 0: no RNG in the math"""
    from nerf_pl_amd.system import NeRFSystem
    from oracle import nerf_oracle as O
    hp = dict(N_samples=S_COARSE, N_importance=S_FINE, use_disp=False, perturb=0.0, noise_std=0.0, chunk=1024 * 32, loss_type="mse",
              lr=5e-4, weight_decay=0, decay_step=[100], decay_gamma=0.5, white_back=True)
    hp.update(hp_extra)
    system = NeRFSystem(Namespace(**hp))
    system.nerf_coarse.load_state_dict(O.make_params(5, 4.0, 0.2))
    system.nerf_fine.load_state_dict(O.make_params(6, 4.0, 0.2))
    for m in system.models:
        m.mlp_dtype = dtype
    return system.to(dev)


def make_batch(rank, i, dev):
    """batch `i` of rank `rank` (i < 7: the seeds of the two ranks do not meet)"""
    from oracle import nerf_oracle as O
    seed = 10 + 7 * rank + i
    return {"rays": O.make_rays(seed, N_RAYS, "blender").to(dev),
            "rgbs": torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(1000 + seed)).to(dev)}


def shard_rays(dev):
    from oracle import nerf_oracle as O
    return O.make_rays(SHARD_SEED, SHARD_RAYS, "blender").to(dev)


def render_fn(system, host=False):
    from nerf_pl_amd.inference import batched_inference

    def render(rays):
        out = batched_inference(system.models, system.embeddings, rays, S_COARSE, S_FINE, False, 1024 * 32, True)
        return {k: v.cpu() for k, v in out.items()} if host else out
    return render


def flat_grads(system):
    """{model name: its 24 gradients in flat_params() order, one CPU vector}"""
    torch.cuda.synchronize()
    return {n: torch.cat([p.grad.detach().reshape(-1) for p in m.flat_params()]).cpu() for n, m in zip(MODEL_NAMES, system.models)}


def named_grads(system):
    torch.cuda.synchronize()
    return torch.cat([p.grad.detach().reshape(-1) for _, p in system.named_parameters()]).cpu()


def train_state(system, opt):
    """parameters as the modules see them + FlatAdam's moments and step counter"""
    torch.cuda.synchronize()
    out = {"step": float(opt.dev_state[0])}
    for i, (n, m) in enumerate(zip(MODEL_NAMES, system.models)):
        out["param_" + n] = torch.cat([p.detach().reshape(-1) for p in m.flat_params()]).cpu()
        out["exp_avg_" + n] = opt.exp_avg[i].detach().cpu().clone()
        out["exp_avg_sq_" + n] = opt.exp_avg_sq[i].detach().cpu().clone()
    return out


# ---- scenarios ----------------------------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self.dev = torch.device("cuda:0")


def sc_cpu_allreduce(ctx):
    t = torch.arange(8, dtype=torch.float32) * (ctx.rank + 1)
    dist.all_reduce(t)
    return {"sum": t}


def sc_cpu_raise_rank1(ctx):
    if ctx.rank == 1:
        raise RuntimeError("world2_rank: rank 1 fails here, before any collective")
    t = torch.ones(4)
    dist.all_reduce(t)                   # rank 0 waits for a peer that is gone
    return {"sum": t}


def sc_agree(ctx):
    from nerf_pl_amd.parallel import GradSync
    sync = GradSync(make_system(ctx.dev).models, overlap=False)
    return {"one_rank_true": bool(sync.agree_any(ctx.rank == 1)), "all_false": bool(sync.agree_any(False))}


def _grad_case(form, overlap):
    def run(ctx):
        from nerf_pl_amd.models.mlp_autograd import flat_grad
        from nerf_pl_amd.parallel import GradSync
        system = make_system(ctx.dev)
        (opt,), _ = system.configure_optimizers()
        sync = GradSync(system.models, form=form, overlap=overlap)
        names = {id(m): n for n, m in zip(MODEL_NAMES, system.models)}
        out = system.training_step(make_batch(ctx.rank, 0, ctx.dev), 0)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()
        log = [[kind, names[what] if kind == "model" else str(what)] for kind, what in sync.issue_log]
        started = sync.started_early
        sync.sync()
        res = flat_grads(system)
        res.update(issue_log=log, started_early=started, loss=float(out["loss"]),
                   adopted=all(flat_grad(m) is not None and GradSync._aliases(list(m.parameters()), flat_grad(m)) for m in system.models))
        sync.detach()
        return res
    return run


def sc_accum(ctx):
    """two backwards on two batches before ONE sync(): the hook's "p.grad is not None" branch"""
    from nerf_pl_amd.parallel import GradSync
    system = make_system(ctx.dev)
    (opt,), _ = system.configure_optimizers()
    sync = GradSync(system.models, form="merged")
    opt.zero_grad(set_to_none=True)
    for i in range(2):
        system.training_step(make_batch(ctx.rank, i, ctx.dev), i)["loss"].backward()
    started = sync.started_early
    sync.sync()
    res = flat_grads(system)
    res["started_early"] = started
    sync.detach()
    return res


def _trajectory(form):
    def run(ctx):
        from nerf_pl_amd.parallel import GradSync
        from nerf_pl_amd.system import GraphedTrainStep, fit
        bf16 = form.startswith("graphed_bf16")
        system = make_system(ctx.dev, "bf16" if bf16 else "fp32")
        system.fuse_adam = bf16
        sync = GradSync(system.models, overlap=not form.endswith("nohook"))
        batches = [make_batch(ctx.rank, i, ctx.dev) for i in range(STEPS)]
        sent, real = [], dist.all_reduce

        def logging_all_reduce(t, *a, **kw):
            sent.append(int(t.numel()))
            return real(t, *a, **kw)
        dist.all_reduce = logging_all_reduce
        try:
            if form == "eager":
                losses = [float(x) for x in fit(system, batches, grad_sync=sync)]
                opt = system.optimizer
                res = {}
            else:
                (opt,), _ = system.configure_optimizers()
                stepper = GraphedTrainStep(system, opt, grad_sync=sync, warmup=2, sync_in_graph=False)
                losses = []
                for b in batches:
                    del sent[:]
                    losses.append(float(stepper(b)["loss"]))
                res = {"graph": stepper.graph is not None, "graph_opt": stepper.graph_opt is not None,
                       "hooks_enabled": bool(sync.hooks_enabled), "capture_fallback": str(stepper.capture_fallback),
                       "last_step_all_reduce_numels": list(sent)}
        finally:
            dist.all_reduce = real
        res.update(train_state(system, opt))
        res["losses"] = losses
        res["optimizer"] = type(opt).__name__
        sync.detach()
        return res
    return run


def sc_ddp(ctx):
    """stock DistributedDataParallel around NeRFSystem, two backwards with set_to_none between them"""
    system = make_system(ctx.dev, flat_optimizer=False)
    ddp = torch.nn.parallel.DistributedDataParallel(system, device_ids=[0])
    for i in range(2):
        b = make_batch(ctx.rank, i, ctx.dev)
        system.zero_grad(set_to_none=True)
        system.loss(ddp(b["rays"]), b["rgbs"]).backward()
    res = {"grad": named_grads(system)}
    del ddp
    return res


def sc_shard(ctx):
    """parallel.render_sharded over 1001 rays (501 / 500); if gloo refuses the device tensor in all_gather_into_tensor (a Python
    exception) both ranks agree on it and the render_fn returns CPU tensors instead: pack and gather then run on the host"""
    from nerf_pl_amd import parallel
    system = make_system(ctx.dev)
    rays = shard_rays(ctx.dev)
    err, full = "", None
    try:
        with torch.no_grad():
            full = parallel.render_sharded(render_fn(system), rays)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        err = repr(e)
    flag = torch.tensor([1 if err else 0], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    host = bool(int(flag))
    with torch.no_grad():
        if host:
            full = parallel.render_sharded(render_fn(system, host=True), rays)
        one = parallel.render_sharded(render_fn(system, host=host), rays, keys=("rgb_fine",))
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in full.items()}
    res.update(one_key_names=sorted(one), one_key_rgb_fine=one["rgb_fine"].cpu(), host_gather=host, gather_error=err)
    return res


SCENARIOS = {"cpu_allreduce": sc_cpu_allreduce, "cpu_raise_rank1": sc_cpu_raise_rank1, "agree": sc_agree, "accum": sc_accum,
             "ddp": sc_ddp, "shard": sc_shard}
SCENARIOS.update({grad_case_name(f, o): _grad_case(f, o) for f, o in GRAD_CASES})
SCENARIOS.update({"traj_" + f: _trajectory(f) for f in TRAJ_FORMS})
GPU_SCENARIOS = (["agree"] + [grad_case_name(f, o) for f, o in GRAD_CASES] + ["accum"] + ["traj_" + f for f in TRAJ_FORMS]
                 + ["ddp", "shard"])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("rank", type=int)
    ap.add_argument("world", type=int)
    ap.add_argument("rendezvous")
    ap.add_argument("out")
    ap.add_argument("scenarios")
    ap.add_argument("--timeout", type=float, default=120.0, help="gloo collective timeout, seconds")
    a = ap.parse_args(argv)
    out = "%s.rank%d" % (a.out, a.rank)
    with open(out + ".pid", "w") as f:
        f.write(str(os.getpid()))
    # a rank ended at its time limit (SIGTERM from `timeout`) leaves the stack it was waiting in, then dies as it would have
    import faulthandler
    import signal
    faulthandler.register(signal.SIGTERM, all_threads=True, chain=True)
    names = [s for s in a.scenarios.split(",") if s]
    results = {}
    try:
        unknown = [s for s in names if s not in SCENARIOS]
        if unknown:
            raise ValueError("unknown scenarios %r" % (unknown,))
        if any(not s.startswith("cpu_") for s in names):
            torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method="file://" + os.path.abspath(a.rendezvous), rank=a.rank, world_size=a.world,
                                timeout=datetime.timedelta(seconds=a.timeout))
        ctx = Ctx(a.rank, a.world)
        for s in names:
            results["failed_in"] = s
            results[s] = SCENARIOS[s](ctx)
            print("rank %d: %s done" % (a.rank, s), flush=True)
        del results["failed_in"]
    except BaseException:  # noqa: BLE001 - whatever it was: leave the evidence and stop
        results["traceback"] = traceback.format_exc()
        sys.stderr.write("rank %d failed in %r\n%s" % (a.rank, results.get("failed_in"), results["traceback"]))
        sys.stderr.flush()
        try:
            torch.save(results, out + ".pt")
        finally:
            os._exit(1)                  # not through the process group's teardown, which may wait for the peer
    torch.save(results, out + ".pt")
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Multi-GPU plumbing for the hot path: one process per GPU (`torch.distributed`, backend "nccl" = RCCL
over xGMI on ROCm; "gloo" in the CPU tests).

* Rays are independent units: inference shards the ray list contiguously across ranks with no
  collective on the data path and one gather of the finished pixels (eval.py:58-86 sharded).
* Training is the reference's DDP (train.py:174-175): replicated models, each rank draws its own
  batch, gradients are averaged.  Each model's 24 gradients live in ONE flat fp32 buffer written by
  the dW-reduce kernel (2.38 MB), and the fused step's backward writes both models' buffers as consecutive
  slices of one allocation: a step needs exactly ONE all-reduce (4.77 MB) — a message that on the 8-GPU xGMI
  mesh is latency-bound.  `GradSync(form="merged")` (the default) keeps the one-rank step's launches (one chain, one dW,
  one reduce launch for both models) and issues that all-reduce from the backward's grads-ready hook;
  `form="per_model"` runs the two models' backwards one after the other and issues the fine model's all-reduce while the
  coarse model's backward is still running (autograd runs the fine model first; `GradSync._on_grad_ready`) — what DDP's
  bucket hooks give the reference, at the price of un-merging the launches (7.6 % of the step at world 1).
"""
import contextlib
import warnings

import torch
import torch.distributed as dist

from .models.mlp_autograd import clear_grad_hooks, flat_grad, set_grad_hooks


def shard_bounds(n, rank, world):
    """Contiguous [lo, hi) of `n` rays owned by `rank` (sizes differ by at most 1)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def render_sharded(render_fn, rays, keys=("rgb_fine", "depth_fine", "opacity_fine"), group=None):
    """Ray-sharded full-image inference: every rank renders its contiguous slice with
    `render_fn(rays_slice) -> dict`, then the requested keys are all-gathered (padded to equal length)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    n = rays.shape[0]
    lo, hi = shard_bounds(n, rank, world)
    local = render_fn(rays[lo:hi])
    if world == 1:
        return {k: local[k] for k in keys if k in local}
    # ONE collective per image: the requested keys travel as the columns of one (maxlen, C) buffer (rgb 3 + depth 1 + opacity 1
    # = 5 floats per ray; at 8 ranks the 0.96 MB gather is latency-bound, so the count of collectives is what matters)
    have = [k for k in keys if k in local]
    if not have:
        return {}
    cols = [int(torch.Size(local[k].shape[1:]).numel()) for k in have]          # (rows, ...) -> columns per row (1 for a vector)
    maxlen = shard_bounds(n, 0, world)[1]
    v0 = local[have[0]]
    pack = torch.zeros(maxlen, sum(cols), dtype=v0.dtype, device=v0.device)
    c = 0
    for k, w in zip(have, cols):
        pack[: hi - lo, c:c + w] = local[k].reshape(hi - lo, w)
        c += w
    gathered = torch.empty(world * maxlen, sum(cols), dtype=v0.dtype, device=v0.device)
    dist.all_gather_into_tensor(gathered, pack, group=group)
    rows = torch.cat([gathered[r * maxlen: r * maxlen + (shard_bounds(n, r, world)[1] - shard_bounds(n, r, world)[0])]
                      for r in range(world)], 0)
    out, c = {}, 0
    for k, w in zip(have, cols):
        col = rows[:, c:c + w]
        out[k] = col.reshape((n,) + tuple(local[k].shape[1:])) if local[k].dim() > 1 else col.reshape(n)
        c += w
    return out


class _InFlight:
    """One all-reduce a backward hook issued and sync() has not settled yet."""
    __slots__ = ("work", "buffer", "needs_division", "owners", "done")

    def __init__(self, work, buffer, needs_division, owners):
        self.work = work                        # the async handle
        self.buffer = buffer                    # the tensor the all-reduce rewrites: one model's flat buffer, or the joint range
        self.needs_division = needs_division
        self.owners = owners                    # [(model, flat)]: one pair per model whose gradients `buffer` holds
        self.done = False                       # waited for and divided: `buffer` holds the rank average


class GradSync:
    """Average gradients across ranks (the reference's DDP, train.py:174-175): one all-reduce per model on the flat
    gradient buffer the dW-reduce kernel wrote (2.38 MB), else a flatten/all-reduce/unflatten of the parameter grads.

    Overlap with backward (what DDP's bucket hooks give the reference): `attach()` registers a grad-ready hook on each
    model; the fused MLP backward calls it the moment the model's flat gradient buffer is complete
    (models/mlp_autograd.py:_param_grads), and the hook issues that model's all-reduce asynchronously on the
    communicator's stream.  Autograd runs the fine model's backward first, so its all-reduce travels over xGMI while
    compositing / importance sampling / the coarse model's backward still execute; `sync()` then waits for whatever
    was started, launches whatever was not, and divides by the world size."""

    def __init__(self, models, group=None, force=False, overlap=True, form=None):
        self.models = list(models)
        self.group = group
        self.force = force          # run the collectives even at world size 1 (tests the RCCL path on one GPU)
        self.overlap = overlap
        # form of the fused step's backward under this sync: "merged" (also None) = the one-rank launches + ONE all-reduce of the
        # step's joint gradient buffer; "per_model" = per model chain -> dW -> reduce -> all-reduce (the fine model's travels under
        # the coarse model's backward; tools/launch_scale.sh measures both).
        self.form = form if form is not None else "merged"
        if self.form not in ("merged", "per_model"):
            raise ValueError("GradSync form must be 'merged' or 'per_model', got %r" % (self.form,))
        self.issue_log = []         # ("model", id(model)) / ("joint", n_models) per hook-issued collective since the last sync() (tests)
        self.hooks_enabled = True   # GraphedTrainStep switches the hooks off while it captures/replays a graph that
                                    # must not contain the collective (two-graph mode)
        self._inflight = []         # the _InFlight records of the all-reduces issued from the hooks since the last sync()
        self.started_early = 0      # statistics: all-reduces issued from the hook (tests assert on it)
        self._coalesce = True       # the per-model all-reduces of sync() as one grouped RCCL launch
        self._coalesce_backends = ("nccl",)     # (the gloo CPU test adds "gloo" to drive the same branch)
        if overlap:
            self.attach()

    # -- plumbing ---------------------------------------------------------------------------------------------------
    def active(self):
        return dist.is_initialized() and (dist.get_world_size(self.group) > 1 or self.force)

    def attach(self):
        for m in self.models:
            set_grad_hooks(m, self._on_grad_ready, self._on_grads_ready if self.form == "merged" else None)

    def detach(self):
        for m in self.models:
            clear_grad_hooks(m, self._on_grad_ready, self._on_grads_ready)

    def agree_any(self, flag):
        """True on every rank if `flag` is true on any (one small eager MAX all-reduce): ranks that must take the same branch —
        e.g. GraphedTrainStep falling back to two graphs when the one-graph capture failed somewhere — decide it here."""
        if not self.active():
            return bool(flag)
        dev = next(self.models[0].parameters()).device
        t = torch.tensor([1 if flag else 0], device=dev, dtype=torch.int32)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return bool(int(t.item()))

    def _avg_op(self):
        """(reduce op, needs_division): RCCL averages in the collective itself; gloo (CPU tests) has no AVG."""
        backend = dist.get_backend(self.group)
        if backend == "nccl" and hasattr(dist.ReduceOp, "AVG"):
            return dist.ReduceOp.AVG, False
        return dist.ReduceOp.SUM, True

    @staticmethod
    def joint_of(flats):
        """The ONE tensor whose consecutive slices `flats` are (ops.mlp_bwd_multi allocates a step's flat gradient buffers that
        way), or None."""
        base = getattr(flats[0], "_base", None)
        if base is None or any(getattr(f, "_base", None) is not base for f in flats) or not base.is_contiguous():
            return None
        off = flats[0].storage_offset()
        for f in flats:
            if f.storage_offset() != off or not f.is_contiguous():
                return None
            off += f.numel()
        lo = flats[0].storage_offset() - base.storage_offset()
        return base.reshape(-1)[lo:lo + sum(f.numel() for f in flats)]

    # -- the backward's hooks ---------------------------------------------------------------------------------------
    def _on_grad_ready(self, model, flat):
        """form="per_model" (and the modular backward): called when `flat` (the model's 24 gradients) is complete.  The one-model
        case of `_on_grads_ready`, always that model's own all-reduce."""
        self._on_grads_ready([model], [flat], joint=False)

    def _on_grads_ready(self, models, flats, joint=True):
        """Called by the fused backward when the flat gradient buffers `flats` of `models` are complete (form="merged": ONCE, for
        ALL its models — one reduce launch wrote them), BEFORE autograd hands the views to the parameters.  Issues ONE all-reduce
        over the joint buffer (`joint`), else one per model, asynchronously on the communicator's stream.  The all-reduce is started
        here only when autograd is going to adopt the views as `p.grad` (every `p.grad` is None: zero_grad(set_to_none=True), no
        accumulation): otherwise autograd would accumulate the views into existing `.grad` tensors on the compute stream while the
        collective rewrites the buffer on the communicator's."""
        if not (self.hooks_enabled and self.overlap and self.active()):
            return
        # a second backward before sync(): its accumulation into p.grad (views of the first buffer) must be ordered after
        # the collective that is still rewriting that buffer — finish (wait, divide) what is in flight for these models
        self._finish(r for r in self._inflight if any(m is o for o, _ in r.owners for m in models))
        if any(p.grad is not None for m in models for p in m.parameters()):
            return                                     # gradient accumulation: sync() reduces the accumulated p.grad
        whole = self.joint_of(flats) if joint else None
        op, div = self._avg_op()
        if whole is not None:
            sends = [(whole, list(zip(models, flats)))]
            self.issue_log.append(("joint", len(models)))
        else:                                          # per model, or not one allocation (an older caller): one collective per model
            sends = [(f, [(m, f)]) for m, f in zip(models, flats)]
            self.issue_log.extend(("model", id(m)) for m in models)
        for buf, owners in sends:
            work = dist.all_reduce(buf, op=op, group=self.group, async_op=True)
            self._inflight.append(_InFlight(work, buf, div, owners))
            self.started_early += 1

    def _finish(self, records):
        """wait for hook-issued collectives and apply their division: afterwards each buffer holds the rank average"""
        for r in records:
            if not r.done:
                r.work.wait()
                if r.needs_division:
                    r.buffer.div_(dist.get_world_size(self.group))
                r.done = True

    def reset(self):
        """Drop the hook-issued collectives WITHOUT waiting for them: an aborted graph capture recorded them, nothing launched."""
        self._inflight.clear()

    @staticmethod
    def _aliases(params, flat):
        """autograd adopted the views of `flat` as the parameters' .grad (first and last parameter checked)"""
        sp = flat.untyped_storage().data_ptr()
        return (params[0].grad.untyped_storage().data_ptr() == sp and params[-1].grad.untyped_storage().data_ptr() == sp)

    # -- the step-level call ----------------------------------------------------------------------------------------
    def sync(self):
        """Leave the rank average in every model's p.grad.  A wait is (work or None, buffer, needs_division, params to copy the
        buffer back into or None)."""
        if not self.active():
            self.reset()
            return
        del self.issue_log[:-64]                        # (a diagnostic: keep the tail)
        op, div = self._avg_op()
        waits, covered, issued_early = self._settle_hook_issued()
        direct = []
        for m in self.models:
            if id(m) in covered:
                continue
            flat = flat_grad(m)
            params = [p for p in m.parameters() if p.grad is not None]
            if flat is not None and params and self._aliases(params, flat) and id(m) not in issued_early:
                direct.append(flat)                                      # issued below, together
            elif params:
                buf = torch.cat([p.grad.reshape(-1) for p in params])
                waits.append((dist.all_reduce(buf, op=op, group=self.group, async_op=True), buf, div, params))
        waits += self._send_direct(direct, op, div)
        world = dist.get_world_size(self.group)
        for work, buf, needs_division, params in waits:
            if work is not None:
                work.wait()
            if needs_division:
                buf.div_(world)
            off = 0
            for p in params or ():
                n = p.grad.numel()
                p.grad.copy_(buf[off:off + n].view_as(p.grad))
                off += n

    def _is_step_gradient(self, rec, records):
        """The hook-issued collective IS the step's gradient: still running, and each of its buffers is exactly what autograd
        adopted as p.grad of a model of ours that nothing else was issued for."""
        if rec.done or any(m is o for r in records if r is not rec for o, _ in r.owners for m, _ in rec.owners):
            return False
        for m, flat in rec.owners:
            params = [p for p in m.parameters() if p.grad is not None]
            if not (any(m is x for x in self.models) and params and flat_grad(m) is flat
                    and self._aliases(params, flat)):
                return False
        return True

    def _settle_hook_issued(self):
        """-> (waits for the collectives that are the step's gradient, ids of the models those cover, ids of the models named by
        the others).  The others' buffers are not simply p.grad (a later backward accumulated on top): finish them and let sync()
        reduce p.grad.  If p.grad still views that buffer, averaging again is exact — the averaged part is identical on every
        rank; if autograd COPIED the views instead of adopting them, the copy raced with the collective and p.grad is undefined:
        refuse."""
        records, self._inflight = self._inflight, []
        mine = [r for r in records if self._is_step_gradient(r, records)]
        rest = [r for r in records if not any(r is x for x in mine)]
        self._finish(rest)
        for m, flat in (o for r in rest for o in r.owners):
            params = [p for x in self.models if x is m for p in m.parameters() if p.grad is not None]
            if params and not self._aliases(params, flat):
                raise RuntimeError("GradSync: the gradient buffer all-reduced from the backward's hook was not adopted as "
                                   "p.grad (autograd copied it while the collective was in flight); construct "
                                   "GradSync(overlap=False) for this training loop")
        waits = [(r.work, r.buffer, r.needs_division, None) for r in mine]
        covered = {id(m) for r in mine for m, _ in r.owners}
        issued_early = {id(m) for r in rest for m, _ in r.owners}
        return waits, covered, issued_early

    def _send_direct(self, direct, op, div):
        """The flat buffers that are reduced as they are (the two-graph step: nothing was started from the hooks) -> waits.  The
        fused step's backward wrote them as consecutive slices of one allocation: ONE all-reduce over that range.  Buffers that
        are not adjacent (a modular-graph step) go over RCCL as ONE grouped launch (ncclGroupStart / End around the per-model
        all-reduces: same values — each buffer is still its own all-reduce), elsewhere (gloo: the CPU tests) one call each."""
        # (in the order of their storage, not of `self.models`: the backward lays the fine model's buffer first, the system lists the
        # coarse model first — taken in the models' order the slices never looked consecutive and each went as its own message)
        joint = self.joint_of(sorted(direct, key=lambda f: f.storage_offset())) if len(direct) > 1 else None
        if joint is not None:
            return [(dist.all_reduce(joint, op=op, group=self.group, async_op=True), joint, div, None)]
        if (len(direct) > 1 and self._coalesce and dist.get_backend(self.group) in self._coalesce_backends
                and hasattr(dist, "_coalescing_manager")):
            grouped = self._send_grouped(direct, op)
            if grouped is not None:                     # one handle for the launch, then each buffer's division
                return [(grouped, direct[0], False, None)] + [(None, flat, div, None) for flat in direct]
        return [(dist.all_reduce(flat, op=op, group=self.group, async_op=True), flat, div, None) for flat in direct]

    def _send_grouped(self, direct, op):
        """-> the handle of ONE grouped launch of the all-reduces of `direct`, or None where the stack has no grouped form."""
        # Only a stack WITHOUT the grouped form is a reason to fall back, and only before anything can have launched: the manager
        # launches on exit, so an error from inside the block or from the exit (a communicator error, a partial enqueue) propagates —
        # re-issuing after it would double or mismatch collectives across the ranks.
        with contextlib.ExitStack() as stack:
            try:
                grouped = stack.enter_context(dist._coalescing_manager(group=self.group, async_ops=True))
            except (AttributeError, TypeError, NotImplementedError) as e:
                warnings.warn("GradSync: grouped all-reduce unavailable on this stack (%r); one call per model from now on" % (e,))
                self._coalesce = False
                return None
            for flat in direct:
                dist.all_reduce(flat, op=op, group=self.group)
        return grouped

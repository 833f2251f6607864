"""Adam over flat parameter storage ("fused Adam for the 48 small tensors").

The reference builds `torch.optim.Adam(lr, eps=1e-8, weight_decay)` over every parameter of both models
(utils/__init__.py:10-30): 48 tensors, 1.19 M floats.  Here each model's 24 tensors become views of ONE flat fp32
buffer (in the order of `NeRF.flat_params()`, which is also the order of the flat gradient buffer the dW-reduce kernel
writes), and the update of all models is ONE hand-written HIP launch (`nerfhip_adam_step`, csrc/optim.hip) whose
`.grad` inputs are adopted from the HIP backward without a copy.  The step counter lives on the device, so a whole
training step replays as a hipGraph.

`state_dict()` / `load_state_dict()` speak the PER-PARAMETER layout of `torch.optim.Adam` over
`[p for m in models for p in m.parameters()]` (48 entries: `step`, `exp_avg`, `exp_avg_sq`), i.e. what the reference's
optimizer — and a Lightning checkpoint's `optimizer_states` (train.py `resume_from_checkpoint`) — holds, so optimizer
state moves between this class and the reference's Adam in both directions.

`FlatRAdam` and `FlatRanger` are the reference's `--optimizer radam|ranger` (utils/optimizers.py:6-95 and :266-405, built by
utils/__init__.py:21-26) over the same flat storage: one launch of `nerfhip_radam_step` / `nerfhip_ranger_step` per step, the
same device-resident step counter — the rectification term depends on the step number, which under graph replay exists only on
the device — and the per-parameter `state_dict()` layout of the reference's classes.  `_FlatOptimizer` holds what the three share.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .models.mlp_autograd import flat_grad, flat_grad_reset
from .models.nerf import NeRF


class _FlatOptimizer(torch.optim.Optimizer):
    """Flat parameter storage, gradient adoption, the shared device-resident step counter and the weights serial.

    Must be built AFTER the models' final device placement: `.to()/.cuda()/.float()` re-create parameter storage
    and break the aliasing with the flat buffers (`step()` verifies the aliasing and re-aliases or raises)."""

    def __init__(self, models, defaults):
        self.models = list(models)
        self.flats = []
        for m in self.models:
            self.flats.append(torch.nn.Parameter(self._flatten(m), requires_grad=True))
            # this optimizer announces every update (NeRF.weights_changed): weight images packed AHEAD of a step
            # (RayStore.sample(pack_models=...)) may be trusted while the serial stands — and only while THIS optimizer is alive.
            # (A module that is not a NeRF — anything with flat_params() can be stepped — packs no images: nothing to announce.)
            if isinstance(m, NeRF):
                m.announced_by(self)
        super().__init__(self.flats, defaults)
        dev = self.flats[0].device
        if not self.flats[0].is_cuda:
            raise _lib.NerfHipError("%s runs on MI355X only (no CPU fallback); use %s on CPU tensors" % (self._name, self._elsewhere))
        self.exp_avg = [torch.zeros_like(f.data) for f in self.flats]
        self.exp_avg_sq = [torch.zeros_like(f.data) for f in self.flats]
        # [step count (float), arrival ticket (uint32 bits)] — device-resident: graph replays advance the counter
        self.dev_state = torch.zeros(2, device=dev, dtype=torch.float32)
        self._tables = None
        self._stepped = None          # indices of the models the first step updated (must stay the same: one shared step counter)

    _elsewhere = "a per-tensor optimizer"     # what the error texts point to for CPU tensors / partially frozen training

    @property
    def _name(self):
        return type(self).__name__

    @staticmethod
    def _require(ok, what, value):
        if not ok:
            raise ValueError("%s out of range: %r" % (what, value))

    # ---------------------------------------------------------------------------------------------- flat storage
    @staticmethod
    def _flatten(model):
        ps = model.flat_params()
        flat = torch.empty(sum(p.numel() for p in ps), device=ps[0].device, dtype=torch.float32)
        off = 0
        for p in ps:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view(p.shape)          # the module's parameters now alias the flat buffer
            off += n
        return flat

    def _check_alias(self):
        """Every module parameter must still be a view of its slice of the flat buffer (a later model.to()/.float()/
        p.data assignment silently breaks this: the optimizer would update the flat buffer while the kernels read the detached
        module parameters).  Re-alias when the detached parameters still have the right shape/device, else raise."""
        for m, flat in zip(self.models, self.flats):
            off = 0
            base = flat.data_ptr()
            broken = False
            for p in m.flat_params():
                if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                    broken = True
                off += p.numel()
            if not broken:
                continue
            ps = m.flat_params()
            if any(p.device != flat.device for p in ps):
                raise _lib.NerfHipError("%s: model parameters moved to another device after the optimizer was built; "
                                        "rebuild the optimizer after the final .to()/.cuda()" % self._name)
            off = 0
            with torch.no_grad():
                for p in ps:                                   # adopt the detached values, then alias again
                    n = p.numel()
                    flat.data[off:off + n].copy_(p.data.reshape(-1).float())
                    p.data = flat.data[off:off + n].view(p.shape)
                    off += n
            self._tables = None

    def _gather_grads(self):
        for m, flat in zip(self.models, self.flats):
            ps = m.flat_params()
            fg = flat_grad(m)
            g0, g1 = ps[0].grad, ps[-1].grad
            if (fg is not None and g0 is not None and g1 is not None and g0.data_ptr() == fg.data_ptr()
                    and g1.data_ptr() + g1.numel() * 4 == fg.data_ptr() + fg.numel() * 4):
                flat.grad = fg                                    # written in place by mlp_bwd_reduce: no copy
                # (first and last parameter's .grad alias the two ends of the flat buffer => autograd adopted the views)
            elif any(p.grad is not None for p in ps):
                g = torch.zeros_like(flat)
                off = 0
                for p in ps:
                    n = p.numel()
                    if p.grad is not None:
                        g[off:off + n].copy_(p.grad.reshape(-1))
                    off += n
                flat.grad = g
            else:
                flat.grad = None

    # ---------------------------------------------------------------------------------------------- the update
    def _begin_step(self):
        """Everything of a step before the launch: aliasing, gradients, the same-models guard, the weights serial.  Returns the
        indices of the models to update (empty: no gradients, nothing to do)."""
        self._check_alias()
        self._gather_grads()
        idx = [i for i, f in enumerate(self.flats) if f.grad is not None]
        if not idx:
            return idx
        # ONE device-resident step counter serves every model (torch's optimizers keep one per parameter): that is only the same
        # thing while the same models are stepped every time — a model that sat out a step would get the others' bias correction
        if self._stepped is None:
            self._stepped = tuple(idx)
        elif self._stepped != tuple(idx):
            raise _lib.NerfHipError("%s: the set of models with gradients changed between steps (%s -> %s); one shared step "
                                    "counter cannot represent that — use %s for partially frozen training"
                                    % (self._name, self._stepped, tuple(idx), self._elsewhere))
        for i in idx:                                   # packed weight images made before this point are stale
            if isinstance(self.models[i], NeRF):
                self.models[i].weights_changed()
        return idx

    def _pointer_arrays(self, idx, *buffers):
        """HOST arrays of the launch: params, grads, then one per list in `buffers`, and the element counts."""
        n = len(idx)
        arr = ctypes.c_void_p * n
        out = [arr(*[self.flats[i].data_ptr() for i in idx]), arr(*[self.flats[i].grad.data_ptr() for i in idx])]
        out += [arr(*[b[i].data_ptr() for i in idx]) for b in buffers]
        return out, (ctypes.c_int64 * n)(*[self.flats[i].numel() for i in idx])

    def zero_grad(self, set_to_none=True):
        for m, flat in zip(self.models, self.flats):
            flat.grad = None
            flat_grad_reset(m)
            for p in m.flat_params():
                if set_to_none or p.grad is None:
                    p.grad = None
                else:
                    p.grad.zero_()

    # ---------------------------------------------------------------------------------------------- checkpoints
    def _param_slices(self):
        """(model index, flat offset, shape) of every parameter in `[p for m in models for p in m.parameters()]` order —
        the order the reference's optimizer (utils/__init__.py:12-14) numbers its parameters in."""
        out = []
        for mi, m in enumerate(self.models):
            offs, off = {}, 0
            for p in m.flat_params():
                offs[id(p)] = off
                off += p.numel()
            for p in m.parameters():
                out.append((mi, offs[id(p)], tuple(p.shape)))
        return out

    def _moment_state(self, tensor_step, extra=()):
        """{parameter index: {step, exp_avg, exp_avg_sq, ...}} over the module parameters; `extra`: (key, flat buffers) pairs.
        `step` is a CPU tensor (torch.optim.Adam) or an int (the reference's own classes).  Empty before the first step."""
        step = float(self.dev_state[0])
        state = {}
        if step > 0:
            step = torch.tensor(step, dtype=torch.float32) if tensor_step else int(step)
            for i, (mi, off, shape) in enumerate(self._param_slices()):
                n = 1
                for s in shape:
                    n *= s
                state[i] = {"step": step.clone() if tensor_step else step, "exp_avg": self.exp_avg[mi][off:off + n].view(shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[mi][off:off + n].view(shape).clone()}
                for key, bufs in extra:
                    state[i][key] = bufs[mi][off:off + n].view(shape).clone()
        return state

    def _load_moments(self, sd, what, group_keys, extra=()):
        """The inverse of `_moment_state` plus the group's hyper-parameters named in `group_keys`."""
        sl = self._param_slices()
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(sl):
            raise ValueError("%s.load_state_dict expects %s state over the %d model parameters" % (self._name, what, len(sl)))
        g = self.param_groups[0]
        for k in group_keys + ("initial_lr",):
            if k in groups[0]:
                g[k] = tuple(groups[0][k]) if k == "betas" else groups[0][k]
        ids = groups[0]["params"]
        step = 0.0
        for e in self.exp_avg + self.exp_avg_sq:
            e.zero_()
        for i, (mi, off, shape) in enumerate(sl):
            st = sd["state"].get(ids[i])
            if st is None:
                continue
            n = st["exp_avg"].numel()
            self.exp_avg[mi][off:off + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[mi][off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            for key, bufs in extra:
                if key not in st:
                    raise ValueError("%s.load_state_dict: parameter %d has no %r" % (self._name, i, key))
                bufs[mi][off:off + n].copy_(st[key].reshape(-1))
            step = max(step, float(st["step"]))
        self.dev_state.zero_()
        self.dev_state[0] = step


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam(lr, eps, weight_decay) — the reference's default optimizer (utils/__init__.py:18-20)."""
    _elsewhere = "torch.optim.Adam"

    def __init__(self, models, lr=5e-4, eps=1e-8, weight_decay=0, betas=(0.9, 0.999)):
        super().__init__(models, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._applied = None          # ids of the models whose update the last backward already applied (fused reduce + Adam)

    # ---------------------------------------------------------------------------------------------- update inside the backward
    def handle(self, models):
        """nerfhip_adam_fused for `models` (in that order): the fused training step's reduce kernel applies this optimizer's
        update to the flat parameter storage while it writes the gradients (models/train_step.py; single-GPU steps only —
        with several ranks the all-reduce sits between gradients and update)."""
        self._check_alias()
        h = _lib.AdamFused()
        h.n_models = len(models)
        for k, m in enumerate(models):
            i = next(j for j, mm in enumerate(self.models) if mm is m)
            h.param[k] = self.flats[i].data_ptr()
            h.exp_avg[k] = self.exp_avg[i].data_ptr()
            h.exp_avg_sq[k] = self.exp_avg_sq[i].data_ptr()
        g = self.param_groups[0]
        h.state = self.dev_state.data_ptr()
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), \
            float(g['weight_decay'])
        return h

    def applied_in_backward(self, models):
        self._applied = {id(m) for m in models}
        for m in models:                                # (all of them this optimizer's: handle(models) found each)
            m.weights_changed()

    # ---------------------------------------------------------------------------------------------- the update
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._applied is not None:
            # the backward that produced these gradients already updated the parameters (and advanced the step counter)
            done, self._applied = self._applied, None
            if done != {id(m) for m in self.models}:
                raise _lib.NerfHipError("FlatAdam: the fused backward updated only some of the optimizer's models")
            if self._stepped is None:
                self._stepped = tuple(range(len(self.models)))
            return loss
        idx = self._begin_step()
        if not idx:
            return loss
        g = self.param_groups[0]
        (pp, gp, mp, vp), nn = self._pointer_arrays(idx, self.exp_avg, self.exp_avg_sq)
        with torch.cuda.device(self.flats[0].device):
            check(_lib.load().nerfhip_adam_step(pp, gp, mp, vp, nn, len(idx), ptr(self.dev_state), float(g['lr']), float(g['betas'][0]),
                                                float(g['betas'][1]), float(g['eps']), float(g['weight_decay']), stream_ptr()),
                  "nerfhip_adam_step")
        return loss

    def zero_grad(self, set_to_none=True):
        self._applied = None
        super().zero_grad(set_to_none)

    # ---------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        """torch.optim.Adam's layout over the 48 module parameters (loadable by the reference's optimizer)."""
        state = self._moment_state(tensor_step=True)
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"],
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "decoupled_weight_decay": False, "params": list(range(len(self._param_slices())))}
        if "initial_lr" in g:
            group["initial_lr"] = g["initial_lr"]
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        self._load_moments(sd, "torch.optim.Adam", ("lr", "eps", "weight_decay", "betas"))


def _run_closure(closure):
    if closure is None:
        return None
    with torch.enable_grad():
        return closure()


class FlatRAdam(_FlatOptimizer):
    """The reference's RAdam (utils/optimizers.py:6-95; NOT torch.optim.RAdam, which places eps differently): rectified Adam
    once N_sma(t) >= 5, below that momentum SGD (`degenerated_to_sgd`) or no parameter update at all; weight decay as
    p -= wd lr p, only when the parameter is updated.  One `nerfhip_radam_step` launch per step; N_sma and the step size are
    formed on the device in double from the device-resident step counter, so the step replays inside a hipGraph."""

    _elsewhere = "the reference's RAdam"

    def __init__(self, models, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True):
        # the ranges nerfhip_radam_step accepts, refused here before any storage is flattened
        self._require(lr >= 0, "lr", lr)
        self._require(eps >= 0, "eps", eps)
        self._require(all(0 <= b < 1 for b in betas) and len(betas) == 2, "betas", betas)
        self.degenerated_to_sgd = bool(degenerated_to_sgd)
        super().__init__(models, {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay})

    @torch.no_grad()
    def step(self, closure=None):
        loss = _run_closure(closure)
        idx = self._begin_step()
        if not idx:
            return loss
        g = self.param_groups[0]
        (pp, gp, mp, vp), nn = self._pointer_arrays(idx, self.exp_avg, self.exp_avg_sq)
        with torch.cuda.device(self.flats[0].device):
            check(_lib.load().nerfhip_radam_step(pp, gp, mp, vp, nn, len(idx), ptr(self.dev_state), float(g['lr']), float(g['betas'][0]),
                                                 float(g['betas'][1]), float(g['eps']), float(g['weight_decay']),
                                                 int(bool(self.degenerated_to_sgd)), stream_ptr()),
                  "nerfhip_radam_step")
        return loss

    def state_dict(self):
        """The layout of the reference's RAdam over the 48 module parameters: per parameter `step` (int), `exp_avg`,
        `exp_avg_sq`; the group carries its `buffer` of ten cached [step, N_sma, step_size] triples, all unset here (the
        reference recomputes an entry whose step does not match)."""
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"],
                 "buffer": [[None, None, None] for _ in range(10)], "params": list(range(len(self._param_slices())))}
        if "initial_lr" in g:
            group["initial_lr"] = g["initial_lr"]
        return {"state": self._moment_state(tensor_step=False), "param_groups": [group]}

    def load_state_dict(self, sd):
        self._load_moments(sd, "the reference's RAdam", ("lr", "eps", "weight_decay", "betas"))


class FlatRanger(_FlatOptimizer):
    """The reference's Ranger (utils/optimizers.py:266-405): RAdam rectified when N_sma(t) > N_sma_threshhold and always
    degenerating to momentum SGD below it, weight decay on every step, plus lookahead — every k-th step
    slow += alpha (p - slow), p = slow.  One `nerfhip_ranger_step` launch per step.

    The slow weights start as the weights the FIRST step finds, not those of construction time (the reference copies p.data
    inside its first step()): a checkpoint loaded after configure_optimizers is honoured.  The launch that sees step counter 0
    does that copy itself, so a first step that is captured into a graph still does it exactly once."""

    _elsewhere = "the reference's Ranger"

    def __init__(self, models, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0):
        # the ranges nerfhip_ranger_step accepts (the reference also wants lr and eps strictly positive)
        self._require(lr > 0, "lr", lr)
        self._require(eps > 0, "eps", eps)
        self._require(0 <= alpha <= 1, "alpha", alpha)
        self._require(k >= 1, "k", k)
        self._require(all(0 <= b < 1 for b in betas) and len(betas) == 2, "betas", betas)
        # As in the reference, the interpolation rate and the rectification threshold are the constructor's for the life of
        # the optimizer (its step reads self.alpha / self.N_sma_threshhold); only k is read from the group, so only k follows a
        # loaded checkpoint.  The group still lists all of them: that is the layout of the reference's state_dict.
        self.alpha, self.k, self.N_sma_threshhold = alpha, k, N_sma_threshhold
        group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay}
        group.update(alpha=alpha, k=k, N_sma_threshhold=N_sma_threshhold, step_counter=0)
        super().__init__(models, group)
        self.slow = [torch.zeros_like(f.data) for f in self.flats]        # filled by the first step's launch

    @torch.no_grad()
    def step(self, closure=None):
        loss = _run_closure(closure)
        idx = self._begin_step()          # bumps the weights serial: every step moves the weights, a sync step rewrites them
        if not idx:
            return loss
        g = self.param_groups[0]
        (pp, gp, mp, vp, sp), nn = self._pointer_arrays(idx, self.exp_avg, self.exp_avg_sq, self.slow)
        with torch.cuda.device(self.flats[0].device):
            check(_lib.load().nerfhip_ranger_step(pp, gp, mp, vp, nn, len(idx), ptr(self.dev_state), sp, float(self.alpha), int(g['k']),
                                                  float(self.N_sma_threshhold), float(g['lr']), float(g['betas'][0]),
                                                  float(g['betas'][1]), float(g['eps']), float(g['weight_decay']), stream_ptr()),
                  "nerfhip_ranger_step")
        return loss

    def state_dict(self):
        """The layout of the reference's Ranger over the 48 module parameters: per parameter `step` (int), `exp_avg`,
        `exp_avg_sq`, `slow_buffer`."""
        g = self.param_groups[0]
        group = {"lr": g["lr"], "alpha": g["alpha"], "k": g["k"], "step_counter": g["step_counter"], "betas": tuple(g["betas"]),
                 "N_sma_threshhold": g["N_sma_threshhold"], "eps": g["eps"], "weight_decay": g["weight_decay"],
                 "params": list(range(len(self._param_slices())))}
        if "initial_lr" in g:
            group["initial_lr"] = g["initial_lr"]
        return {"state": self._moment_state(tensor_step=False, extra=(("slow_buffer", self.slow),)), "param_groups": [group]}

    def load_state_dict(self, sd):
        self._load_moments(sd, "the reference's Ranger", ("lr", "alpha", "k", "step_counter", "N_sma_threshhold", "eps",
                                                           "weight_decay", "betas"), extra=(("slow_buffer", self.slow),))

"""Mint tests/golden/reference_optim.npz and tests/golden/reference_warmup_lrs.json (CPU, no GPU needed).

    python tests/tools/make_golden_optim.py /path/to/reference

The reference's `utils/optimizers.py` (RAdam, Ranger) and `utils/warmup_scheduler.py` (GradualWarmupScheduler) are loaded BY
PATH at mint time and run unmodified; this file holds none of their text.  What it does hold is a float64 restatement of the two
updates (`radam_f64`, `ranger_f64`): the GPU tests use it as the real-valued update that both the reference's fp32 run and the HIP
kernels approximate, and the fixture records the reference's own distance to it (`ref_vs_f64`), which sets the tests' bound.

Fixture contents (reference_optim.npz):
    p0_a (4099), p0_b (517)              shared start, 0.1 N(0,1)
    g_a (14, 4099), g_b (14, 517)        shared gradients, N(0,1) 10^U{-9..0}
    hyper                                [lr, eps, weight_decay]
    <opt>_p<t>_<a|b>                     parameters after step t in SNAP_STEPS             (<opt> = radam | ranger)
    <opt>_state<t>_<key>_<a|b>           per-parameter state after step t in STATE_STEPS   (key = step, exp_avg, exp_avg_sq, [slow_buffer])
    <opt>_ref_vs_f64                     per snapshot in SNAP_STEPS: max |reference fp32 - float64 restatement|
    <opt>_state_keys, <opt>_group_keys   the key names of the reference's state_dict()
"""
import importlib.util
import json
import math
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SIZES = (4099, 517)                # > one 4096-element workgroup with a ragged tail; a sub-workgroup tensor
N_STEPS = 14
SNAP_STEPS = (1, 5, 6, 7, 12, 14)
STATE_STEPS = (7, 14)
LR, EPS, WD = 5e-4, 1e-8, 1e-4
RADAM_BETAS, RANGER_BETAS = (0.9, 0.999), (0.95, 0.999)
RANGER_ALPHA, RANGER_K, RANGER_THRESHOLD = 0.5, 6, 5


# ------------------------------------------------------------------------------------------------ float64 restatement
def rectification(t, beta1, beta2, threshold, strict):
    """(N_sma, rectified?, step_size) at step t (1-based), in Python floats (= float64), as utils/optimizers.py forms them.
    RAdam rectifies when N_sma >= 5 (`strict=False`), Ranger when N_sma > N_sma_threshhold (`strict=True`)."""
    beta2_t = beta2 ** t
    n_max = 2.0 / (1.0 - beta2) - 1.0
    n_sma = n_max - 2.0 * t * beta2_t / (1.0 - beta2_t)
    rect = n_sma > threshold if strict else n_sma >= threshold
    if rect:
        step = math.sqrt((1.0 - beta2_t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) \
            / (1.0 - beta1 ** t)
    else:
        step = 1.0 / (1.0 - beta1 ** t)
    return n_sma, rect, step


def radam_f64(p, g, m, v, t, lr, betas=RADAM_BETAS, eps=EPS, wd=WD, degenerated_to_sgd=True):
    """One RAdam step on float64 numpy arrays, in place; t is the 1-based step number."""
    beta1, beta2 = betas
    v *= beta2
    v += (1.0 - beta2) * g * g
    m *= beta1
    m += (1.0 - beta1) * g
    _, rect, step = rectification(t, beta1, beta2, 5, strict=False)
    if rect:
        if wd != 0:
            p += -wd * lr * p
        p += -step * lr * m / (np.sqrt(v) + eps)
    elif degenerated_to_sgd:
        if wd != 0:
            p += -wd * lr * p
        p += -step * lr * m


def ranger_f64(p, g, m, v, slow, t, lr, betas=RANGER_BETAS, eps=EPS, wd=WD, alpha=RANGER_ALPHA, k=RANGER_K,
               threshold=RANGER_THRESHOLD):
    """One Ranger step on float64 numpy arrays, in place (`slow` must hold the weights as they were before step 1)."""
    beta1, beta2 = betas
    v *= beta2
    v += (1.0 - beta2) * g * g
    m *= beta1
    m += (1.0 - beta1) * g
    _, rect, step = rectification(t, beta1, beta2, threshold, strict=True)
    if wd != 0:
        p += -wd * lr * p
    if rect:
        p += -step * lr * m / (np.sqrt(v) + eps)
    else:
        p += -step * lr * m
    if t % k == 0:
        slow += alpha * (p - slow)
        p[...] = slow


# ------------------------------------------------------------------------------------------------ minting
def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs():
    g = torch.Generator().manual_seed(20240)
    p0 = [0.1 * torch.randn(n, generator=g) for n in SIZES]
    grads = []
    for _ in range(N_STEPS):
        grads.append([torch.randn(n, generator=g) * (10.0 ** torch.randint(-9, 1, (n,), generator=g).float()) for n in SIZES])
    return p0, grads


def mint_optim(ref_root):
    mod = _load(os.path.join(ref_root, "utils", "optimizers.py"), "_reference_optimizers")
    p0, grads = make_inputs()
    out = {"p0_a": p0[0].numpy(), "p0_b": p0[1].numpy(),
           "g_a": torch.stack([g[0] for g in grads]).numpy(), "g_b": torch.stack([g[1] for g in grads]).numpy(),
           "hyper": np.array([LR, EPS, WD], dtype=np.float64),
           "snap_steps": np.array(SNAP_STEPS), "state_steps": np.array(STATE_STEPS)}
    for name in ("radam", "ranger"):
        params = [torch.nn.Parameter(p.clone()) for p in p0]
        if name == "radam":
            opt = mod.RAdam(params, lr=LR, eps=EPS, weight_decay=WD)
        else:
            opt = mod.Ranger(params, lr=LR, eps=EPS, weight_decay=WD)
        p64 = [p.double().numpy().copy() for p in p0]
        m64 = [np.zeros_like(p) for p in p64]
        v64 = [np.zeros_like(p) for p in p64]
        s64 = [p.copy() for p in p64]
        dist = []
        for t in range(1, N_STEPS + 1):
            for i, p in enumerate(params):
                p.grad = grads[t - 1][i].clone()
                g64 = grads[t - 1][i].double().numpy()
                if name == "radam":
                    radam_f64(p64[i], g64, m64[i], v64[i], t, LR)
                else:
                    ranger_f64(p64[i], g64, m64[i], v64[i], s64[i], t, LR)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")            # the deprecated add_/addcmul_ overloads the reference calls
                opt.step()
            if t in SNAP_STEPS:
                dist.append(max(float(np.abs(p.detach().double().numpy() - q).max()) for p, q in zip(params, p64)))
                for tag, p in zip("ab", params):
                    out["%s_p%d_%s" % (name, t, tag)] = p.detach().numpy().copy()
            if t in STATE_STEPS:
                for tag, p in zip("ab", params):
                    for key, val in opt.state[p].items():
                        arr = val.detach().numpy().copy() if torch.is_tensor(val) else np.array(val)
                        out["%s_state%d_%s_%s" % (name, t, key, tag)] = arr
        sd = opt.state_dict()
        out[name + "_ref_vs_f64"] = np.array(dist, dtype=np.float64)
        out[name + "_state_keys"] = np.array(sorted(sd["state"][0].keys()))
        out[name + "_group_keys"] = np.array(sorted(sd["param_groups"][0].keys()))
        print(name, "ref_vs_f64 at steps", SNAP_STEPS, ":", " ".join("%.2e" % d for d in dist))
    path = os.path.join(GOLDEN, "reference_optim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


WARMUP_SETTINGS = ((1.0, 2), (2.0, 3), (4.0, 5))
WARMUP_EPOCHS = 12
# after-schedulers as the reference's get_scheduler builds them (utils/__init__.py:32-43); num_epochs 16, eta_min = 1e-8
AFTER = {"steplr_inside": dict(kind="steplr", decay_step=[2, 8], decay_gamma=0.5),
         "steplr_after": dict(kind="steplr", decay_step=[7, 10], decay_gamma=0.1),
         "cosine": dict(kind="cosine", num_epochs=16),
         "poly": dict(kind="poly", num_epochs=16, poly_exp=0.9)}


def build_after(optimizer, spec):
    from torch.optim import lr_scheduler as L
    if spec["kind"] == "steplr":
        return L.MultiStepLR(optimizer, milestones=spec["decay_step"], gamma=spec["decay_gamma"])
    if spec["kind"] == "cosine":
        return L.CosineAnnealingLR(optimizer, T_max=spec["num_epochs"], eta_min=1e-8)
    n_ep, pexp = spec["num_epochs"], spec["poly_exp"]
    return L.LambdaLR(optimizer, lambda epoch: (1 - epoch / n_ep) ** pexp)


def warmup_lrs(scheduler_cls, opt_name, multiplier, total_epoch, spec):
    """The lr seen by each of WARMUP_EPOCHS epochs with `optimizer.step(); scheduler.step()` per epoch."""
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.Adam([p], lr=LR, eps=1e-8) if opt_name == "adam" else torch.optim.SGD([p], lr=LR, momentum=0.9)
    sched = scheduler_cls(opt, multiplier=multiplier, total_epoch=total_epoch, after_scheduler=build_after(opt, spec))
    lrs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(WARMUP_EPOCHS):
            lrs.append(opt.param_groups[0]["lr"])
            p.grad = torch.ones_like(p)
            opt.step()
            sched.step()
    return lrs


def mint_warmup(ref_root):
    mod = _load(os.path.join(ref_root, "utils", "warmup_scheduler.py"), "_reference_warmup")
    cases = []
    for opt_name in ("adam", "sgd"):
        for multiplier, total_epoch in WARMUP_SETTINGS:
            for after, spec in AFTER.items():
                cases.append({"optimizer": opt_name, "multiplier": multiplier, "total_epoch": total_epoch, "after": after,
                              "after_spec": spec, "base_lr": LR,
                              "lrs": warmup_lrs(mod.GradualWarmupScheduler, opt_name, multiplier, total_epoch, spec)})
    path = os.path.join(GOLDEN, "reference_warmup_lrs.json")
    with open(path, "w") as f:
        json.dump({"epochs": WARMUP_EPOCHS, "cases": cases}, f, indent=1)
    print("wrote", path, len(cases), "cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mint_optim(sys.argv[1])
    mint_warmup(sys.argv[1])

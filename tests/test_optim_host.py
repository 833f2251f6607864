"""CPU: the warm-up scheduler against the reference's recorded learning rates, the optimizer dispatch of
`NeRFSystem.configure_optimizers`, and the argument checks of the RAdam / Ranger entry points (nothing is launched).

Fixture: tests/golden/reference_warmup_lrs.json, minted by tests/tools/make_golden_optim.py from the reference's
utils/warmup_scheduler.py over torch.optim.Adam / SGD on a CPU parameter."""
import ctypes
import json
import os
import warnings
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _warmup_cases():
    with open(os.path.join(ROOT, "tests", "golden", "reference_warmup_lrs.json")) as f:
        return json.load(f)


def _after(optimizer, spec):
    """The after-scheduler as configure_optimizers / the reference's get_scheduler builds it."""
    L = torch.optim.lr_scheduler
    if spec["kind"] == "steplr":
        return L.MultiStepLR(optimizer, milestones=spec["decay_step"], gamma=spec["decay_gamma"])
    if spec["kind"] == "cosine":
        return L.CosineAnnealingLR(optimizer, T_max=spec["num_epochs"], eta_min=1e-8)
    n_ep, pexp = spec["num_epochs"], spec["poly_exp"]
    return L.LambdaLR(optimizer, lambda epoch: (1 - epoch / n_ep) ** pexp)


def test_warmup_lrs_equal_the_reference():
    from nerf_pl_amd.schedulers import GradualWarmupScheduler
    fx = _warmup_cases()
    assert len(fx["cases"]) == 2 * 3 * 4
    for case in fx["cases"]:
        p = torch.nn.Parameter(torch.zeros(3))
        if case["optimizer"] == "adam":
            opt = torch.optim.Adam([p], lr=case["base_lr"], eps=1e-8)
        else:
            opt = torch.optim.SGD([p], lr=case["base_lr"], momentum=0.9)
        sched = GradualWarmupScheduler(opt, multiplier=case["multiplier"], total_epoch=case["total_epoch"],
                                       after_scheduler=_after(opt, case["after_spec"]))
        lrs = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(fx["epochs"]):
                lrs.append(opt.param_groups[0]["lr"])
                p.grad = torch.ones_like(p)
                opt.step()
                sched.step()
        tag = (case["optimizer"], case["multiplier"], case["total_epoch"], case["after"])
        assert len(lrs) == len(case["lrs"]) == 12
        for e, (a, b) in enumerate(zip(lrs, case["lrs"])):
            assert abs(a - b) <= 1e-12 * abs(b), (tag, e, a, b)
        for e in range(case["total_epoch"] + 1):                       # the fixture really holds the ramp
            ramp = case["base_lr"] * ((case["multiplier"] - 1.0) * e / case["total_epoch"] + 1.0)
            assert case["lrs"][e] == pytest.approx(ramp, rel=1e-12), (tag, e)


def test_warmup_refuses_multiplier_below_one_and_plateau():
    from nerf_pl_amd.schedulers import GradualWarmupScheduler
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=0.1)
    with pytest.raises(ValueError):
        GradualWarmupScheduler(opt, multiplier=0.5, total_epoch=3)
    with pytest.raises(NotImplementedError):
        GradualWarmupScheduler(opt, multiplier=2.0, total_epoch=3, after_scheduler=torch.optim.lr_scheduler.ReduceLROnPlateau(opt))


def _hparams(**kw):
    hp = dict(N_samples=8, N_importance=8, use_disp=False, perturb=0.0, noise_std=0.0, chunk=1024, loss_type="mse", lr=5e-4,
              weight_decay=0, momentum=0.9, lr_scheduler="steplr", decay_step=[20], decay_gamma=0.1, num_epochs=16, white_back=True)
    hp.update(kw)
    return Namespace(**hp)


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_configure_optimizers_wraps_the_scheduler_for_adam_and_sgd(name):
    from nerf_pl_amd.schedulers import GradualWarmupScheduler
    from nerf_pl_amd.system import NeRFSystem
    system = NeRFSystem(_hparams(optimizer=name, warmup_epochs=3, warmup_multiplier=2.0))
    (opt,), (sched,) = system.configure_optimizers()
    assert isinstance(sched, GradualWarmupScheduler)
    assert sched.total_epoch == 3 and sched.multiplier == 2.0
    assert isinstance(sched.after_scheduler, torch.optim.lr_scheduler.MultiStepLR)
    assert type(opt).__name__ == ("Adam" if name == "adam" else "SGD")
    # and without warm-up the scheduler is the bare one, as before
    (_,), (plain,) = NeRFSystem(_hparams(optimizer=name)).configure_optimizers()
    assert isinstance(plain, torch.optim.lr_scheduler.MultiStepLR)


@pytest.mark.parametrize("name", ["radam", "ranger"])
def test_radam_and_ranger_have_no_cpu_form(name):
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.system import NeRFSystem
    system = NeRFSystem(_hparams(optimizer=name, warmup_epochs=3))
    with pytest.raises(NerfHipError):
        system.configure_optimizers()


def test_flat_optimizers_keep_out_of_the_fused_update():
    """`fuse_adam` (the update inside the reduce kernel) is Adam's alone: the new classes offer no handle for it."""
    from nerf_pl_amd import optim
    assert hasattr(optim.FlatAdam, "handle")
    assert not hasattr(optim.FlatRAdam, "handle") and not hasattr(optim.FlatRanger, "handle")
    assert issubclass(optim.FlatRAdam, optim._FlatOptimizer) and issubclass(optim.FlatAdam, optim._FlatOptimizer)


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def test_radam_and_ranger_entry_points_validate_arguments_without_a_gpu(lib):
    vp = ctypes.c_void_p
    fake = 0x10000                                       # never dereferenced: every call below returns from the checks

    def arrays(n):
        return [(vp * max(n, 1))(*([fake] * max(n, 1))) for _ in range(5)], (ctypes.c_int64 * max(n, 1))(*([64] * max(n, 1)))

    def radam(n=1, state=fake, params="ok", lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, numel=None):
        (pp, gp, mp, vv, _), nn = arrays(n)
        if numel is not None:
            nn[0] = numel
        return lib.nerfhip_radam_step(None if params is None else pp, gp, mp, vv, nn, n, vp(state) if state else None,
                                      lr, b1, b2, eps, wd, 1, None)

    def ranger(n=1, state=fake, slow="ok", alpha=0.5, k=6, lr=5e-4, b1=0.95, b2=0.999, eps=1e-8, wd=0.0, null_slow_entry=False):
        (pp, gp, mp, vv, sp), nn = arrays(n)
        if null_slow_entry:
            sp[0] = None
        return lib.nerfhip_ranger_step(pp, gp, mp, vv, nn, n, vp(state) if state else None, None if slow is None else sp,
                                       alpha, k, 5.0, lr, b1, b2, eps, wd, None)

    BADARG = -1
    for call in (radam, ranger):
        assert call(n=0) == BADARG and call(n=9) == BADARG
        assert call(state=None) == BADARG
        assert call(eps=-1e-8) == BADARG
        assert call(b2=1.0) == BADARG and call(b1=-0.1) == BADARG
        assert call(lr=-1.0) == BADARG and call(wd=-1.0) == BADARG
    assert radam(params=None) == BADARG
    assert radam(numel=0) == BADARG
    assert ranger(slow=None) == BADARG and ranger(null_slow_entry=True) == BADARG
    assert ranger(k=0) == BADARG
    assert ranger(alpha=-0.1) == BADARG and ranger(alpha=1.5) == BADARG
    # a null entry inside a pointer array
    (pp, gp, mp, vv, _), nn = arrays(2)
    gp[1] = None
    assert lib.nerfhip_radam_step(pp, gp, mp, vv, nn, 2, vp(fake), 5e-4, 0.9, 0.999, 1e-8, 0.0, 1, None) == BADARG

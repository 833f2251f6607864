"""GPU: FlatRAdam / FlatRanger (nerfhip_radam_step / nerfhip_ranger_step) against the reference's utils/optimizers.py.

The reference's behaviour travels as data: tests/golden/reference_optim.npz, minted on the CPU by tests/tools/make_golden_optim.py
from the reference's unmodified classes (two tensors of 4099 and 517 elements, 14 steps, lr 5e-4, eps 1e-8, weight decay 1e-4;
crosses the degenerate -> rectified switch at step 6 and the lookahead syncs at steps 6 and 12).  `ref_vs_f64` in the fixture is
the reference's own fp32 distance to a float64 restatement of the update; the kernels are allowed three times that to the
reference (reference and kernel are each one fp32 evaluation of the same real-valued update: twice the reference's own distance
to float64, plus that distance)."""
import os

import numpy as np
import pytest
import torch

# The float64 restatement (radam_f64 / ranger_f64) lives in the fixture's recipe.  It is a fair yardstick here because the recipe
# checks it against the reference itself: the fixture's `ref_vs_f64` is the distance between the reference's unmodified fp32 run
# and this restatement (<= 2.5e-7 over 14 steps), so a mistake in it would show there, not hide in these tests.
from tests.tools import make_golden_optim as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = "ab"


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_optim.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


class _Flat(torch.nn.Module):
    """Stands in for a NeRF model: one parameter tensor, which is also its flat storage order."""

    def __init__(self, values):
        super().__init__()
        self.w = torch.nn.Parameter(values.clone())

    def flat_params(self):
        return [self.w]


def _models(dev, values):
    return [_Flat(torch.as_tensor(v, dtype=torch.float32)).to(dev) for v in values]


def _make(name, models, fx, **kw):
    from nerf_pl_amd.optim import FlatRAdam, FlatRanger
    lr, eps, wd = (float(x) for x in fx["hyper"])
    args = dict(lr=lr, eps=eps, weight_decay=wd)
    args.update(kw)
    return (FlatRAdam if name == "radam" else FlatRanger)(models, **args)


def _set_grads(models, fx, t):
    for m, tag in zip(models, TAGS):
        m.w.grad = torch.from_numpy(fx["g_" + tag][t - 1]).to(m.w.device)


def _worst(models, fx, name, t):
    return max(float((m.w.detach().cpu() - torch.from_numpy(fx["%s_p%d_%s" % (name, t, tag)])).abs().max())
               for m, tag in zip(models, TAGS))


def _bound(fx, name, t):
    return 3.0 * float(fx[name + "_ref_vs_f64"][list(fx["snap_steps"]).index(t)])


@pytest.mark.parametrize("name", ["radam", "ranger"])
def test_trajectory_follows_the_reference(dev, fx, name):
    """(1) Every snapshot (steps 1, 5, 6, 7, 12, 14) within 3 x ref_vs_f64 of the reference's parameters; the device-side
    counter has counted the 14 steps."""
    models = _models(dev, [fx["p0_a"], fx["p0_b"]])
    opt = _make(name, models, fx)
    for t in range(1, 15):
        _set_grads(models, fx, t)
        opt.step()
        if t in fx["snap_steps"]:
            worst, bound = _worst(models, fx, name, t), _bound(fx, name, t)
            print("%s step %2d: max |kernel - reference| %.3e (bound %.3e = 3 x ref_vs_f64)" % (name, t, worst, bound))
            assert worst <= bound, (name, t, worst, bound)
    assert float(opt.dev_state[0]) == 14.0
    assert int(opt.dev_state.view(torch.int32)[1]) == 0            # the arrival ticket is back at zero


@pytest.mark.parametrize("name", ["radam", "ranger"])
def test_coefficients_are_formed_in_double(dev, name):
    """(2) p = 0 before every step, weight_decay = 0, a constant per-element gradient of magnitude 1e-6 .. 1: what a step leaves in
    p is that step's increment alone (no rounding of an accumulated p on top of it), compared per element with the float64
    restatement at 2e-5 relative — far above a dozen fp32 roundings (~1e-6), far below the 1.6e-3 that fp32 rectification
    coefficients are off by at step 6 (and an fp32 N_sma takes the wrong branch at step 5 or 6 outright)."""
    n = 4099
    gen = torch.Generator().manual_seed(7)
    g32 = (10.0 ** (-6.0 * torch.rand(n, generator=gen))) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g32[:7] = torch.tensor([1.0, -1.0, 1e-6, -1e-6, 1e-3, 0.5, 1e-5])
    g64 = g32.double().numpy()
    lr, eps = 5e-4, 1e-8
    (model,) = _models(dev, [torch.zeros(n)])
    if name == "radam":
        from nerf_pl_amd.optim import FlatRAdam
        opt = FlatRAdam([model], lr=lr, eps=eps, weight_decay=0)
    else:
        from nerf_pl_amd.optim import FlatRanger
        opt = FlatRanger([model], lr=lr, eps=eps, weight_decay=0)
    p64, m64, v64, s64 = (np.zeros(n) for _ in range(4))
    worst_all = 0.0
    for t in range(1, 15):
        with torch.no_grad():
            model.w.zero_()
        p64[...] = 0.0
        model.w.grad = g32.to(dev)
        opt.step()
        if name == "radam":
            G.radam_f64(p64, g64, m64, v64, t, lr, eps=eps, wd=0.0)
        else:
            G.ranger_f64(p64, g64, m64, v64, s64, t, lr, eps=eps, wd=0.0)
        got = model.w.detach().cpu().double().numpy()
        assert np.all(p64 != 0.0)
        rel = float(np.max(np.abs(got - p64) / np.abs(p64)))
        worst_all = max(worst_all, rel)
        print("%s step %2d: max relative error of the increment %.3e (bound 2e-5)" % (name, t, rel))
        assert rel <= 2e-5, (name, t, rel)
    assert float(opt.dev_state[0]) == 14.0


def test_radam_without_sgd_degeneration_leaves_parameters_alone(dev, fx):
    """(3) degenerated_to_sgd=False: bit-unchanged parameters through step 5 (N_sma(5) = 4.996 < 5) while exp_avg moves; step 6
    (N_sma = 5.994) is the first to move them."""
    models = _models(dev, [fx["p0_a"], fx["p0_b"]])
    opt = _make("radam", models, fx, degenerated_to_sgd=False)
    start = [m.w.detach().clone() for m in models]
    prev_m = [e.clone() for e in opt.exp_avg]
    for t in range(1, 6):
        _set_grads(models, fx, t)
        opt.step()
        for m, s in zip(models, start):
            assert torch.equal(m.w.detach(), s), t
        for e, pm in zip(opt.exp_avg, prev_m):
            assert not torch.equal(e, pm), t
        prev_m = [e.clone() for e in opt.exp_avg]
        assert all(float(e.abs().max()) > 0 for e in opt.exp_avg_sq)
    _set_grads(models, fx, 6)
    opt.step()
    for m, s in zip(models, start):
        assert not torch.equal(m.w.detach(), s)
    assert float(opt.dev_state[0]) == 6.0


def _fixture_state_dict(fx, name, t, template):
    keys = [str(k) for k in fx[name + "_state_keys"]]
    state = {}
    for i, tag in enumerate(TAGS):
        state[i] = {}
        for k in keys:
            a = fx["%s_state%d_%s_%s" % (name, t, k, tag)]
            state[i][k] = int(a) if k == "step" else torch.from_numpy(a)
    group = dict(template["param_groups"][0])
    return {"state": state, "param_groups": [group]}


@pytest.mark.parametrize("name", ["radam", "ranger"])
def test_state_dict_round_trip_with_the_reference(dev, fx, name):
    """(4) The reference's step-7 state loads and steps 8-14 meet its step-12 and step-14 snapshots; after 7 own steps
    state_dict() carries the reference's key names, one entry per parameter in parameters() order, values within the bound."""
    # --- load the reference's state, continue
    models = _models(dev, [fx["%s_p7_%s" % (name, tag)] for tag in TAGS])
    opt = _make(name, models, fx)
    opt.load_state_dict(_fixture_state_dict(fx, name, 7, opt.state_dict()))
    assert float(opt.dev_state[0]) == 7.0
    for t in range(8, 15):
        _set_grads(models, fx, t)
        opt.step()
        if t in (12, 14):
            worst, bound = _worst(models, fx, name, t), _bound(fx, name, t)
            print("%s resumed from the reference's step 7, step %d: %.3e (bound %.3e)" % (name, t, worst, bound))
            assert worst <= bound, (name, t, worst, bound)
    assert float(opt.dev_state[0]) == 14.0
    # --- own state after 7 steps, in the reference's layout
    models = _models(dev, [fx["p0_a"], fx["p0_b"]])
    opt = _make(name, models, fx)
    assert opt.state_dict()["state"] == {}
    for t in range(1, 8):
        _set_grads(models, fx, t)
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd["param_groups"][0].keys()) == [str(k) for k in fx[name + "_group_keys"]]
    assert sd["param_groups"][0]["params"] == [0, 1] and sorted(sd["state"].keys()) == [0, 1]
    if name == "radam":
        assert sd["param_groups"][0]["buffer"] == [[None, None, None] for _ in range(10)]
    bound = _bound(fx, name, 7)
    for i, tag in enumerate(TAGS):
        st = sd["state"][i]
        assert sorted(st.keys()) == [str(k) for k in fx[name + "_state_keys"]]
        assert st["step"] == 7 and isinstance(st["step"], int)
        for k in st:
            if k == "step":
                continue
            ref = torch.from_numpy(fx["%s_state7_%s_%s" % (name, k, tag)])
            assert tuple(st[k].shape) == tuple(ref.shape) == tuple(models[i].w.shape)
            d = float((st[k].cpu() - ref).abs().max())
            print("%s state_dict after 7 steps, %s[%s]: max diff %.3e (bound %.3e)" % (name, k, tag, d, bound))
            assert d <= bound, (name, k, tag, d, bound)


@pytest.mark.parametrize("name", ["radam", "ranger"])
def test_graph_replay_is_bit_identical_to_eager(dev, fx, name):
    """(5) opt.step captured ONCE over static gradient buffers and replayed for all 14 steps == 14 eager steps, bit for bit: the
    device-side counter, the branch switch at step 6, Ranger's slow-buffer start at step 1 and both lookahead syncs under replay."""
    eager = _models(dev, [fx["p0_a"], fx["p0_b"]])
    opt_e = _make(name, eager, fx)
    for t in range(1, 15):
        _set_grads(eager, fx, t)
        opt_e.step()
    graphed = _models(dev, [fx["p0_a"], fx["p0_b"]])
    opt_g = _make(name, graphed, fx)
    for m in graphed:
        m.w.grad = torch.zeros_like(m.w)                     # static buffers: every replay reads these addresses
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        opt_g.step()
    assert float(opt_g.dev_state[0]) == 0.0                  # capturing ran nothing
    for t in range(1, 15):
        for m, tag in zip(graphed, TAGS):
            m.w.grad.copy_(torch.from_numpy(fx["g_" + tag][t - 1]))
        graph.replay()
    torch.cuda.synchronize()
    assert float(opt_g.dev_state[0]) == 14.0
    for a, b in zip(eager, graphed):
        assert torch.equal(a.w.detach(), b.w.detach())
    for bufs in ("exp_avg", "exp_avg_sq") + (("slow",) if name == "ranger" else ()):
        for a, b in zip(getattr(opt_e, bufs), getattr(opt_g, bufs)):
            assert torch.equal(a, b), bufs


def _system(dev, name):
    from argparse import Namespace
    from oracle import nerf_oracle as O
    from nerf_pl_amd.system import NeRFSystem
    hp = Namespace(N_samples=64, N_importance=64, use_disp=False, perturb=0.0, noise_std=0.0, chunk=1024 * 32, loss_type="mse",
                   lr=5e-4, weight_decay=0, decay_step=[100], decay_gamma=0.5, white_back=True, optimizer=name, warmup_epochs=2)
    system = NeRFSystem(hp)
    system.nerf_coarse.load_state_dict(O.make_params(5, 4.0, 0.2))
    system.nerf_fine.load_state_dict(O.make_params(6, 4.0, 0.2))
    for m in system.models:
        m.mlp_dtype = "fp32"
    batch = {"rays": O.make_rays(3, 192, "blender").to(dev),
             "rgbs": torch.rand(192, 3, generator=torch.Generator().manual_seed(0)).to(dev)}
    return system.to(dev), batch


@pytest.mark.parametrize("name", ["radam", "ranger"])
def test_system_trains_with_radam_and_ranger(dev, name):
    """(6) NeRFSystem(optimizer=radam|ranger), fp32, perturb = 0, noise_std = 0: through fit and through GraphedTrainStep the
    loss falls over 20 steps; every eager step advances the weights serial; warm-up is ignored for these optimizers."""
    from nerf_pl_amd.system import GraphedTrainStep, fit
    want = "FlatRAdam" if name == "radam" else "FlatRanger"
    system, batch = _system(dev, name)
    serials = []

    def batches():
        for _ in range(20):
            serials.append([m.weights_serial() for m in system.models])
            yield batch
    losses = [float(x) for x in fit(system, batches())]
    assert type(system.optimizer).__name__ == want
    print("%s fit: loss %.6f -> %.6f" % (name, losses[0], losses[-1]))
    assert len(losses) == 20 and losses[-1] < losses[0], losses
    assert float(system.optimizer.dev_state[0]) == 20.0
    for a, b in zip(serials, serials[1:]):
        assert all(y > x for x, y in zip(a, b)), serials
    (_,), (sched,) = system.configure_optimizers()
    assert isinstance(sched, torch.optim.lr_scheduler.MultiStepLR)           # warmup_epochs = 2 is ignored, as in the reference

    system, batch = _system(dev, name)
    (opt,), _ = system.configure_optimizers()
    stepper = GraphedTrainStep(system, opt, warmup=2)
    glosses = [float(stepper(batch)["loss"]) for _ in range(20)]
    assert stepper.graph is not None
    print("%s GraphedTrainStep: loss %.6f -> %.6f" % (name, glosses[0], glosses[-1]))
    assert glosses[-1] < glosses[0], glosses
    assert float(opt.dev_state[0]) == 20.0
    assert glosses == pytest.approx(losses, rel=1e-4)                        # replay trains like eager issue


def test_ranger_slow_buffer_starts_from_the_weights_of_the_first_step(dev):
    """(6) Weights loaded after configure_optimizers and before the first step end up in Ranger's slow buffer (the reference
    copies p.data inside its first step())."""
    from oracle import nerf_oracle as O
    system, batch = _system(dev, "ranger")
    (opt,), _ = system.configure_optimizers()
    built_with = [f.detach().clone() for f in opt.flats]
    system.nerf_coarse.load_state_dict(O.make_params(15, 4.0, 0.2))
    system.nerf_fine.load_state_dict(O.make_params(16, 4.0, 0.2))
    loaded = [f.detach().clone() for f in opt.flats]
    assert all(not torch.equal(a, b) for a, b in zip(built_with, loaded))    # load_state_dict wrote through the aliases
    out = system.training_step(batch, 0)
    opt.zero_grad(set_to_none=True)
    out["loss"].backward()
    opt.step()
    for slow, want, flat in zip(opt.slow, loaded, opt.flats):
        assert torch.equal(slow, want)
        assert not torch.equal(flat.detach(), want)                          # and the step itself moved the weights
    sd = opt.state_dict()
    assert len(sd["state"]) == 48 and sd["state"][0]["step"] == 1
    first = next(iter(system.nerf_coarse.parameters()))
    assert tuple(sd["state"][0]["slow_buffer"].shape) == tuple(first.shape)
    assert torch.equal(sd["state"][0]["slow_buffer"].cpu(), O.make_params(15, 4.0, 0.2)["xyz_encoding_1.0.weight"])

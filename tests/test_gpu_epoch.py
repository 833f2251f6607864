"""GPU: epoch sampling (csrc/epoch.hip, rays.EpochSampler, system.fit_epochs) — the device ids against the host
entry, every sampler batch against the existing nerfhip_sample_batch on its ids, the walk through epochs eager and captured, the
untouched Philox stream, the sampler as the batch source of the graphed step, the scheduler stepping per epoch, and resuming."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 4097, 65536, 65537)
SEEDS = (0, 0x5EED5EED, 2 ** 64 - 1)
EPOCHS = (0, 1, 4095)


def _store(dev, H=8, W=8, use_ndc=False):
    from nerf_pl_amd.rays import RayStore
    g = torch.Generator().manual_seed(8)
    n_img = 3
    c = torch.nn.functional.normalize(torch.randn(n_img, 3, generator=g), dim=-1) * 4.0
    poses = torch.cat([torch.linalg.qr(torch.randn(n_img, 3, 3, generator=g))[0], c[..., None]], -1).float().contiguous()
    rgbs = torch.rand(n_img * H * W, 3, generator=g)
    return RayStore(poses.to(dev), rgbs.to(dev), H, W, 11.0, 2.0, 6.0, use_ndc=use_ndc)


def _gen(dev):
    return torch.cuda.default_generators[dev.index]


def _host_ids(s, epoch, cursor):
    """the ids the host entry gives for batch `cursor` of `epoch` of sampler `s`"""
    from nerf_pl_amd import ops
    return ops.epoch_ids_host(s.seed, epoch, s.store.n_pixels, s.rank, s.world, first=cursor * s.batch_size, count=s.rows(cursor))


def _device_state(s):
    seed, epoch, cursor, ticket = (int(v) for v in s.state.cpu())
    assert ticket == 0 and seed & (2 ** 64 - 1) == s.seed
    return epoch, cursor


def _sample_batch(st, ids):
    from nerf_pl_amd import _lib
    from nerf_pl_amd._lib import check, ptr, stream_ptr
    n = ids.numel()
    rays = torch.empty(n, 8, device=ids.device)
    rgbs = torch.empty(n, 3, device=ids.device)
    check(_lib.load().nerfhip_sample_batch(ptr(st.poses), ptr(ids), ptr(st.rgbs), n, st.H, st.W, st.focal, st.near, st.far,
                                           int(st.use_ndc), st.ndc_near_plane, ptr(rays), ptr(rgbs), stream_ptr()), "sample_batch")
    return rays, rgbs


# ---- 1. the id kernel ------------------------------------------------------------------------------------------------------------
def test_device_ids_equal_host_ids(dev):
    from nerf_pl_amd import ops
    for n in SIZES:
        for seed in SEEDS:
            for epoch in EPOCHS:
                got = ops.epoch_ids(seed, epoch, n, dev).cpu().numpy()
                assert np.array_equal(got, ops.epoch_ids_host(seed, epoch, n)), (n, seed, epoch)
    n = 100 * 800 * 800
    for kw in (dict(first=63990000, count=10000), dict(rank=1, world=2, first=31990000, count=10000), dict(first=5, count=0)):
        got = ops.epoch_ids(3, 17, n, dev, **kw).cpu().numpy()
        assert np.array_equal(got, ops.epoch_ids_host(3, 17, n, **kw)), kw
    assert np.array_equal(ops.epoch_ids(1, 0, 195, dev, rank=2, world=3).cpu().numpy(), ops.epoch_ids_host(1, 0, 195, rank=2, world=3))


# ---- 2. one batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_ndc", [False, True])
@pytest.mark.parametrize("shape,B,rank,world", [((8, 8), 80, 0, 1), ((5, 13), 64, 1, 2), ((5, 13), 300, 0, 1)])
def test_batch_is_sample_batch_on_the_permuted_ids(dev, use_ndc, shape, B, rank, world):
    """rays / rgbs == nerfhip_sample_batch (the existing entry) on the returned ids, bit for bit; the ids == the host entry's for
    the (epoch, cursor) the mirror reports — over more than one epoch, partial batches included."""
    st = _store(dev, *shape, use_ndc=use_ndc)
    s = st.epoch_sampler(B, seed=21, rank=rank, world=world)
    for _ in range(2 * s.steps_per_epoch + 1):
        epoch, cursor = s.epoch, s.cursor
        b = s.sample(return_ids=True)
        want = _host_ids(s, epoch, cursor)
        assert b["ids"].dtype == torch.int64 and np.array_equal(b["ids"].cpu().numpy(), want), (epoch, cursor)
        assert b["rays"].shape == (len(want), 8) and b["rgbs"].shape == (len(want), 3)
        rays, rgbs = _sample_batch(st, b["ids"].contiguous())
        assert torch.equal(b["rays"], rays) and torch.equal(b["rgbs"], rgbs), (epoch, cursor)
    plain = st.epoch_sampler(B, seed=21, rank=rank, world=world).sample()
    assert set(plain) == {"rays", "rgbs"}


# ---- 3. two epochs, eager ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,last", [(64, "partial"), (80, "partial"), (80, "drop")])
def test_two_epoch_walk(dev, B, last):
    st = _store(dev)
    n = st.n_pixels
    s = st.epoch_sampler(B, seed=4, last=last)
    epochs = []
    for e in range(2):
        seen = []
        for k in range(s.steps_per_epoch):
            assert (s.epoch, s.cursor) == (e, k)
            b = s.sample(return_ids=True)
            assert s.epoch_done == (k == s.steps_per_epoch - 1)
            assert _device_state(s) == (s.epoch, s.cursor)              # the host mirror never read the device: it counted
            assert b["ids"].shape[0] == b["rays"].shape[0] == b["rgbs"].shape[0] == s.rows(k)
            seen.append(b["ids"].cpu().numpy())
        ids = np.concatenate(seen)
        assert len(np.unique(ids)) == len(ids)                          # within an epoch: every ray at most once
        if last == "partial":
            assert np.array_equal(np.sort(ids), np.arange(n))
            assert len(seen[-1]) == (n % B or B)
        else:
            assert len(ids) == n - n % B
            missing = np.setdiff1d(np.arange(n), ids)
            from nerf_pl_amd import ops
            assert np.array_equal(np.sort(ops.epoch_ids_host(4, e, n)[n - n % B:]), missing)    # exactly the permutation's tail
        epochs.append(ids)
    assert (s.epoch, s.cursor) == (2, 0)
    assert not np.array_equal(epochs[0], epochs[1])
    if B == 80 and last == "partial":
        assert len(seen[-1]) == 32


# ---- 4. captured -----------------------------------------------------------------------------------------------------------------
def test_captured_sampler_walks_through_epochs(dev):
    from nerf_pl_amd._lib import NerfHipError
    st = _store(dev)
    s = st.epoch_sampler(64, seed=5).prepare()
    bad = st.epoch_sampler(80, seed=5).prepare()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        b = s.sample(return_ids=True)
        with pytest.raises(NerfHipError):
            bad.sample()                       # a partial last batch: refused before anything is launched
    torch.cuda.synchronize()
    assert (s.epoch, s.cursor) == (0, 0) and _device_state(s) == (0, 0)    # capturing ran nothing
    assert _device_state(bad) == (0, 0)
    for k in range(7):                         # 3 batches per epoch: the replays cross two epoch boundaries
        g.replay()
        s.replayed()
        torch.cuda.synchronize()
        epoch, cursor = divmod(k, 3)
        assert np.array_equal(b["ids"].cpu().numpy(), _host_ids(s, epoch, cursor)), k
        rays, rgbs = _sample_batch(st, b["ids"])
        assert torch.equal(b["rays"], rays) and torch.equal(b["rgbs"], rgbs)
        assert _device_state(s) == (s.epoch, s.cursor) == divmod(k + 1, 3)
        assert s.epoch_done == (k % 3 == 2)
    nxt = s.sample(return_ids=True)             # an eager call continues where the replays stopped
    assert np.array_equal(nxt["ids"].cpu().numpy(), _host_ids(s, 2, 1)) and _device_state(s) == (2, 2)


# ---- 5. the Philox stream ----------------------------------------------------------------------------------------------------------
def test_sampler_leaves_the_generator_alone(dev):
    from nerf_pl_amd import draws as D
    st = _store(dev)
    S, N = 8, 8
    torch.manual_seed(4)
    torch.rand(5, device=dev)
    off = _gen(dev).get_offset()
    s = st.epoch_sampler(64)                               # seed=None: torch.initial_seed(), a read
    assert s.seed == 4
    s.sample()
    s.sample(return_ids=True)
    assert _gen(dev).get_offset() == off
    b = s.sample(step_draws=(S, N, 1.0, 1.0))
    off1 = _gen(dev).get_offset()
    torch.manual_seed(4)
    torch.rand(5, device=dev)
    keys, specs = D.step_specs(64, S, N, 1.0, 1.0)
    want = dict(zip(keys, D.draws(specs, dev)))
    assert _gen(dev).get_offset() == off1 and off1 > off
    assert set(b["draws"]) == set(keys)
    for k in keys:
        assert torch.equal(b["draws"][k], want[k]), k


def test_sampler_packs_the_models_with_the_draws(dev):
    from helpers import build_models
    from nerf_pl_amd import ops
    from nerf_pl_amd.models.nerf import pack_ticket
    st = _store(dev)
    models = build_models([O.make_params(5, 4.0, 0.2), O.make_params(6, 4.0, 0.2)], dev, "bf16")[0]
    want = [(a.clone(), b.clone()) for a, b in ops.pack_models_train(models, "bf16")]
    for with_draws in (True, False):
        for m in models:
            for buf in m.train_buffers("bf16", dev):
                buf.zero_()
        b = st.epoch_sampler(64, seed=1).sample(step_draws=(8, 8, 1.0, 0.0) if with_draws else None, pack_models=(models, "bf16"))
        assert b["packed"] == pack_ticket(models, "bf16") and ("draws" in b) == with_draws
        for m, (pf, pb) in zip(models, want):
            a, c = m.train_buffers("bf16", dev)
            assert torch.equal(a, pf) and torch.equal(c, pb)


# ---- 6. the graphed step ---------------------------------------------------------------------------------------------------------
def _system(dev, **over):
    from nerf_pl_amd.system import NeRFSystem
    kw = dict(N_samples=8, N_importance=8, use_disp=False, perturb=0.0, noise_std=0.0, chunk=1024 * 32, loss_type="mse", lr=5e-4,
              weight_decay=0, decay_step=[100], decay_gamma=0.5, white_back=True)
    kw.update(over)
    system = NeRFSystem(Namespace(**kw))
    system.nerf_coarse.load_state_dict(O.make_params(5, 4.0, 0.2))
    system.nerf_fine.load_state_dict(O.make_params(6, 4.0, 0.2))
    for m in system.models:
        m.mlp_dtype = "bf16"
    return system.to(dev)


def test_graphed_step_with_the_sampler_equals_eager_fit(dev):
    """GraphedTrainStep(batch_source=sampler.sample), warm-up 3 then 6 replays = 3 epochs of 3 batches, against the same 9 batches
    fed eagerly through fit.  Tolerance: rtol 1e-5, atol 1e-7 — what tests/test_gpu_training.py
    (test_graphed_train_step_equals_eager) asks of graph against eager; perturb = noise_std = 0, no draw enters the math."""
    from nerf_pl_amd.system import GraphedTrainStep, fit
    st = _store(dev)
    system = _system(dev)
    (opt,), _ = system.configure_optimizers()
    s = st.epoch_sampler(64, seed=9)
    stepper = GraphedTrainStep(system, opt, warmup=3, batch_source=s.sample)
    losses = [stepper()["loss"].item() for _ in range(9)]
    torch.cuda.synchronize()
    assert stepper.graph is not None and all(np.isfinite(losses))
    assert (s.epoch, s.cursor) == (3, 0) and s.epoch_done and _device_state(s) == (3, 0)

    eager = _system(dev)
    s2 = st.epoch_sampler(64, seed=9)
    batches = [s2.sample() for _ in range(9)]
    want = [float(x) for x in fit(eager, batches)]
    assert losses == pytest.approx(want, rel=1e-5)
    got_sd, want_sd = system.state_dict(), eager.state_dict()
    for k in want_sd:
        assert torch.allclose(got_sd[k], want_sd[k], rtol=1e-5, atol=1e-7), k


def test_source_carries_the_steps_draws_and_hears_replays(dev):
    """sampler.source(step_draws=..., pack_models=...) as the batch source: the step consumes batch['draws'] / batch['packed'], and
    the mirror follows the replays (it equals the device state after warm-up 2 + 3 replays, across an epoch boundary)."""
    from nerf_pl_amd.system import GraphedTrainStep
    st = _store(dev)
    system = _system(dev, perturb=1.0)
    (opt,), _ = system.configure_optimizers()
    s = st.epoch_sampler(64, seed=9)
    src = s.source(step_draws=(8, 8, 1.0, 0.0), pack_models=(system.models, "bf16"))
    assert {"rays", "rgbs", "draws", "packed"} <= set(src()) and (s.epoch, s.cursor) == (0, 1)
    stepper = GraphedTrainStep(system, opt, warmup=2, batch_source=src)
    losses = [stepper()["loss"].item() for _ in range(5)]
    torch.cuda.synchronize()
    assert stepper.graph is not None and all(np.isfinite(losses))
    assert (s.epoch, s.cursor) == (2, 0) == _device_state(s)


# ---- 7. fit_epochs ---------------------------------------------------------------------------------------------------------------
def test_fit_epochs_steps_the_scheduler_once_per_epoch(dev):
    from nerf_pl_amd.system import fit_epochs
    st = _store(dev)
    system = _system(dev, decay_step=[1], decay_gamma=0.5)
    lrs = []
    inner = system.training_step

    def recording_step(batch, nb):
        out = inner(batch, nb)
        lrs.append(out["log"]["lr"])
        return out
    system.training_step = recording_step
    s = st.epoch_sampler(64, seed=2)
    epochs = fit_epochs(system, s, 2)
    assert [len(e) for e in epochs] == [3, 3] and (s.epoch, s.cursor) == (2, 0)
    assert all(bool(torch.isfinite(x)) for e in epochs for x in e)
    assert lrs[:3] == [5e-4] * 3
    assert lrs[3:] == pytest.approx([0.5 * 5e-4] * 3, rel=1e-12)


# ---- 8. resume -------------------------------------------------------------------------------------------------------------------
def test_resume_inside_an_epoch(dev):
    st = _store(dev, 5, 13)
    a = st.epoch_sampler(64, seed=6, last="partial")
    for _ in range(5):                          # 4 batches per epoch: one batch into epoch 1
        a.sample()
    sd = a.state_dict()
    assert (sd["epoch"], sd["cursor"]) == (1, 1)
    b = st.epoch_sampler(64, seed=0, last="partial")
    b.sample()                                  # a sampler that has already run is reloaded, device state included
    b.load_state_dict(sd)
    for _ in range(5):
        x, y = a.sample(return_ids=True), b.sample(return_ids=True)
        assert torch.equal(x["ids"], y["ids"]) and torch.equal(x["rays"], y["rays"]) and torch.equal(x["rgbs"], y["rgbs"])
        assert (a.epoch, a.cursor, a.epoch_done) == (b.epoch, b.cursor, b.epoch_done) and _device_state(b) == (b.epoch, b.cursor)

"""CPU: the epoch shuffle (csrc/epoch_core.h) through its host entry nerfhip_epoch_ids_host — a bijection for every
key, bit-equal to the numpy restatement tests/epoch_ref.py, statistically a shuffle (the same statistics put numpy's own
permutations through inside the tests), DistributedSampler's rank split, the argument checks, and EpochSampler's host arithmetic."""
import ctypes
import types

import numpy as np
import pytest

import epoch_ref as E

SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 4097, 65536, 65537, 1000003)
SEEDS = (0, 0x5EED5EED, 2 ** 64 - 1)
EPOCHS = (0, 1, 4095)


@pytest.fixture(scope="module")
def ops():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import ops
    return ops


@pytest.fixture(scope="module")
def lib(ops):
    from nerf_pl_amd import _lib
    return _lib.load()


# ---- 1. bijection, the reference, slices -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_bijection_and_reference(ops, n):
    for seed in SEEDS:
        for epoch in EPOCHS:
            ids = ops.epoch_ids_host(seed, epoch, n)
            assert ids.dtype == np.int64 and ids.shape == (n,)
            assert np.array_equal(np.sort(ids), np.arange(n)), (n, seed, epoch)
            assert np.array_equal(ids, E.rank_ids(seed, epoch, n)), (n, seed, epoch)


@pytest.mark.parametrize("n", (5, 257, 65537))
def test_slices_are_slices_of_the_whole(ops, n):
    whole = ops.epoch_ids_host(11, 3, n)
    for first, count in ((0, 0), (0, 1), (n - 1, 1), (n // 3, n // 2), (n, 0), (1, n - 1)):
        assert np.array_equal(ops.epoch_ids_host(11, 3, n, first=first, count=count), whole[first:first + count]), (n, first, count)


def test_large_domain_matches_the_reference(ops):
    """64-bit ids: a slice of n = 2^40 and of the first loader scene's 100 x 800 x 800 rays."""
    for n, first in ((1 << 40, (1 << 40) - 700), (100 * 800 * 800, 12345678)):
        got = ops.epoch_ids_host(9, 2, n, first=first, count=700)
        assert np.array_equal(got, E.rank_ids(9, 2, n, first=first, count=700))
        assert got.min() >= 0 and got.max() < n and len(np.unique(got)) == 700


# ---- 2. keys matter ----------------------------------------------------------------------------------------------------------
def test_epoch_and_seed_change_the_permutation(ops):
    n = 65537
    base = ops.epoch_ids_host(1, 0, n)
    for other in (ops.epoch_ids_host(1, 1, n), ops.epoch_ids_host(2, 0, n)):
        assert int((base == other).sum()) < 20                 # two independent permutations agree at 1 position on average


# ---- 3. marginal uniformity --------------------------------------------------------------------------------------------------
CHI2_225 = (138.1, 340.6)        # the 1e-6 and 1 - 1e-6 quantiles of chi^2 with 15 x 15 = 225 degrees of freedom


def _cell_statistic(perms, n):
    cells = np.zeros((16, 16))
    pos = np.arange(n) * 16 // n
    for ids in perms:
        np.add.at(cells, (pos, ids * 16 // n), 1)
    expect = cells.sum() / 256
    return float(((cells - expect) ** 2 / expect).sum())


def test_marginals_are_uniform(ops):
    """Over 4096 epochs of one seed, (position, id) falls into 16 x 16 equal cells like a uniform permutation's: Pearson's statistic
    follows chi^2(225) (row and column sums are fixed).  numpy's permutations pass the same code here."""
    n, epochs = 1024, 4096
    rng = np.random.default_rng(1)
    control = _cell_statistic((rng.permutation(n) for _ in range(epochs)), n)
    print("numpy", control)
    assert CHI2_225[0] < control < CHI2_225[1]
    ours = _cell_statistic((ops.epoch_ids_host(7, e, n) for e in range(epochs)), n)
    print("epoch_perm", ours)
    assert CHI2_225[0] < ours < CHI2_225[1]


# ---- 4. neighbours are independent -------------------------------------------------------------------------------------------
def _neighbour_statistic(ids):
    x = ids.astype(np.float64)
    return abs(np.corrcoef(x[:-1], x[1:])[0, 1]) * np.sqrt(len(x))


def test_neighbouring_positions_are_uncorrelated(ops):
    """|corr(ids[:-1], ids[1:])| sqrt(n) is |N(0,1)| under independence: P(> 5) = 6e-7 per epoch."""
    n = 65537
    rng = np.random.default_rng(1)
    control = max(_neighbour_statistic(rng.permutation(n)) for _ in range(64))
    worst = max(_neighbour_statistic(ops.epoch_ids_host(7, e, n)) for e in range(64))
    print("numpy", control, "epoch_perm", worst)
    assert control < 5 and worst < 5
    two_rounds = max(_neighbour_statistic(E.perm(7, e, n, np.arange(n), rounds=2)) for e in range(8))
    assert two_rounds > 5                                      # the statistic tells a weak network from a shuffle


# ---- 5. batches mix images ---------------------------------------------------------------------------------------------------
def test_batches_touch_nearly_every_image(ops):
    hw = 640000
    ids = ops.epoch_ids_host(7, 0, 100 * hw, first=0, count=65536)
    for k in range(64):
        images = np.unique(ids[k * 1024:(k + 1) * 1024] // hw)
        assert len(images) >= 95, (k, len(images))


# ---- 6. ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,world", [(65537, 2), (195, 3)])
def test_ranks_split_an_epoch_as_distributed_sampler(ops, n, world):
    share = -(-n // world)
    whole = ops.epoch_ids_host(5, 1, n)
    ranks = [ops.epoch_ids_host(5, 1, n, rank=r, world=world) for r in range(world)]
    for r, ids in enumerate(ranks):
        assert ids.shape == (share,)
        assert np.array_equal(ids, whole[(np.arange(share) * world + r) % n])
    joined = np.concatenate(ranks)
    values, counts = np.unique(joined, return_counts=True)
    assert np.array_equal(values, np.arange(n))
    assert int((counts == 2).sum()) == share * world - n and counts.max() <= 2        # the padding: 1 id twice (n = 65537), 0 (195)
    if n == 65537:
        assert share == 32769 and int((counts == 2).sum()) == 1


# ---- 7. bad arguments --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(lib):
    BADARG = -1
    buf = np.zeros(16, np.int64)
    out = buf.ctypes.data

    def host(n=10, rank=0, world=1, first=0, count=4, p=out):
        return lib.nerfhip_epoch_ids_host(1, 0, n, rank, world, first, count, p)

    def dev(n=10, rank=0, world=1, first=0, count=4, p=out):           # (refused before anything is launched: no GPU needed)
        return lib.nerfhip_epoch_ids(1, 0, n, rank, world, first, count, p, None)
    assert host() == 0
    for call in (host, dev):
        assert call(n=0) == BADARG and call(n=-3) == BADARG and call(n=(1 << 40) + 1) == BADARG
        assert call(world=0) == BADARG
        assert call(rank=-1) == BADARG and call(rank=1) == BADARG and call(rank=2, world=2) == BADARG
        assert call(first=-1) == BADARG and call(count=-1) == BADARG
        assert call(first=8, count=3) == BADARG                    # past the share of 10
        assert call(world=2, first=3, count=3) == BADARG           # past rank 0's share of 5
        assert call(p=None) == BADARG
        assert call(p=out + 4) == BADARG                           # int64 ids on a 4-byte boundary
    assert host(first=6, count=4) == 0 and host(world=2, first=1, count=4) == 0

    from nerf_pl_amd import _lib
    fake = 0x10000                                                  # never dereferenced: every call below returns from the checks
    rb = _lib.RayBatch()

    def batch(n=192, B=64, rank=0, world=1, drop=0, state=fake, ids=None, rb_ptr=None, **fields):
        rb.c2w, rb.rgbs_all, rb.rays, rb.rgbs, rb.H, rb.W = fake, fake, fake, fake, 8, 8
        for k, v in fields.items():
            setattr(rb, k, v)
        return lib.nerfhip_epoch_batch(ctypes.addressof(rb) if rb_ptr is None else rb_ptr, n, B, rank, world, drop, state, ids, None)
    assert batch(n=0) == BADARG and batch(world=0) == BADARG and batch(rank=1) == BADARG and batch(rank=-1) == BADARG
    assert batch(B=0) == BADARG and batch(B=-64) == BADARG
    assert batch(B=193, drop=1) == BADARG                           # nothing left after dropping the only batch
    assert batch(state=None) == BADARG and batch(state=fake + 4) == BADARG
    assert batch(ids=fake + 4) == BADARG
    for field in ("c2w", "rgbs_all", "rays", "rgbs"):
        assert batch(**{field: None}) == BADARG, field
        assert batch(**{field: fake + 2}) == BADARG, field
    assert batch(rays=fake + 8) == BADARG                           # rays rows are written as 16-byte vectors
    assert batch(H=0) == BADARG


# ---- 8. the sampler's host arithmetic ----------------------------------------------------------------------------------------
def _sampler(n, B, world=1, last="partial", rank=0, seed=3):
    from nerf_pl_amd.rays import EpochSampler
    return EpochSampler(types.SimpleNamespace(n_pixels=n), B, seed=seed, rank=rank, world=world, last=last)


def test_sampler_steps_per_epoch():
    for last in ("partial", "drop"):
        s = _sampler(192, 64, last=last)
        assert (s.n_rank, s.steps_per_epoch, s.rows(2)) == (192, 3, 64)
        s = _sampler(195, 64, world=2, last=last, rank=1)
        assert s.n_rank == 98 and s.steps_per_epoch == (2 if last == "partial" else 1)
    s = _sampler(192, 80)
    assert s.steps_per_epoch == 3 and s.rows(0) == 80 and s.rows(2) == 32
    s = _sampler(192, 80, last="drop")
    assert s.steps_per_epoch == 2 and s.rows(1) == 80
    assert _sampler(195, 64, world=2).rows(1) == 34
    for bad in (dict(B=0), dict(world=0), dict(rank=1), dict(last="pad"), dict(B=193, last="drop")):
        kw = dict(n=192, B=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            _sampler(**kw)


def test_sampler_mirror_and_state_dict_round_trip():
    s = _sampler(192, 80, seed=2 ** 64 - 5)
    seen = []
    for _ in range(7):
        s.replayed()                                               # the mirror counts; nothing is launched
        seen.append((s.epoch, s.cursor, s.epoch_done))
    assert seen == [(0, 1, False), (0, 2, False), (1, 0, True), (1, 1, False), (1, 2, False), (2, 0, True), (2, 1, False)]
    sd = s.state_dict()
    assert sd == {"seed": 2 ** 64 - 5, "epoch": 2, "cursor": 1, "rank": 0, "world": 1, "batch_size": 80, "last": "partial"}
    t = _sampler(192, 80, seed=0)
    t.load_state_dict(sd)
    assert t.state_dict() == sd and not t.epoch_done
    with pytest.raises(ValueError):
        _sampler(192, 64).load_state_dict(sd)                      # another batch size: the cursor means nothing
    with pytest.raises(ValueError):
        t.load_state_dict(dict(sd, cursor=3))


def test_default_seed_reads_torch_initial_seed_without_drawing():
    import torch
    torch.manual_seed(1234)
    before = torch.get_rng_state()
    s = _sampler(192, 64, seed=None)
    assert s.seed == 1234 and torch.equal(torch.get_rng_state(), before)


def test_abi_is_additive(lib):
    assert lib.nerfhip_abi_version() == 3

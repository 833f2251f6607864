"""CPU: the two small protocols of the training step's Python state, through the calls the product itself makes.

Weight-image freshness (models/nerf.py): whether packed MFMA weight images still belong to the current weights — the ticket an
ahead-of-step pack hands to the fused training node, and the serial a backward must find.  A wrong answer trains on old weights
and reports nothing.  Gradient hand-off (models/mlp_autograd.py): what a backward does with complete flat gradient buffers.
Nothing here launches anything."""
import gc

import pytest
import torch

from nerf_pl_amd.models import NeRF
from nerf_pl_amd.models.mlp_autograd import flat_grad, grad_hooks, grads_ready, set_grad_hooks
from nerf_pl_amd.models.nerf import pack_ticket, ticket_fresh


class _Opt:                      # stands in for optim.FlatAdam (which needs a GPU): what matters is that it can be weakly referenced
    pass


def _packed_pair(dtype="bf16"):
    """a coarse / fine pair under a live announcing optimizer, images just packed -> (models, optimizer, ticket)"""
    models, opt = [NeRF(), NeRF()], _Opt()
    for m in models:
        m.announced_by(opt)
        m.images_packed()
    return models, opt, pack_ticket(models, dtype)


def test_ahead_of_step_ticket_freshness_table():
    """Fresh iff the ticket names the same models in the same order and the same dtype, and every model has a live announcing
    optimizer, its weights' serial == the ticket's, and its packed serial == the ticket's."""
    models, opt, ticket = _packed_pair()
    assert ticket_fresh(ticket, models, "bf16")                                  # just packed under a live announcer

    bare = [NeRF(), NeRF()]
    for m in bare:
        m.images_packed()
    assert not ticket_fresh(pack_ticket(bare, "bf16"), bare, "bf16")             # no announcer

    assert not ticket_fresh(ticket, models, "fp32")                              # other dtype
    assert not ticket_fresh(ticket, models[::-1], "bf16")                        # models swapped
    other = NeRF()
    other.announced_by(opt)
    other.images_packed()
    assert not ticket_fresh(ticket, [models[0], other], "bf16")                  # another model
    assert not ticket_fresh(ticket, models[:1], "bf16")
    assert not ticket_fresh(None, models, "bf16")                                # ticket None

    for m in models:                                                             # a later forward re-packed identical images
        m.images_packed()
    assert ticket_fresh(ticket, models, "bf16")

    models[1].weights_changed()                                                  # "weights changed" after the pack
    assert not ticket_fresh(ticket, models, "bf16")
    models[1].images_packed()                                                    # ... then re-packed: both serials moved on,
    assert not ticket_fresh(ticket, models, "bf16")                              # the ticket did not
    assert ticket_fresh(pack_ticket(models, "bf16"), models, "bf16")

    models, opt, ticket = _packed_pair()
    models[0].load_state_dict(NeRF().state_dict())                               # load_state_dict after the pack
    assert not ticket_fresh(ticket, models, "bf16")

    models, opt, ticket = _packed_pair()
    del opt
    gc.collect()
    assert not ticket_fresh(ticket, models, "bf16")                              # announcer collected


def test_backward_finds_the_serial_its_forward_packed_or_raises():
    m = NeRF()
    m.images_packed()
    serial = m.pack_serial()
    m.check_pack_serial(serial)                                                  # the serial taken at forward time passes
    m.images_packed()                                                            # a later forward, same weights: identical images
    m.check_pack_serial(serial)
    m.weights_changed()
    m.check_pack_serial(serial)                                                  # an update alone leaves the images alone
    m.images_packed()                                                            # a later forward packed the UPDATED weights
    with pytest.raises(RuntimeError, match="re-packed from UPDATED weights by a later training forward"):
        m.check_pack_serial(serial)
    m.check_pack_serial(m.pack_serial())

    never = NeRF()
    assert never.pack_serial() is None
    for s in (0, 1, None):
        with pytest.raises(RuntimeError, match="re-packed from UPDATED weights"):
            never.check_pack_serial(s)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(2, 2)


class _Recorder:
    def __init__(self):
        self.calls = []

    def one(self, model, flat):
        self.calls.append(("one", model, flat))

    def many(self, models, flats):
        self.calls.append(("many", list(models), list(flats)))


def _pair():
    return [_Tiny(), _Tiny()], [torch.zeros(3), torch.ones(3)]


def test_grads_ready_hand_off():
    # no hooks: buffers recorded, nothing called
    ms, fl = _pair()
    assert grad_hooks(ms) == (False, None) and flat_grad(ms[0]) is None
    grads_ready(ms, fl)
    assert flat_grad(ms[0]) is fl[0] and flat_grad(ms[1]) is fl[1]

    # one joint hook shared by all: called ONCE with all models and buffers
    ms, fl = _pair()
    r = _Recorder()
    for m in ms:
        set_grad_hooks(m, r.one, r.many)
    hooked, joint = grad_hooks(ms)
    assert hooked and joint == r.many
    grads_ready(ms, fl)
    assert r.calls == [("many", ms, fl)]
    assert flat_grad(ms[0]) is fl[0] and flat_grad(ms[1]) is fl[1]

    # distinct joint hooks: per-model hooks, each once
    ms, fl = _pair()
    ra, rb = _Recorder(), _Recorder()
    set_grad_hooks(ms[0], ra.one, ra.many)
    set_grad_hooks(ms[1], rb.one, rb.many)
    assert grad_hooks(ms) == (True, None)
    grads_ready(ms, fl)
    assert ra.calls == [("one", ms[0], fl[0])] and rb.calls == [("one", ms[1], fl[1])]
    assert flat_grad(ms[0]) is fl[0] and flat_grad(ms[1]) is fl[1]

    # missing joint hooks (GradSync(form="per_model")): per-model hooks, each once, in the models' order
    ms, fl = _pair()
    r = _Recorder()
    for m in ms:
        set_grad_hooks(m, r.one, None)
    assert grad_hooks(ms) == (True, None)
    grads_ready(ms, fl)
    assert r.calls == [("one", ms[0], fl[0]), ("one", ms[1], fl[1])]

    # a model with no hook among hooked ones: skipped, no exception, its buffer still recorded
    for hooked_k in (0, 1):
        ms, fl = _pair()
        r = _Recorder()
        set_grad_hooks(ms[hooked_k], r.one, r.many)
        assert grad_hooks(ms) == (True, None)
        grads_ready(ms, fl)
        assert r.calls == [("one", ms[hooked_k], fl[hooked_k])]
        assert flat_grad(ms[0]) is fl[0] and flat_grad(ms[1]) is fl[1]

"""autograd glue between nn.Module parameters and the fused HIP MLP kernels.

Training forward = the same fused kernel with `save_acts` (every layer's B-operand slabs written once,
in register order); backward = nerfhip_mlp_bwd.  Gradients flow to the 24 parameter tensors only:
the reference detaches the importance samples (rendering.py:226) and its rays carry no grad, so
d/d(rays, z) is never needed; d/dx of pre-embedded inputs (NeRF.forward called directly) comes from
nerfhip_mlp_dx_embedded."""
import torch

from .. import ops


# -- the gradient hand-off: what a backward leaves on a module for parallel.GradSync and optim's flat optimizers.  Plain attributes
# on any nn.Module (GradSync also serves modules that are not NeRF), named in this module only.
def set_grad_hooks(model, ready, joint):
    """ready(model, flat) / joint(models, flats), or None: what grads_ready calls for this model"""
    model._grad_ready_hook, model._grads_ready_hook = ready, joint


def clear_grad_hooks(model, ready, joint):
    """take back the hooks that are still `ready` / `joint` (another owner's stay)"""
    if getattr(model, "_grad_ready_hook", None) == ready:
        model._grad_ready_hook = None
    if getattr(model, "_grads_ready_hook", None) == joint:
        model._grads_ready_hook = None


def flat_grad(model):
    """the flat buffer the model's last backward wrote its gradients into (None: none yet, or since flat_grad_reset)"""
    return getattr(model, "_flat_grad", None)


def flat_grad_reset(model):
    model._flat_grad = None


def grad_hooks(models):
    """-> (any model has a grad-ready hook, the ONE joint hook all of them share or None): which of its three cases grads_ready will
    take — _TrainRender.backward chooses its launch groups by it ahead of its launches"""
    hooked = any(getattr(m, "_grad_ready_hook", None) is not None for m in models)
    joint = getattr(models[0], "_grads_ready_hook", None) if hooked else None
    shared = joint is not None and all(getattr(m, "_grads_ready_hook", None) == joint for m in models)
    return hooked, joint if shared else None


def grads_ready(models, flats):
    """A backward calls this when the flat gradient buffers `flats` of `models` are complete, before autograd hands their views to
    the parameters: records each model's buffer, then calls the joint hook ONCE if all share one, else each model's own where it
    has one (parallel.GradSync: the all-reduce starts while autograd keeps going)."""
    for m, flat in zip(models, flats):
        m._flat_grad = flat
    joint = grad_hooks(models)[1]
    if joint is not None:
        return joint(models, flats)
    for m, flat in zip(models, flats):
        if getattr(m, "_grad_ready_hook", None) is not None:
            m._grad_ready_hook(m, flat)


def _param_grads(model, out, acts, dtype, g_out, packed_bwd, workspace=None):
    """nerfhip_mlp_bwd (chain + dW + reduce kernels) -> gradients in `flat_params()` order.  `packed_bwd`: the W^T image the
    forward packed together with its own (NeRF.packed_weights_train)."""
    gw, gb, flat = ops.mlp_bwd(g_out, out, packed_bwd, acts, dtype, workspace=workspace)
    grads_ready([model], [flat])
    need = [p.requires_grad for p in model.flat_params()]
    return [g if nd else None for g, nd in zip(gw + gb, need)]


def _needs_grad(model):
    return torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())


class _MLPRays(torch.autograd.Function):
    """raw = MLP(posenc(o + d z), posenc(d)) for every sample of every ray (rendering.py:115-141)."""

    @staticmethod
    def forward(ctx, model, rays, z, *params):
        dtype = model.mlp_dtype
        acts = ops.alloc_acts(z.numel(), dtype, z.device)
        packed, packed_bwd = model.packed_weights_train(dtype)
        out = ops.mlp_fwd_rays(rays, z, packed, False, dtype, save=acts)
        ctx.model, ctx.dtype, ctx.acts, ctx.packed_bwd = model, dtype, acts, packed_bwd
        ctx.serial = model.pack_serial()
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (out,) = ctx.saved_tensors
        ctx.model.check_pack_serial(ctx.serial)
        grads = _param_grads(ctx.model, out, ctx.acts, ctx.dtype, g_out, ctx.packed_bwd)
        ctx.acts = ctx.packed_bwd = None
        return (None, None, None) + tuple(grads)


class _MLPEmbedded(torch.autograd.Function):
    """NeRF.forward on pre-embedded inputs (nerf.py:83-124)."""

    @staticmethod
    def forward(ctx, model, x, *params):
        dtype = model.mlp_dtype
        if dtype == "bf16_f8" and ctx.needs_input_grad[1]:
            # d/dx needs dY of three layers at full bf16 precision (nerfhip_mlp_dx_embedded); the 8-bit mode keeps dY only as
            # e5m2 copies for the dW GEMM.  Same bf16 MFMA forward and chain: this call simply saves its tensors in bf16.
            dtype = "bf16"
        acts = ops.alloc_acts(x.shape[0], dtype, x.device)
        packed, packed_bwd = model.packed_weights_train(dtype)
        out = ops.mlp_fwd_embedded(x, packed, False, dtype, save=acts)
        ctx.model, ctx.dtype, ctx.acts, ctx.packed_bwd = model, dtype, acts, packed_bwd
        ctx.serial = model.pack_serial()
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (out,) = ctx.saved_tensors
        ctx.model.check_pack_serial(ctx.serial)
        ws = {} if ctx.needs_input_grad[1] else None
        grads = _param_grads(ctx.model, out, ctx.acts, ctx.dtype, g_out, ctx.packed_bwd, workspace=ws)
        ctx.acts = ctx.packed_bwd = None
        gx = None
        if ctx.needs_input_grad[1]:          # nerf.py:100-124 is differentiable w.r.t. x: dx from the chain's dY slabs
            m = ctx.model
            gx = ops.mlp_dx_embedded(ws["dys"], out.shape[0], m.xyz_encoding_1[0].weight, m.xyz_encoding_5[0].weight,
                                     m.dir_encoding[0].weight, ctx.dtype)
        return (None, gx) + tuple(grads)


def mlp_rays(model, rays, z, sigma_only):
    if _needs_grad(model):
        out = _MLPRays.apply(model, rays, z, *model.flat_params())
        # sigma_only under grad (render_rays(test_time=True) outside no_grad): the reference's sigma-only forward is
        # differentiable (nerf.py:103-114), so evaluate the full network and keep the density channel; the colour
        # branch then simply receives zero gradient.
        return out[..., 3] if sigma_only else out
    return ops.mlp_fwd_rays(rays, z, model.packed_weights(), sigma_only, model.mlp_dtype)


def mlp_embedded(model, x, sigma_only):
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1]).float()
    if _needs_grad(model) or (torch.is_grad_enabled() and x2.requires_grad):
        if sigma_only:
            # differentiable sigma-only forward (nerf.py:103-114): full network on [xyz | 0 direction channels], density
            # channel kept; colour-branch parameters get zero gradient
            if x2.shape[1] != model.in_channels_xyz:
                raise ValueError("NeRF.forward expects %d input channels, got %d" % (model.in_channels_xyz, x2.shape[1]))
            x2 = torch.cat([x2, x2.new_zeros(x2.shape[0], model.in_channels_dir)], 1)
            out = _MLPEmbedded.apply(model, x2, *model.flat_params())[:, 3:4]
        else:
            out = _MLPEmbedded.apply(model, x2, *model.flat_params())
    else:
        out = ops.mlp_fwd_embedded(x2, model.packed_weights(), sigma_only, model.mlp_dtype)
    return out.reshape(*lead, out.shape[-1])

"""Python-side operators over libnerfhip's C ABI (include/nerfhip.h).

Each function allocates its outputs with torch (torch owns all HBM), passes raw device pointers +
the current HIP stream through ctypes, and raises `NerfHipError` on any non-zero return.  There is
no CPU path and no eager-PyTorch fallback: tensors must live on an MI355X.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import BF16, BF16_F8, F32, NerfHipError, check, device_guard, ptr, require_gpu, stream_ptr

# 'bf16_f8': bf16 MFMA forward and dX chain; the tensors saved for the weight-gradient GEMM (activations, dY) are stored
# block-scaled in 8 bits (activations: e4m3, dY: e5m2) and consumed by the MX-scaled fp8 MFMA (include/nerfhip.h: NERFHIP_BF16_F8)
_DTYPES = {"fp32": F32, "f32": F32, "float32": F32, torch.float32: F32, F32: F32,
           "bf16": BF16, "bfloat16": BF16, torch.bfloat16: BF16, "bf16_f8": BF16_F8}


def mlp_dtype_code(d):
    if isinstance(d, bool) or d not in _DTYPES:
        raise ValueError("mlp dtype must be 'fp32', 'bf16' or 'bf16_f8', got %r" % (d,))
    return _DTYPES[d]


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------- argument rules shared by the operators
# Each helper returns the (contiguous) TENSOR, never only its pointer: the caller keeps it alive across the C call.
def _check_draw(op, name, t, numel):
    """caller-supplied draw tensors (batch['draws'] may have been made for other hyper-parameters): a wrong size would be an
    out-of-bounds device read, not an error"""
    if t is not None and (t.numel() != numel or t.dtype != torch.float32):
        raise ValueError("%s: %s must hold %d fp32 draws, got %s %s" % (op, name, numel, tuple(t.shape), t.dtype))


def _noise_arg(op, name, noise, noise_std, numel):
    """rendering.py:152-153: noise_std == 0 means no noise, whatever was drawn; else `numel` fp32 draws (or None)"""
    if noise_std == 0 or noise is None:
        return None
    noise = _c(noise)
    _check_draw(op, name, noise, numel)
    return noise


def _u_arg(op, u, B, K):
    """sample_pdf's uniforms: None (deterministic linspace), (K,) shared by every ray, or (B,K).  Returns (u, row stride)."""
    if u is None:
        return None, 0
    if tuple(u.shape) not in ((B, K), (K,)) or u.dtype != torch.float32:
        raise ValueError("%s: u must be (N_importance,) or (B, N_importance) = (%d, %d) fp32, got %s %s"
                         % (op, B, K, tuple(u.shape), u.dtype))
    return _c(u), (K if u.dim() == 2 else 0)


def _perturb_arg(op, perturb, perturb_rand, numel):
    """rendering.py:199-204: the B*S uniforms are read only when perturb > 0, and are needed then"""
    if not perturb > 0:
        return None
    if perturb_rand is None:
        raise ValueError("%s: perturb>0 needs perturb_rand" % op)
    perturb_rand = _c(perturb_rand)
    _check_draw(op, "perturb_rand", perturb_rand, numel)
    return perturb_rand


def _train_composite_args(op, raw, z, rays, target):
    """contiguous (raw (B,S,4), z (B,S), rays, target (B,3)) of the composite_train* operators + B, S"""
    raw, z, rays, target = _c(raw), _c(z), _c(rays), _c(target)
    B, S = z.shape
    if raw.numel() != B * S * 4 or target.numel() != B * 3:
        raise ValueError("%s: raw must be (B,S,4) and target (B,3)" % op)
    return raw, z, rays, target, B, S


def _train_composite_outs(B, S, dev):
    """(opacity (B,), rgb (B,3), depth (B,), g_raw (B,S,4)) that every composite_train* launch writes"""
    f32 = dict(device=dev, dtype=torch.float32)
    return torch.empty(B, **f32), torch.empty(B, 3, **f32), torch.empty(B, **f32), torch.empty(B, S, 4, **f32)


# ticket words of the arrival-ticket kernels (composite_train_loss, render_train_fwd)
_TICKETS = {}
_CAPTURES = {}
_EAGER_SLOTS = {}
_TICKET_WORDS = 1024


def _ticket(device):
    """One zero-initialised device word for the arrival-ticket kernels (they leave it at zero).  Eager launches on one stream are
    ordered and share the word of their (GPU, stream).  A hipGraph is different: it is replayed on whatever stream is current then,
    so two graphs CAPTURED on one stream may run concurrently — every capture therefore gets a word of its own: a new
    capture is recognised by the stream's capture status going from "none" to "active" between two calls.
    Known defect, left as it is here: captures on different streams can share a slot (first finding)."""
    st = torch.cuda.current_stream(device)
    capturing = torch.cuda.is_current_stream_capturing()
    rec = _CAPTURES.setdefault((device.index, st.stream_id), [False, 0])
    if capturing and not rec[0]:
        rec[1] += 1
    rec[0] = capturing
    pool = _TICKETS.get(device.index)
    if pool is None:
        if capturing:
            raise NerfHipError("the ticket words of this GPU must exist before a capture: run the step once eagerly first")
        pool = _TICKETS[device.index] = torch.zeros(_TICKET_WORDS * 4, device=device, dtype=torch.int32)
    # slots 0..31: eager use, one per stream in order of first use; 32..: captures, in order (16-byte pitch)
    if capturing:
        slot = 32 + rec[1] % (_TICKET_WORDS - 32)
    else:
        slot = _EAGER_SLOTS.setdefault((device.index, st.stream_id), len([k for k in _EAGER_SLOTS if k[0] == device.index]) % 32)
    return pool[4 * slot:4 * slot + 4]


# ------------------------------------------------------------------------------- posenc (a2)
class _PosEnc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_freqs, bands):
        require_gpu(x, bands)
        x = _c(x)
        n, C = x.shape
        out = torch.empty(n, C * (2 * n_freqs + 1), device=x.device, dtype=torch.float32)
        check(_lib.load().nerfhip_posenc_bands(ptr(x), ptr(bands), ptr(out), n, C, n_freqs, stream_ptr()), "nerfhip_posenc")
        ctx.save_for_backward(x)
        ctx.n_freqs, ctx.bands = n_freqs, bands
        return out

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        gout = _c(gout.float())
        gx = torch.empty_like(x)
        n, C = x.shape
        check(_lib.load().nerfhip_posenc_bands_bwd(ptr(x), ptr(ctx.bands), ptr(gout), ptr(gx), n, C, ctx.n_freqs, stream_ptr()),
              "nerfhip_posenc_bwd")
        return gx, None, None


@device_guard
def posenc(x, n_freqs, bands=None):
    """Embedding.forward (reference models/nerf.py:21-38). x (n,C) -> (n, C(2F+1)).
    bands None: the logscale bands 2^k; else a device tensor of n_freqs frequency bands (`logscale=False`, nerf.py:16-19)."""
    if x.dim() != 2:
        raise ValueError("posenc expects (n, C)")
    if bands is not None:
        if bands.numel() != int(n_freqs):
            raise ValueError("posenc: need one band per frequency")
        bands = bands.to(x.device, torch.float32).contiguous()
    return _PosEnc.apply(x, int(n_freqs), bands)


# ------------------------------------------------------------------------------- sampling (a5, a8-a10)
@device_guard
def sample_coarse_z(rays, n_samples, use_disp=False, perturb=0.0, perturb_rand=None):
    """rendering.py:183-204.  rays (B,8) -> z (B,S)."""
    require_gpu(rays, perturb_rand)
    rays = _c(rays)
    B = rays.shape[0]
    perturb_rand = _perturb_arg("sample_coarse_z", perturb, perturb_rand, B * n_samples)
    z = torch.empty(B, n_samples, device=rays.device, dtype=torch.float32)
    check(_lib.load().nerfhip_sample_coarse_z(ptr(rays), ptr(perturb_rand), ptr(z), B, n_samples, int(bool(use_disp)),
                                              float(perturb), stream_ptr()), "nerfhip_sample_coarse_z")
    return z


@device_guard
def searchsorted(a, v, out=None, side="left"):
    """Drop-in for torchsearchsorted.searchsorted (reference models/rendering.py:2,42): batched
    row-wise numpy-style searchsorted; a (B,M), v (B,K) float32 -> int64 (B,K).  Like the extension, `a` or `v` may have ONE
    row, which then serves every row of the other (the reference itself never uses that form: rendering.py:42)."""
    require_gpu(a, v)
    if side not in ("left", "right"):
        raise ValueError("side must be 'left' or 'right'")
    if a.dim() != 2 or v.dim() != 2 or not (a.shape[0] == v.shape[0] or a.shape[0] == 1 or v.shape[0] == 1):
        raise ValueError("searchsorted expects a (B,M) and v (B,K), or one of them with a single row")
    rows = max(a.shape[0], v.shape[0])
    a, v = _c(a.expand(rows, a.shape[1])), _c(v.expand(rows, v.shape[1]))
    B, M = a.shape
    K = v.shape[1]
    if out is None:
        out = torch.empty(B, K, device=a.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or not out.is_contiguous() or tuple(out.shape) != (B, K):
        raise ValueError("out must be a contiguous int64 (B,K) tensor")
    fn = _lib.load().nerfhip_searchsorted_right if side == "right" else _lib.load().nerfhip_searchsorted_left
    check(fn(ptr(a), ptr(v), ptr(out), B, M, K, stream_ptr()), "nerfhip_searchsorted_" + side)
    return out


# Rounding of sample_pdf's normaliser `torch.sum(weights, -1)` (rendering.py:30; include/nerfhip.h NERFHIP_ROW_TOTAL_*):
#   "aten"  (default) the reference's own bits: ATen's fp32 addition order on a CPU.  The searchsorted indices of rendering.py:42
#           have knife edges on the last bit of this total; under this mode the (cdf, u) -> inds triples recorded at the
#           reference's call site are reproduced on EVERY element, and the fine model's gradients agree with the reference's to
#           ~1e-6 of each tensor's maximum instead of ~1e-2 (0.1-0.5 % of the fine samples land in another bin otherwise:
#           tests/test_gpu_training.py).  Costs ~30 dependent fp32 additions per ray.
#   "exact" the correctly rounded fp32 sum (host-independent); what the plain C entry points nerfhip_sample_pdf / nerfhip_fine_z use.
# Process-wide (every sample_pdf / fine_z / fused training launch reads it at call time); NERFHIP_ROW_TOTAL=exact in the environment.
_ROW_TOTAL_MODES = {"exact": 0, "aten": 1}
_row_total = _ROW_TOTAL_MODES[os.environ.get("NERFHIP_ROW_TOTAL", "aten")]


def set_row_total(mode):
    """Select the rounding of sample_pdf's row total: "exact" | "aten".  Returns the previous mode's name."""
    global _row_total
    prev = [k for k, v in _ROW_TOTAL_MODES.items() if v == _row_total][0]
    _row_total = _ROW_TOTAL_MODES[mode]
    return prev


@device_guard
def sample_pdf_u(bins, weights, n_importance, u=None, eps=1e-5, return_cdf_inds=False):
    """sample_pdf with explicit uniforms: u None -> deterministic linspace; (K,) or (B,K) otherwise.
    return_cdf_inds: also return the kernel's cdf (B,M+1) and searchsorted indices (B,K) int64 (rendering.py:31-42)."""
    require_gpu(bins, weights, u)
    if bins.stride(-1) != 1:
        bins = bins.contiguous()
    if weights.stride(-1) != 1:
        weights = weights.contiguous()
    B, M = weights.shape
    if bins.shape != (B, M + 1):
        raise ValueError("bins must be (N_rays, N_samples_+1)")
    u, u_stride = _u_arg("sample_pdf", u, B, n_importance)
    samples = torch.empty(B, n_importance, device=bins.device, dtype=torch.float32)
    cdf = torch.empty(B, M + 1, device=bins.device, dtype=torch.float32) if return_cdf_inds else None
    inds = torch.empty(B, n_importance, device=bins.device, dtype=torch.int64) if return_cdf_inds else None
    check(_lib.load().nerfhip_sample_pdf_ex(ptr(bins), bins.stride(0), ptr(weights), weights.stride(0), ptr(u), u_stride,
                                            ptr(samples), B, M, n_importance, float(eps), ptr(cdf), ptr(inds), _row_total,
                                            stream_ptr()),
          "nerfhip_sample_pdf")
    return (samples, cdf, inds) if return_cdf_inds else samples


@device_guard
def fine_z(z_coarse, w_coarse, n_importance, u=None, eps=1e-5, return_new=False, return_cdf_inds=False):
    """rendering.py:223-229 in one launch: z_fine = sort(cat(z_coarse, sample_pdf(z_mid, w[:,1:-1]))).
    return_cdf_inds: append the fused kernel's cdf (B,S-1) and searchsorted indices (B,N_i) to the result."""
    require_gpu(z_coarse, w_coarse, u)
    z_coarse, w_coarse = _c(z_coarse), _c(w_coarse)
    B, S = z_coarse.shape
    u, u_stride = _u_arg("fine_z", u, B, n_importance)
    zf = torch.empty(B, S + n_importance, device=z_coarse.device, dtype=torch.float32)
    zn = torch.empty(B, n_importance, device=z_coarse.device, dtype=torch.float32) if return_new else None
    cdf = torch.empty(B, S - 1, device=z_coarse.device, dtype=torch.float32) if return_cdf_inds else None
    inds = torch.empty(B, n_importance, device=z_coarse.device, dtype=torch.int64) if return_cdf_inds else None
    check(_lib.load().nerfhip_fine_z_ex(ptr(z_coarse), ptr(w_coarse), ptr(u), u_stride, ptr(zf), ptr(zn), B, S,
                                        n_importance, float(eps), ptr(cdf), ptr(inds), _row_total, stream_ptr()), "nerfhip_fine_z")
    out = (zf, zn) if return_new else (zf,)
    if return_cdf_inds:
        out = out + (cdf, inds)
    return out if len(out) > 1 else out[0]


# ------------------------------------------------------------------------------- compositing (a7)
class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, z, rays, noise, noise_std, white_back):
        require_gpu(raw, z, rays, noise)
        raw, z, rays = _c(raw), _c(z), _c(rays)
        B, S = z.shape
        raw_ch = 4 if raw.dim() == 3 else 1
        if raw.numel() != B * S * raw_ch:
            raise ValueError("raw must be (B,S,4) or (B,S)")
        if noise is not None:
            noise = _c(noise)
        dev = z.device
        weights = torch.empty(B, S, device=dev, dtype=torch.float32)
        opacity = torch.empty(B, device=dev, dtype=torch.float32)
        rgb = torch.empty(B, 3, device=dev, dtype=torch.float32) if raw_ch == 4 else None
        depth = torch.empty(B, device=dev, dtype=torch.float32) if raw_ch == 4 else None
        check(_lib.load().nerfhip_composite_fwd(ptr(raw), raw_ch, ptr(z), ptr(rays), ptr(noise), float(noise_std),
                                                int(bool(white_back)), ptr(weights), ptr(rgb), ptr(depth),
                                                ptr(opacity), B, S, stream_ptr()), "nerfhip_composite_fwd")
        ctx.save_for_backward(raw, z, rays, noise)
        ctx.cfg = (raw_ch, float(noise_std), int(bool(white_back)))
        ctx.set_materialize_grads(False)     # unused outputs (weights/depth/opacity) arrive as None, not as zero fills
        if raw_ch == 4:
            return weights, opacity, rgb, depth
        return weights, opacity

    @staticmethod
    def backward(ctx, g_weights, g_opacity, g_rgb=None, g_depth=None):
        raw, z, rays, noise = ctx.saved_tensors
        raw_ch, noise_std, white_back = ctx.cfg
        B, S = z.shape

        def prep(g):
            return None if g is None else _c(g.float())

        g_raw = torch.empty_like(raw)
        check(_lib.load().nerfhip_composite_bwd(ptr(raw), raw_ch, ptr(z), ptr(rays), ptr(noise), noise_std, white_back,
                                                ptr(prep(g_rgb)), ptr(prep(g_depth)), ptr(prep(g_opacity)),
                                                ptr(prep(g_weights)), ptr(g_raw), B, S, stream_ptr()),
              "nerfhip_composite_bwd")
        return g_raw, None, None, None, None, None


@device_guard
def composite(raw, z, rays, noise=None, noise_std=0.0, white_back=False):
    """Volume-rendering quadrature (rendering.py:143-172).
    raw (B,S,4) -> (weights, opacity, rgb, depth);  raw (B,S) sigma-only -> (weights, opacity)."""
    if noise_std == 0:
        noise = None
    return _Composite.apply(raw, z, rays, noise, float(noise_std), bool(white_back))


@device_guard
def composite_train(raw, z, rays, noise, noise_std, white_back, target, grad_scale, want_weights=True):
    """composite (raw (B,S,4)) + d MSE / d rgb against `target` (B,3) + the compositing backward for it, one launch
    (nerfhip_composite_train).  Returns (weights | None, opacity, rgb, depth, g_raw = d loss / d raw); nothing is recorded for
    autograd — the caller (models/train_step.py) owns the backward."""
    require_gpu(raw, z, rays, noise, target)
    raw, z, rays, target, B, S = _train_composite_args("composite_train", raw, z, rays, target)
    noise = _noise_arg("composite_train", "noise", noise, noise_std, B * S)
    weights = torch.empty(B, S, device=z.device, dtype=torch.float32) if want_weights else None
    opacity, rgb, depth, g_raw = _train_composite_outs(B, S, z.device)
    check(_lib.load().nerfhip_composite_train(ptr(raw), ptr(z), ptr(rays), ptr(noise), float(noise_std), int(bool(white_back)),
                                              ptr(target), float(grad_scale), ptr(weights), ptr(rgb), ptr(depth), ptr(opacity),
                                              ptr(g_raw), B, S, stream_ptr()), "nerfhip_composite_train")
    return weights, opacity, rgb, depth, g_raw


@device_guard
def composite_train_fine_z(raw, z, rays, noise, noise_std, white_back, target, grad_scale, n_importance, u=None, eps=1e-5,
                           want_weights=False):
    """The coarse pass of a training step in one launch (nerfhip_composite_train_fine_z): composite_train + fine_z on the
    ray's weights (which stay in LDS unless want_weights).  Returns (weights | None, opacity, rgb, depth, g_raw, z_fine)."""
    require_gpu(raw, z, rays, noise, target, u)
    raw, z, rays, target, B, S = _train_composite_args("composite_train_fine_z", raw, z, rays, target)
    noise = _noise_arg("composite_train_fine_z", "noise", noise, noise_std, B * S)
    u, u_stride = _u_arg("composite_train_fine_z", u, B, n_importance)
    dev = z.device
    weights = torch.empty(B, S, device=dev, dtype=torch.float32) if want_weights else None
    opacity, rgb, depth, g_raw = _train_composite_outs(B, S, dev)
    zf = torch.empty(B, S + n_importance, device=dev, dtype=torch.float32)
    check(_lib.load().nerfhip_composite_train_fine_z(ptr(raw), ptr(z), ptr(rays), ptr(noise), float(noise_std), int(bool(white_back)),
                                                     ptr(target), float(grad_scale), ptr(weights), ptr(rgb), ptr(depth), ptr(opacity),
                                                     ptr(g_raw), B, S, ptr(u), u_stride, int(n_importance), float(eps), ptr(zf),
                                                     _row_total, stream_ptr()), "nerfhip_composite_train_fine_z")
    return weights, opacity, rgb, depth, g_raw, zf


@device_guard
def composite_train_loss(raw, z, rays, noise, noise_std, white_back, target, grad_scale, rgb_coarse=None):
    """The last pass of a training step in one launch (nerfhip_composite_train_loss): composite_train + the values of mse_psnr
    over (rgb_coarse, this pass's rgb).  Returns (opacity, rgb, depth, g_raw, out3 = [loss, psnr, mse])."""
    require_gpu(raw, z, rays, noise, target, rgb_coarse)
    raw, z, rays, target, B, S = _train_composite_args("composite_train_loss", raw, z, rays, target)
    if rgb_coarse is not None:
        rgb_coarse = _c(rgb_coarse)
        if rgb_coarse.numel() != B * 3:
            raise ValueError("composite_train_loss: rgb_coarse must be (B,3)")
    noise = _noise_arg("composite_train_loss", "noise", noise, noise_std, B * S)
    dev = z.device
    opacity, rgb, depth, g_raw = _train_composite_outs(B, S, dev)
    out3 = torch.empty(3, device=dev, dtype=torch.float32)
    check(_lib.load().nerfhip_composite_train_loss(ptr(raw), ptr(z), ptr(rays), ptr(noise), float(noise_std), int(bool(white_back)),
                                                   ptr(target), float(grad_scale), None, ptr(rgb), ptr(depth), ptr(opacity), ptr(g_raw),
                                                   B, S, ptr(rgb_coarse), ptr(out3), ptr(_ticket(dev)), stream_ptr()),
          "nerfhip_composite_train_loss")
    return opacity, rgb, depth, g_raw, out3


# ------------------------------------------------------------------------------- loss + PSNR (N2)
class _MsePsnr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb_c, rgb_f, target):
        require_gpu(rgb_c, rgb_f, target)
        rgb_c, target = _c(rgb_c), _c(target)
        rgb_f = _c(rgb_f) if rgb_f is not None else None
        n = target.numel()
        if rgb_c.numel() != n or (rgb_f is not None and rgb_f.numel() != n):
            raise ValueError("mse_psnr: shape mismatch")
        out3 = torch.empty(3, device=target.device, dtype=torch.float32)
        g_c = torch.empty_like(rgb_c)
        g_f = torch.empty_like(rgb_f) if rgb_f is not None else None
        check(_lib.load().nerfhip_mse_psnr(ptr(rgb_c), ptr(rgb_f), ptr(target), n, ptr(out3), ptr(g_c), ptr(g_f), stream_ptr()),
              "nerfhip_mse_psnr")
        ctx.save_for_backward(g_c, g_f)
        ctx.mark_non_differentiable(out3)
        ctx.set_materialize_grads(False)      # no zeros(3) launch for the unused gradient of out3
        return out3[0], out3

    @staticmethod
    def backward(ctx, g_loss, _g_out3):
        g_c, g_f = ctx.saved_tensors
        if g_loss is None:
            return None, None, None
        if is_unit_seed(g_loss):              # d loss / d loss == 1 (loss.backward(unit_seed(loss))): no scaling launch
            return g_c, g_f, None
        if g_f is None:
            return g_c * g_loss, None, None
        g_c, g_f = torch._foreach_mul([g_c, g_f], g_loss)      # one launch for both images
        return g_c, g_f, None


_UNIT_SEEDS = {}


def unit_seed(like):
    """A cached scalar 1.0 on `like`'s device to pass as `loss.backward(unit_seed(loss))`: the fused backward nodes recognise it
    (by storage) and skip the multiplication by d loss / d loss.  Never modify it in place."""
    key = (like.device.type, like.device.index)
    t = _UNIT_SEEDS.get(key)
    if t is None:
        t = _UNIT_SEEDS[key] = torch.ones((), device=like.device, dtype=torch.float32)
    return t


def is_unit_seed(g):
    t = _UNIT_SEEDS.get((g.device.type, g.device.index))
    return t is not None and g.data_ptr() == t.data_ptr() and g.numel() == 1


@device_guard
def mse_psnr_values(rgb_coarse, rgb_fine, target):
    """[loss, psnr, mse] (losses.py:9-14 + metrics.py:4-13) without gradients: the value half of nerfhip_mse_psnr."""
    require_gpu(rgb_coarse, rgb_fine, target)
    rgb_coarse, target = _c(rgb_coarse), _c(target)
    rgb_fine = _c(rgb_fine) if rgb_fine is not None else None
    out3 = torch.empty(3, device=target.device, dtype=torch.float32)
    check(_lib.load().nerfhip_mse_psnr(ptr(rgb_coarse), ptr(rgb_fine), ptr(target), target.numel(), ptr(out3), None, None, stream_ptr()),
          "nerfhip_mse_psnr")
    return out3


@device_guard
def mse_psnr(rgb_coarse, rgb_fine, target):
    """MSELoss.forward (losses.py:9-14) + psnr (metrics.py:4-13) + d loss/d rgb in one launch.
    Returns (loss [differentiable scalar], out3 = [loss, psnr, mse] detached)."""
    return _MsePsnr.apply(rgb_coarse, rgb_fine, target)


# ------------------------------------------------------------------------------- MLP (a3, a4, a6)
PARAM_ORDER = ["xyz_encoding_1.0", "xyz_encoding_2.0", "xyz_encoding_3.0", "xyz_encoding_4.0",
               "xyz_encoding_5.0", "xyz_encoding_6.0", "xyz_encoding_7.0", "xyz_encoding_8.0",
               "xyz_encoding_final", "dir_encoding.0", "sigma", "rgb.0"]
PARAM_SHAPES = [(256, 63), (256, 256), (256, 256), (256, 256), (256, 319), (256, 256), (256, 256), (256, 256),
                (256, 256), (128, 283), (1, 256), (3, 128)]


DEFAULT_ARCH_ONLY = "the fused HIP MLP implements the reference's default architecture (D=8, W=256, skips=[4], 63/27 inputs) only"


def packed_bytes(dtype):
    return int(_lib.load().nerfhip_mlp_packed_bytes(mlp_dtype_code(dtype)))


def packed_bwd_bytes(dtype):
    return int(_lib.load().nerfhip_mlp_packed_bwd_bytes(mlp_dtype_code(dtype)))


def pack_arg_tables(weights, biases):
    """Validate the 12 (weight, bias) tensors once and return ctypes pointer tables (wp, bp) for the pack entry points."""
    if len(weights) != 12 or len(biases) != 12:
        raise ValueError("need 12 weights and 12 biases")
    for i, (w, b) in enumerate(zip(weights, biases)):
        require_gpu(w, b)
        if tuple(w.shape) != PARAM_SHAPES[i] or tuple(b.shape) != (PARAM_SHAPES[i][0],):
            raise NerfHipError("%s; got %s for %s" % (DEFAULT_ARCH_ONLY, tuple(w.shape), PARAM_ORDER[i]))
        if not (w.is_contiguous() and b.is_contiguous()):
            raise NerfHipError("NeRF parameters must be contiguous")
    wp = (ctypes.c_void_p * 12)(*[w.data_ptr() for w in weights])
    bp = (ctypes.c_void_p * 12)(*[b.data_ptr() for b in biases])
    return wp, bp


@device_guard
def pack_weights_raw(wp, bp, out, dtype):
    check(_lib.load().nerfhip_mlp_pack_weights(wp, bp, ptr(out), mlp_dtype_code(dtype), stream_ptr()), "nerfhip_mlp_pack_weights")


@device_guard
def pack_weights_bwd_raw(wp, bp, out, dtype):
    check(_lib.load().nerfhip_mlp_pack_weights_bwd(wp, bp, ptr(out), mlp_dtype_code(dtype), stream_ptr()),
          "nerfhip_mlp_pack_weights_bwd")


@device_guard
def pack_weights_train_raw(wp, bp, out, out_bwd, dtype):
    check(_lib.load().nerfhip_mlp_pack_weights_train(wp, bp, ptr(out), ptr(out_bwd), mlp_dtype_code(dtype), stream_ptr()),
          "nerfhip_mlp_pack_weights_train")


def alloc_acts(n_points, dtype, device):
    nbytes = int(_lib.load().nerfhip_mlp_act_bytes(int(n_points), mlp_dtype_code(dtype)))
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


@device_guard
def mlp_fwd_embedded(x, packed, sigma_only, dtype, save=None):
    require_gpu(x)
    if x.dim() != 2 or x.stride(1) != 1:
        x = x.reshape(-1, x.shape[-1]).contiguous()
    n = x.shape[0]
    need = 63 if sigma_only else 90
    if x.shape[1] != need:
        raise ValueError("NeRF.forward expects %d input channels, got %d" % (need, x.shape[1]))
    out = torch.empty(n, 1 if sigma_only else 4, device=x.device, dtype=torch.float32)
    check(_lib.load().nerfhip_mlp_fwd_embedded(ptr(x), x.stride(0), n, ptr(packed), ptr(out), int(bool(sigma_only)),
                                               mlp_dtype_code(dtype), ptr(save), stream_ptr()),
          "nerfhip_mlp_fwd_embedded")
    return out


@device_guard
def mlp_fwd_rays(rays, z, packed, sigma_only, dtype, save=None):
    require_gpu(rays, z)
    rays, z = _c(rays), _c(z)
    B, S = z.shape
    out = torch.empty((B, S) if sigma_only else (B, S, 4), device=z.device, dtype=torch.float32)
    check(_lib.load().nerfhip_mlp_fwd_rays(ptr(rays), ptr(z), B, S, ptr(packed), ptr(out), int(bool(sigma_only)),
                                           mlp_dtype_code(dtype), ptr(save), stream_ptr()), "nerfhip_mlp_fwd_rays")
    return out


@device_guard
def mlp_fwd_rays_coarse(rays, n_samples, packed, sigma_only, dtype, use_disp=False, perturb=0.0, perturb_rand=None, save=None):
    """The coarse pass's sample_coarse_z + mlp_fwd_rays in one launch (nerfhip_mlp_fwd_rays_coarse): the depths are formed in the
    MLP kernel's prologue.  Returns (z (B,S), out)."""
    require_gpu(rays, perturb_rand)
    rays = _c(rays)
    B, S = rays.shape[0], int(n_samples)
    perturb_rand = _perturb_arg("mlp_fwd_rays_coarse", perturb, perturb_rand, B * S)
    z = torch.empty(B, S, device=rays.device, dtype=torch.float32)
    out = torch.empty((B, S) if sigma_only else (B, S, 4), device=rays.device, dtype=torch.float32)
    check(_lib.load().nerfhip_mlp_fwd_rays_coarse(ptr(rays), ptr(perturb_rand), ptr(z), B, S,
                                                  int(bool(use_disp)), float(perturb), ptr(packed), ptr(out), int(bool(sigma_only)),
                                                  mlp_dtype_code(dtype), ptr(save), stream_ptr()), "nerfhip_mlp_fwd_rays_coarse")
    return z, out


# ------------------------------------------------------------------------------- render_rays in one launch
_render_fused = os.environ.get("NERFHIP_RENDER_FUSED", "1") != "0"


def set_render_fused(on):
    """Let render_rays / the fused training node use the single-launch render kernels where they apply (default) or keep them on
    the multi-launch path (A/B, bit-equality tests).  Returns the previous setting.  NERFHIP_RENDER_FUSED=0 in the environment."""
    global _render_fused
    prev, _render_fused = _render_fused, bool(on)
    return prev


def render_supported(B, S_c, N_i, dtype):
    """True when the single-launch render kernels take this shape (include/nerfhip.h nerfhip_render_supported: B % 4 == 0, 4 S_c and
    4 (S_c + N_i) multiples of the points per sub-pass) and set_render_fused has not switched them off."""
    if not _render_fused:
        return False
    return bool(_lib.load().nerfhip_render_supported(int(B), int(S_c), int(N_i), mlp_dtype_code(dtype)))


def _render_args(rays, S, N, packed_c, packed_f, use_disp, perturb, perturb_rand, noise_c, noise_f, noise_std, white_back, u, eps,
                 want_coarse, coarse_sigma_only=False):
    B = rays.shape[0]
    dev = rays.device
    f32 = dict(device=dev, dtype=torch.float32)
    a = _lib.RenderArgs()
    bufs = {"z_coarse": torch.empty(B, S, **f32), "opacity_coarse": torch.empty(B, **f32),
            "raw_coarse": torch.empty((B, S) if coarse_sigma_only else (B, S, 4), **f32)}
    if want_coarse:
        bufs.update(rgb_coarse=torch.empty(B, 3, **f32), depth_coarse=torch.empty(B, **f32))
    if N > 0:
        bufs.update(z_fine=torch.empty(B, S + N, **f32), raw_fine=torch.empty(B, S + N, 4, **f32), rgb_fine=torch.empty(B, 3, **f32),
                    depth_fine=torch.empty(B, **f32), opacity_fine=torch.empty(B, **f32))
    perturb_rand = _perturb_arg("render", perturb, perturb_rand, B * S)
    noise_c = _noise_arg("render", "noise_coarse", noise_c, noise_std, B * S)
    noise_f = _noise_arg("render", "noise_fine", noise_f if N > 0 else None, noise_std, B * (S + N))
    if noise_std != 0 and (noise_c is None or (N > 0 and noise_f is None)):
        raise ValueError("render: noise_std != 0 needs the noise draws")
    u, u_stride = _u_arg("render", u if N > 0 else None, B, N)
    a.rays, a.B, a.S_c, a.N_i = rays.data_ptr(), B, int(S), int(N)
    a.packed_coarse = packed_c.data_ptr()
    a.packed_fine = packed_f.data_ptr() if packed_f is not None else None
    for k, t in bufs.items():
        setattr(a, k, t.data_ptr())
    a.perturb_rand = perturb_rand.data_ptr() if perturb_rand is not None else None
    a.perturb, a.use_disp = float(perturb), int(bool(use_disp))
    a.noise_coarse = noise_c.data_ptr() if noise_c is not None else None
    a.noise_fine = noise_f.data_ptr() if noise_f is not None else None
    a.noise_std, a.white_back = float(noise_std), int(bool(white_back))
    a.u, a.u_stride, a.eps, a.row_total = (u.data_ptr() if u is not None else None), u_stride, float(eps), _row_total
    keep = (rays, packed_c, packed_f, perturb_rand, noise_c, noise_f, u)
    return a, bufs, keep


@device_guard
def render_fwd(rays, n_samples, n_importance, packed_coarse, packed_fine, dtype, use_disp=False, perturb=0.0, perturb_rand=None,
               noise_coarse=None, noise_fine=None, noise_std=0.0, white_back=False, u=None, eps=1e-5, want_coarse=True, test_time=False):
    """render_rays (rendering.py:58-244) for one ray chunk in ONE launch (nerfhip_render_fwd).  Returns the dict of every buffer
    the launch wrote: rgb / depth / opacity of both passes (rgb_coarse / depth_coarse only with want_coarse), z_* and raw_*.
    test_time (rendering.py:209-213, N_importance > 0): nerfhip_render_test_fwd — the coarse sub-passes run the network's sigma-only
    body, raw_coarse is (B, S) and the coarse pass leaves opacity_coarse only."""
    require_gpu(rays, perturb_rand, noise_coarse, noise_fine, u)
    rays = _c(rays)
    tt = bool(test_time) and int(n_importance) > 0
    a, bufs, keep = _render_args(rays, n_samples, n_importance, packed_coarse, packed_fine, use_disp, perturb, perturb_rand,
                                 noise_coarse, noise_fine, noise_std, white_back, u, eps, want_coarse and not tt, coarse_sigma_only=tt)
    if tt:
        check(_lib.load().nerfhip_render_test_fwd(ctypes.addressof(a), mlp_dtype_code(dtype), stream_ptr()), "nerfhip_render_test_fwd")
    else:
        check(_lib.load().nerfhip_render_fwd(ctypes.addressof(a), mlp_dtype_code(dtype), stream_ptr()), "nerfhip_render_fwd")
    return bufs


@device_guard
def render_train_fwd(rays, target, grad_scale, n_samples, n_importance, packed_coarse, packed_fine, dtype, acts_coarse, acts_fine,
                     use_disp=False, perturb=0.0, perturb_rand=None, noise_coarse=None, noise_fine=None, noise_std=0.0,
                     white_back=False, u=None, eps=1e-5, regen_enc=False):
    """The forward of a training step in ONE launch (nerfhip_render_train_fwd): render_fwd + saved activations + per pass the
    loss gradient and the compositing backward (g_raw_*) + out3 = [loss, psnr, mse].  Returns the dict of written buffers.
    regen_enc (bf16): the input-encoding slabs are not saved; the backward must be mlp_bwd_multi with (rays, z, S) entries."""
    require_gpu(rays, target, perturb_rand, noise_coarse, noise_fine, u)
    rays, target = _c(rays), _c(target)
    B, S, N = rays.shape[0], int(n_samples), int(n_importance)
    if target.numel() != 3 * B or target.dtype != torch.float32:
        raise ValueError("render_train_fwd: target must be (B,3) fp32")
    a, bufs, keep = _render_args(rays, S, N, packed_coarse, packed_fine, use_disp, perturb, perturb_rand, noise_coarse, noise_fine,
                                 noise_std, white_back, u, eps, True)
    dev = rays.device
    bufs["g_raw_coarse"] = torch.empty(B, S, 4, device=dev, dtype=torch.float32)
    if N > 0:
        bufs["g_raw_fine"] = torch.empty(B, S + N, 4, device=dev, dtype=torch.float32)
    bufs["out3"] = torch.empty(3, device=dev, dtype=torch.float32)
    a.g_raw_coarse = bufs["g_raw_coarse"].data_ptr()
    a.g_raw_fine = bufs["g_raw_fine"].data_ptr() if N > 0 else None
    a.out3 = bufs["out3"].data_ptr()
    a.save_coarse = acts_coarse.data_ptr()
    a.save_fine = acts_fine.data_ptr() if N > 0 else None
    a.target, a.grad_scale = target.data_ptr(), float(grad_scale)
    a.ticket = _ticket(dev).data_ptr()
    a.regen_enc = int(bool(regen_enc) and mlp_dtype_code(dtype) == BF16)
    check(_lib.load().nerfhip_render_train_fwd(ctypes.addressof(a), mlp_dtype_code(dtype), stream_ptr()), "nerfhip_render_train_fwd")
    return bufs


# ------------------------------------------------------------------------------- MLP backward (K2b)
FLAT_GRAD_FLOATS = sum(s[0] * s[1] + s[0] for s in PARAM_SHAPES)      # 595,844: a model's 24 gradients (16-byte multiple)


def flat_grad_views(n_points, device, shapes=PARAM_SHAPES, out=None):
    """One flat fp32 buffer for a model's 24 gradients + the 12 weight and 12 bias views of it (the layout FlatAdam mirrors).
    out: the slice of a larger buffer to use as that flat buffer (mlp_bwd_multi: the models' buffers are consecutive slices of ONE
    allocation, so that the gradients of a whole step are one contiguous message for the all-reduce).
    n_points == 0: the C entry points launch nothing, so the gradients of an empty batch are explicit zeros."""
    sizes = [s[0] * s[1] for s in shapes] + [s[0] for s in shapes]
    if out is not None:
        flat = out
        if n_points == 0:
            flat.zero_()
    else:
        flat = (torch.zeros if n_points == 0 else torch.empty)(sum(sizes), device=device, dtype=torch.float32)
    views, off = [], 0
    for sz in sizes:
        views.append(flat[off:off + sz])
        off += sz
    return [v.view(s) for v, s in zip(views[:12], shapes)], views[12:], flat


@device_guard
def mlp_bwd(g_out, out, packed_bwd, acts, dtype, shapes=PARAM_SHAPES, phases=7, workspace=None):
    """Gradients of all 24 parameter tensors given dL/d(out).  Returns ([gw0..gw11], [gb0..gb11], flat buffer).
    phases / workspace: measurement hooks (bench.py): run only some of the three kernels (bit 0 chain, 1 dW GEMM, 2 reduce)
    on caller-kept scratch buffers (dys, dw workspace, flat gradients)."""
    require_gpu(g_out, out)
    code = mlp_dtype_code(dtype)
    g_out = _c(g_out.float()).reshape(-1, 4)
    out = _c(out).reshape(-1, 4)
    n = out.shape[0]
    dev = out.device
    lib = _lib.load()
    if workspace is not None and "dys" in workspace:
        dys, ws = workspace["dys"], workspace["ws"]
    else:
        dys = torch.empty(int(lib.nerfhip_mlp_dy_bytes(n, code)), device=dev, dtype=torch.uint8)
        ws = torch.empty(int(lib.nerfhip_mlp_dw_workspace_bytes(n, code)), device=dev, dtype=torch.uint8)
        if workspace is not None:
            workspace["dys"], workspace["ws"] = dys, ws
    # one flat fp32 buffer for all 24 gradients: autograd adopts the views as p.grad, so a model's gradients are contiguous
    # => ONE RCCL all-reduce per model, no flatten copies
    gw, gb, flat = flat_grad_views(n, dev, shapes)
    gwp = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in gw])
    gbp = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in gb])
    check(lib.nerfhip_mlp_bwd_phases(ptr(g_out), ptr(out), n, ptr(packed_bwd), ptr(acts), ptr(dys), ptr(ws), gwp, gbp, 0, code,
                                     int(phases), stream_ptr()), "nerfhip_mlp_bwd")
    return gw, gb, flat


@device_guard
def mlp_dx_embedded(dys, n, w_xyz1, w_xyz5, w_dir, dtype):
    """dL/dx (n, 90) of NeRF.forward on pre-embedded inputs from the dY slabs of the preceding mlp_bwd call."""
    code = mlp_dtype_code(dtype)
    if code == BF16_F8:
        raise NotImplementedError("nerfhip_mlp_dx_embedded reads bf16 / fp32 dY slabs ('bf16_f8' keeps dY only as e5m2: NeRF.forward "
                                  "saves in bf16 for calls whose input requires grad, models/mlp_autograd.py)")
    require_gpu(w_xyz1, w_xyz5, w_dir)
    gx = torch.empty(n, 90, device=dys.device, dtype=torch.float32)
    check(_lib.load().nerfhip_mlp_dx_embedded(ptr(dys), n, ptr(_c(w_xyz1.detach())), ptr(_c(w_xyz5.detach())), ptr(_c(w_dir.detach())),
                                              ptr(gx), 90, code, stream_ptr()), "nerfhip_mlp_dx_embedded")
    return gx


# ------------------------------------------------------------------------------- several models per launch (training step)
def pack_tables(models, dtype):
    """ctypes argument tables (weights, biases, forward images, W^T images) + the [(packed, packed_bwd)] buffers of `models` for
    the multi-model pack entry points (nerfhip_mlp_pack_weights_train_multi, nerfhip_train_prologue)."""
    if not 1 <= len(models) <= 4:
        raise ValueError("pack_models_train packs 1..4 models")
    tabs, bufs = [], []
    for m in models:
        if not m.is_default_arch():
            raise NotImplementedError(DEFAULT_ARCH_ONLY)
        wp, bp, dev = m._pack_args()
        tabs.append((wp, bp))
        bufs.append(m.train_buffers(dtype, dev))
    n = len(models)
    W = (ctypes.c_void_p * (12 * n))(*[t[0][i] for t in tabs for i in range(12)])
    Bv = (ctypes.c_void_p * (12 * n))(*[t[1][i] for t in tabs for i in range(12)])
    P = (ctypes.c_void_p * n)(*[b[0].data_ptr() for b in bufs])
    Pb = (ctypes.c_void_p * n)(*[b[1].data_ptr() for b in bufs])
    return W, Bv, P, Pb, bufs


def pack_models_train(models, dtype):
    """Forward + W^T images of every model in ONE launch (nerfhip_mlp_pack_weights_train_multi).  Returns [(packed, packed_bwd)]
    in the models' cached buffers (NeRF.packed_weights_train's)."""
    W, Bv, P, Pb, bufs = pack_tables(models, dtype)
    with torch.cuda.device(bufs[0][0].device):
        check(_lib.load().nerfhip_mlp_pack_weights_train_multi(W, Bv, P, Pb, len(models), mlp_dtype_code(dtype), stream_ptr()),
              "nerfhip_mlp_pack_weights_train_multi")
    for m in models:
        m.images_packed()
    return bufs


def mlp_bwd_multi(entries, dtype, adam=None, phases=7, workspace=None, g_scale=None):
    """Backward of several models with ONE dW launch and ONE reduce launch (nerfhip_mlp_bwd_multi).
    entries: [(g_out (n,4), out (n,4), packed_bwd, acts)] or [(g_out, out, packed_bwd, acts, rays (B,8), z (B,S))] — the latter for
    a bf16 model whose forward did not save its input encodings (render_train_fwd(regen_enc=True)): the weight-gradient launch forms
    them again from the rays and the depths (nerfhip_mlp_bwd_multi_rays); n > 0.  adam: an _lib.AdamFused (the update then happens
    inside the reduce kernel).  g_scale: device scalar multiplying every g_out inside the chain kernels (the upstream gradient of the loss).
    Returns [(gw list, gb list, flat)] per model."""
    code = mlp_dtype_code(dtype)
    lib = _lib.load()
    M = len(entries)
    dev = entries[0][1].device
    gs, outs, ns, dys, grads = [], [], [], [], []
    enc, keep_enc = None, []
    for m, e in enumerate(entries):
        g_out, out = e[0], e[1]
        if len(e) > 4 and e[4] is not None:
            if enc is None:
                enc = _lib.EncSource()
            rays_e, z_e = _c(e[4]), _c(e[5])
            require_gpu(rays_e, z_e)
            if rays_e.dtype != torch.float32 or z_e.dtype != torch.float32 or z_e.dim() != 2 or rays_e.shape[0] != z_e.shape[0]:
                raise ValueError("mlp_bwd_multi: (rays (B,8), z (B,S)) fp32 expected")
            enc.rays[m], enc.z[m], enc.S[m] = rays_e.data_ptr(), z_e.data_ptr(), int(z_e.shape[1])
            keep_enc.append((rays_e, z_e))
        require_gpu(g_out, out)
        g_out = _c(g_out.float()).reshape(-1, 4)
        out = _c(out).reshape(-1, 4)
        gs.append(g_out)
        outs.append(out)
        ns.append(out.shape[0])
    with torch.cuda.device(dev):
        n_arr = (ctypes.c_int64 * M)(*ns)
        key = ("multi", tuple(ns), code)
        if workspace is not None and key in workspace:
            dys, ws = workspace[key]
        else:
            dys = [torch.empty(int(lib.nerfhip_mlp_dy_bytes(n, code)), device=dev, dtype=torch.uint8) for n in ns]
            ws = torch.empty(int(lib.nerfhip_mlp_dw_workspace_bytes_multi(n_arr, M, code)), device=dev, dtype=torch.uint8)
            if workspace is not None:
                workspace[key] = (dys, ws)
        # the M flat gradient buffers are consecutive slices of ONE allocation (`flat._base`): parallel.GradSync all-reduces a step's
        # gradients as one message
        joint = torch.empty(M * FLAT_GRAD_FLOATS, device=dev, dtype=torch.float32)
        for m, n in enumerate(ns):
            grads.append(flat_grad_views(n, dev, out=joint[m * FLAT_GRAD_FLOATS:(m + 1) * FLAT_GRAD_FLOATS]))
        vp = ctypes.c_void_p
        G = (vp * M)(*[t.data_ptr() for t in gs])
        O = (vp * M)(*[t.data_ptr() for t in outs])
        PB = (vp * M)(*[e[2].data_ptr() for e in entries])
        AC = (vp * M)(*[e[3].data_ptr() for e in entries])
        DY = (vp * M)(*[t.data_ptr() for t in dys])
        GW = (vp * (12 * M))(*[t.data_ptr() for g in grads for t in g[0]])
        GB = (vp * (12 * M))(*[t.data_ptr() for g in grads for t in g[1]])
        if adam is not None:
            for m in range(M):
                adam.grad_flat[m] = grads[m][2].data_ptr()
        if g_scale is not None:
            require_gpu(g_scale)
        check(lib.nerfhip_mlp_bwd_multi_rays(M, G, O, n_arr, PB, AC, DY, ptr(ws), GW, GB, 0, code, int(phases), ptr(g_scale),
                                             ctypes.addressof(adam) if adam is not None else None,
                                             ctypes.addressof(enc) if enc is not None else None, stream_ptr()), "nerfhip_mlp_bwd_multi_rays")
    return grads


# ------------------------------------------------------------------------------- layer-by-layer path (non-default NeRF shapes)
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def _rows(t):
    """(n, c) fp32 device tensor with unit column stride (a column slice of a wider tensor is fine: row stride = ld)"""
    if t.dim() != 2:
        raise ValueError("expected a (n, channels) tensor")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _off(t, col):
    """device pointer of t[:, col:] (row-major fp32)"""
    return ctypes.c_void_p(t.data_ptr() + 4 * col)


class _LinearAct(torch.autograd.Function):
    """act(cat(xs, -1) @ w.T + b) without the cat: one nerfhip_linear_fwd per input segment (the second accumulates on the first)."""

    @staticmethod
    def forward(ctx, act, dtype, w, b, *xs):
        xs = [_rows(x.float()) for x in xs]
        require_gpu(w, b, *xs)
        w, b = _c(w), _c(b)
        n, n_out, k_tot = xs[0].shape[0], w.shape[0], w.shape[1]
        if sum(x.shape[1] for x in xs) != k_tot or any(x.shape[0] != n for x in xs) or b.numel() != n_out:
            raise ValueError("linear: input segments %s do not match the weight %s" % ([tuple(x.shape) for x in xs], tuple(w.shape)))
        lib = _lib.load()
        code = mlp_dtype_code(dtype)
        y = torch.empty(n, n_out, device=w.device, dtype=torch.float32)
        col = 0
        for s, x in enumerate(xs):
            last = s == len(xs) - 1
            check(lib.nerfhip_linear_fwd(ptr(x), x.stride(0), _off(w, col), k_tot, ptr(b) if last else None, ptr(y), n_out, n,
                                         x.shape[1], n_out, act if last else ACT_NONE, int(s > 0), code, stream_ptr()),
                  "nerfhip_linear_fwd")
            col += x.shape[1]
        ctx.cfg = (act, code)
        ctx.save_for_backward(w, y, *xs)
        return y

    @staticmethod
    def backward(ctx, gy):
        w, y, *xs = ctx.saved_tensors
        act, code = ctx.cfg
        lib = _lib.load()
        gy = _c(gy.float())
        n, n_out, k_tot = y.shape[0], w.shape[0], w.shape[1]
        need_w, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gw = gb = None
        gxs = []
        if (need_w or need_b) and n > 0:
            gw = torch.empty_like(w)
            gb = torch.empty(n_out, device=w.device, dtype=torch.float32)
            ws_bytes = max(lib.nerfhip_linear_bwd_weight_workspace_bytes(n, x.shape[1], n_out) for x in xs)
            ws = torch.empty(ws_bytes, device=w.device, dtype=torch.uint8)
        elif need_w or need_b:
            gw, gb = torch.zeros_like(w), torch.zeros(n_out, device=w.device, dtype=torch.float32)
        col = 0
        for s, x in enumerate(xs):
            if (need_w or need_b) and n > 0:
                check(lib.nerfhip_linear_bwd_weight(ptr(gy), n_out, ptr(y), n_out, act, ptr(x), x.stride(0), _off(gw, col), k_tot,
                                                    ptr(gb) if s == 0 else None, ptr(ws), n, x.shape[1], n_out, 0, code,
                                                    stream_ptr()), "nerfhip_linear_bwd_weight")
            gx = None
            if ctx.needs_input_grad[4 + s]:
                gx = torch.empty(n, x.shape[1], device=w.device, dtype=torch.float32)
                check(lib.nerfhip_linear_bwd_input(ptr(gy), n_out, ptr(y), n_out, act, _off(w, col), k_tot, ptr(gx), x.shape[1], n,
                                                   x.shape[1], n_out, 0, code, stream_ptr()), "nerfhip_linear_bwd_input")
            gxs.append(gx)
            col += x.shape[1]
        return (None, None, gw if need_w else None, gb if need_b else None) + tuple(gxs)


@device_guard
def linear_act(xs, weight, bias, act, dtype):
    """nn.Linear (+ activation) on the concatenation of the (n, c_i) tensors `xs` (nerf.py:59-81, 108-118), differentiable in
    weight, bias and every segment.  act: ACT_NONE | ACT_RELU | ACT_SIGMOID."""
    return _LinearAct.apply(int(act), dtype, weight, bias, *xs)


# ------------------------------------------------------------------------------- mesh extraction (extract_color_mesh.py:144-285)
_INT32_MAX = 2 ** 31 - 1


def _require_mesh(name, t, dtype, shape_len=None, cols=None):
    if not torch.is_tensor(t):
        raise NerfHipError("%s: expected a torch tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise NerfHipError("nerf_pl_amd runs on MI355X only: %s is a %s tensor (no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise NerfHipError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if shape_len is not None and t.dim() != shape_len:
        raise NerfHipError("%s: expected rank %d, got shape %s" % (name, shape_len, tuple(t.shape)))
    if cols is not None and t.shape[-1] != cols:
        raise NerfHipError("%s: expected %d columns, got shape %s" % (name, cols, tuple(t.shape)))
    return _c(t)


def _check_vertex_ids(triangles, V):
    if triangles.numel() and (int(triangles.min()) < 0 or int(triangles.max()) >= V):
        raise NerfHipError("triangles reference vertices outside [0, %d)" % V)


@device_guard
def marching_cubes(volume, iso):
    """nerfhip_marching_cubes_{count,emit}: (vertices (V,3) float64 in index coordinates, triangles (T,3) int32), on the device.
    One 16-byte device-to-host read of (V, T) between the two launches sizes the outputs."""
    volume = _require_mesh("marching_cubes volume", volume, torch.float32, 3)
    n0, n1, n2 = volume.shape
    if min(n0, n1, n2) < 2:
        raise NerfHipError("marching_cubes: every dimension must be >= 2, got %s" % (tuple(volume.shape),))
    lib = _lib.load()
    ws_bytes = lib.nerfhip_marching_cubes_workspace_bytes(n0, n1, n2)
    if ws_bytes == 0:
        raise NerfHipError("marching_cubes: volume %s has 2^31 or more lattice points" % (tuple(volume.shape),))
    ws = torch.empty(ws_bytes, device=volume.device, dtype=torch.uint8)
    totals = torch.empty(2, device=volume.device, dtype=torch.int64)
    check(lib.nerfhip_marching_cubes_count(ptr(volume), n0, n1, n2, float(iso), ptr(ws), ptr(totals), stream_ptr()),
          "nerfhip_marching_cubes_count")
    V, T = (int(x) for x in totals.cpu())
    if V > _INT32_MAX or T > _INT32_MAX:
        raise NerfHipError("marching_cubes: %d vertices / %d triangles do not fit int32" % (V, T))
    verts = torch.empty(V, 3, device=volume.device, dtype=torch.float64)
    tris = torch.empty(T, 3, device=volume.device, dtype=torch.int32)
    if V or T:
        check(lib.nerfhip_marching_cubes_emit(ptr(volume), n0, n1, n2, float(iso), ptr(ws), ptr(totals), ptr(verts), ptr(tris),
                                              stream_ptr()), "nerfhip_marching_cubes_emit")
    return verts, tris


@device_guard
def largest_cluster(triangles, n_vertices):
    """(kept_vertex_ids (V',) int64 ascending, kept_triangles (T',3) int32 remapped) of the largest edge-connected cluster."""
    triangles = _require_mesh("triangles", triangles, torch.int32, 2, 3)
    T, V = triangles.shape[0], int(n_vertices)
    dev = triangles.device
    if T == 0 or V == 0:
        return torch.empty(0, device=dev, dtype=torch.int64), torch.empty(0, 3, device=dev, dtype=torch.int32)
    if V > _INT32_MAX or 3 * T > _INT32_MAX:
        raise NerfHipError("largest_cluster: mesh too large (V=%d, T=%d)" % (V, T))
    _check_vertex_ids(triangles, V)
    lib = _lib.load()
    keys = torch.empty(3 * T, device=dev, dtype=torch.int64)
    check(lib.nerfhip_mesh_edge_keys(ptr(triangles), T, ptr(keys), stream_ptr()), "nerfhip_mesh_edge_keys")
    sorted_keys, order = torch.sort(keys, stable=True)
    ws = torch.empty(lib.nerfhip_mesh_cluster_workspace_bytes(V, T), device=dev, dtype=torch.uint8)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    check(lib.nerfhip_mesh_largest_cluster(ptr(triangles), V, T, ptr(sorted_keys), ptr(order), ptr(ws), ptr(totals), stream_ptr()),
          "nerfhip_mesh_largest_cluster")
    t_kept, v_kept, status = (int(x) for x in totals.cpu())
    if status:
        raise NerfHipError("largest_cluster: the union-find gave up after its retry bound")
    kept_ids = torch.empty(v_kept, device=dev, dtype=torch.int64)
    kept_tris = torch.empty(t_kept, 3, device=dev, dtype=torch.int32)
    check(lib.nerfhip_mesh_cluster_compact(ptr(triangles), V, T, ptr(ws), ptr(kept_ids), ptr(kept_tris), stream_ptr()),
          "nerfhip_mesh_cluster_compact")
    return kept_ids, kept_tris


@device_guard
def vertex_normals(vertices, triangles):
    """open3d's compute_vertex_normals on float32 vertices: (V,3) float64 unit normals ((0,0,1) where the sum is zero)."""
    vertices = _require_mesh("vertices", vertices, torch.float32, 2, 3)
    triangles = _require_mesh("triangles", triangles, torch.int32, 2, 3)
    V, T = vertices.shape[0], triangles.shape[0]
    out = torch.empty(V, 3, device=vertices.device, dtype=torch.float64)
    if V == 0:
        return out
    _check_vertex_ids(triangles, V)
    check(_lib.load().nerfhip_mesh_vertex_normals(ptr(vertices), V, ptr(triangles), T, ptr(out), stream_ptr()),
          "nerfhip_mesh_vertex_normals")
    return out


@device_guard
def normal_rays(vertices, normals, near, far, near_t):
    vertices = _require_mesh("vertices", vertices, torch.float32, 2, 3)
    normals = _require_mesh("normals", normals, torch.float64, 2, 3)
    V = vertices.shape[0]
    rays = torch.empty(V, 8, device=vertices.device, dtype=torch.float32)
    if V:
        check(_lib.load().nerfhip_mesh_normal_rays(ptr(vertices), ptr(normals), V, float(near), float(far), float(near_t), ptr(rays),
                                                   stream_ptr()), "nerfhip_mesh_normal_rays")
    return rays


@device_guard
def view_rays(vertices, w2c, origin, focal, image, near):
    """One view: (colors (V,4) uint8, depth (V,) float64, rays (V,8) float32).  w2c: (3,4) float32 numpy, origin: (3,) float32."""
    import numpy as np
    vertices = _require_mesh("vertices", vertices, torch.float32, 2, 3)
    image = _require_mesh("image", image, torch.uint8, 3, 3)
    H, W = image.shape[0], image.shape[1]
    V = vertices.shape[0]
    dev = vertices.device
    colors = torch.empty(V, 4, device=dev, dtype=torch.uint8)
    depth = torch.empty(V, device=dev, dtype=torch.float64)
    rays = torch.empty(V, 8, device=dev, dtype=torch.float32)
    if V:
        w = np.ascontiguousarray(np.asarray(w2c, np.float32).reshape(3, 4))
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3))
        fp = ctypes.POINTER(ctypes.c_float)
        check(_lib.load().nerfhip_mesh_view_rays(ptr(vertices), V, w.ctypes.data_as(fp), o.ctypes.data_as(fp), float(np.float32(focal)),
                                                 W, H, ptr(image), float(near), ptr(colors), ptr(depth), ptr(rays), stream_ptr()),
              "nerfhip_mesh_view_rays")
    return colors, depth, rays


@device_guard
def color_accumulate(colors, depth, opacity, occ_threshold, accum):
    colors = _require_mesh("colors", colors, torch.uint8, 2, 4)
    depth = _require_mesh("depth", depth, torch.float64, 1)
    opacity = _require_mesh("opacity", opacity, torch.float32, 1)
    accum = _require_mesh("accum", accum, torch.float64, 2, 4)
    V = colors.shape[0]
    if V:
        check(_lib.load().nerfhip_mesh_color_accumulate(ptr(colors), ptr(depth), ptr(opacity), V, float(occ_threshold), ptr(accum),
                                                        stream_ptr()), "nerfhip_mesh_color_accumulate")
    return accum


@device_guard
def color_finish(accum):
    accum = _require_mesh("accum", accum, torch.float64, 2, 4)
    V = accum.shape[0]
    out = torch.empty(V, 3, device=accum.device, dtype=torch.uint8)
    if V:
        check(_lib.load().nerfhip_mesh_color_finish(ptr(accum), V, ptr(out), stream_ptr()), "nerfhip_mesh_color_finish")
    return out


@device_guard
def rgb_to_u8(rgb):
    rgb = _require_mesh("rgb", rgb, torch.float32)
    out = torch.empty(rgb.shape, device=rgb.device, dtype=torch.uint8)
    if rgb.numel():
        check(_lib.load().nerfhip_mesh_rgb_to_u8(ptr(rgb), rgb.numel(), ptr(out), stream_ptr()), "nerfhip_mesh_rgb_to_u8")
    return out


# ------------------------------------------------------------------------------- image metrics (metrics.py:15-20, visualization.py)
IMAGE_PLANAR, IMAGE_INTERLEAVED = 0, 1


@device_guard
def ssim(img1, img2, B, C, H, W, window_size=3, layout=IMAGE_PLANAR, want_map=False, want_mean=True):
    """nerfhip_ssim: 1 - 2 * dssim of kornia 0.2.0 for B images of C channels, H x W, planar (B,C,H,W) or interleaved (B,H,W,C).
    Returns (map in the images' layout or None, mean as a 0-dim device tensor or None).  No host synchronisation."""
    require_gpu(img1, img2)
    B, C, H, W, window_size = int(B), int(C), int(H), int(W), int(window_size)
    if min(B, C, H, W) < 0 or img1.numel() != B * C * H * W or img2.numel() != img1.numel():
        raise NerfHipError("ssim: images of %s and %s elements are not %d x %d x %d x %d" % (img1.numel(), img2.numel(), B, C, H, W))
    if window_size % 2 == 0 or not 3 <= window_size <= 11:
        raise NerfHipError("ssim: window_size must be odd and in 3..11, got %d" % window_size)
    img1, img2 = _c(img1), _c(img2)
    dev = img1.device
    lib = _lib.load()
    shape = (B, C, H, W) if layout == IMAGE_PLANAR else (B, H, W, C)
    out_map = torch.empty(shape, device=dev, dtype=torch.float32) if want_map else None
    mean = ws = None
    if want_mean:
        mean = torch.full((), float("nan"), device=dev, dtype=torch.float32) if img1.numel() == 0 else \
            torch.empty((), device=dev, dtype=torch.float32)
        ws = torch.empty(max(1, lib.nerfhip_ssim_workspace_bytes(B, C, H, W) // 8), device=dev, dtype=torch.float64)
    check(lib.nerfhip_ssim(ptr(img1), ptr(img2), B, C, H, W, window_size, int(layout), ptr(out_map), ptr(mean), ptr(ws), stream_ptr()),
          "nerfhip_ssim")
    return out_map, mean


def _require_depth_table(table, device):
    if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.uint8 or tuple(table.shape) != (256, 3) \
            or table.device != device:
        raise NerfHipError("depth_colormap: the colour table must be a (256, 3) uint8 tensor on %s" % (device,))
    return _c(table)


@device_guard
def depth_colormap(depth, table, want_float=True, want_bytes=False):
    """nerfhip_depth_colormap: visualize_depth of an (H, W) or (n,) depth image through a (256, 3) uint8 device table.
    Returns (float image (3, *depth.shape) or None, byte image (*depth.shape, 3) or None).  No host read of the minimum / maximum."""
    require_gpu(depth)
    table = _require_depth_table(table, depth.device)
    depth = _c(depth)
    n, dev = depth.numel(), depth.device
    lib = _lib.load()
    out_f = torch.empty((3,) + tuple(depth.shape), device=dev, dtype=torch.float32) if want_float else None
    out_b = torch.empty(tuple(depth.shape) + (3,), device=dev, dtype=torch.uint8) if want_bytes else None
    ws = torch.empty(max(1, lib.nerfhip_depth_colormap_workspace_bytes(n) // 4), device=dev, dtype=torch.float32)
    check(lib.nerfhip_depth_colormap(ptr(depth), n, ptr(table), ptr(out_f), ptr(out_b), ptr(ws), stream_ptr()),
          "nerfhip_depth_colormap")
    return out_f, out_b


# ------------------------------------------------------------------------------- animated GIF (eval.py:145)
GIF_STRIP = 3838            # NERFHIP_GIF_STRIP


def gif_workspace(F, H, W, device):
    """The scratch buffer both GIF calls take (about 38.5 KB per 3838-pixel strip plus 168 KB per frame)."""
    nbytes = _lib.load().nerfhip_gif_workspace_bytes(F, H, W)
    if F > 0 and nbytes == 0:
        raise NerfHipError("gif: %d frames of %d x %d are refused (1..65535 per side, at most 2^26 pixels, at most 65535 frames)"
                           % (F, H, W))
    return torch.empty(max(1, nbytes // 8), device=device, dtype=torch.int64)


@device_guard
def gif_quantize(frames, workspace=None):
    """nerfhip_gif_quantize: frames (F, H, W, 3) uint8 on the device -> (indices (F, H*W) uint8, palettes (F, 256, 3) uint8,
    box_counts (F,) int32): every frame's own median-cut palette.  No host synchronisation."""
    frames = _require_u8("gif_quantize: frames", frames)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise NerfHipError("gif_quantize: expected (F, H, W, 3), got %s" % (tuple(frames.shape),))
    F, H, W = frames.shape[:3]
    dev = frames.device
    lib = _lib.load()
    ws = workspace if workspace is not None else gif_workspace(F, H, W, dev)
    indices = torch.empty((F, H * W), device=dev, dtype=torch.uint8)
    palettes = torch.empty((F, 256, 3), device=dev, dtype=torch.uint8)
    boxes = torch.empty((F,), device=dev, dtype=torch.int32)
    check(lib.nerfhip_gif_quantize(ptr(frames), F, H, W, ptr(indices), ptr(palettes), ptr(boxes), ptr(ws), stream_ptr()),
          "nerfhip_gif_quantize")
    return indices, palettes, boxes


@device_guard
def gif_lzw(indices, H, W, workspace=None):
    """nerfhip_gif_lzw: indices (F, H*W) uint8 on the device -> (data (F, stride) uint8, lengths (F,) int32): per frame the
    sub-blocked LZW image data (strips of GIF_STRIP pixels, each behind a clear code) and its length in bytes; the bytes behind
    a frame's length are undefined.  No host synchronisation: a length of -1 (a dictionary probe bound was hit) is for the
    caller to check when it reads the lengths (imageio_min.gif_bytes does)."""
    indices = _require_u8("gif_lzw: indices", indices)
    if indices.dim() != 2 or indices.shape[1] != H * W:
        raise NerfHipError("gif_lzw: expected (F, %d) indices for %d x %d frames, got %s" % (H * W, H, W, tuple(indices.shape)))
    F = indices.shape[0]
    dev = indices.device
    lib = _lib.load()
    ws = workspace if workspace is not None else gif_workspace(F, H, W, dev)
    stride = lib.nerfhip_gif_data_stride(H, W)
    data = torch.empty((F, stride), device=dev, dtype=torch.uint8)
    lengths = torch.empty((F,), device=dev, dtype=torch.int32)
    check(lib.nerfhip_gif_lzw(ptr(indices), F, H, W, ptr(data), ptr(lengths), ptr(ws), stream_ptr()), "nerfhip_gif_lzw")
    return data, lengths


# ------------------------------------------------------------------------------- PNG encoder (eval.py:138)
PNG_STRIP = 8192            # NERFHIP_PNG_STRIP


def png_workspace(n, stream_bytes, device):
    """The scratch buffer png_deflate takes (about 15.9 KB per 8192-byte strip)."""
    nbytes = _lib.load().nerfhip_png_workspace_bytes(n, stream_bytes)
    if n > 0 and nbytes == 0:
        raise NerfHipError("png: %d streams of %d bytes are refused (1..2^31 - 1 bytes, at most 65535 streams)" % (n, stream_bytes))
    return torch.empty(max(1, nbytes // 8), device=device, dtype=torch.int64)


@device_guard
def png_filter(images):
    """nerfhip_png_filter: images (n, H, W, C) uint8 on the device, C in (1, 3, 4) -> streams (n, H * (1 + W*C)) uint8: every
    scanline behind the type of the filter with the smallest absolute sum.  No host synchronisation."""
    images = _require_u8("png_filter: images", images)
    if images.dim() != 4 or images.shape[3] not in (1, 3, 4) or images.shape[1] < 1 or images.shape[2] < 1:
        raise NerfHipError("png_filter: expected (n, H, W, C) with H, W >= 1 and C in (1, 3, 4), got %s" % (tuple(images.shape),))
    n, H, W, C = images.shape
    if H * (1 + W * C) >= 2 ** 31 or n > 65535:
        raise NerfHipError("png_filter: %d images of %d x %d x %d are refused (H * (1 + W*C) < 2^31, n <= 65535)" % (n, H, W, C))
    streams = torch.empty((n, H * (1 + W * C)), device=images.device, dtype=torch.uint8)
    check(_lib.load().nerfhip_png_filter(ptr(images), n, H, W, C, ptr(streams), stream_ptr()), "nerfhip_png_filter")
    return streams


@device_guard
def png_deflate(streams, workspace=None, meta=None):
    """nerfhip_png_deflate: streams (n, stream_bytes) uint8 on the device -> (data (n, stride) uint8, lengths (n,) int32,
    adler (n,) int32).  Per stream the raw deflate data (strips of PNG_STRIP bytes, one dynamic-Huffman block each), its length
    in bytes and the stream's Adler-32 — the 32 bits of the unsigned sum in an int32 (`& 0xffffffff` on the host); the bytes
    behind a length are undefined.  lengths and adler are rows 0 and 1 of `meta`, a (2, n) int32 device tensor (allocated when
    not given), so that one copy brings both to the host.  No host synchronisation: a length of -1 (a strip exceeded its worst
    case) is for the caller to check when it reads the lengths (imageio_min.png_bytes_device does)."""
    streams = _require_u8("png_deflate: streams", streams)
    if streams.dim() != 2 or streams.shape[1] < 1:
        raise NerfHipError("png_deflate: expected (n, stream_bytes >= 1), got %s" % (tuple(streams.shape),))
    n, nbytes = streams.shape
    dev = streams.device
    lib = _lib.load()
    ws = workspace if workspace is not None else png_workspace(n, nbytes, dev)
    if not torch.is_tensor(ws) or ws.device != dev or ws.numel() * ws.element_size() < lib.nerfhip_png_workspace_bytes(n, nbytes):
        raise NerfHipError("png_deflate: the workspace must be a tensor on %s of png_workspace(%d, %d)'s size" % (dev, n, nbytes))
    stride = lib.nerfhip_png_data_stride(nbytes)
    if meta is None:
        meta = torch.empty((2, n), device=dev, dtype=torch.int32)
    elif not torch.is_tensor(meta) or meta.device != dev or meta.dtype != torch.int32 or tuple(meta.shape) != (2, n) \
            or not meta.is_contiguous():
        raise NerfHipError("png_deflate: meta must be a contiguous (2, %d) int32 tensor on %s" % (n, dev))
    data = torch.empty((n, stride), device=dev, dtype=torch.uint8)
    lengths, adler = meta[0], meta[1]
    check(lib.nerfhip_png_deflate(ptr(streams), n, nbytes, ptr(data), ptr(lengths), ptr(adler), ptr(ws), stream_ptr()),
          "nerfhip_png_deflate")
    return data, lengths, adler


# ------------------------------------------------------------------------------- scene loading (datasets/blender.py:47-58, 90-95)
def _require_u8(name, t):
    if not torch.is_tensor(t):
        raise NerfHipError("%s: expected a torch tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise NerfHipError("nerf_pl_amd runs on MI355X only: %s is a %s tensor (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.uint8:
        raise NerfHipError("%s: expected uint8, got %s" % (name, t.dtype))
    return _c(t)


@device_guard
def decode_png_batch(streams, H, W, ch, return_flags=False):
    """nerfhip_png_unfilter: `streams` (n, H * (1 + W * ch)) uint8 on the device — the inflated IDAT data of n PNG files of one
    size (imageio_min.png_inflate) — -> (n, H, W, ch) uint8 pixels.  A scanline with a filter type above 4 raises; with
    return_flags the per-image int32 flags come back beside the pixels instead (no device-to-host read then)."""
    streams = _require_u8("decode_png_batch streams", streams)
    H, W, ch = int(H), int(W), int(ch)
    if ch not in (1, 3, 4) or H < 1 or W < 1:
        raise NerfHipError("decode_png_batch: H, W >= 1 and ch in (1, 3, 4), got %d x %d x %d" % (H, W, ch))
    if streams.dim() != 2 or streams.shape[1] != H * (1 + W * ch):
        raise NerfHipError("decode_png_batch: expected (n, %d) bytes per %d x %d x %d image, got %s"
                           % (H * (1 + W * ch), H, W, ch, tuple(streams.shape)))
    n = streams.shape[0]
    out = torch.empty(n, H, W, ch, device=streams.device, dtype=torch.uint8)
    flags = torch.empty(n, device=streams.device, dtype=torch.int32)
    check(_lib.load().nerfhip_png_unfilter(ptr(streams), ptr(out), ptr(flags), n, H, W, ch, stream_ptr()), "nerfhip_png_unfilter")
    if return_flags:
        return out, flags
    if n and bool(flags.any()):
        raise NerfHipError("decode_png_batch: image(s) %s hold a scanline filter type above 4" % flags.nonzero().flatten().tolist())
    return out


_TAPS = {}


def _lanczos_taps_device(in_size, out_size, device):
    key = (int(in_size), int(out_size), str(device))
    if key not in _TAPS:
        from .imageio_min import lanczos_taps
        if len(_TAPS) > 16:
            _TAPS.clear()
        _TAPS[key] = tuple(torch.from_numpy(a).to(device) for a in lanczos_taps(in_size, out_size))
    return _TAPS[key]


@device_guard
def resize_rgba_lanczos(u8, w, h):
    """nerfhip_resize_rgba_lanczos: `PIL.Image.resize((w, h), Image.LANCZOS)` of 8-bit RGBA images (n, H, W, 4) or (H, W, 4) on
    the device, byte for byte (equal size: a copy)."""
    u8 = _require_u8("resize_rgba_lanczos image", u8)
    if u8.dim() not in (3, 4) or u8.shape[-1] != 4:
        raise NerfHipError("resize_rgba_lanczos: expected (n, H, W, 4) or (H, W, 4), got %s" % (tuple(u8.shape),))
    w, h = int(w), int(h)
    single = u8.dim() == 3
    n, H, W = (1,) + tuple(u8.shape[:2]) if single else tuple(u8.shape[:3])
    if min(w, h, H, W) < 1:
        raise NerfHipError("resize_rgba_lanczos: empty image")
    dev = u8.device
    out = torch.empty(n, h, w, 4, device=dev, dtype=torch.uint8)
    th = _lanczos_taps_device(W, w, dev) if W != w else (None, None, None)
    tv = _lanczos_taps_device(H, h, dev) if H != h else (None, None, None)
    ws = torch.empty(n, H, w, 4, device=dev, dtype=torch.uint8) if (W != w and H != h) else None
    check(_lib.load().nerfhip_resize_rgba_lanczos(ptr(u8), ptr(out), ptr(ws), n, H, W, h, w, ptr(th[0]), ptr(th[1]), ptr(th[2]),
                                                  th[2].shape[1] if th[2] is not None else 0, ptr(tv[0]), ptr(tv[1]), ptr(tv[2]),
                                                  tv[2].shape[1] if tv[2] is not None else 0, stream_ptr()),
          "nerfhip_resize_rgba_lanczos")
    return out[0] if single else out


@device_guard
def rgba_to_rgb_white(u8, out=None):
    """nerfhip_rgba_to_rgb_white: (..., 4) uint8 RGBA -> (rgb (pixels, 3) float32 = ToTensor + the blend onto white of
    blender.py:56-58, valid_mask (pixels,) bool = alpha > 0).  `out`: a contiguous (pixels, 3) float32 slice to write into."""
    u8 = _require_u8("rgba_to_rgb_white image", u8)
    if u8.dim() < 1 or u8.shape[-1] != 4:
        raise NerfHipError("rgba_to_rgb_white: expected (..., 4) uint8, got %s" % (tuple(u8.shape),))
    n = u8.numel() // 4
    if out is None:
        out = torch.empty(n, 3, device=u8.device, dtype=torch.float32)
    else:
        require_gpu(out)
        if out.device != u8.device or tuple(out.shape) != (n, 3) or not out.is_contiguous():
            raise NerfHipError("rgba_to_rgb_white: out must be a contiguous (%d, 3) float32 tensor on %s" % (n, u8.device))
    mask = torch.empty(n, device=u8.device, dtype=torch.uint8)
    check(_lib.load().nerfhip_rgba_to_rgb_white(ptr(u8), ptr(out), ptr(mask), n, stream_ptr()), "nerfhip_rgba_to_rgb_white")
    return out, mask.view(torch.bool)


# --------------------------------------------------------------------------------------- JPEG decoding (datasets/llff.py:226, 312)
def jpeg_entropy_decode(parsed):
    """nerfhip_jpeg_entropy_decode (host, no GPU): the dict of imageio_min.jpeg_parse -> [per component: (blocks_y, blocks_x, 64)
    int16 numpy coefficient blocks], natural order, DC prediction resolved, not dequantised, padded to whole MCUs."""
    import numpy as np
    comps = parsed["components"]
    mx, my = int(parsed["mcus_x"]), int(parsed["mcus_y"])
    table = np.zeros((8, 272), np.uint8)
    mask = 0
    for (tc, th), (counts, symbols) in parsed["huffman"].items():
        table[4 * tc + th, :16] = counts
        table[4 * tc + th, 16:16 + len(symbols)] = symbols
        mask |= 1 << (4 * tc + th)
    comp = np.ascontiguousarray([[c[1], c[2], c[4], c[5]] for c in comps], dtype=np.int32)
    coef = [np.zeros((my * c[2], mx * c[1], 64), np.int16) for c in comps]
    scan = np.frombuffer(parsed["scan"], np.uint8)
    ptrs = (ctypes.c_void_p * len(comps))(*[a.ctypes.data for a in coef])
    caps = (ctypes.c_int64 * len(comps))(*[a.shape[0] * a.shape[1] for a in coef])
    code = _lib.load().nerfhip_jpeg_entropy_decode(scan.ctypes.data, len(scan), len(comps), comp.ctypes.data, table.ctypes.data, mask,
                                                   mx, my, int(parsed["restart_interval"]), ptrs, caps)
    if code != 0:
        msg = _lib.load().nerfhip_error_string(code).decode()
        raise NerfHipError("%s: nerfhip_jpeg_entropy_decode failed: %s (code %d)" % (parsed.get("name", "JPEG data"), msg, code))
    return coef


def _require_i16(name, t, device, shape):
    if not torch.is_tensor(t):
        raise NerfHipError("%s: expected a torch tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise NerfHipError("nerf_pl_amd runs on MI355X only: %s is a %s tensor (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.int16 or tuple(t.shape) != tuple(shape) or (device is not None and t.device != device):
        raise NerfHipError("%s: expected int16 %s on %s, got %s %s on %s" % (name, tuple(shape), device, t.dtype, tuple(t.shape), t.device))
    return _c(t)


@device_guard
def decode_jpeg_batch(coefs, quant, H, W, hs=1, vs=1):
    """nerfhip_jpeg_decode: n JPEG images of one size and sampling -> (n, H, W, 4) uint8 RGBX (X = 255) on the device, the bytes
    of PIL's `Image.open(p).convert('RGB')`.  coefs: per component (1, or 3 = Y Cb Cr) an int16 tensor (n, blocks_c, 64) — or
    (n, blocks_y, blocks_x, 64) — as jpeg_entropy_decode leaves them; quant (n, n_comp, 64) int16: each image's quantisation
    tables in natural order, per component; hs, vs: the luma sampling factors (chroma is 1 x 1)."""
    if torch.is_tensor(coefs):
        coefs = [coefs]
    coefs = list(coefs)
    H, W, hs, vs = int(H), int(W), int(hs), int(vs)
    n_comp = len(coefs)
    lib = _lib.load()
    plane_bytes = lib.nerfhip_jpeg_planes_bytes(H, W, n_comp, hs, vs) if n_comp in (1, 3) else 0
    if plane_bytes == 0:
        raise NerfHipError("decode_jpeg_batch: %d component(s) of %d x %d with luma sampling %dx%d is not supported (1 component, "
                           "or 3 with 1x1, 2x1 or 2x2)" % (n_comp, W, H, hs, vs))
    if not torch.is_tensor(coefs[0]) or coefs[0].dim() < 2:
        raise NerfHipError("decode_jpeg_batch: coefs must be (n, blocks, 64) int16 tensors")
    n, dev = coefs[0].shape[0], coefs[0].device
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    flat = []
    for c, t in enumerate(coefs):
        blocks = mx * my * (hs * vs if c == 0 else 1)
        if torch.is_tensor(t) and t.dim() == 4:
            t = t.reshape(t.shape[0], -1, 64)
        flat.append(_require_i16("decode_jpeg_batch coefs[%d]" % c, t, dev, (n, blocks, 64)))
    quant = _require_i16("decode_jpeg_batch quant", quant, dev, (n, n_comp, 64))
    out = torch.empty(n, H, W, 4, device=dev, dtype=torch.uint8)
    planes = torch.empty(n * plane_bytes, device=dev, dtype=torch.uint8)
    check(lib.nerfhip_jpeg_decode(ptr(flat[0]), ptr(flat[1]) if n_comp == 3 else None, ptr(flat[2]) if n_comp == 3 else None,
                                  ptr(quant), ptr(planes), ptr(out), n, H, W, n_comp, hs, vs, stream_ptr()), "nerfhip_jpeg_decode")
    return out


# ----------------------------------------------------------------------- the entropy stage on the device (csrc/jpeg_entropy.hip)
def _jpeg_batch_arrays(what, parsed_list, subseq_bits):
    """What nerfhip_jpeg_batch holds for these files (dicts of imageio_min.jpeg_parse, all of one size, sampling and component
    count) as numpy arrays: (scans, offsets, huffman, masks, restart, comp, (mx, my), max_scan_bytes, max_intervals)."""
    import numpy as np
    parsed_list = list(parsed_list)
    if not parsed_list:
        raise NerfHipError("%s: no files" % what)
    subseq_bits = int(subseq_bits)
    if subseq_bits < 32 or subseq_bits > 4096 or subseq_bits % 32:
        raise NerfHipError("%s: subseq_bits must be a multiple of 32 between 32 and 4096, got %d" % (what, subseq_bits))

    def shape_of(p):
        return (int(p["width"]), int(p["height"]), int(p["mcus_x"]), int(p["mcus_y"]), tuple((c[1], c[2]) for c in p["components"]))

    def name_of(i):
        return parsed_list[i].get("name", "file %d of the batch" % i)
    first = parsed_list[0]
    for i, p in enumerate(parsed_list[1:], 1):
        if shape_of(p) != shape_of(first):
            raise NerfHipError("%s: %s (%d x %d, sampling %s) and %s (%d x %d, sampling %s) differ in size, sampling or component "
                               "count: one batch holds files of one shape" % ((what, name_of(0)) + shape_of(first)[:2]
                                                                              + (shape_of(first)[4], name_of(i)) + shape_of(p)[:2]
                                                                              + (shape_of(p)[4],)))
    n = len(parsed_list)
    mx, my = int(first["mcus_x"]), int(first["mcus_y"])
    huffman = np.zeros((n, 8, 272), np.uint8)
    masks = np.zeros(n, np.int32)
    restart = np.zeros(n, np.int32)
    offsets = np.zeros(n + 1, np.int64)
    for i, p in enumerate(parsed_list):
        for (tc, th), (counts, symbols) in p["huffman"].items():
            huffman[i, 4 * tc + th, :16] = counts
            huffman[i, 4 * tc + th, 16:16 + len(symbols)] = symbols
            masks[i] |= 1 << (4 * tc + th)
        restart[i] = int(p["restart_interval"])
        offsets[i + 1] = offsets[i] + len(p["scan"])
        if len(p["scan"]) < 1:
            raise NerfHipError("%s: %s has an empty scan" % (what, name_of(i)))
    scans = np.frombuffer(b"".join(bytes(p["scan"]) for p in parsed_list), np.uint8)
    # the component rows may name different tables from file to file only if the tables' ids do: they are the scan header's
    comp = np.ascontiguousarray([[c[1], c[2], c[4], c[5]] for c in first["components"]], dtype=np.int32)
    for i, p in enumerate(parsed_list[1:], 1):
        if [tuple(c[4:6]) for c in p["components"]] != [tuple(c[4:6]) for c in first["components"]]:
            raise NerfHipError("%s: %s and %s assign their Huffman tables to the components differently" % (what, name_of(0), name_of(i)))
    n_mcu = mx * my
    max_intervals = max(-(-n_mcu // int(r)) if r > 0 else 1 for r in restart)
    return scans, offsets, huffman, masks, restart, comp, (mx, my), int(np.diff(offsets).max()), int(max_intervals)


def _jpeg_batch_struct(ptr_of, arrays, subseq_bits, workspace, status, progress):
    scans, offsets, huffman, masks, restart, comp, (mx, my), max_scan, max_int = arrays
    b = _lib.JpegBatch()
    b.scans, b.offsets, b.huffman, b.huffman_masks, b.restart_intervals = (ptr_of(scans), ptr_of(offsets), ptr_of(huffman), ptr_of(masks),
                                                                           ptr_of(restart))
    b.total_bytes, b.max_scan_bytes, b.max_intervals, b.n_images, b.n_comp = int(scans.shape[0]), max_scan, max_int, len(masks), len(comp)
    for i, v in enumerate(comp.reshape(-1).tolist()):
        b.comp[i] = v
    b.mcus_x, b.mcus_y, b.subseq_bits = mx, my, int(subseq_bits)
    b.workspace, b.status, b.progress = ptr_of(workspace), ptr_of(status), ptr_of(progress)
    return b


def _jpeg_status_error(what, parsed_list, status):
    bad = [i for i, s in enumerate(status) if s != 0]
    if bad:
        lib = _lib.load()
        raise NerfHipError("; ".join("%s: %s failed: %s (code %d)" % (parsed_list[i].get("name", "file %d of the batch" % i), what,
                                                                      lib.nerfhip_error_string(int(status[i])).decode(), int(status[i]))
                                     for i in bad))


def jpeg_entropy_decode_split(parsed_list, subseq_bits=1024, return_status=False):
    """nerfhip_jpeg_entropy_decode_split (host, no GPU): the device entropy decoder's four steps run on the CPU over the same
    subsequences -> per component an (n, blocks_y, blocks_x, 64) int16 numpy array.  For tests of the algorithm and its error
    paths on a machine without a GPU; jpeg_entropy_decode is the host decoder to use.  return_status: (coefs, status (n,), rounds
    between workgroups) instead of raising for a damaged file."""
    import numpy as np
    what = "jpeg_entropy_decode_split"
    parsed_list = list(parsed_list)
    arrays = _jpeg_batch_arrays(what, parsed_list, subseq_bits)
    comp, (mx, my) = arrays[5], arrays[6]
    n = len(parsed_list)
    lib = _lib.load()
    nbytes = lib.nerfhip_jpeg_entropy_workspace_bytes(n, arrays[7], arrays[8], int(subseq_bits))
    if nbytes == 0:
        raise NerfHipError("%s: sizes refused (scan of %d bytes, %d restart intervals)" % (what, arrays[7], arrays[8]))
    raw = np.zeros(nbytes + 256, np.uint8)
    workspace = raw[(-raw.ctypes.data) % 256:][:nbytes]
    status, progress = np.zeros(n, np.int32), np.zeros(1, np.int32)
    coefs = [np.zeros((n, my * c[1], mx * c[0], 64), np.int16) for c in comp]
    b = _jpeg_batch_struct(lambda a: a.ctypes.data, arrays, subseq_bits, workspace, status, progress)
    check(lib.nerfhip_jpeg_entropy_decode_split(ctypes.addressof(b), *[coefs[c].ctypes.data if c < len(coefs) else None for c in range(3)]),
          "nerfhip_jpeg_entropy_decode_split")
    if return_status:
        return coefs, status, int(progress[0])
    _jpeg_status_error("nerfhip_jpeg_entropy_decode_split", parsed_list, status)
    return coefs


_JPEG_ROUNDS_PER_CALL = 4     # rounds between workgroups enqueued before the host looks at the progress word


def jpeg_entropy_decode_batch(parsed_list, device, subseq_bits=1024, return_rounds=False):
    """nerfhip_jpeg_entropy_sync / _rounds / _emit: the scans of n JPEG files of one size and sampling (dicts of
    imageio_min.jpeg_parse) are uploaded as the files' bytes and Huffman-decoded on the device -> per component an
    (n, blocks_y, blocks_x, 64) int16 device tensor, bit-equal to jpeg_entropy_decode's and ready for decode_jpeg_batch.
    One host synchronisation per batch (status and progress); more rounds between workgroups are enqueued only while the progress
    word asks, at most (workgroups + 1).  subseq_bits: 1024 from the sweep of DESIGN §11 (256 to 1024 measure alike on a 12 MP
    file, 2048 and 4096 slower).  Raises NerfHipError naming every file whose scan is damaged.  return_rounds: also the
    number of rounds between workgroups that ran."""
    import numpy as np
    what = "jpeg_entropy_decode_batch"
    device = torch.device(device)
    if device.type != "cuda":
        raise NerfHipError("nerf_pl_amd runs on MI355X only: %s got device %s (no CPU fallback)" % (what, device))
    parsed_list = list(parsed_list)
    arrays = _jpeg_batch_arrays(what, parsed_list, subseq_bits)
    comp, (mx, my) = arrays[5], arrays[6]
    n = len(parsed_list)
    lib = _lib.load()
    nbytes = lib.nerfhip_jpeg_entropy_workspace_bytes(n, arrays[7], arrays[8], int(subseq_bits))
    wgs = lib.nerfhip_jpeg_entropy_workgroups(arrays[7], arrays[8], int(subseq_bits))
    if nbytes == 0 or wgs == 0:
        raise NerfHipError("%s: sizes refused (scan of %d bytes, %d restart intervals)" % (what, arrays[7], arrays[8]))
    with torch.cuda.device(device):
        dev = [torch.from_numpy(a.copy() if not a.flags.writeable else a).to(device) for a in arrays[:5]]
        workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)
        flags = torch.zeros(n + 1, device=device, dtype=torch.int32)             # status (n) and the progress word
        coefs = [torch.zeros((n, my * int(c[1]), mx * int(c[0]), 64), device=device, dtype=torch.int16) for c in comp]
        b = _jpeg_batch_struct(ptr, tuple(dev) + arrays[5:], subseq_bits, workspace, flags, flags[n:])
        b.status, b.progress = flags.data_ptr(), flags.data_ptr() + 4 * n
        enqueued = min(_JPEG_ROUNDS_PER_CALL, wgs + 1) if wgs > 1 else 0
        check(lib.nerfhip_jpeg_entropy_sync(ctypes.addressof(b), enqueued, stream_ptr()), "nerfhip_jpeg_entropy_sync")
        host = flags.cpu().numpy()
        while wgs > 1 and host[n] >= enqueued and enqueued < wgs + 1 and not host[:n].all():
            more = min(_JPEG_ROUNDS_PER_CALL, wgs + 1 - enqueued)
            check(lib.nerfhip_jpeg_entropy_rounds(ctypes.addressof(b), enqueued + 1, more, stream_ptr()), "nerfhip_jpeg_entropy_rounds")
            enqueued += more
            host = flags.cpu().numpy()
        check(lib.nerfhip_jpeg_entropy_emit(ctypes.addressof(b), *[ptr(coefs[c]) if c < len(coefs) else None for c in range(3)],
                                            stream_ptr()), "nerfhip_jpeg_entropy_emit")
        status = flags[:n].cpu().numpy()
    _jpeg_status_error("nerfhip_jpeg_entropy_emit", parsed_list, status)
    if return_rounds:
        return coefs, int(host[n]) + 1 if wgs > 1 else 0
    return coefs


# --------------------------------------------------------------------------- inflating PNG data (csrc/inflate.hip)
def _inflate_arrays(what, streams, out_bytes):
    """The zlib streams (bytes-like) joined: (data uint8 (total,), offsets int64 (n + 1,))."""
    import numpy as np
    streams = [bytes(s) for s in streams]
    out_bytes = int(out_bytes)
    if out_bytes < 0:
        raise NerfHipError("%s: out_bytes must not be negative, got %d" % (what, out_bytes))
    if len(streams) > 65535:
        raise NerfHipError("%s: at most 65535 streams per call, got %d" % (what, len(streams)))
    offsets = np.zeros(len(streams) + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    return np.frombuffer(b"".join(streams), np.uint8), offsets, out_bytes


def _inflate_status_error(what, names, status):
    bad = [i for i, s in enumerate(status) if s != 0]
    if bad:
        lib = _lib.load()
        raise NerfHipError("; ".join("%s: %s failed: %s (code %d)" % (names[i] if names is not None else "stream %d of the batch" % i, what,
                                                                      lib.nerfhip_error_string(int(status[i])).decode(), int(status[i]))
                                     for i in bad))


def inflate_host(streams, out_bytes, return_status=False, names=None):
    """nerfhip_inflate_host (host, no GPU): n zlib streams -> (n, out_bytes) uint8 numpy array, by the device decoder's own
    per-symbol code with the lanes in lockstep.  For tests of the algorithm and its error paths on a machine without a GPU;
    zlib.decompress is the host decoder to use.  return_status: (out, status (n,)) instead of raising for a damaged stream."""
    import numpy as np
    data, offsets, out_bytes = _inflate_arrays("inflate_host", streams, out_bytes)
    n = len(offsets) - 1
    out = np.zeros((n, out_bytes), np.uint8)
    status = np.zeros(n, np.int32)
    check(_lib.load().nerfhip_inflate_host(data.ctypes.data if data.size else None, offsets.ctypes.data, int(data.size), n,
                                           out.ctypes.data if out.size else None, out_bytes, out_bytes, status.ctypes.data),
          "nerfhip_inflate_host")
    if return_status:
        return out, status
    _inflate_status_error("nerfhip_inflate_host", names, status)
    return out


def inflate_batch(streams, out_bytes, device, return_status=False, names=None):
    """nerfhip_inflate: n zlib streams (bytes-like, e.g. imageio_min.png_idat's) are uploaded joined, in one copy with their
    offsets, and inflated on the device -> (n, out_bytes) uint8 device tensor, ready for decode_png_batch.  One status read per
    batch.  Raises NerfHipError naming every damaged stream (by `names[i]` where given); return_status: (out, status (n,) numpy)
    instead."""
    import numpy as np
    what = "inflate_batch"
    device = torch.device(device)
    if device.type != "cuda":
        raise NerfHipError("nerf_pl_amd runs on MI355X only: %s got device %s (no CPU fallback)" % (what, device))
    data, offsets, out_bytes = _inflate_arrays(what, streams, out_bytes)
    n = len(offsets) - 1
    head = 8 * (n + 1)                                   # one upload: the offsets in front of the bytes
    packed = np.empty(head + data.size, np.uint8)
    packed[:head] = offsets.view(np.uint8)
    packed[head:] = data
    with torch.cuda.device(device):
        up = torch.from_numpy(packed).to(device)
        out = torch.empty((n, out_bytes), device=device, dtype=torch.uint8)
        status = torch.zeros(max(n, 1), device=device, dtype=torch.int32)
        check(_lib.load().nerfhip_inflate(up.data_ptr() + head, up.data_ptr(), int(data.size), n, out.data_ptr(), out_bytes, out_bytes,
                                          status.data_ptr(), stream_ptr()), "nerfhip_inflate")
        host = status[:n].cpu().numpy()
    if return_status:
        return out, host
    _inflate_status_error("nerfhip_inflate", names, host)
    return out


# ------------------------------------------------------------ skipping empty space at eval (csrc/occupancy.hip)
OCCUPANCY_MAX_N = 1025


def occupancy_words(M):
    """int32 words of the bitfield of an M^3-cell grid."""
    return (int(M) ** 3 + 31) // 32


def _ranges_arg(what, ranges):
    """((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)) -> the 6 host floats of the C call."""
    flat = [float(v) for r in ranges for v in r]
    if len(flat) != 6:
        raise ValueError("%s: ranges must be three (lo, hi) pairs, got %r" % (what, ranges))
    return (ctypes.c_float * 6)(*flat)


def _require_dev(what, name, t, dtype, shape_tail=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise NerfHipError("nerf_pl_amd runs on MI355X only: %s needs %s on the device (no CPU fallback)" % (what, name))
    if t.dtype != dtype or (shape_tail is not None and tuple(t.shape[1:]) != shape_tail):
        raise NerfHipError("%s: %s must be %s (n%s), got %s %s" % (what, name, dtype, "".join(", %d" % s for s in shape_tail or ()),
                                                                    tuple(t.shape), t.dtype))
    return _c(t)


def _same_device(what, *tensors):
    """the tensors of one call live on one GPU: a pointer of another device would be an illegal access, not an error"""
    devs = {t.device for t in tensors if t is not None}
    if len(devs) > 1:
        raise NerfHipError("%s: tensors of one call live on different GPUs (%s)" % (what, ", ".join(sorted(str(d) for d in devs))))


def _np16(a, dtype):
    """a C-contiguous numpy array of `dtype` whose data is 16-byte aligned, as device buffers are"""
    import numpy as np
    a = np.ascontiguousarray(a, dtype)
    if a.ctypes.data & 15:
        buf = np.empty(a.nbytes + 16, np.uint8)
        off = (-buf.ctypes.data) & 15
        out = buf[off:off + a.nbytes].view(dtype).reshape(a.shape)
        out[...] = a
        a = out
    return a


class _DeviceArrays:
    """The arrays of a device call: tensors on one GPU.  A ray unit's device wrapper and its _host twin share one body (the
    `_name(B, ...)` functions below) written against this and `_HostArrays`; dtypes are named as numpy names them."""
    suffix = ""

    @staticmethod
    def array(what, name, a, dtype, tail=None):
        """`a` as the call reads it: (n,) + tail of `dtype` (tail None: any shape).  NerfHipError for anything else."""
        return _require_dev(what, name, a, getattr(torch, dtype), tail)

    same_device = staticmethod(_same_device)

    @staticmethod
    def empty(like, shape, dtype):
        return torch.empty(shape, device=like.device, dtype=getattr(torch, dtype))

    ptr = staticmethod(ptr)

    @staticmethod
    def sort(keys):
        return torch.sort(keys)[0]

    @staticmethod
    def sort_stable(keys):
        """(the keys in ascending order, the position each came from); equal keys keep their order"""
        return torch.sort(keys, stable=True)

    @staticmethod
    def take(a, index):
        return a[index]

    @staticmethod
    def host(a):
        """a small array read back to the host (synchronises)"""
        return a.cpu().numpy()

    @staticmethod
    def call(name, *args):
        check(getattr(_lib.load(), name)(*args, stream_ptr()), name)


class _HostArrays:
    """The arrays of a _host call: numpy, 16-byte aligned as device buffers are."""
    suffix = "_host"

    @staticmethod
    def array(what, name, a, dtype, tail=None):
        a = _np16(a, dtype)
        if tail is not None and (a.ndim != 1 + len(tail) or a.shape[1:] != tail):
            raise ValueError("%s: %s must be (n%s), got %s" % (what, name, "".join(", %d" % s for s in tail), a.shape))
        return a

    same_device = staticmethod(lambda what, *arrays: None)

    @staticmethod
    def empty(like, shape, dtype):
        import numpy as np
        return _np16(np.zeros(shape, dtype), dtype)

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data

    @staticmethod
    def sort(keys):
        import numpy as np
        return _np16(np.sort(keys), keys.dtype)

    @staticmethod
    def sort_stable(keys):
        import numpy as np
        order = np.argsort(keys, kind="stable")
        return _np16(keys[order], keys.dtype), order

    @staticmethod
    def take(a, index):
        return _np16(a[index], a.dtype)

    @staticmethod
    def host(a):
        return a

    @staticmethod
    def call(name, *args):
        check(getattr(_lib.load(), name + "_host")(*args), name + "_host")


def _numel(a):
    return a.numel() if torch.is_tensor(a) else a.size


@device_guard
def occupancy_build(sigma, threshold=0.0, dilate=1):
    """nerfhip_occupancy_build: sigma (N, N, N) fp32 on the device, indexed [iy, ix, iz] (grid.sigma_grid) -> the bitfield of its
    (N-1)^3 cells, (ceil((N-1)^3 / 32),) int32 on the device."""
    sigma = _require_dev("occupancy_build", "sigma", sigma, torch.float32)
    if sigma.dim() != 3 or len(set(sigma.shape)) != 1 or not 2 <= sigma.shape[0] <= OCCUPANCY_MAX_N:
        raise ValueError("occupancy_build: sigma must be (N, N, N) with 2 <= N <= %d, got %s" % (OCCUPANCY_MAX_N, tuple(sigma.shape)))
    if int(dilate) < 0:
        raise ValueError("occupancy_build: dilate must be >= 0, got %r" % (dilate,))
    lib = _lib.load()
    N = sigma.shape[0]
    words = torch.empty(occupancy_words(N - 1), device=sigma.device, dtype=torch.int32)
    ws = torch.empty(lib.nerfhip_occupancy_workspace_bytes(N), device=sigma.device, dtype=torch.uint8)
    check(lib.nerfhip_occupancy_build(ptr(sigma), N, float(threshold), int(dilate), ptr(words), ptr(ws), stream_ptr()),
          "nerfhip_occupancy_build")
    return words


def _cull_grid_args(what, words, M, ranges):
    """`words` (a tensor or an array) must hold the whole grid: a short one would be an out-of-bounds read, not an error."""
    M = int(M)
    if 1 <= M < OCCUPANCY_MAX_N and _numel(words) < occupancy_words(M):
        raise ValueError("%s: %d words for a grid of %d^3 cells (needs %d)" % (what, _numel(words), M, occupancy_words(M)))
    return M, _ranges_arg(what, ranges)


def _cull_rays(B, rays, words, M, ranges):
    what = "cull_rays" + B.suffix
    rays = B.array(what, "rays", rays, "float32", (8,))
    words = B.array(what, "words", words, "int32")
    B.same_device(what, rays, words)
    M, rg = _cull_grid_args(what, words, M, ranges)
    n = rays.shape[0]
    hit, t0, t1 = B.empty(rays, n, "uint8"), B.empty(rays, n, "float32"), B.empty(rays, n, "float32")
    B.call("nerfhip_cull_rays", B.ptr(rays), n, B.ptr(words), M, rg, B.ptr(hit), B.ptr(t0), B.ptr(t1))
    return hit, t0, t1


@device_guard
def cull_rays(rays, words, M, ranges):
    """nerfhip_cull_rays: rays (n, 8) fp32 against the bitfield `words` of an M^3 grid over `ranges` -> (hit (n,) uint8,
    t0 (n,), t1 (n,)) on the device."""
    return _cull_rays(_DeviceArrays, rays, words, M, ranges)


def cull_rays_host(rays, words, M, ranges):
    """nerfhip_cull_rays_host (host, no GPU): numpy rays (n, 8) float32 and int32 words -> numpy (hit, t0, t1), by the kernel's
    own per-ray routine.  For tests of the traversal on a machine without a GPU."""
    return _cull_rays(_HostArrays, rays, words, M, ranges)


@device_guard
def cull_compact(hit, rays, t0=None, t1=None):
    """nerfhip_cull_compact: -> (slot (n,) int32, index (n,) int32, rays_out (n, 8), n_hit (1,) int32), all on the device and
    sized for every ray hitting: the first n_hit rows of index and rays_out are written.  t0 / t1 None: the rows keep their own
    near / far.  No host synchronisation."""
    rays = _require_dev("cull_compact", "rays", rays, torch.float32, (8,))
    hit = _require_dev("cull_compact", "hit", hit, torch.uint8, ())
    t0 = None if t0 is None else _require_dev("cull_compact", "t0", t0, torch.float32, ())
    t1 = None if t1 is None else _require_dev("cull_compact", "t1", t1, torch.float32, ())
    n = rays.shape[0]
    _same_device("cull_compact", rays, hit, t0, t1)
    if any(t.shape[0] != n for t in (hit, t0, t1) if t is not None):
        raise ValueError("cull_compact: hit, t0, t1 must have one entry per ray (%d)" % n)
    dev = rays.device
    lib = _lib.load()
    slot = torch.empty(n, device=dev, dtype=torch.int32)
    index = torch.empty(n, device=dev, dtype=torch.int32)
    rays_out = torch.empty(n, 8, device=dev, dtype=torch.float32)
    n_hit = torch.empty(1, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.nerfhip_cull_compact_workspace_bytes(n), device=dev, dtype=torch.uint8)
    check(lib.nerfhip_cull_compact(ptr(hit), ptr(rays), ptr(t0), ptr(t1), n, ptr(slot), ptr(index), ptr(rays_out), ptr(n_hit), ptr(ws),
                                   stream_ptr()), "nerfhip_cull_compact")
    return slot, index, rays_out, n_hit


@device_guard
def cull_scatter(slot, white_back, rgb=None, depth=None, opacity_a=None, opacity_b=None):
    """nerfhip_cull_scatter: compact values (n_compact rows each; any may be None) -> full-size tensors of slot.shape[0] rows in
    the same order (None stays None): row i is the compact row slot[i], or the background (rgb: 1.0 with white_back, else 0.0;
    the others 0.0) where slot[i] is -1."""
    slot = _require_dev("cull_scatter", "slot", slot, torch.int32, ())
    n = slot.shape[0]
    src = [None if t is None else _require_dev("cull_scatter", name, t, torch.float32, tail)
           for name, t, tail in (("rgb", rgb, (3,)), ("depth", depth, ()), ("opacity_a", opacity_a, ()), ("opacity_b", opacity_b, ()))]
    _same_device("cull_scatter", slot, *src)
    rows = {t.shape[0] for t in src if t is not None}
    if len(rows) > 1 or (rows and max(rows) > n):
        raise ValueError("cull_scatter: the compact tensors must have the same number of rows, at most %d; got %s" % (n, sorted(rows)))
    n_compact = rows.pop() if rows else 0
    out = [None if t is None else torch.empty((n,) + tuple(t.shape[1:]), device=slot.device, dtype=torch.float32) for t in src]
    args = [p for s, o in zip(src, out) for p in (ptr(s), ptr(o))]
    check(_lib.load().nerfhip_cull_scatter(ptr(slot), n, n_compact, int(bool(white_back)), *args, stream_ptr()), "nerfhip_cull_scatter")
    return tuple(out)


# ---- epoch sampling (csrc/epoch.hip) -----------------------------------------------------------------------------
def _u64(v):
    return int(v) & ((1 << 64) - 1)


def epoch_share(n, world=1):
    """Positions a rank owns per epoch: ceil(n / world) (torch's DistributedSampler without drop_last)."""
    return (int(n) + int(world) - 1) // int(world)


def epoch_ids_host(seed, epoch, n, rank=0, world=1, first=0, count=None):
    """nerfhip_epoch_ids_host (host, no GPU): the ids of positions [first, first + count) of `rank`'s share of epoch `epoch` under
    `seed`, as an int64 numpy array, by the kernel's own per-id routine.  count None: up to the end of the share."""
    import numpy as np
    if count is None:
        count = epoch_share(n, world) - int(first)
    out = np.empty(max(int(count), 0), np.int64)
    check(_lib.load().nerfhip_epoch_ids_host(_u64(seed), _u64(epoch), int(n), int(rank), int(world), int(first), int(count),
                                             out.ctypes.data if out.size else None), "nerfhip_epoch_ids_host")
    return out


def epoch_ids(seed, epoch, n, device, rank=0, world=1, first=0, count=None):
    """nerfhip_epoch_ids: the same ids as an int64 tensor on `device`, one thread per id."""
    device = torch.device(device)
    if device.type != "cuda":
        raise NerfHipError("nerf_pl_amd runs on MI355X only: epoch_ids got device %s (epoch_ids_host is the host entry)" % device)
    if count is None:
        count = epoch_share(n, world) - int(first)
    with torch.cuda.device(device):
        out = torch.empty(max(int(count), 0), device=device, dtype=torch.int64)
        check(_lib.load().nerfhip_epoch_ids(_u64(seed), _u64(epoch), int(n), int(rank), int(world), int(first), int(count), ptr(out),
                                            stream_ptr()), "nerfhip_epoch_ids")
    return out


# ---- rendering the baked RGBA volume (csrc/baked.hip) -------------------------------------------------------------
BAKED_MAX_N = 1625


def _baked_N(what, N):
    N = int(N)
    if not 2 <= N <= BAKED_MAX_N:
        raise ValueError("%s: N must be in [2, %d] (N^3 < 2^32), got %d" % (what, BAKED_MAX_N, N))
    return N


def baked_bytes(N):
    """Bytes of the bricked volume of an N^3 lattice: ceil(N / 8)^3 bricks of 2 KiB."""
    return ((int(N) + 7) // 8) ** 3 * 2048


def baked_brick_words(N):
    """int32 words of the bitfield of the ceil((N - 1) / 8)^3 cell bricks of an N^3 lattice."""
    return (((int(N) - 1 + 7) // 8) ** 3 + 31) // 32


@device_guard
def baked_scatter(records, N):
    """nerfhip_baked_scatter: the (K, 2) int32 records of a .vol file (volume.vol_records / export_vol, on the device) -> the
    bricked volume (baked_bytes(N),) uint8 of the N^3 lattice.  ValueError for a record whose index is >= N^3 (one host read of
    the kernel's count), as volume.read_vol raises for the same file."""
    N = _baked_N("baked_scatter", N)
    records = _require_dev("baked_scatter", "records", records, torch.int32, (2,))
    dev = records.device
    data = torch.empty(baked_bytes(N), device=dev, dtype=torch.uint8)
    n_bad = torch.empty(1, device=dev, dtype=torch.int32)
    check(_lib.load().nerfhip_baked_scatter(ptr(records), records.shape[0], N, ptr(data), ptr(n_bad), stream_ptr()),
          "nerfhip_baked_scatter")
    bad = int(n_bad.item())
    if bad:
        raise ValueError("baked_scatter: %d records with an index outside the %d^3 lattice" % (bad, N))
    return data


@device_guard
def baked_from_dense(rgba):
    """nerfhip_baked_from_dense: a dense (N, N, N, 4) uint8 lattice on the device, indexed [iy, ix, iz] as volume.read_vol
    returns it -> the bricked volume."""
    if not torch.is_tensor(rgba) or not rgba.is_cuda:
        raise NerfHipError("nerf_pl_amd runs on MI355X only: baked_from_dense needs rgba on the device (no CPU fallback)")
    if rgba.dtype != torch.uint8 or rgba.dim() != 4 or rgba.shape[3] != 4 or len(set(rgba.shape[:3])) != 1:
        raise ValueError("baked_from_dense: rgba must be (N, N, N, 4) uint8, got %s %s" % (tuple(rgba.shape), rgba.dtype))
    N = _baked_N("baked_from_dense", rgba.shape[0])
    rgba = _c(rgba)
    data = torch.empty(baked_bytes(N), device=rgba.device, dtype=torch.uint8)
    check(_lib.load().nerfhip_baked_from_dense(ptr(rgba), N, ptr(data), stream_ptr()), "nerfhip_baked_from_dense")
    return data


def _baked_data(what, data, N, B=_DeviceArrays):
    data = B.array(what, "data", data, "uint8", ())
    if _numel(data) != baked_bytes(N):
        raise ValueError("%s: the bricked volume of a %d^3 lattice has %d bytes, got %d" % (what, N, baked_bytes(N), _numel(data)))
    return data


@device_guard
def baked_bricks(data, N):
    """nerfhip_baked_bricks: the bricked volume -> the bitfield of its occupied cell bricks, (baked_brick_words(N),) int32."""
    N = _baked_N("baked_bricks", N)
    data = _baked_data("baked_bricks", data, N)
    words = torch.empty(baked_brick_words(N), device=data.device, dtype=torch.int32)
    check(_lib.load().nerfhip_baked_bricks(ptr(data), N, ptr(words), stream_ptr()), "nerfhip_baked_bricks")
    return words


def _baked_render(B, rays, data, bits, N, ranges, cell, step, t_stop, white_back):
    what = "baked_render" + B.suffix
    N = _baked_N(what, N)
    rays = B.array(what, "rays", rays, "float32", (8,))
    data = _baked_data(what, data, N, B)
    if bits is not None:
        bits = B.array(what, "bits", bits, "int32", ())
        if _numel(bits) < baked_brick_words(N):
            raise ValueError("%s: %d words for the bricks of a %d^3 lattice (needs %d)" % (what, _numel(bits), N, baked_brick_words(N)))
    B.same_device(what, rays, data, bits)
    rg = _ranges_arg(what, ranges)
    n = rays.shape[0]
    rgb, depth, opacity = B.empty(rays, (n, 3), "float32"), B.empty(rays, n, "float32"), B.empty(rays, n, "float32")
    B.call("nerfhip_baked_render", B.ptr(rays), n, B.ptr(data), B.ptr(bits), N, rg, float(cell), float(step), float(t_stop),
           int(bool(white_back)), B.ptr(rgb), B.ptr(depth), B.ptr(opacity))
    return rgb, depth, opacity


@device_guard
def baked_render(rays, data, bits, N, ranges, cell, step=0.5, t_stop=0.0, white_back=False):
    """nerfhip_baked_render: rays (n, 8) fp32 marched through the bricked volume `data` of an N^3 lattice over `ranges` ->
    (rgb (n, 3), depth (n,), opacity (n,)) on the device.  bits: the cell-brick bitfield, or None (no skipping; the same bits
    of output)."""
    return _baked_render(_DeviceArrays, rays, data, bits, N, ranges, cell, step, t_stop, white_back)


def baked_render_host(rays, data, bits, N, ranges, cell, step=0.5, t_stop=0.0, white_back=False):
    """nerfhip_baked_render_host (host, no GPU): numpy rays (n, 8) float32, the bricked volume as a uint8 array and the bitfield
    as int32 words (or None) -> numpy (rgb, depth, opacity), by the kernel's own per-ray routine."""
    import numpy as np
    data, bits = (None if a is None else np.asarray(a).ravel() for a in (data, bits))      # of any shape
    return _baked_render(_HostArrays, rays, data, bits, N, ranges, cell, step, t_stop, white_back)


# ---- ray casting against a triangle mesh (csrc/meshcast.hip) -------------------------------------------------------
MESH_MAX_TRIANGLES = 1 << 28
MIXED_MODES = {"ztest": 0, "clip": 1}


def mesh_bvh_levels(T):
    """[(offset, nodes)] of the hierarchy's levels in `boxes`, from the leaves to the root (include/nerfhip.h): ceil(T / 4)
    leaves, every level above an eighth (rounded up) of the one below.  [] for T = 0."""
    T = int(T)
    if not 0 <= T <= MESH_MAX_TRIANGLES:
        raise ValueError("mesh_bvh_levels: T must be in [0, 2^28], got %d" % T)
    out, off, n = [], 0, (T + 3) // 4
    while n:
        out.append((off, n))
        off += n
        n = (n + 7) // 8 if n > 1 else 0
    return out


def mesh_bvh_nodes(T):
    """nerfhip_mesh_bvh_nodes: the rows of `boxes`."""
    levels = mesh_bvh_levels(T)
    return levels[-1][0] + levels[-1][1] if levels else 0


def _mesh_arrays(B, what, vertices, triangles):
    vertices = B.array(what, "vertices", vertices, "float32", (3,))
    triangles = B.array(what, "triangles", triangles, "int32", (3,))
    if triangles.shape[0] > MESH_MAX_TRIANGLES:
        raise ValueError("%s: at most 2^28 triangles, got %d" % (what, triangles.shape[0]))
    B.same_device(what, vertices, triangles)
    return vertices, triangles


def _mesh_bvh_build(B, vertices, triangles):
    what = "mesh_bvh_build" + B.suffix
    vertices, triangles = _mesh_arrays(B, what, vertices, triangles)
    V, T = vertices.shape[0], triangles.shape[0]
    keys, state = B.empty(vertices, T, "int64"), B.empty(vertices, 8, "int32")
    B.call("nerfhip_mesh_bvh_keys", B.ptr(vertices), V, B.ptr(triangles), T, B.ptr(keys), B.ptr(state))
    sorted_keys = B.sort(keys)
    tris, boxes = B.empty(vertices, (T, 12), "float32"), B.empty(vertices, (mesh_bvh_nodes(T), 6), "float32")
    B.call("nerfhip_mesh_bvh_boxes", B.ptr(vertices), V, B.ptr(triangles), T, B.ptr(sorted_keys), B.ptr(tris), B.ptr(boxes))
    return tris, boxes, sorted_keys & 0xffffffff, state[:1]


@device_guard
def mesh_bvh_build(vertices, triangles):
    """nerfhip_mesh_bvh_keys, torch.sort, nerfhip_mesh_bvh_boxes: vertices (V, 3) fp32 and triangles (T, 3) int32 on the device ->
    (tris (T, 12) fp32: the sorted triangles' vertices with their original numbers; boxes (mesh_bvh_nodes(T), 6) fp32; order (T,)
    int32: the original number of every sorted triangle; n_bad (1,) int32 on the device: triangles with an index outside [0, V) or a
    non-finite coordinate, which no cast returns).  The keys are distinct, so the sort decides nothing."""
    tris, boxes, order, n_bad = _mesh_bvh_build(_DeviceArrays, vertices, triangles)
    return tris, boxes, order.to(torch.int32), n_bad


def mesh_bvh_build_host(vertices, triangles):
    """The _host twins of `mesh_bvh_build` with numpy's sort between them (host, no GPU): numpy in, numpy (tris, boxes, order,
    n_bad (1,) int32) out, bit for bit what the device builds."""
    import numpy as np
    tris, boxes, order, n_bad = _mesh_bvh_build(_HostArrays, vertices, triangles)
    return tris, boxes, order.astype(np.int32), n_bad.copy()


def _mesh_cast(B, rays, tris, boxes, brute=False):
    what = "mesh_cast" + B.suffix
    rays = B.array(what, "rays", rays, "float32", (8,))
    tris = B.array(what, "tris", tris, "float32", (12,))
    T = tris.shape[0]
    boxes = None if brute else B.array(what, "boxes", boxes, "float32", (6,))
    if boxes is not None and boxes.shape[0] != mesh_bvh_nodes(T):
        raise ValueError("%s: a hierarchy of %d triangles has %d boxes, got %d" % (what, T, mesh_bvh_nodes(T), boxes.shape[0]))
    B.same_device(what, rays, tris, boxes)
    n = rays.shape[0]
    tri, t, b1, b2 = (B.empty(rays, n, dtype) for dtype in ("int32", "float32", "float32", "float32"))
    only_host = (int(bool(brute)),) if B is _HostArrays else ()
    B.call("nerfhip_mesh_cast", B.ptr(rays), n, B.ptr(tris), B.ptr(boxes), T, *only_host, B.ptr(tri), B.ptr(t), B.ptr(b1), B.ptr(b2))
    return tri, t, b1, b2


@device_guard
def mesh_cast(rays, tris, boxes):
    """nerfhip_mesh_cast: rays (n, 8) fp32 against the hierarchy of `mesh_bvh_build` -> (tri (n,) int32: the original number of the
    nearest triangle hit within [near, far], -1 for a miss; t (n,); b1 (n,); b2 (n,)), on the device."""
    return _mesh_cast(_DeviceArrays, rays, tris, boxes)


def mesh_cast_host(rays, tris, boxes, brute=False):
    """nerfhip_mesh_cast_host (host, no GPU): numpy rays (n, 8) against a numpy hierarchy -> numpy (tri, t, b1, b2), by the kernel's
    own per-ray routine.  brute=True tests every triangle and reads no box (boxes may be None)."""
    return _mesh_cast(_HostArrays, rays, tris, boxes, brute)


def _mesh_shade(B, rays, tri, b1, b2, vertices, triangles, colors, ambient, background):
    what = "mesh_shade" + B.suffix
    rays = B.array(what, "rays", rays, "float32", (8,))
    tri, b1, b2 = B.array(what, "tri", tri, "int32", ()), B.array(what, "b1", b1, "float32", ()), B.array(what, "b2", b2, "float32", ())
    vertices, triangles = _mesh_arrays(B, what, vertices, triangles)
    if colors is not None:
        colors = B.array(what, "colors", colors, "uint8", (3,))
        if colors.shape[0] != vertices.shape[0]:
            raise ValueError("%s: %d colours for %d vertices" % (what, colors.shape[0], vertices.shape[0]))
    n = rays.shape[0]
    if not tri.shape[0] == b1.shape[0] == b2.shape[0] == n:
        raise ValueError("%s: tri, b1 and b2 must have one entry per ray" % what)
    B.same_device(what, rays, tri, b1, b2, vertices, triangles, colors)
    ambient, background = float(ambient), float(background)
    if not 0.0 <= ambient <= 1.0:
        raise ValueError("%s: ambient must be in [0, 1], got %r" % (what, ambient))
    rgb = B.empty(rays, (n, 3), "float32")
    B.call("nerfhip_mesh_shade", B.ptr(rays), n, B.ptr(tri), B.ptr(b1), B.ptr(b2), B.ptr(vertices), vertices.shape[0], B.ptr(triangles),
           triangles.shape[0], B.ptr(colors), ambient, background, B.ptr(rgb))
    return rgb


@device_guard
def mesh_shade(rays, tri, b1, b2, vertices, triangles, colors=None, ambient=1.0, background=0.0):
    """nerfhip_mesh_shade: the hits of `mesh_cast` -> rgb (n, 3): the barycentric blend of the vertex colours (colors (V, 3) uint8 /
    255; None: white) times ambient + (1 - ambient) |n . d|, n the triangle's unit normal and d the unit direction; `background`
    for a miss."""
    return _mesh_shade(_DeviceArrays, rays, tri, b1, b2, vertices, triangles, colors, ambient, background)


def mesh_shade_host(rays, tri, b1, b2, vertices, triangles, colors=None, ambient=1.0, background=0.0):
    """nerfhip_mesh_shade_host (host, no GPU): numpy in, numpy rgb (n, 3) out."""
    return _mesh_shade(_HostArrays, rays, tri, b1, b2, vertices, triangles, colors, ambient, background)


def _mixed_compose(B, mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background):
    what = "mixed_compose" + B.suffix
    if mode not in MIXED_MODES:
        raise ValueError("%s: mode must be 'ztest' or 'clip', got %r" % (what, mode))
    tau = float(tau)
    if not tau > 0.0:
        raise ValueError("%s: tau must be > 0, got %r" % (what, tau))
    rgb_n, rgb_m = B.array(what, "rgb_n", rgb_n, "float32", (3,)), B.array(what, "rgb_m", rgb_m, "float32", (3,))
    depth_n, opacity_n = B.array(what, "depth_n", depth_n, "float32", ()), B.array(what, "opacity_n", opacity_n, "float32", ())
    tri, t = B.array(what, "tri", tri, "int32", ()), B.array(what, "t", t, "float32", ())
    n = rgb_n.shape[0]
    if not rgb_m.shape[0] == depth_n.shape[0] == opacity_n.shape[0] == tri.shape[0] == t.shape[0] == n:
        raise ValueError("%s: every input must have one row per ray" % what)
    B.same_device(what, rgb_n, depth_n, opacity_n, tri, t, rgb_m)
    rgb, depth, opacity, mask = (B.empty(rgb_n, shape, dtype)
                                 for shape, dtype in (((n, 3), "float32"), (n, "float32"), (n, "float32"), (n, "uint8")))
    B.call("nerfhip_mixed_compose", MIXED_MODES[mode], n, B.ptr(rgb_n), B.ptr(depth_n), B.ptr(opacity_n), B.ptr(tri), B.ptr(t),
           B.ptr(rgb_m), tau, float(background), B.ptr(rgb), B.ptr(depth), B.ptr(opacity), B.ptr(mask))
    return rgb, depth, opacity, mask


@device_guard
def mixed_compose(mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau=0.5, background=0.0):
    """nerfhip_mixed_compose: a render (rgb_n (n, 3), depth_n (n,), opacity_n (n,)) and a mesh layer (tri, t of `mesh_cast`, rgb_m of
    `mesh_shade`) -> (rgb, depth, opacity, mask (n,) uint8).  'ztest': the mesh wins where it is hit and t < depth_n / opacity_n
    (+inf where opacity_n < tau).  'clip': the render was made with far = min(far, t) on the hit rays and no background; the mesh,
    or `background` on a miss, fills the transmittance it left (include/nerfhip.h)."""
    return _mixed_compose(_DeviceArrays, mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background)


def mixed_compose_host(mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau=0.5, background=0.0):
    """nerfhip_mixed_compose_host (host, no GPU): numpy in, numpy (rgb, depth, opacity, mask) out."""
    return _mixed_compose(_HostArrays, mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background)


# ---- shadows for mixed renders (csrc/shadow.hip) -----------------------------------------------------------------
LIGHT_KINDS = {"directional": 0, "point": 1}
SHADOW_MAX_SAMPLES = 64


def _mesh_occluded(B, rays, tris, boxes, brute=False):
    what = "mesh_occluded" + B.suffix
    rays = B.array(what, "rays", rays, "float32", (8,))
    tris = B.array(what, "tris", tris, "float32", (12,))
    T = tris.shape[0]
    boxes = None if brute else B.array(what, "boxes", boxes, "float32", (6,))
    if boxes is not None and boxes.shape[0] != mesh_bvh_nodes(T):
        raise ValueError("%s: a hierarchy of %d triangles has %d boxes, got %d" % (what, T, mesh_bvh_nodes(T), boxes.shape[0]))
    B.same_device(what, rays, tris, boxes)
    n = rays.shape[0]
    hit = B.empty(rays, n, "uint8")
    only_host = (int(bool(brute)),) if B is _HostArrays else ()
    B.call("nerfhip_mesh_occluded", B.ptr(rays), n, B.ptr(tris), B.ptr(boxes), T, *only_host, B.ptr(hit))
    return hit


@device_guard
def mesh_occluded(rays, tris, boxes):
    """nerfhip_mesh_occluded: rays (n, 8) fp32 against the hierarchy of `mesh_bvh_build` -> hit (n,) uint8 on the device: 1 iff
    `mesh_cast` would return tri >= 0, found by leaving the walk at the first accepted triangle."""
    return _mesh_occluded(_DeviceArrays, rays, tris, boxes)


def mesh_occluded_host(rays, tris, boxes, brute=False):
    """nerfhip_mesh_occluded_host (host, no GPU): numpy in, numpy hit (n,) uint8 out.  brute=True tests every triangle and reads no
    box (boxes may be None)."""
    return _mesh_occluded(_HostArrays, rays, tris, boxes, brute)


def _samples_arg(what, samples):
    K = int(samples)
    if K != samples or not 1 <= K <= SHADOW_MAX_SAMPLES:
        raise ValueError("%s: samples must be an integer in [1, %d], got %r" % (what, SHADOW_MAX_SAMPLES, samples))
    return K


def _shadow_rays(B, rays, s, kind, light, bias, reach, samples, radius, rotate, tri, vertices, triangles, cosine):
    import math
    what = "shadow_rays" + B.suffix
    if kind not in LIGHT_KINDS:
        raise ValueError("%s: kind must be 'directional' or 'point', got %r" % (what, kind))
    light = [float(v) for v in light]
    if len(light) != 3 or not all(math.isfinite(v) for v in light):
        raise ValueError("%s: the light must be three finite numbers, got %r" % (what, light))
    if kind == "directional" and not any(light):
        raise ValueError("%s: a directional light needs a non-zero direction" % what)
    K = _samples_arg(what, samples)
    bias, reach, radius = float(bias), float(reach), float(radius)
    if not (bias > 0.0 and math.isfinite(bias)):
        raise ValueError("%s: bias must be finite and > 0, got %r" % (what, bias))
    if not (reach > 0.0 and math.isfinite(reach)):
        raise ValueError("%s: reach must be finite and > 0, got %r" % (what, reach))
    if not (radius >= 0.0 and math.isfinite(radius)):
        raise ValueError("%s: radius must be finite and >= 0, got %r" % (what, radius))
    rays = B.array(what, "rays", rays, "float32", (8,))
    s = B.array(what, "s", s, "float32", ())
    n = rays.shape[0]
    if s.shape[0] != n:
        raise ValueError("%s: s must have one entry per ray, got %d for %d rays" % (what, s.shape[0], n))
    if n * K > 1 << 30:
        raise ValueError("%s: at most 2^30 rows per call, got %d x %d" % (what, n, K))
    V = T = 0
    if tri is not None:
        if vertices is None or triangles is None:
            raise ValueError("%s: tri needs the mesh's vertices and triangles" % what)
        tri = B.array(what, "tri", tri, "int32", ())
        if tri.shape[0] != n:
            raise ValueError("%s: tri must have one entry per ray, got %d for %d rays" % (what, tri.shape[0], n))
        vertices, triangles = _mesh_arrays(B, what, vertices, triangles)
        V, T = vertices.shape[0], triangles.shape[0]
    else:
        vertices = triangles = None
    B.same_device(what, rays, s, tri, vertices, triangles)
    rows = B.empty(rays, (n * K, 8), "float32")
    cos = B.empty(rays, n, "float32") if cosine else None
    B.call("nerfhip_shadow_rays", B.ptr(rays), B.ptr(s), n, B.ptr(tri), B.ptr(vertices), V, B.ptr(triangles), T, LIGHT_KINDS[kind],
           light[0], light[1], light[2], bias, reach, K, radius, int(bool(rotate)), B.ptr(rows), B.ptr(cos))
    return rows, cos


@device_guard
def shadow_rays(rays, s, kind, light, bias, reach, samples=1, radius=0.0, rotate=True, tri=None, vertices=None, triangles=None,
                cosine=True):
    """nerfhip_shadow_rays: primary rays (n, 8) and the surface distance s (n,) of each -> (rows (n samples, 8): sample k of pixel i
    at row i samples + k, from p = o + s d towards sample k of the light, near = bias, far = reach or the distance to a point
    light; cosine (n,) or None).  `kind` 'directional' (`light` the direction towards it) or 'point' (`light` its position);
    the light is a square of half-width `radius`.  A pixel without a surface (s not finite or <= 0) gets zero rows, which hit
    nothing.  `tri` (n,) int32 with `vertices`, `triangles`: the mesh layer's hit, for cosine = max(n . l, 0); -1 or no `tri`: 1."""
    return _shadow_rays(_DeviceArrays, rays, s, kind, light, bias, reach, samples, radius, rotate, tri, vertices, triangles, cosine)


def shadow_rays_host(rays, s, kind, light, bias, reach, samples=1, radius=0.0, rotate=True, tri=None, vertices=None, triangles=None,
                     cosine=True):
    """nerfhip_shadow_rays_host (host, no GPU): numpy in, numpy (rows, cosine or None) out."""
    return _shadow_rays(_HostArrays, rays, s, kind, light, bias, reach, samples, radius, rotate, tri, vertices, triangles, cosine)


def _light_compose(B, rgb, mask, cosine, hit, trans, ambient, strength, visibility):
    what = "light_compose" + B.suffix
    ambient, strength = float(ambient), float(strength)
    if not 0.0 <= ambient <= 1.0:
        raise ValueError("%s: ambient must be in [0, 1], got %r" % (what, ambient))
    if not 0.0 <= strength <= 1.0:
        raise ValueError("%s: strength must be in [0, 1], got %r" % (what, strength))
    rgb = B.array(what, "rgb", rgb, "float32", (3,))
    mask, hit = B.array(what, "mask", mask, "uint8", ()), B.array(what, "hit", hit, "uint8", ())
    cosine = B.array(what, "cosine", cosine, "float32", ())
    n = rgb.shape[0]
    if not mask.shape[0] == cosine.shape[0] == n:
        raise ValueError("%s: mask and cosine must have one entry per pixel" % what)
    K = hit.shape[0] // n if n else 1
    if hit.shape[0] != (n * K if n else 0) or not 1 <= K <= SHADOW_MAX_SAMPLES:
        raise ValueError("%s: hit must hold 1 to %d samples for each of the %d pixels, got %d" % (what, SHADOW_MAX_SAMPLES, n, hit.shape[0]))
    if trans is not None:
        trans = B.array(what, "trans", trans, "float32", ())
        if trans.shape[0] != hit.shape[0]:
            raise ValueError("%s: trans must have one entry per row, got %d for %d rows" % (what, trans.shape[0], hit.shape[0]))
    B.same_device(what, rgb, mask, cosine, hit, trans)
    out = B.empty(rgb, (n, 3), "float32")
    vis = B.empty(rgb, n, "float32") if visibility else None
    B.call("nerfhip_light_compose", n, B.ptr(rgb), B.ptr(mask), B.ptr(cosine), B.ptr(hit), B.ptr(trans), K, ambient, strength, B.ptr(out),
           B.ptr(vis))
    return out, vis


@device_guard
def light_compose(rgb, mask, cosine, hit, trans=None, ambient=0.3, strength=0.7, visibility=True):
    """nerfhip_light_compose: rgb (n, 3), mask (n,) uint8 of `mixed_compose`, cosine (n,) of `shadow_rays`, hit (n K,) uint8 of
    `mesh_occluded` on its rows, trans (n K,) or None: the scene's transmittance along each row -> (rgb_out (n, 3), V (n,) or
    None).  Mesh pixel: V = mean_k((1 - hit) trans), rgb (ambient + (1 - ambient) cosine V); scene pixel: V = mean_k(1 - hit),
    rgb (1 - strength (1 - V)).  ambient = 1 and strength = 0 pass every bit of rgb through."""
    return _light_compose(_DeviceArrays, rgb, mask, cosine, hit, trans, ambient, strength, visibility)


def light_compose_host(rgb, mask, cosine, hit, trans=None, ambient=0.3, strength=0.7, visibility=True):
    """nerfhip_light_compose_host (host, no GPU): numpy in, numpy (rgb_out, V or None) out."""
    return _light_compose(_HostArrays, rgb, mask, cosine, hit, trans, ambient, strength, visibility)


# ---- texturing a triangle mesh (csrc/texture.hip) ----------------------------------------------------------------
TEX_MAX_RES = 64
TEX_MAX_SIDE = 16384
TEX_MAX_SAMPLES = 1 << 30
TEX_FILTERS = {"nearest": 0, "bilinear": 1}


def mesh_tex_samples(res):
    """nerfhip_mesh_tex_samples: the samples of one triangle at `res` texel intervals per leg, (res + 2)(res + 3) / 2."""
    res = int(res)
    if not 1 <= res <= TEX_MAX_RES:
        raise ValueError("mesh_tex_samples: res must be in [1, %d], got %d" % (TEX_MAX_RES, res))
    return (res + 2) * (res + 3) // 2


def mesh_tex_height(n_triangles, res, width):
    """nerfhip_mesh_tex_height: the rows of the atlas of `n_triangles` triangles that is `width` texels wide (include/nerfhip.h)."""
    T, res, width = int(n_triangles), int(res), int(width)
    mesh_tex_samples(res)
    B = res + 3
    if not 0 <= T <= MESH_MAX_TRIANGLES:
        raise ValueError("mesh_tex_height: at most 2^28 triangles, got %d" % T)
    if width % 4 or not B <= width <= TEX_MAX_SIDE:
        raise ValueError("mesh_tex_height: width must be a multiple of 4 in [%d, %d], got %d" % (B, TEX_MAX_SIDE, width))
    nb = width // B
    height = B * -(-((T + 1) // 2) // nb)
    if height > TEX_MAX_SIDE:
        raise ValueError("mesh_tex_height: %d triangles at res %d and width %d need %d rows, more than %d"
                         % (T, res, width, height, TEX_MAX_SIDE))
    return height


def _mesh_tex_points(B, vertices, triangles, res, normals):
    what = "mesh_tex_points" + B.suffix
    vertices, triangles = _mesh_arrays(B, what, vertices, triangles)
    T, K = triangles.shape[0], triangles.shape[0] * mesh_tex_samples(res)
    if K > TEX_MAX_SAMPLES:
        raise ValueError("%s: at most 2^30 samples per call, got %d" % (what, K))
    points = B.empty(vertices, (K, 3), "float32")
    nrm = B.empty(vertices, (K, 3), "float64") if normals else None
    B.call("nerfhip_mesh_tex_points", B.ptr(vertices), vertices.shape[0], B.ptr(triangles), T, int(res), B.ptr(points), B.ptr(nrm))
    return points, nrm


@device_guard
def mesh_tex_points(vertices, triangles, res, normals=True):
    """nerfhip_mesh_tex_points: vertices (V, 3) fp32 and triangles (T, 3) int32 on the device -> (points (K, 3) fp32, normals (K, 3)
    fp64 or None), K = T mesh_tex_samples(res): the point of every sample of the atlas on its triangle's plane, and its triangle's
    unit normal.  A bad triangle (mesh_bvh_build's rule) gives (0, 0, 0) and (0, 0, 1)."""
    return _mesh_tex_points(_DeviceArrays, vertices, triangles, res, normals)


def mesh_tex_points_host(vertices, triangles, res, normals=True):
    """nerfhip_mesh_tex_points_host (host, no GPU): numpy in, numpy (points, normals or None) out."""
    return _mesh_tex_points(_HostArrays, vertices, triangles, res, normals)


def _mesh_tex_atlas(B, colors, n_triangles, res, width):
    what = "mesh_tex_atlas" + B.suffix
    colors = B.array(what, "colors", colors, "uint8", (3,))
    T, height = int(n_triangles), mesh_tex_height(n_triangles, res, width)
    if colors.shape[0] != T * mesh_tex_samples(res):
        raise ValueError("%s: %d triangles at res %d have %d samples, got %d colours"
                         % (what, T, res, T * mesh_tex_samples(res), colors.shape[0]))
    atlas = B.empty(colors, (height, int(width), 3), "uint8")
    B.call("nerfhip_mesh_tex_atlas", B.ptr(colors), T, int(res), int(width), height, B.ptr(atlas))
    return atlas


@device_guard
def mesh_tex_atlas(colors, n_triangles, res, width):
    """nerfhip_mesh_tex_atlas: colors (K, 3) uint8 on the device, one per sample in `mesh_tex_points`' order -> the atlas
    (mesh_tex_height(n_triangles, res, width), width, 3) uint8 in the layout of include/nerfhip.h, every byte written."""
    return _mesh_tex_atlas(_DeviceArrays, colors, n_triangles, res, width)


def mesh_tex_atlas_host(colors, n_triangles, res, width):
    """nerfhip_mesh_tex_atlas_host (host, no GPU): numpy in, numpy atlas out."""
    return _mesh_tex_atlas(_HostArrays, colors, n_triangles, res, width)


def _mesh_shade_tex(B, rays, tri, b1, b2, vertices, triangles, atlas, res, filter, ambient, background):
    what = "mesh_shade_tex" + B.suffix
    if filter not in TEX_FILTERS:
        raise ValueError("%s: filter must be 'nearest' or 'bilinear', got %r" % (what, filter))
    rays = B.array(what, "rays", rays, "float32", (8,))
    tri, b1, b2 = B.array(what, "tri", tri, "int32", ()), B.array(what, "b1", b1, "float32", ()), B.array(what, "b2", b2, "float32", ())
    vertices, triangles = _mesh_arrays(B, what, vertices, triangles)
    atlas = B.array(what, "atlas", atlas, "uint8")
    if atlas.ndim != 3 or atlas.shape[2] != 3:
        raise ValueError("%s: atlas must be (height, width, 3), got %s" % (what, tuple(atlas.shape)))
    T, height, width = triangles.shape[0], atlas.shape[0], atlas.shape[1]
    if height != mesh_tex_height(T, res, width):
        raise ValueError("%s: the atlas of %d triangles at res %d and width %d has %d rows, got %d"
                         % (what, T, res, width, mesh_tex_height(T, res, width), height))
    n = rays.shape[0]
    if not tri.shape[0] == b1.shape[0] == b2.shape[0] == n:
        raise ValueError("%s: tri, b1 and b2 must have one entry per ray" % what)
    B.same_device(what, rays, tri, b1, b2, vertices, triangles, atlas)
    ambient, background = float(ambient), float(background)
    if not 0.0 <= ambient <= 1.0:
        raise ValueError("%s: ambient must be in [0, 1], got %r" % (what, ambient))
    rgb = B.empty(rays, (n, 3), "float32")
    B.call("nerfhip_mesh_shade_tex", B.ptr(rays), n, B.ptr(tri), B.ptr(b1), B.ptr(b2), B.ptr(vertices), vertices.shape[0],
           B.ptr(triangles), T, B.ptr(atlas), int(res), width, height, TEX_FILTERS[filter], ambient, background, B.ptr(rgb))
    return rgb


@device_guard
def mesh_shade_tex(rays, tri, b1, b2, vertices, triangles, atlas, res, filter="bilinear", ambient=1.0, background=0.0):
    """nerfhip_mesh_shade_tex: the hits of `mesh_cast` -> rgb (n, 3): the hit triangle's patch of `atlas` ((height, width, 3) uint8
    of `mesh_tex_atlas` at `res`) at (b1, b2), the nearest texel or the bilinear blend of the four around it, times `mesh_shade`'s
    ambient term; `background` for a miss."""
    return _mesh_shade_tex(_DeviceArrays, rays, tri, b1, b2, vertices, triangles, atlas, res, filter, ambient, background)


def mesh_shade_tex_host(rays, tri, b1, b2, vertices, triangles, atlas, res, filter="bilinear", ambient=1.0, background=0.0):
    """nerfhip_mesh_shade_tex_host (host, no GPU): numpy in, numpy rgb (n, 3) out."""
    return _mesh_shade_tex(_HostArrays, rays, tri, b1, b2, vertices, triangles, atlas, res, filter, ambient, background)


# ---- mesh decimation (csrc/decimate.hip) -----------------------------------------------------------------------
DECIMATE_MAX_ITEMS = 1 << 28
DECIMATE_PLACEMENTS = {"mean": 0, "quadric": 1}
DECIMATE_COUNTS = ("clusters", "bad", "collapsed", "duplicate", "unreferenced")


def _mesh_decimate(B, vertices, triangles, colors, cell, placement, origin, eps):
    import numpy as np
    what = "mesh_decimate" + B.suffix
    vertices, triangles = _mesh_arrays(B, what, vertices, triangles)
    V, T = vertices.shape[0], triangles.shape[0]
    if V > DECIMATE_MAX_ITEMS:
        raise ValueError("%s: at most 2^28 vertices, got %d" % (what, V))
    if colors is not None:
        colors = B.array(what, "colors", colors, "uint8", (3,))
        if colors.shape[0] != V:
            raise ValueError("%s: %d colours for %d vertices" % (what, colors.shape[0], V))
    B.same_device(what, vertices, triangles, colors)
    if placement not in DECIMATE_PLACEMENTS:
        raise ValueError("%s: placement must be 'mean' or 'quadric', got %r" % (what, placement))
    cell32, eps = np.float32(cell), float(eps)
    if not (np.isfinite(cell32) and cell32 > 0):
        raise ValueError("%s: cell must be > 0 and finite as fp32, got %r" % (what, cell))
    if not 0.0 < eps <= 1.0:
        raise ValueError("%s: eps must be in (0, 1], got %r" % (what, eps))
    if origin is not None:
        origin = np.asarray(origin, np.float32).reshape(-1)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError("%s: origin must be 3 finite floats, got %r" % (what, origin))

    def result(n_v, n_t, cluster_of, counts, arrays=None):
        out_v, out_t = B.empty(vertices, (max(n_v, 1), 3), "float32"), B.empty(vertices, (max(n_t, 1), 3), "int32")
        out_c = None if colors is None else B.empty(vertices, (max(n_v, 1), 3), "uint8")
        if arrays is not None:
            arrays(out_v, out_t, out_c)
        return out_v[:n_v], out_t[:n_t], None if out_c is None else out_c[:n_v], cluster_of, dict(zip(DECIMATE_COUNTS, counts))

    def nothing(bad):
        cluster_of = B.empty(vertices, V, "int32")
        cluster_of[...] = -1
        return result(0, 0, cluster_of, (0, bad, 0, 0, 0))

    if V == 0 or T == 0:
        return nothing(0)
    state = B.empty(vertices, 8, "int32")
    B.call("nerfhip_mesh_decimate_bounds", B.ptr(vertices), V, B.ptr(state))
    words = np.ascontiguousarray(B.host(state), np.int32).view(np.uint32)
    if int(words[0]) == V:                         # no finite vertex: every triangle is bad
        return nothing(T)
    bits = np.where(words[2:] >> 31, words[2:] & np.uint32(0x7fffffff), ~words[2:]).astype(np.uint32)      # mesh_core.h mesh_unordered
    v_lo, v_hi = bits.view(np.float32)[:3], bits.view(np.float32)[3:]
    lo = v_lo if origin is None else origin
    if (v_lo < lo).any():
        raise ValueError("%s: a vertex lies below the origin %s (the mesh starts at %s)" % (what, lo.tolist(), v_lo.tolist()))
    with np.errstate(all="ignore"):
        q_max = np.floor((v_hi - lo) / cell32)     # the kernel's fp32 operations: q is monotonic in v
    if not np.isfinite(q_max).all() or (int(q_max[0]) + 1) * (int(q_max[1]) + 1) * (int(q_max[2]) + 1) >= 1 << 31:
        raise ValueError("%s: cell too small for this mesh (2^31 cells or more)" % what)
    lo_c, res_c = (ctypes.c_float * 3)(*lo.tolist()), (ctypes.c_int32 * 3)(*(int(q) + 1 for q in q_max))
    grid = (lo_c, float(cell32), res_c)

    def blocks(n):
        return (n + 255) // 256

    keys = B.empty(vertices, V, "int64")
    B.call("nerfhip_mesh_decimate_keys", B.ptr(vertices), V, *grid, B.ptr(keys))
    sorted_keys = B.sort(keys)
    blk, off = B.empty(vertices, blocks(V), "int32"), B.empty(vertices, blocks(V), "int64")
    cluster_of, seg_start, totals = B.empty(vertices, V, "int32"), B.empty(vertices, V + 1, "int32"), B.empty(vertices, 5, "int64")
    B.call("nerfhip_mesh_decimate_clusters", B.ptr(sorted_keys), V, B.ptr(blk), B.ptr(off), B.ptr(cluster_of), B.ptr(seg_start),
           B.ptr(totals))
    C = int(B.host(totals)[0])
    entries = None
    if placement == "quadric":
        entries = B.empty(vertices, 3 * T, "int64")
        B.call("nerfhip_mesh_decimate_entries", B.ptr(triangles), T, V, B.ptr(cluster_of), B.ptr(entries))
        entries = B.sort(entries)
    mean, positions = B.empty(vertices, (C, 3), "float64"), B.empty(vertices, (C, 3), "float32")
    cluster_colors = None if colors is None else B.empty(vertices, (C, 3), "uint8")
    B.call("nerfhip_mesh_decimate_place", B.ptr(vertices), V, B.ptr(colors), B.ptr(triangles), T, B.ptr(sorted_keys), B.ptr(seg_start), C,
           B.ptr(entries), *grid, eps, DECIMATE_PLACEMENTS[placement], B.ptr(mean), B.ptr(positions), B.ptr(cluster_colors))
    # duplicates: the triangles in ascending (key_hi, key_lo) order, by a sort on the low half and a stable one on the high half
    flags, key_hi, key_lo = B.empty(vertices, T, "uint8"), B.empty(vertices, T, "int64"), B.empty(vertices, T, "int64")
    B.call("nerfhip_mesh_decimate_tri_keys", B.ptr(triangles), T, V, B.ptr(cluster_of), B.ptr(flags), B.ptr(key_hi), B.ptr(key_lo))
    key_lo, order = B.sort_stable(key_lo)
    key_hi, order = B.sort_stable(B.take(key_hi, order))
    key_lo = B.take(key_lo, order)
    B.call("nerfhip_mesh_decimate_duplicates", B.ptr(key_hi), B.ptr(key_lo), T, B.ptr(flags))
    ref = B.empty(vertices, C, "uint8")
    blk_t, off_t = B.empty(vertices, blocks(T), "int32"), B.empty(vertices, blocks(T), "int64")
    blk_c, off_c = B.empty(vertices, blocks(C), "int32"), B.empty(vertices, blocks(C), "int64")
    B.call("nerfhip_mesh_decimate_mark", B.ptr(triangles), T, V, B.ptr(cluster_of), B.ptr(flags), C, B.ptr(ref), B.ptr(blk_t), B.ptr(off_t),
           B.ptr(blk_c), B.ptr(off_c), B.ptr(totals))
    n_t, n_v, bad, collapsed, duplicate = (int(x) for x in B.host(totals))
    vnew, out_cluster_of = B.empty(vertices, C, "int32"), B.empty(vertices, V, "int32")

    def compact(out_v, out_t, out_c):
        B.call("nerfhip_mesh_decimate_compact", B.ptr(triangles), T, V, B.ptr(cluster_of), B.ptr(flags), C, B.ptr(ref), B.ptr(off_t),
               B.ptr(off_c), B.ptr(positions), B.ptr(cluster_colors), B.ptr(vnew), B.ptr(out_v), B.ptr(out_t), B.ptr(out_c),
               B.ptr(out_cluster_of))
    return result(n_v, n_t, out_cluster_of, (C, bad, collapsed, duplicate, C - n_v), compact)


@device_guard
def mesh_decimate(vertices, triangles, colors=None, cell=1.0, placement="mean", origin=None, eps=1e-3):
    """nerfhip_mesh_decimate_*, with torch.sort between them: vertices (V, 3) fp32, triangles (T, 3) int32 and optional colors (V, 3)
    uint8 on the device -> (vertices' (V', 3), triangles' (T', 3), colors' (V', 3) or None, cluster_of (V,) int32, counts: a dict of
    clusters, bad, collapsed, duplicate, unreferenced) by the contract of include/nerfhip.h.  Reads back the bounds and the
    counts.  ValueError for a cell that is not > 0 and finite, a grid of 2^31 cells or more, an origin above a vertex."""
    return _mesh_decimate(_DeviceArrays, vertices, triangles, colors, cell, placement, origin, eps)


def mesh_decimate_host(vertices, triangles, colors=None, cell=1.0, placement="mean", origin=None, eps=1e-3):
    """The _host twins of `mesh_decimate` with numpy's sorts between them (host, no GPU): numpy in, numpy out, bit for bit what
    the device computes."""
    return _mesh_decimate(_HostArrays, vertices, triangles, colors, cell, placement, origin, eps)

"""`metrics.py` of the reference (metrics.py:4-20).  `ssim` is kornia 0.2.0's `kornia.losses.ssim` as one HIP launch
(`nerfhip_ssim`, DESIGN.md "Image metrics"); there is no kornia dependency."""
import torch

from . import ops


def mse(image_pred, image_gt, valid_mask=None, reduction='mean'):
    value = (image_pred - image_gt) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    if reduction == 'mean':
        return torch.mean(value)
    return value


def psnr(image_pred, image_gt, valid_mask=None, reduction='mean'):
    return -10 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))


def _check_reduction(reduction):
    if reduction not in ('mean', 'none'):
        raise ValueError("ssim: reduction must be 'mean' or 'none', got %r" % (reduction,))


def ssim(image_pred, image_gt, reduction='mean', window_size=3):
    """image_pred and image_gt: (B, 3, H, W) on the GPU (metrics.py:15-20: `1 - 2 * dssim`, in [0, 1] after kornia's clamp).
    window_size=3 is the reference's call; 11 is the usual published setting.  reduction='none' returns the (B, C, H, W) map."""
    if image_pred.dim() != 4 or image_pred.shape != image_gt.shape:
        raise ValueError("ssim: expected two (B, C, H, W) images, got %s and %s" % (tuple(image_pred.shape), tuple(image_gt.shape)))
    _check_reduction(reduction)
    B, C, H, W = image_pred.shape
    map_, mean = ops.ssim(image_pred, image_gt, B, C, H, W, window_size, ops.IMAGE_PLANAR, want_map=reduction == 'none',
                          want_mean=reduction == 'mean')
    return mean if reduction == 'mean' else map_


def ssim_hw3(pred, gt, H, W, reduction='mean', window_size=3):
    """The same for a renderer's (H*W, C) colours (`rgb_fine` of render_rays / GraphRenderer, a dataset's `rgbs`) without a
    permute copy.  reduction='none' returns the (H, W, C) map."""
    if pred.dim() != 2 or pred.shape != gt.shape or pred.shape[0] != H * W:
        raise ValueError("ssim_hw3: expected two (%d, C) images, got %s and %s" % (H * W, tuple(pred.shape), tuple(gt.shape)))
    _check_reduction(reduction)
    C = pred.shape[1]
    map_, mean = ops.ssim(pred, gt, 1, C, H, W, window_size, ops.IMAGE_INTERLEAVED, want_map=reduction == 'none',
                          want_mean=reduction == 'mean')
    return mean if reduction == 'mean' else map_[0]

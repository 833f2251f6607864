"""nerf_pl_amd — MI355X-native (gfx950) implementation of the NeRF volume-rendering hot path of
kwea123/nerf_pl: `models/nerf.py` (Embedding, NeRF) + `models/rendering.py` (render_rays, sample_pdf).

Drop-in use from the reference tree:

    import nerf_pl_amd; nerf_pl_amd.install()      # makes `models.nerf` / `models.rendering` /
                                                   # `torchsearchsorted` resolve to this package
    from models.nerf import Embedding, NeRF
    from models.rendering import render_rays

All compute runs in hand-written HIP kernels behind a C ABI (include/nerfhip.h, libnerfhip.so);
there is no CPU or eager fallback.

Beyond the reference: `nerf_pl_amd.occupancy` (OccupancyGrid, CulledRenderer) skips empty space at eval, opt-in;
`nerf_pl_amd.baked` (BakedVolume, BakedRenderer) renders the exported .vol lattice itself, without the network;
`nerf_pl_amd.meshcast` (MeshBVH, MeshRenderer, MixedRenderer) ray-casts the extracted mesh and puts a mesh into any render.
"""
import os
import sys
import types

_DEFAULT_MLP_DTYPE = os.environ.get("NERF_PL_AMD_MLP_DTYPE", "fp32")


def set_default_mlp_dtype(dtype):
    """'fp32' (exact-fp32 MFMA, the parity configuration) or 'bf16' (bf16 MFMA, fp32 accumulate)."""
    global _DEFAULT_MLP_DTYPE
    from .ops import mlp_dtype_code
    mlp_dtype_code(dtype)
    _DEFAULT_MLP_DTYPE = dtype


def default_mlp_dtype():
    return _DEFAULT_MLP_DTYPE


def install(datasets=False, metrics=False):
    """Register this package's modules under the names the reference imports
    (train.py:10-11, eval.py:9-10, models/rendering.py:2).  datasets=True: also `datasets`, `datasets.blender` and
    `datasets.llff` (train.py:8, eval.py:12) — off by default, so that inside a reference tree the reference's own loaders stay in charge.
    metrics=True: also `metrics` (train.py:19, eval.py:15: mse, psnr, ssim) and `utils.visualization` (train.py:14) — off by default
    for the same reason; a `utils` package that is not imported yet is registered as an empty one holding `visualization`."""
    from . import models, ops
    from .models import nerf, rendering
    sys.modules["models"] = models
    sys.modules["models.nerf"] = nerf
    sys.modules["models.rendering"] = rendering
    tss = types.ModuleType("torchsearchsorted")
    tss.searchsorted = ops.searchsorted
    sys.modules["torchsearchsorted"] = tss
    if datasets:
        from . import datasets as ds
        sys.modules["datasets"] = ds
        sys.modules["datasets.blender"] = ds.blender
        sys.modules["datasets.llff"] = ds.llff
    if metrics:
        from . import metrics as m, visualization
        sys.modules["metrics"] = m
        utils = sys.modules.get("utils")
        if utils is None:
            utils = sys.modules["utils"] = types.ModuleType("utils")
            utils.__path__ = []
        utils.visualization = visualization
        sys.modules["utils.visualization"] = visualization

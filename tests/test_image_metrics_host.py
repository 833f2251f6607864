"""CPU: the image-metric entry points' C ABI surface and argument checks (made before any launch), the CPU refusals of the
Python surface, the float64 restatement the GPU tests use as their yardstick, the built-in JET table and install(metrics=True)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import image_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"nerfhip_ssim", "nerfhip_ssim_workspace_bytes", "nerfhip_depth_colormap", "nerfhip_depth_colormap_workspace_bytes"}


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def test_symbols_in_header_exports_and_signatures(lib):
    from nerf_pl_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerfhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nerfhip_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (nerfhip_[a-z0-9_]+)", out))
    assert NEW <= declared and NEW <= exported and NEW <= set(_lib.SIGNATURES)
    assert lib.nerfhip_abi_version() == 3          # additive: the ABI version stays


def test_ssim_argument_checks_without_a_gpu(lib):
    fake = 0x10000                                  # never dereferenced: every call below returns from the checks
    call = lib.nerfhip_ssim
    assert call(None, None, 0, 3, 8, 8, 3, 0, None, None, None, None) == 0         # B*C*H*W == 0: success
    assert call(fake, fake, 1, 3, 0, 8, 11, 1, fake, fake, fake, None) == 0
    assert call(None, fake, 1, 3, 8, 8, 3, 0, fake, fake, fake, None) == -1        # null image with n > 0
    assert call(fake, None, 1, 3, 8, 8, 3, 0, fake, fake, fake, None) == -1
    for ws in (0, 1, 2, 4, 10, 12, 13, -3):                                        # even or out of range
        assert call(fake, fake, 1, 3, 8, 8, ws, 0, fake, fake, fake, None) == -1
    for layout in (-1, 2, 7):                                                      # unknown layout
        assert call(fake, fake, 1, 3, 8, 8, 3, layout, fake, fake, fake, None) == -1
    assert call(fake, fake, 1, 3, -8, 8, 3, 0, fake, fake, fake, None) == -1       # negative size
    assert call(fake, fake, 1, 3, 8, 8, 3, 0, None, fake, None, None) == -1        # a mean without its workspace
    assert call(fake, fake, 1, 3, 8, 8, 3, 0, None, fake, fake + 4, None) == -1    # workspace not 8-byte aligned
    assert call(fake, fake, 1, 3, 8, 8, 3, 0, None, None, None, None) == 0         # nothing asked for: nothing launched
    ws = lib.nerfhip_ssim_workspace_bytes
    assert ws(1, 3, 800, 800) == 3 * 25 * 25 * 8 and ws(2, 3, 17, 67) == 2 * 3 * 1 * 3 * 8 and ws(1, 3, 33, 32) == 3 * 2 * 8
    assert ws(0, 3, 8, 8) == 0 and ws(1, 3, -1, 8) == 0


def test_depth_colormap_argument_checks_without_a_gpu(lib):
    fake = 0x10000
    call = lib.nerfhip_depth_colormap
    assert call(None, 0, None, None, None, None, None) == 0                        # n == 0: success
    assert call(fake, -1, fake, fake, fake, fake, None) == -1
    assert call(None, 8, fake, fake, fake, fake, None) == -1                       # null depth / table / workspace
    assert call(fake, 8, None, fake, fake, fake, None) == -1
    assert call(fake, 8, fake, fake, fake, None, None) == -1
    assert call(fake, 8, fake, None, None, fake, None) == 0                        # both outputs NULL: nothing launched
    ws = lib.nerfhip_depth_colormap_workspace_bytes
    assert ws(0) == 0 and ws(1) == 8 and ws(257) == 16 and ws(1 << 30) == 1024 * 8


def test_python_surface_refuses_cpu_tensors():
    from nerf_pl_amd import inference, metrics, ops, visualization
    from nerf_pl_amd._lib import NerfHipError
    a = torch.rand(1, 3, 8, 8)
    with pytest.raises(NerfHipError):
        metrics.ssim(a, a)
    with pytest.raises(NerfHipError):
        metrics.ssim(a, a, reduction='none', window_size=11)
    with pytest.raises(NerfHipError):
        metrics.ssim_hw3(torch.rand(64, 3), torch.rand(64, 3), 8, 8)
    with pytest.raises(NerfHipError):
        visualization.visualize_depth(torch.rand(8, 8))
    with pytest.raises(NerfHipError):
        visualization.visualize_depth(torch.rand(8, 8), cmap=None)
    with pytest.raises(NerfHipError):
        ops.depth_colormap(torch.rand(8, 8), torch.zeros(256, 3, dtype=torch.uint8))
    with pytest.raises(NerfHipError):
        inference.image_to_u8(torch.rand(8, 3))


def test_float64_restatement_is_one_on_identical_images():
    g = torch.Generator().manual_seed(0)
    for shape, ws in (((1, 3, 1, 1), 3), ((2, 3, 17, 67), 3), ((1, 3, 17, 67), 11), ((1, 1, 2, 5), 11)):
        a = torch.rand(shape, generator=g)
        m = R.ssim_map(a, a, ws, torch.float64)
        assert m.shape == a.shape and m.dtype == torch.float64
        assert bool((m == 1.0).all())


def test_window_weights():
    w = R.gaussian_window(3)
    assert round(float(w[1, 1]), 4) == 0.1478 and round(float(w[0, 0]), 4) == 0.0947 and round(float(w[2, 0]), 4) == 0.0947
    for ws in (3, 5, 7, 9, 11):
        w = R.gaussian_window(ws)
        assert abs(float(w.sum()) - 1.0) < 1e-14 and torch.equal(w, w.t()) and torch.equal(w, w.flip(0))


def _runs(x):
    """signs of the non-zero steps of x, runs collapsed: [1] rising, [1, -1] rising then falling, ..."""
    d = np.sign(np.diff(x.astype(np.int32)))
    d = d[d != 0]
    return [int(s) for i, s in enumerate(d) if i == 0 or s != d[i - 1]]


def test_jet_table():
    from nerf_pl_amd.imageio_min import jet_table
    t = jet_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    b, g, r = t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()           # output channel order: the map's blue comes first
    assert b[0] == round(255 * 33 / 64) == 131 and g[0] == 0 and r[0] == 0
    assert _runs(b) == [1, -1] and _runs(g) == [1, -1] and _runs(r) == [1, -1]   # a ramp up, a plateau, a ramp down
    # plateaus (c = 1 where |4v - k| <= 0.5, v = (i + 1) / 256): blue i in 31..95, green 95..159, red 159..223
    assert (b[31:96] == 255).all() and (g[95:160] == 255).all() and (r[159:224] == 255).all()
    assert b[30] < 255 and b[96] < 255 and g[94] < 255 and g[160] < 255 and r[158] < 255 and r[224] < 255
    assert (b[159:] == 0).all() and (r[:95] == 0).all() and (g[:31] == 0).all() and (g[223:] == 0).all()
    assert r[255] == round(255 * 0.5) == 128          # 127.5 rounds half to even


def test_visualize_depth_refuses_other_colormaps():
    """the check on `cmap` is made before anything else, so it is answered without a GPU"""
    from nerf_pl_amd import visualization
    for cmap in (0, 1, 3, 11, -2, True, "jet", 2.0):
        with pytest.raises(ValueError):
            visualization.visualize_depth(torch.rand(4, 4), cmap=cmap)
    assert visualization.COLORMAP_JET == 2


def test_install_metrics_registers_and_restores():
    import importlib
    import nerf_pl_amd
    names = ("models", "models.nerf", "models.rendering", "torchsearchsorted", "metrics", "utils", "utils.visualization",
             "datasets", "datasets.blender", "datasets.llff")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in ("metrics", "utils", "utils.visualization"):
            sys.modules.pop(k, None)
        nerf_pl_amd.install()                               # off by default
        assert "metrics" not in sys.modules and "utils.visualization" not in sys.modules
        nerf_pl_amd.install(metrics=True)
        from nerf_pl_amd import metrics as ours_m, visualization as ours_v
        m = importlib.import_module("metrics")
        v = importlib.import_module("utils.visualization")
        assert m is ours_m and v is ours_v
        assert callable(m.mse) and callable(m.psnr) and callable(m.ssim) and callable(v.visualize_depth)
        from utils.visualization import visualize_depth          # train.py:14's form
        assert visualize_depth is ours_v.visualize_depth
    finally:
        for k, val in saved.items():
            if val is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = val
    for k, val in saved.items():
        assert sys.modules.get(k) is val

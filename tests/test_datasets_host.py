"""CPU: the host half of scene loading (nerf_pl_amd/datasets) — the PNG container parser, Pillow's Lanczos taps, the argument
checks of the new C entry points and the refusals that need no GPU."""
import math
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "blender_mini")
EXPECTED = os.path.join(ROOT, "tests", "golden", "blender_mini_expected.npz")


def _unfilter_serial(raw, h, w, ch):
    """The PNG specification's reconstruction, byte by byte (48 x 48 fixtures only: this is the loop the GPU kernel replaces)."""
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), np.int64)
    for y in range(h):
        f = int(rows[y, 0])
        for i in range(w * ch):
            a = out[y, i - ch] if i >= ch else 0
            b = out[y - 1, i] if y else 0
            c = out[y - 1, i - ch] if (y and i >= ch) else 0
            if f == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            else:
                pred = (0, a, b, (a + b) // 2)[f]
            out[y, i] = (int(rows[y, 1 + i]) + pred) & 255
    return out.astype(np.uint8).reshape(h, w, ch)


def test_png_inflate_on_the_fixtures_and_on_png_bytes():
    from nerf_pl_amd.imageio_min import png_bytes, png_inflate
    z = np.load(EXPECTED)
    seen = set()
    for k, name in enumerate(z["names"]):
        w, h, ch, raw = png_inflate(os.path.join(SCENE, "%s.png" % name))
        assert (w, h, ch) == (48, 48, 4) and len(raw) == 48 * (1 + 48 * 4)
        seen |= set(np.frombuffer(raw, np.uint8).reshape(h, -1)[:, 0].tolist())
        assert np.array_equal(_unfilter_serial(raw, h, w, ch), z["rgba_%d" % k])
    assert seen == {0, 1, 2, 3, 4}                       # the scene exercises every filter type
    rng = np.random.default_rng(0)
    for shape in ((5, 7), (5, 7, 3), (6, 3, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        w, h, ch, raw = png_inflate(png_bytes(img))      # bytes, not a path
        assert (w, h, ch) == (shape[1], shape[0], 1 if len(shape) == 2 else shape[2])
        rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)
        assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(shape), img)


def _png(depth=8, color=6, interlace=0, w=2, h=2, payload=None):
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[color]
    raw = payload if payload is not None else bytes(h * (1 + w * ch * depth // 8))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, interlace))
            + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_png_inflate_refuses_what_the_kernel_does_not_take():
    from nerf_pl_amd.imageio_min import png_inflate
    assert png_inflate(_png())[:3] == (2, 2, 4)
    with pytest.raises(ValueError, match="bit depth 16"):
        png_inflate(_png(depth=16))
    with pytest.raises(ValueError, match="interlaced"):
        png_inflate(_png(interlace=1))
    with pytest.raises(ValueError, match="palette"):
        png_inflate(_png(color=3))
    with pytest.raises(ValueError, match=r"grey \+ alpha"):
        png_inflate(_png(color=4))
    with pytest.raises(ValueError, match="needs"):
        png_inflate(_png(payload=bytes(5)))              # truncated image data
    with pytest.raises(ValueError, match="not a PNG"):
        png_inflate(b"GIF89a" + bytes(20))


TAP_CASES = ((48, 20), (48, 31), (48, 80), (800, 400))


@pytest.mark.parametrize("n_in,n_out", TAP_CASES)
def test_lanczos_tap_tables(n_in, n_out):
    from nerf_pl_amd.imageio_min import lanczos_taps
    xmin, count, taps = lanczos_taps(n_in, n_out)
    assert xmin.dtype == count.dtype == taps.dtype == np.int32
    assert xmin.shape == count.shape == (n_out,) and taps.shape[0] == n_out
    # each tap is rounded to the nearest 2^-22, so a row's sum is within half a unit per tap of 2^22
    assert (np.abs(taps.sum(1).astype(np.int64) - (1 << 22)) <= count).all()
    assert (xmin >= 0).all() and (count >= 1).all() and (xmin + count <= n_in).all()
    bound = 2 * math.ceil(3 * max(n_in / n_out, 1.0)) + 1
    assert (count <= bound).all() and taps.shape[1] <= bound
    for xx in range(n_out):
        assert not taps[xx, count[xx]:].any()            # nothing beyond a row's window


def _apply_taps(a, n_out):
    """one axis (axis 1) of Pillow's 8-bit resampling with the tables, in numpy"""
    from nerf_pl_amd.imageio_min import lanczos_taps
    xmin, count, taps = lanczos_taps(a.shape[1], n_out)
    out = np.empty((a.shape[0], n_out, a.shape[2]), np.uint8)
    for xx in range(n_out):
        k = taps[xx, :count[xx]].astype(np.int64)
        s = (a[:, xmin[xx]:xmin[xx] + count[xx]].astype(np.int64) * k[None, :, None]).sum(1) + (1 << 21)
        out[:, xx] = np.clip(s >> 22, 0, 255)
    return out


def test_tap_tables_reproduce_pil_on_rgb():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    for (H, W, h, w) in ((48, 48, 20, 20), (48, 48, 31, 31), (48, 48, 80, 80), (64, 40, 57, 23), (800, 800, 400, 400)):
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(a, "RGB").resize((w, h), Image.LANCZOS))
        got = _apply_taps(a, w) if W != w else a
        got = _apply_taps(got.transpose(1, 0, 2), h).transpose(1, 0, 2) if H != h else got
        assert np.array_equal(got, ref), (H, W, h, w)


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def test_image_entry_points_validate_arguments_without_a_gpu(lib):
    import ctypes
    vp = ctypes.c_void_p
    fake = vp(0x10000)                                   # never dereferenced: every call below returns from the checks
    # unfilter: n_images == 0 is success, null pointers with n > 0 and unsupported channel counts are refused
    assert lib.nerfhip_png_unfilter(None, None, None, 0, 4, 4, 4, None) == 0
    assert lib.nerfhip_png_unfilter(None, None, None, 2, 4, 4, 4, None) == -1
    assert lib.nerfhip_png_unfilter(fake, fake, None, 2, 4, 4, 4, None) == -1
    assert lib.nerfhip_png_unfilter(None, fake, fake, 2, 4, 4, 4, None) == -1
    assert lib.nerfhip_png_unfilter(fake, fake, fake, 2, 4, 4, 2, None) == -1
    assert lib.nerfhip_png_unfilter(fake, fake, fake, -1, 4, 4, 4, None) == -1
    assert lib.nerfhip_png_unfilter(fake, vp(0x10001), fake, 1, 4, 4, 4, None) == -1       # RGBA output: 4-byte aligned
    # resize
    r = lib.nerfhip_resize_rgba_lanczos
    assert r(None, None, None, 0, 8, 8, 4, 4, None, None, None, 0, None, None, None, 0, None) == 0
    assert r(None, None, None, 1, 8, 8, 4, 4, None, None, None, 0, None, None, None, 0, None) == -1
    assert r(fake, vp(0x20000), vp(0x30000), 1, 8, 8, 4, 4, None, None, None, 7, fake, fake, fake, 7, None) == -1   # width changes: no taps
    assert r(fake, vp(0x20000), vp(0x30000), 1, 8, 8, 4, 4, fake, fake, fake, 7, None, None, None, 7, None) == -1   # height changes: no taps
    assert r(fake, vp(0x20000), None, 1, 8, 8, 4, 4, fake, fake, fake, 7, fake, fake, fake, 7, None) == -1          # both: no workspace
    assert r(fake, fake, None, 1, 8, 8, 8, 8, None, None, None, 0, None, None, None, 0, None) == -1                 # in place
    assert r(fake, vp(0x20000), None, 1, 8, 0, 4, 4, None, None, None, 0, None, None, None, 0, None) == -1
    # blend
    b = lib.nerfhip_rgba_to_rgb_white
    assert b(None, None, None, 0, None) == 0
    assert b(None, None, None, 16, None) == -1
    assert b(fake, None, None, 16, None) == -1
    assert b(fake, fake, None, -1, None) == -1


def test_dataset_and_ops_refuse_the_cpu():
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.datasets import BlenderDataset, dataset_dict
    assert dataset_dict == {"blender": BlenderDataset}
    with pytest.raises(NerfHipError):
        BlenderDataset(SCENE, "train", (20, 20), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(NerfHipError):
            BlenderDataset(SCENE, "train", (20, 20))
    with pytest.raises(AssertionError):
        BlenderDataset(SCENE, "train", (20, 24), device="cpu")
    with pytest.raises(NerfHipError):
        ops.decode_png_batch(torch.zeros(1, 4 * 17, dtype=torch.uint8), 4, 4, 4)
    with pytest.raises(NerfHipError):
        ops.resize_rgba_lanczos(torch.zeros(8, 8, 4, dtype=torch.uint8), 4, 4)
    with pytest.raises(NerfHipError):
        ops.rgba_to_rgb_white(torch.zeros(8, 4, dtype=torch.uint8))


def test_install_registers_datasets_only_on_request():
    import nerf_pl_amd
    names = ("models", "models.nerf", "models.rendering", "torchsearchsorted", "datasets", "datasets.blender")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        sys.modules.pop("datasets", None)
        sys.modules.pop("datasets.blender", None)
        nerf_pl_amd.install()
        assert "datasets" not in sys.modules and "datasets.blender" not in sys.modules
        nerf_pl_amd.install(datasets=True)
        import importlib
        ds = importlib.import_module("datasets")
        from nerf_pl_amd.datasets import BlenderDataset
        assert ds.dataset_dict["blender"] is BlenderDataset
        assert importlib.import_module("datasets.blender").BlenderDataset is BlenderDataset
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v

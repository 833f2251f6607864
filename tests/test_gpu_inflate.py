"""GPU: the device inflate (csrc/inflate.hip, ops.inflate_batch) against the machine's zlib over the corpus of
tests/inflate_streams.py — status == 0 <=> zlib.decompress succeeds with exactly out_bytes bytes, and then the bytes are equal —
and the loaders' png_inflate="gpu" against the default datasets, bit for bit.  tests/test_inflate_host.py holds the host twin to
the same corpus without a GPU."""
import os
import shutil
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_streams  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENE = os.path.join(GOLDEN, "blender_mini")
SCENE_PNG = os.path.join(GOLDEN, "llff_mini_png")
E_DATA = -4


@pytest.fixture(scope="module")
def corpus():
    return inflate_streams.corpus()


def test_valid_and_refused_streams_in_mixed_batches(dev, corpus):
    from nerf_pl_amd import ops
    cases = [c for c in corpus if c.group in ("zlib", "hand", "refused")]
    assert len(cases) >= 190
    for batch in inflate_streams.batches(cases, 64):
        out, status = ops.inflate_batch([c.stream for c in batch], batch[0].out_bytes, dev, return_status=True)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (len(batch), batch[0].out_bytes)
        host = out.cpu().numpy()
        for k, c in enumerate(batch):
            assert status[k] == (0 if c.expect is not None else E_DATA), (c.name, int(status[k]))
            if c.expect is not None:
                assert host[k].tobytes() == c.expect, c.name


def test_damaged_streams_status_and_guard_bytes(dev, corpus):
    """The truncations and the first 64 mutations beside good streams, rows at every alignment with a gap between them: every
    verdict is zlib's, the good rows are whole, and no byte outside the rows changes."""
    from nerf_pl_amd import _lib
    n_out = inflate_streams.N
    cases = [c for c in corpus if c.group == "truncated"] + [c for c in corpus if c.group == "mutated"][:64] \
        + [c for c in corpus if c.group == "zlib" and c.out_bytes == n_out][:8]
    assert len(cases) == 96 + 64 + 8
    longer = zlib.compress(inflate_streams.random_bytes(n_out + 700, 5), 6)      # holds more than out_bytes
    streams = [c.stream for c in cases] + [longer]
    n = len(streams)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in streams])
    data = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(offsets).to(dev)
    stride, guard, shift = n_out + 37, 4096, 5
    buf = torch.full((guard + shift + n * stride + guard,), 0xa5, device=dev, dtype=torch.uint8)
    base = (-buf.data_ptr()) % 16 + guard - 16 + shift
    status = torch.full((n,), 77, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        code = _lib.load().nerfhip_inflate(data.data_ptr(), d_off.data_ptr(), data.numel(), n, buf.data_ptr() + base, n_out, stride,
                                           status.data_ptr(), _lib.stream_ptr())
    assert code == 0
    host, got = buf.cpu().numpy(), status.cpu().numpy()
    rows = host[base:base + n * stride].reshape(n, stride)
    for k, c in enumerate(cases):
        assert got[k] == (0 if c.expect is not None else E_DATA), (c.name, int(got[k]))
        if c.expect is not None:
            assert rows[k, :n_out].tobytes() == c.expect, c.name
    assert got[-1] == E_DATA
    assert (rows[:, n_out:] == 0xa5).all() and (host[:base] == 0xa5).all() and (host[base + n * stride:] == 0xa5).all()


def test_bad_offsets_and_empty_batch(dev, corpus):
    from nerf_pl_amd import _lib, ops
    good = next(c for c in corpus if c.name == "distance 3 length 258")
    L = len(good.stream)
    data = torch.from_numpy(np.frombuffer(good.stream * 3, np.uint8).copy()).to(dev)
    offsets = torch.tensor([0, L, L - 1, 3 * L + 1, 3 * L + 1], dtype=torch.int64, device=dev)
    out = torch.zeros((4, good.out_bytes), device=dev, dtype=torch.uint8)
    status = torch.zeros(4, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        assert _lib.load().nerfhip_inflate(data.data_ptr(), offsets.data_ptr(), data.numel(), 4, out.data_ptr(), good.out_bytes,
                                           good.out_bytes, status.data_ptr(), _lib.stream_ptr()) == 0
    assert status.cpu().tolist() == [0, -1, -1, -1]
    assert out[0].cpu().numpy().tobytes() == good.expect and not bool(out[1:].any())
    assert tuple(ops.inflate_batch([], 7, dev).shape) == (0, 7)


def _fixture_pngs():
    out = []
    for base, _, files in os.walk(GOLDEN):
        out += [os.path.join(base, f) for f in sorted(files) if f.endswith(".png")]
    return sorted(out)


def test_decoded_pixels_equal_the_host_inflated_ones(dev):
    from nerf_pl_amd import ops
    from nerf_pl_amd.imageio_min import png_idat, png_inflate
    groups = {}
    for path in _fixture_pngs():
        w, h, ch, stream = png_idat(path)
        groups.setdefault((w, h, ch), []).append((path, stream, png_inflate(path)[3]))
    assert sum(len(g) for g in groups.values()) >= 5
    for (w, h, ch), items in groups.items():
        size = h * (1 + w * ch)
        device = ops.inflate_batch([it[1] for it in items], size, dev, names=[it[0] for it in items])
        host = torch.from_numpy(np.stack([np.frombuffer(it[2], np.uint8) for it in items])).to(dev)
        assert torch.equal(device, host)
        assert torch.equal(ops.decode_png_batch(device, h, w, ch), ops.decode_png_batch(host, h, w, ch))


def test_blender_dataset_gpu_inflate_equals_host(dev):
    from nerf_pl_amd.datasets import BlenderDataset
    for wh in ((48, 48), (40, 40)):
        host = BlenderDataset(SCENE, "train", wh, device=dev)
        gpu = BlenderDataset(SCENE, "train", wh, device=dev, png_inflate="gpu")
        assert host.png_inflate == "host" and gpu.png_inflate == "gpu"
        assert torch.equal(gpu.all_rgbs, host.all_rgbs)
    a, b = BlenderDataset(SCENE, "val", (40, 40), device=dev)[0], BlenderDataset(SCENE, "val", (40, 40), device=dev, png_inflate="gpu")[0]
    assert torch.equal(a["rgbs"], b["rgbs"]) and torch.equal(a["valid_mask"], b["valid_mask"]) and torch.equal(a["rays"], b["rays"])


def test_llff_dataset_gpu_inflate_equals_host(dev):
    from nerf_pl_amd.datasets import LLFFDataset
    host = LLFFDataset(SCENE_PNG, "train", (64, 48), device=dev)
    assert sum(p.endswith(".png") for p in host.image_paths) == 1
    for kw in (dict(png_inflate="gpu"), dict(png_inflate="gpu", jpeg_entropy="gpu")):
        gpu = LLFFDataset(SCENE_PNG, "train", (64, 48), device=dev, **kw)
        assert torch.equal(gpu.all_rgbs, host.all_rgbs)
        assert torch.equal(gpu._load(gpu.image_paths), host._load(host.image_paths))       # every file, the val image included


def test_a_damaged_file_is_named(dev, tmp_path):
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.datasets import BlenderDataset
    scene = str(tmp_path / "scene")
    shutil.copytree(SCENE, scene)
    victim = os.path.join(scene, "train", "r_1.png")
    data = bytearray(open(victim, "rb").read())
    at = data.index(b"IDAT") + 4 + 40                    # a byte inside the deflate data (the container's CRC is not read)
    data[at] ^= 0x5a
    with open(victim, "wb") as f:
        f.write(bytes(data))
    with pytest.raises(NerfHipError) as e:
        BlenderDataset(scene, "train", (40, 40), device=dev, png_inflate="gpu")
    assert "r_1.png" in str(e.value) and "r_0.png" not in str(e.value) and "r_2.png" not in str(e.value)


def test_option_is_validated(dev):
    from nerf_pl_amd.datasets import BlenderDataset, LLFFDataset
    for cls, scene in ((BlenderDataset, SCENE), (LLFFDataset, SCENE_PNG)):
        with pytest.raises(ValueError, match='png_inflate must be "host" or "gpu"'):
            cls(scene, "train", device=dev, png_inflate="device")

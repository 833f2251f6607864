"""GPU: the PNG encoder (csrc/png.hip, ops.png_filter / png_deflate, imageio_min.png_bytes_device,
inference.evaluate(png_encoder="gpu")) equals the numpy restatement tests/png_ref.py byte for byte: filtered streams, deflate
data, lengths, Adler-32 and whole files.  The reference of every case is computed on the CPU, never by a second GPU run; that
the restatement's files are valid PNGs is tests/test_png_host.py's half."""
import os

import numpy as np
import pytest
import torch

import png_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return png_ref.image_cases(dict(np.load(os.path.join(ROOT, "tests", "golden", "gif_mini", "frames.npz"))))


@pytest.fixture(scope="module")
def reference(cases):
    """name -> (stream S, deflate bytes, Adler-32, file), computed once"""
    out = {}
    for name, img in cases.items():
        s = png_ref.filter_stream(img)
        out[name] = (s, png_ref.deflate(s), png_ref.adler32(s), png_ref.png_bytes(img))
    return out


def _as_batch(img):
    return img[None, :, :, None] if img.ndim == 2 else img[None]


def _deflate(streams, dev):
    """(n, bytes) uint8 -> [(deflate bytes, Adler-32)] through ops.png_deflate"""
    from nerf_pl_amd import ops
    data, lengths, adler = ops.png_deflate(torch.from_numpy(np.ascontiguousarray(streams)).to(dev))
    data, lengths, adler = data.cpu().numpy(), lengths.cpu().numpy(), adler.cpu().numpy()
    assert np.all(lengths >= 0), lengths
    return [(data[i, :lengths[i]].tobytes(), int(adler[i]) & 0xffffffff) for i in range(len(lengths))]


def test_filter_equals_the_restatement(dev, cases, reference):
    from nerf_pl_amd import ops
    for name, img in cases.items():
        got = ops.png_filter(torch.from_numpy(np.ascontiguousarray(_as_batch(img))).to(dev)).cpu().numpy()
        want = reference[name][0]
        assert got.shape == (1, want.size), name
        assert np.array_equal(got[0].reshape(want.shape)[:, 0], want[:, 0]), (name, "filter types")
        assert np.array_equal(got[0], want.reshape(-1)), name


def test_deflate_equals_the_restatement(dev, reference):
    for name, (s, raw, adler, _) in reference.items():
        (got, got_adler), = _deflate(s.reshape(1, -1), dev)
        assert got_adler == adler, name
        assert len(got) == len(raw), (name, len(got), len(raw))
        assert got == raw, name


def test_crafted_streams_reach_the_coder_directly(dev):
    for name, stream in png_ref.stream_cases().items():
        (got, got_adler), = _deflate(stream.reshape(1, -1), dev)
        assert got_adler == png_ref.adler32(stream), name
        assert got == png_ref.deflate(stream), name


def runs_and_literals(n, seed):
    """n bytes over a 16-value alphabet: a seeded mix of short pieces (1..3 bytes: literals) and runs of up to 300 (matches)."""
    rng = np.random.RandomState(seed)
    count = n // 40                                                # mean piece length is about 76: more than n bytes in all
    length = np.where(rng.rand(count) < 0.5, rng.randint(1, 4, count), rng.randint(1, 301, count))
    out = np.repeat(rng.randint(0, 16, count).astype(np.uint8), length)
    assert out.size >= n
    return np.ascontiguousarray(out[:n])


def test_more_strips_than_one_pass_of_the_offsets_scan(dev):
    """1025 strips, the last of one byte: png_scan's 1024-wide workgroup carries its sums into a second pass, and png_gather
    searches offsets written by both.  The restatement's per-strip Python is too slow here: the oracle is zlib on the host."""
    import zlib
    from nerf_pl_amd import ops
    stream = runs_and_literals(1024 * ops.PNG_STRIP + 1, seed=11)
    data, lengths, adler = ops.png_deflate(torch.from_numpy(stream[None]).to(dev))
    length = int(lengths[0])
    assert length >= 0
    assert int(adler[0]) & 0xffffffff == zlib.adler32(stream.tobytes())
    assert zlib.decompress(data[0, :length].cpu().numpy().tobytes(), -15) == stream.tobytes()


def test_batches_give_the_same_bytes_per_image(dev, cases):
    from nerf_pl_amd import imageio_min
    frames = dict(np.load(os.path.join(ROOT, "tests", "golden", "gif_mini", "frames.npz")))
    batch = np.ascontiguousarray(frames["movie"])                  # 3 distinct 64 x 200 frames
    assert not np.array_equal(batch[0], batch[1]) and not np.array_equal(batch[1], batch[2])
    want = [png_ref.png_bytes(f) for f in batch]
    three = imageio_min.png_bytes_device(torch.from_numpy(batch).to(dev))
    assert three == want
    for i in range(3):
        assert imageio_min.png_bytes_device(torch.from_numpy(batch[i:i + 1]).to(dev)) == [want[i]]
    grey = np.stack([cases["noise_31x45_grey"], cases["noise_31x45_grey"][::-1], np.zeros((31, 45), np.uint8)])
    assert imageio_min.png_bytes_device(torch.from_numpy(np.ascontiguousarray(grey)).to(dev)) == [png_ref.png_bytes(g) for g in grey]


def test_files_equal_the_restatement_and_decode_on_the_device(dev, cases, reference):
    """png_bytes_device -> png_inflate -> ops.decode_png_batch: the encoder against the project's own all-filter decoder."""
    from nerf_pl_amd import imageio_min, ops
    for name, img in cases.items():
        t = torch.from_numpy(np.ascontiguousarray(_as_batch(img))).to(dev)
        data, = imageio_min.png_bytes_device(t)
        assert data == reference[name][3], name
        w, h, ch, raw = imageio_min.png_inflate(data)
        back = ops.decode_png_batch(torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(1, -1).to(dev), h, w, ch)
        assert torch.equal(back, t), name
    assert imageio_min.png_bytes_device(torch.zeros((0, 4, 4, 3), device=dev, dtype=torch.uint8)) == []


def test_two_calls_give_identical_bytes(dev, cases):
    from nerf_pl_amd import imageio_min
    for name in ("render_64x200", "stripes_rgb", "noise_67x117"):
        t = torch.from_numpy(np.ascontiguousarray(_as_batch(cases[name]))).to(dev)
        assert imageio_min.png_bytes_device(t) == imageio_min.png_bytes_device(t), name


def test_write_png_device_and_wrappers_validate(dev, cases, reference, tmp_path):
    from nerf_pl_amd import imageio_min, ops
    from nerf_pl_amd._lib import NerfHipError
    img = cases["render_96x96_grey"]
    path = str(tmp_path / "grey.png")
    imageio_min.write_png_device([path], torch.from_numpy(img[None].copy()).to(dev))       # (n, H, W): grey
    assert open(path, "rb").read() == reference["render_96x96_grey"][3]
    with pytest.raises(ValueError):
        imageio_min.write_png_device([path, path], torch.from_numpy(img[None].copy()).to(dev))
    with pytest.raises(NerfHipError):
        ops.png_filter(torch.zeros((1, 4, 4, 2), device=dev, dtype=torch.uint8))            # grey + alpha
    with pytest.raises(NerfHipError):
        ops.png_filter(torch.zeros((1, 4, 4, 3), device=dev, dtype=torch.float32))
    with pytest.raises(NerfHipError):
        ops.png_filter(torch.zeros((1, 0, 4, 3), device=dev, dtype=torch.uint8))
    with pytest.raises(NerfHipError):
        ops.png_deflate(torch.zeros((1, 0), device=dev, dtype=torch.uint8))
    with pytest.raises(NerfHipError):
        ops.png_deflate(torch.zeros((2, 9), device=dev, dtype=torch.uint8), meta=torch.zeros((2, 3), device=dev, dtype=torch.int32))
    with pytest.raises(NerfHipError):                                                       # a workspace for fewer streams
        ops.png_deflate(torch.zeros((2, 9), device=dev, dtype=torch.uint8), workspace=ops.png_workspace(1, 9, dev))
    s = reference["render_96x96_grey"][0].reshape(1, -1)                                    # a caller's workspace, larger than needed
    data, lengths, adler = ops.png_deflate(torch.from_numpy(s.copy()).to(dev), workspace=ops.png_workspace(2, s.size, dev))
    assert data[0, :int(lengths[0])].cpu().numpy().tobytes() == reference["render_96x96_grey"][1]
    assert int(adler[0]) & 0xffffffff == reference["render_96x96_grey"][2]


class _Stub:
    """a dataset of 2 views of 20 x 24 with ground truth, and the renderer that 'renders' view i from rays[0, 0] = i"""
    img_wh = (24, 20)

    def __init__(self, dev):
        rng = np.random.RandomState(8)
        y, x = np.mgrid[0:20, 0:24]
        self.views = [torch.from_numpy(np.clip(np.stack([x / 24.0 + 0.3 * i, y / 20.0, rng.rand(20, 24) * i], axis=-1), 0, 1)
                                       .astype(np.float32).reshape(-1, 3)).to(dev) for i in range(2)]
        self.truth = [torch.from_numpy(np.clip(v.cpu().numpy() + 0.05 * rng.randn(480, 3), 0, 1).astype(np.float32)) for v in self.views]

    def __len__(self):
        return len(self.views)

    def __getitem__(self, i):
        rays = torch.zeros(20 * 24, 8)
        rays[:, 0] = i
        return {"rays": rays, "rgbs": self.truth[i]}

    def render(self, rays):
        i = int(rays[0, 0])
        return {"rgb_fine": self.views[i], "depth_fine": self.views[i][:, 0].contiguous()}


def test_evaluate_writes_the_files_of_either_encoder(dev, tmp_path):
    from nerf_pl_amd import imageio_min, inference
    stub = _Stub(dev)
    a_dir, b_dir = str(tmp_path / "host"), str(tmp_path / "gpu")
    host = inference.evaluate(stub, stub.render, dir_name=a_dir, png_encoder="host")
    gpu = inference.evaluate(stub, stub.render, dir_name=b_dir, png_encoder="gpu")
    assert sorted(host) == sorted(gpu) and len(gpu["images"]) == 2
    assert all(np.array_equal(a, b) for a, b in zip(host["images"], gpu["images"]))
    assert host["psnr"] == gpu["psnr"] and host["ssim"] == gpu["ssim"] and len(host["psnr"]) == 2
    assert host["mean_psnr"] == gpu["mean_psnr"] and host["mean_ssim"] == gpu["mean_ssim"]
    assert sorted(os.listdir(a_dir)) == sorted(os.listdir(b_dir)) == ["000.png", "001.png"]
    for i, img in enumerate(gpu["images"]):
        assert img.shape == (20, 24, 3)
        assert open(os.path.join(b_dir, "%03d.png" % i), "rb").read() == png_ref.png_bytes(img), i
        assert open(os.path.join(a_dir, "%03d.png" % i), "rb").read() == imageio_min.png_bytes(img), i
    with pytest.raises(ValueError):
        inference.evaluate(stub, stub.render, dir_name=a_dir, png_encoder="zlib")

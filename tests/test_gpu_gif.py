"""GPU: the animated GIF of eval.py:145 (csrc/gif.hip, imageio_min.gif_bytes, inference.evaluate(gif_path=...)) equals the numpy
restatement tests/gif_ref.py byte for byte: indices, palettes, box counts, per-frame data and lengths, and the whole file.  The
reference of every case is computed on the CPU, never by a second GPU run."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gif_ref

pytestmark = pytest.mark.gpu
K = gif_ref.STRIP


def _debruijn_pairs(n):
    seq = []
    for i in range(256):
        seq.append(i)
        for j in range(i + 1, 256):
            seq += [i, j]
    return np.array(seq[:n], np.uint8)


def _noise(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def _case(name):
    """name -> (F, H, W, 3) uint8"""
    if name.startswith("noise_"):                    # noise_HxW
        h, w = (int(v) for v in name[6:].split("x"))
        return _noise(h, w, h * 1000 + w)[None]
    if name.startswith("strip_"):                    # a frame of K-1, K, K+1, 2K+3 pixels: strip edges, a one-pixel last strip
        n = {"strip_km1": K - 1, "strip_k": K, "strip_kp1": K + 1, "strip_2kp3": 2 * K + 3}[name]
        return _noise(1, n, n)[None] >> 5 << 5       # 512 colours: dictionary hits and misses in every strip
    if name == "render_64x200":
        return gif_ref.render_like(64, 200, seed=0)[None]
    if name == "flat":
        return np.full((1, 90, 100, 3), 201, np.uint8)            # one box, the longest strings, 3 strips
    if name == "checkerboard":
        yy, xx = np.mgrid[0:50, 0:90]
        return np.where(((yy + xx) & 1)[..., None] == 1, np.uint8(250), np.uint8(3)).astype(np.uint8).repeat(3, axis=2)[None]
    if name == "bins256":
        return gif_ref.bins_frame(256, 20, 20, seed=2)[None]
    if name == "bins257":
        return gif_ref.bins_frame(257, 20, 20, seed=3)[None]
    if name == "widest_codes":                       # no byte pair repeats: every pixel is an emission, 12-bit codes by the strip's end
        return _pairs_frame(_debruijn_pairs(K + 40))
    if name == "three_frames":
        return np.stack([gif_ref.render_like(33, 150, seed=4), _noise(33, 150, 9), np.full((33, 150, 3), 255, np.uint8)])
    if name == "sub_blocks_255x1":                   # found with the restatement: the frame's data is exactly 256 = 255 + 1 bytes
        return np.random.RandomState(75).randint(0, 256, (3, 75, 3)).astype(np.uint8)[None]
    if name == "sub_blocks_255x2":                   # ... exactly 510 = 2 * 255 bytes
        return np.random.RandomState(144).randint(0, 256, (3, 144, 3)).astype(np.uint8)[None]
    raise KeyError(name)


def _pairs_frame(v):
    """colours that fall into 256 distinct bins, in the order of the byte sequence v: 256 occupied bins -> index = a
    permutation of v, and still no index pair repeats"""
    r, g = (v.astype(np.int32) >> 4) * 8 + 1, (v.astype(np.int32) & 15) * 8 + 2
    return np.stack([r, g, np.full_like(r, 100)], axis=-1).astype(np.uint8).reshape(1, 1, len(v), 3)


CASES = ["noise_1x1", "noise_1x2", "noise_3x5", "noise_17x67", "strip_km1", "strip_k", "strip_kp1", "strip_2kp3", "render_64x200",
         "flat", "checkerboard", "bins256", "bins257", "noise_64x200", "widest_codes", "three_frames", "sub_blocks_255x1",
         "sub_blocks_255x2"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.mark.parametrize("name", CASES)
def test_gpu_equals_the_restatement(dev, name):
    from nerf_pl_amd import imageio_min, ops
    frames = _case(name)
    F, H, W = frames.shape[:3]
    want = [gif_ref.quantize(f) for f in frames]
    want_data = [gif_ref.lzw(q[0]) for q in want]
    if name == "sub_blocks_255x1":
        assert len(want_data[0]) == 256 + 2
    if name == "sub_blocks_255x2":
        assert len(want_data[0]) == 510 + 2
    if name in ("bins256", "bins257", "flat", "widest_codes"):
        assert want[0][2] == {"bins256": 256, "bins257": 256, "flat": 1, "widest_codes": 256}[name]
    if name == "widest_codes":
        assert gif_ref.lzw_codes(want[0][0])[1].max() == 12
    d = torch.from_numpy(frames).to(dev)
    idx, pal, boxes = ops.gif_quantize(d)
    data, lengths = ops.gif_lzw(idx, H, W)
    assert data.shape == (F, gif_ref.data_stride(H, W))
    idx, pal, boxes, data, lengths = (t.cpu().numpy() for t in (idx, pal, boxes, data, lengths))
    for k in range(F):
        print("%s[%d]: %d boxes, %d bytes of data" % (name, k, want[k][2], len(want_data[k])))
        assert boxes[k] == want[k][2]
        assert np.array_equal(idx[k], want[k][0])
        assert np.array_equal(pal[k], want[k][1])
        assert lengths[k] == len(want_data[k])
        assert data[k, :lengths[k]].tobytes() == want_data[k]
    whole = imageio_min.gif_bytes(d, fps=30)
    assert whole == gif_ref.gif_bytes(frames, fps=30)
    if name == "three_frames":                       # a batch boundary inside the movie changes nothing; another fps only the delays
        assert imageio_min.gif_bytes(d, fps=30, batch=2) == whole
        assert imageio_min.gif_bytes(d, fps=12.5) == gif_ref.gif_bytes(frames, fps=12.5)
        got = imageio_min.read_gif(whole)
        assert got["delays"] == [3, 3, 3] and got["loop"] == 0
        assert all(np.array_equal(got["palettes"][k][got["indices"][k]], want[k][1][want[k][0]].reshape(H, W, 3)) for k in range(F))


def patched_indices(H, W, seed):
    """(H, W) uint8 indices: constant tiles of 61 x 47 (long LZW strings) with 40 patches of noise (a new string per pixel)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    idx = ((yy // 61) * 7 + (xx // 47) * 13).astype(np.uint8)
    for _ in range(40):
        y, x, h, w = rng.randint(0, H - 100), rng.randint(0, W - 100), rng.randint(5, 100), rng.randint(5, 100)
        idx[y:y + h, x:x + w] = rng.randint(0, 256, (h, w))
    return idx


def test_more_strips_than_one_pass_of_the_offsets_scan(dev):
    """1025 strips, the last of 194 pixels: gif_scan's 1024-wide workgroup carries its sum into a second pass, and gif_gather
    searches offsets written by both.  The LZW data goes into the container by the pieces GifWriter uses, with a grey palette,
    and Pillow decodes it: the red channel is the index."""
    import io
    Image = pytest.importorskip("PIL.Image")
    from nerf_pl_amd import imageio_min, ops
    H, W = 1983, 1982
    assert -(-H * W // K) == 1025 and H * W - 1024 * K == 194
    idx = patched_indices(H, W, seed=12)
    data, lengths = ops.gif_lzw(torch.from_numpy(idx.reshape(1, -1)).to(dev), H, W)
    length = int(lengths[0])
    assert length >= 0
    grey = np.arange(256, dtype=np.uint8).repeat(3).tobytes()
    whole = b"".join([imageio_min._gif_header(W, H), imageio_min._gif_frame_header(W, H, 30), grey, b"\x08",
                      data[0, :length].cpu().numpy().tobytes(), b"\x00\x3b"])
    im = Image.open(io.BytesIO(whole))
    assert im.n_frames == 1 and im.size == (W, H)
    assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, 0], idx)


def test_no_frames_and_write_gif(dev, tmp_path):
    from nerf_pl_amd import imageio_min, ops
    idx, pal, boxes = ops.gif_quantize(torch.zeros((0, 5, 7, 3), device=dev, dtype=torch.uint8))
    assert idx.shape == (0, 35) and pal.shape == (0, 256, 3) and boxes.shape == (0,)
    data, lengths = ops.gif_lzw(idx, 5, 7)
    assert data.shape == (0, gif_ref.data_stride(5, 7)) and lengths.shape == (0,)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        imageio_min.gif_bytes(torch.zeros((0, 5, 7, 3), device=dev, dtype=torch.uint8))
    frames = _case("noise_3x5")
    path = str(tmp_path / "a.gif")
    imageio_min.write_gif(path, torch.from_numpy(frames).to(dev), fps=10)
    assert open(path, "rb").read() == gif_ref.gif_bytes(frames, fps=10)


def test_argument_errors_are_codes_and_exceptions(dev):
    from nerf_pl_amd import _lib, ops
    from nerf_pl_amd._lib import NerfHipError
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=dev, dtype=torch.int64)
    p = ctypes.c_void_p(buf.data_ptr())
    q = lib.nerfhip_gif_quantize
    assert q(None, 0, 4, 4, None, None, None, None, None) == 0                       # F == 0: success, nothing touched
    assert q(None, 1, 4, 4, p, p, p, p, None) == -1 and q(p, 1, 4, 4, p, p, p, None, None) == -1      # null pointers
    assert q(p, 1, 0, 4, p, p, p, p, None) == -1 and q(p, 1, 4, 0, p, p, p, p, None) == -1            # H * W == 0
    assert q(p, 1, 65536, 1, p, p, p, p, None) == -1 and q(p, 1, 1, 65536, p, p, p, p, None) == -1    # a side over 65535
    assert q(p, 1, 65535, 65535, p, p, p, p, None) == -1 and q(p, -1, 4, 4, p, p, p, p, None) == -1
    assert q(p, 1, 4, 4, p, p, p, ctypes.c_void_p(buf.data_ptr() + 4), None) == -3                     # workspace alignment
    z = lib.nerfhip_gif_lzw
    assert z(None, 0, 4, 4, None, None, None, None) == 0
    assert z(None, 1, 4, 4, p, p, p, None) == -1 and z(p, 1, 4, 4, None, p, p, None) == -1 and z(p, 1, 0, 4, p, p, p, None) == -1
    assert z(p, 1, 65536, 1, p, p, p, None) == -1 and z(p, 1, 4, 4, p, p, ctypes.c_void_p(buf.data_ptr() + 4), None) == -3
    assert lib.nerfhip_gif_workspace_bytes(1, 65536, 1) == 0 and lib.nerfhip_gif_workspace_bytes(0, 4, 4) == 0
    assert lib.nerfhip_gif_data_stride(0, 4) == 0 and lib.nerfhip_gif_data_stride(800, 800) == gif_ref.data_stride(800, 800)
    assert lib.nerfhip_gif_workspace_bytes(2, 800, 800) >= 2 * 167 * (8192 * 4 + 1440 * 4)
    torch.cuda.synchronize()
    with pytest.raises(NerfHipError):
        ops.gif_quantize(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))               # a host tensor
    with pytest.raises(NerfHipError):
        ops.gif_quantize(torch.zeros((1, 4, 4, 3), device=dev))                      # float32
    with pytest.raises(NerfHipError):
        ops.gif_quantize(torch.zeros((1, 4, 4, 4), device=dev, dtype=torch.uint8))   # RGBA
    with pytest.raises(NerfHipError):
        ops.gif_quantize(torch.zeros((1, 0, 4, 3), device=dev, dtype=torch.uint8))   # no pixels
    with pytest.raises(NerfHipError):
        ops.gif_lzw(torch.zeros((1, 15), device=dev, dtype=torch.uint8), 4, 4)        # indices of another size


class _Stub:
    """a dataset of 10 views of 9 x 14 without ground truth, and the renderer that 'renders' view i from rays[0, 0] = i"""
    img_wh = (14, 9)

    def __init__(self, dev):
        rng = np.random.RandomState(5)
        y, x = np.mgrid[0:9, 0:14]
        self.views = [torch.from_numpy(np.clip(np.stack([x / 14.0 + 0.05 * i, y / 9.0, rng.rand(9, 14) * (i % 3 == 0)], axis=-1), 0, 1)
                                       .astype(np.float32).reshape(-1, 3)).to(dev) for i in range(10)]

    def __len__(self):
        return len(self.views)

    def __getitem__(self, i):
        rays = torch.zeros(9 * 14, 8)
        rays[:, 0] = i
        return {"rays": rays}

    def render(self, rays):
        i = int(rays[0, 0])
        return {"rgb_fine": self.views[i], "depth_fine": self.views[i][:, 0].contiguous()}


def test_evaluate_writes_the_gif(dev, tmp_path):
    from nerf_pl_amd import inference
    stub = _Stub(dev)
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    gif_path = str(tmp_path / "scene.gif")
    plain = inference.evaluate(stub, stub.render, dir_name=a_dir, save_depth=True)
    with_gif = inference.evaluate(stub, stub.render, dir_name=b_dir, save_depth=True, gif_path=gif_path, fps=30)
    assert sorted(plain) == sorted(with_gif) and len(with_gif["images"]) == 10
    assert all(np.array_equal(a, b) for a, b in zip(plain["images"], with_gif["images"]))
    assert plain["psnr"] == with_gif["psnr"] == [] and plain["mean_ssim"] is with_gif["mean_ssim"] is None
    assert open(gif_path, "rb").read() == gif_ref.gif_bytes(with_gif["images"], fps=30)
    names = sorted(os.listdir(a_dir))
    assert names == sorted(os.listdir(b_dir)) == sorted(["%03d.png" % i for i in range(10)] + ["depth_%03d.pfm" % i for i in range(10)])
    for n in names:
        assert open(os.path.join(a_dir, n), "rb").read() == open(os.path.join(b_dir, n), "rb").read(), n
    assert sorted(os.listdir(str(tmp_path))) == ["a", "b", "scene.gif"]

"""CPU: the PNG encoder's definition as tests/png_ref.py restates it.  What the restatement writes is a valid
PNG: Pillow (which checks the chunk CRCs), zlib.decompress on the IDAT body (which checks the Adler-32) and
imageio_min.png_inflate all read the input back.  The library's host-side code-length construction (nerfhip_png_code_lengths,
the function the strip kernel runs) equals the restatement's on histograms no image produces.  The GPU half is
tests/test_gpu_png.py.

Sizes in bytes of the whole file, restatement / png_bytes(level 6), recorded from this test's cases (DESIGN.md §15 holds the
table): render_64x200 9,637 / 18,164; render_96x96 8,067 / 13,777; gradient_48x64 1,680 / 8,237; noise_67x117 23,754 / 23,657."""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest

import png_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = png_ref.STRIP


@pytest.fixture(scope="module")
def cases():
    return png_ref.image_cases(dict(np.load(os.path.join(ROOT, "tests", "golden", "gif_mini", "frames.npz"))))


@pytest.fixture(scope="module")
def files(cases):
    return {name: png_ref.png_bytes(img) for name, img in cases.items()}


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def _idat(data):
    pos, out = 8, b""
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            out += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out


def test_cases_cover_the_channel_counts_and_strip_edges(cases):
    assert {1 if img.ndim == 2 else img.shape[2] for img in cases.values()} == {1, 3, 4}
    sizes = {name: png_ref.filter_stream(img).size for name, img in cases.items()}
    assert sizes["stream_k_grey"] == K and sizes["stream_kp1_grey"] == sizes["stream_kp1_rgba"] == K + 1
    assert sizes["stream_2kp1_grey"] == 2 * K + 1
    row = cases["straddle_7x1000_rgb"].shape[1] * 3 + 1
    assert all(k % row for k in range(K, sizes["straddle_7x1000_rgb"], K))          # every strip ends inside a row
    for name in ("stripes_grey", "stripes_rgb", "stripes_rgba"):                      # every edge of the token rule is met
        runs = {L for _, L in png_ref.runs_of(png_ref.filter_stream(cases[name]).reshape(-1))}
        assert set(png_ref.RUN_EDGES) <= runs, (name, sorted(runs))
    tokens = png_ref.strip_tokens(png_ref.filter_stream(cases["noise_67x117"]).reshape(-1)[:K])
    assert all(sym < 256 for sym, _, _ in tokens)                                     # no match: the strip declares HDIST = 0


def test_token_rule_at_its_edges():
    def lengths(L):
        toks = png_ref.strip_tokens(np.zeros(L, np.uint8))
        return [0 if sym < 256 else png_ref.LEN_BASE[sym - 257] + ev for sym, _, ev in toks]
    assert lengths(1) == [0] and lengths(2) == [0, 0] and lengths(3) == [0, 0, 0] and lengths(4) == [0, 3]
    assert lengths(258) == [0, 257] and lengths(259) == [0, 258] and lengths(260) == [0, 258, 0]
    assert lengths(261) == [0, 258, 0, 0] and lengths(262) == [0, 258, 3] and lengths(517) == [0, 258, 258]
    for L in (1, 2, 5, 300, 8192):
        assert sum(max(v, 1) for v in lengths(L)) == L


def test_every_file_is_a_valid_png_of_its_pixels(cases, files):
    from PIL import Image
    from nerf_pl_amd import imageio_min
    for name, img in cases.items():
        data = files[name]
        ch = 1 if img.ndim == 2 else img.shape[2]
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[ch], name
            assert np.array_equal(np.asarray(im), img), name
        stream = png_ref.filter_stream(img)
        body = _idat(data)
        assert body[:2] == b"\x78\x01"
        assert zlib.decompress(body) == stream.tobytes(), name                        # (checks the Adler-32)
        assert struct.unpack(">I", body[-4:])[0] == zlib.adler32(stream.tobytes()), name
        w, h, c, raw = imageio_min.png_inflate(data)
        assert (h, w, c) == (img.shape[0], img.shape[1], ch) and raw == stream.tobytes(), name
        # filters reversed independently of the restatement's forward form
        got = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * c)
        assert np.array_equal(_unfilter(got, c).reshape(img.shape), img), name


def _unfilter(rows, bpp):
    h, n = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((h + 1, n + bpp), np.int64)
    for y in range(h):
        t = rows[y, 0]
        for i in range(n):
            a, b, c = out[y + 1, i], out[y, i + bpp], out[y, i]
            p = a + b - c
            pred = (0, a, b, (a + b) >> 1,
                    a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else b if abs(p - b) <= abs(p - c) else c)[t]
            out[y + 1, i + bpp] = (rows[y, 1 + i] + pred) & 255
    return out[1:, bpp:].astype(np.uint8)


def test_crafted_streams_inflate_back():
    for name, stream in png_ref.stream_cases().items():
        raw = png_ref.deflate(stream)
        assert zlib.decompress(raw, -15) == stream.tobytes(), name
        assert png_ref.adler32(stream) == zlib.adler32(stream.tobytes()), name


def test_fibonacci_stream_reaches_the_15_bit_limit():
    stream = png_ref.fibonacci_stream()
    assert stream.size == 2583 and np.all(stream[1:] != stream[:-1])
    hist = np.bincount(stream, minlength=286)
    hist[256] = 1
    assert sorted(hist[hist > 0].tolist()) == [1, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987]
    assert max(png_ref.code_lengths(hist, 32)) == 16                                   # unlimited, the chain is 16 deep
    lengths = png_ref.code_lengths(hist, 15)
    assert max(lengths) == 15 and sum(2.0 ** -l for l in lengths if l) == 1.0


def _library_lengths(lib, counts, limit):
    counts = np.ascontiguousarray(counts, np.uint32)
    out = np.full(counts.size, 99, np.uint8)
    assert lib.nerfhip_png_code_lengths(counts.ctypes.data, counts.size, limit, out.ctypes.data) == 0
    return out.tolist()


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def test_library_code_lengths_equal_the_restatement(lib):
    rng = np.random.RandomState(0)
    hists = []
    for trial in range(40):                                     # random: sparse and dense, small and large counts, many ties
        n = (286, 19, 30, 2, 286)[trial % 5]
        counts = rng.randint(0, (3, 50, 9000)[trial % 3], n) * (rng.rand(n) < (0.1, 0.5, 1.0)[(trial // 3) % 3])
        hists.append((counts, 15 if n > 19 else (7, 15)[trial % 2]))
    for n, limit in ((286, 15), (19, 7)):
        for sym in (0, n // 2, n - 1):                          # one symbol
            one = np.zeros(n, np.int64)
            one[sym] = 5
            hists.append((one, limit))
        for a, b, ca, cb in ((0, 1, 1, 1), (3, n - 1, 7, 2), (n - 2, n - 1, 1, 8000)):      # two symbols
            two = np.zeros(n, np.int64)
            two[a], two[b] = ca, cb
            hists.append((two, limit))
    hists += [(_fib(17), 15), (_fib(9), 7), (_fib(17)[::-1], 15), (_fib(9)[::-1], 7), (_fib(19), 7), (_fib(24), 15),
              ([0] * 100 + _fib(17) + [0] * 50 + [1, 1, 1], 15), (np.zeros(286, np.int64), 15)]
    forced = 0
    for counts, limit in hists:
        counts = np.asarray(counts, np.int64)
        want = png_ref.code_lengths(counts, limit)
        assert _library_lengths(lib, counts, limit) == want, (counts.tolist(), limit)
        used = int((counts > 0).sum())
        assert all((l > 0) == (c > 0) for l, c in zip(want, counts)) and max(want) <= limit
        kraft = sum(2.0 ** -l for l in want if l)
        assert kraft == 1.0 if used >= 2 else (kraft == 0.5 and used == 1) or (kraft == 0 and used == 0), (counts.tolist(), limit)
        forced += max(png_ref.code_lengths(counts, 64), default=0) > limit
    assert max(png_ref.code_lengths(_fib(17), 64)) == 16 and max(png_ref.code_lengths(_fib(9), 64)) == 8
    assert forced >= 6


def test_the_file_is_no_larger_than_the_host_writers(cases, files):
    from nerf_pl_amd import imageio_min
    for name in ("render_64x200", "render_96x96", "gradient_48x64"):
        assert len(files[name]) <= len(imageio_min.png_bytes(cases[name], 6)), name


def test_entry_points_validate_arguments_without_a_gpu(lib):
    """Argument validation returns NERFHIP_E_BADARG (-1) before anything is launched or dereferenced; n == 0 is success."""
    fake = ctypes.c_void_p(0x10000)                               # never dereferenced: every call below returns from the checks
    assert lib.nerfhip_png_filter(fake, 1, 4, 4, 2, fake, None) == -1                 # C = 2
    assert lib.nerfhip_png_filter(fake, 1, 4, 4, 0, fake, None) == -1
    assert lib.nerfhip_png_filter(fake, 1, 0, 4, 3, fake, None) == -1
    assert lib.nerfhip_png_filter(fake, 1, 32768, 16384, 4, fake, None) == -1         # H * (1 + W*C) = 2^31 + 2^15
    assert lib.nerfhip_png_filter(fake, 1, 65536, 32767, 1, fake, None) == -1         # H * (1 + W*C) = 2^31 exactly
    assert lib.nerfhip_png_filter(fake, 65536, 4, 4, 3, fake, None) == -1             # n > 65535
    assert lib.nerfhip_png_filter(fake, -1, 4, 4, 3, fake, None) == -1
    assert lib.nerfhip_png_filter(None, 1, 4, 4, 3, fake, None) == -1                 # null pointers, n > 0
    assert lib.nerfhip_png_filter(fake, 1, 4, 4, 3, None, None) == -1
    assert lib.nerfhip_png_filter(None, 0, 4, 4, 3, None, None) == 0                  # n == 0: nothing to do
    assert lib.nerfhip_png_deflate(fake, 1, 2 ** 31, fake, fake, fake, fake, None) == -1
    assert lib.nerfhip_png_deflate(fake, 1, 0, fake, fake, fake, fake, None) == -1
    assert lib.nerfhip_png_deflate(fake, 65536, 100, fake, fake, fake, fake, None) == -1
    for k in range(5):
        args = [fake, 1, 100, fake, fake, fake, fake, None]
        args[(0, 3, 4, 5, 6)[k]] = None
        assert lib.nerfhip_png_deflate(*args) == -1
    assert lib.nerfhip_png_deflate(fake, 1, 100, fake, fake, fake, ctypes.c_void_p(0x10004), None) == -3      # NERFHIP_E_ALIGN
    assert lib.nerfhip_png_deflate(None, 0, 100, None, None, None, None, None) == 0
    assert lib.nerfhip_png_workspace_bytes(0, 100) == 0 and lib.nerfhip_png_workspace_bytes(1, 2 ** 31) == 0
    assert lib.nerfhip_png_workspace_bytes(65536, 100) == 0 and lib.nerfhip_png_data_stride(0) == 0
    # the derived worst case: per strip 17 + 57 + 287 * 14 + 15 bits around 15 bits per byte
    head = 17 + 57 + 287 * 14 + 15
    for nbytes in (1, K, K + 1, 3 * K + 5, 800 * 2401):
        assert lib.nerfhip_png_data_stride(nbytes) == (-(-nbytes // K) * head + 15 * nbytes + 7) // 8
        assert lib.nerfhip_png_workspace_bytes(2, nbytes) >= 2 * -(-nbytes // K) * (head + 15 * K) // 8
    u32, u8 = (ctypes.c_uint32 * 4)(1, 2, 3, 4), (ctypes.c_uint8 * 4)()
    assert lib.nerfhip_png_code_lengths(None, 4, 15, u8) == -1 and lib.nerfhip_png_code_lengths(u32, 4, 15, None) == -1
    assert lib.nerfhip_png_code_lengths(u32, 4, 16, u8) == -1 and lib.nerfhip_png_code_lengths(u32, 4, 0, u8) == -1
    assert lib.nerfhip_png_code_lengths(u32, 0, 15, u8) == -1 and lib.nerfhip_png_code_lengths(u32, 287, 15, u8) == -1
    assert lib.nerfhip_png_code_lengths(u32, 4, 1, u8) == -1                          # 4 symbols cannot all get 1-bit codes
    assert lib.nerfhip_png_code_lengths(u32, 4, 2, u8) == 0 and list(u8) == [2, 2, 2, 2]


def test_python_surface_refuses_cpu_tensors_and_unknown_encoders():
    import torch
    from nerf_pl_amd import imageio_min, inference, ops
    from nerf_pl_amd._lib import NerfHipError
    assert ops.PNG_STRIP == K
    with pytest.raises(NerfHipError):
        ops.png_filter(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    with pytest.raises(NerfHipError):
        ops.png_deflate(torch.zeros((1, 52), dtype=torch.uint8))
    with pytest.raises(NerfHipError):
        imageio_min.png_bytes_device(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        inference.evaluate(None, None, png_encoder="zlib")

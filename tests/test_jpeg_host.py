"""CPU: the host half of JPEG decoding — imageio_min.jpeg_parse and the C entropy decoder (nerfhip_jpeg_entropy_decode, which
needs no GPU) — on the files of tests/golden/jpeg_mini (tests/tools/make_golden_llff.py).  The decoder's coefficients are pushed
through a numpy restatement of what the kernels of csrc/jpeg.hip compute (dequantise, libjpeg's islow inverse DCT, libjpeg-turbo's
triangle upsampling, fixed-point YCbCr -> RGB) and must give PIL's bytes exactly: that proves the host half and pins the
arithmetic the kernels have to match before a GPU is reached."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEGS = os.path.join(ROOT, "tests", "golden", "jpeg_mini")
E_BADARG, E_DATA = -1, -4


@pytest.fixture(scope="module")
def expected():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_mini_expected.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def _path(name):
    return os.path.join(JPEGS, name + ".jpg")


def _decodable(expected):
    return [(k, n) for k, n in enumerate(expected["names"]) if "progressive" not in n]


# ---- numpy restatement of the device half --------------------------------------------------------------------------------------
def _idct8(v, shift):
    """jidctint.c's 8-point pass along axis 0 of an int64 array (8, ...)"""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0, tmp1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = 1 << (shift - 1)
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                     tmp10 - tmp3]) + half >> shift


def _plane(coef, q):
    """(by, bx, 64) int16 blocks, (64,) table -> (by * 8, bx * 8) samples"""
    by, bx = coef.shape[:2]
    d = (coef.astype(np.int64) * q.astype(np.int64)).reshape(by, bx, 8, 8)
    ws = _idct8(np.moveaxis(d, 2, 0), 11)                          # columns: over the row index -> (8 rows, by, bx, 8 cols)
    out = _idct8(np.moveaxis(ws, 3, 0), 18)                        # rows: over the column index -> (8 cols, 8 rows, by, bx)
    x = out & 1023
    x = np.where(x >= 512, x - 1024, x) + 128
    return np.clip(x, 0, 255).transpose(2, 1, 3, 0).reshape(by * 8, bx * 8)


def _triangle(s, shift, c_even, c_odd):
    """jdsample.c's horizontal triangle filter on (rows, cw): out[2i] = (3 s[i] + s[i-1] + c_even) >> shift, out[2i+1] = (3 s[i] +
    s[i+1] + c_odd) >> shift.  The edge samples are written there as s[0] / s[-1] (h2v1) or (4 s + c) >> 4 (h2v2): both are what
    the general term gives with the missing neighbour replaced by the sample itself, since (4 s + 1) >> 2 = (4 s + 2) >> 2 = s."""
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + left + c_even) >> shift
    out[:, 1::2] = (3 * s + right + c_odd) >> shift
    return out


def _upsample(c, W, H, hs, vs):
    """chroma plane (padded) -> (H, W), as jdsample.c: the real plane is ceil(W / hs) x ceil(H / vs), its last column and row the
    filters' edges; planes of at most 2 columns are replicated"""
    cw, chh = -(-W // hs), -(-H // vs)
    c = c[:chh, :cw].astype(np.int64)
    if hs == 1:
        return c[:H, :W]
    if cw <= 2:
        return np.repeat(np.repeat(c, vs, 0), 2, 1)[:H, :W]
    if vs == 1:
        return _triangle(c, 2, 1, 2)[:H, :W]
    above = np.concatenate([c[:1], c[:-1]])
    below = np.concatenate([c[1:], c[-1:]])
    out = np.empty((2 * chh, 2 * cw), np.int64)
    out[0::2] = _triangle(3 * c + above, 4, 8, 7)
    out[1::2] = _triangle(3 * c + below, 4, 8, 7)
    return out[:H, :W]


def numpy_decode(parsed, coef):
    W, H = parsed["width"], parsed["height"]
    comps = parsed["components"]
    planes = [_plane(coef[i], parsed["quant"][c[3]]) for i, c in enumerate(comps)]
    y = planes[0][:H, :W]
    if len(comps) == 1:
        return np.repeat(y[..., None], 3, 2).astype(np.uint8)
    hs, vs = comps[0][1], comps[0][2]
    cb = _upsample(planes[1], W, H, hs, vs) - 128
    cr = _upsample(planes[2], W, H, hs, vs) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- the parser ----------------------------------------------------------------------------------------------------------------
def test_jpeg_parse_fields_of_every_fixture(expected):
    from nerf_pl_amd.imageio_min import JPEG_ZIGZAG, jpeg_parse
    assert sorted(JPEG_ZIGZAG.tolist()) == list(range(64)) and JPEG_ZIGZAG[:6].tolist() == [0, 1, 8, 16, 9, 2]
    seen = set()
    for k, name in _decodable(expected):
        p = jpeg_parse(_path(name))
        H, W = expected["rgb_%d" % k].shape[:2]
        assert (p["width"], p["height"]) == (W, H) and "%dx%d" % (W, H) in name
        comps = p["components"]
        if "grey" in name:
            assert len(comps) == 1 and comps[0][1:3] == (1, 1)
            sampling = "grey"
        else:
            assert len(comps) == 3 and [c[0] for c in comps] == [1, 2, 3] and comps[1][1:3] == comps[2][1:3] == (1, 1)
            sampling = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[comps[0][1:3]]
            assert comps[0][3] == 0 and comps[1][3] == comps[2][3] == 1          # luma / chroma quantisation tables
            assert comps[0][4:] == (0, 0) and comps[1][4:] == comps[2][4:] == (1, 1)
        assert "_%s_" % sampling in name
        seen.add(sampling)
        hs, vs = comps[0][1], comps[0][2]
        assert (p["mcus_x"], p["mcus_y"]) == (-(-W // (8 * hs)), -(-H // (8 * vs)))
        for c in comps:
            q = p["quant"][c[3]]
            assert q.dtype == np.uint16 and q.shape == (64,) and q.min() >= 1
        if name.startswith("q100"):
            assert all((q == 1).all() for q in p["quant"].values())
        if name.startswith("q30"):
            assert p["quant"][0][0] == 27 and p["quant"][0][1] == 18              # the standard luma table scaled by 5/3, natural order
        assert set(p["huffman"]) == ({(0, 0), (1, 0)} if sampling == "grey" else {(0, 0), (1, 0), (0, 1), (1, 1)})
        for (tc, th), (counts, symbols) in p["huffman"].items():
            assert counts.shape == (16,) and len(symbols) == counts.sum()
            if "optimized" not in name:
                assert len(symbols) == (12 if tc == 0 else 162)                   # the standard tables
        if "optimized" in name:
            assert sum(len(s) for _, s in p["huffman"].values()) < 2 * (12 + 162)
        restart = int(name.rsplit("restart", 1)[1]) if "restart" in name else 0
        assert p["restart_interval"] == restart
        scan = np.frombuffer(p["scan"], np.uint8)
        ff = np.flatnonzero(scan[:-1] == 0xff)
        rst = [int(scan[i + 1]) for i in ff if 0xd0 <= scan[i + 1] <= 0xd7]
        n_mcu = p["mcus_x"] * p["mcus_y"]
        assert rst == ([0xd0 + (i & 7) for i in range(-(-n_mcu // restart) - 1)] if restart else [])
        assert all(scan[i + 1] == 0 or 0xd0 <= scan[i + 1] <= 0xd7 for i in ff) and scan[-1] != 0xff
    assert seen == {"444", "422", "420", "grey"}
    with open(_path("q90_420_8x8"), "rb") as f:
        assert jpeg_parse(f.read())["width"] == 8                                 # bytes, not a path


def test_refusals_name_the_problem_and_the_file(expected):
    from nerf_pl_amd.imageio_min import jpeg_parse
    path = _path("q90_420_32x32_progressive")
    with pytest.raises(ValueError, match="progressive") as e:
        jpeg_parse(path)
    assert path in str(e.value)
    data = bytearray(open(_path("q90_420_61x45"), "rb").read())
    sof = data.index(b"\xff\xc0")

    def patched(offset, value):
        d = bytearray(data)
        d[sof + offset] = value
        return bytes(d)
    with pytest.raises(ValueError, match="12-bit"):
        jpeg_parse(patched(4, 12))
    with pytest.raises(ValueError, match="arithmetic"):
        jpeg_parse(patched(1, 0xc9))
    with pytest.raises(ValueError, match="sampling factors"):
        jpeg_parse(patched(11, 0x12))                                             # luma 1x2
    with pytest.raises(ValueError, match="sampling factors"):
        jpeg_parse(patched(14, 0x21))                                             # chroma 2x1
    with pytest.raises(ValueError, match="not a JPEG"):
        jpeg_parse(b"\x89PNG\r\n\x1a\n" + bytes(32))
    four = bytearray(data)
    four[sof + 9] = 4                                                             # 4 components: the segment length no longer fits
    with pytest.raises(ValueError):
        jpeg_parse(bytes(four))


# ---- the entropy decoder -------------------------------------------------------------------------------------------------------
def test_coefficients_give_pils_bytes_through_the_numpy_restatement(lib, expected):
    from nerf_pl_amd import ops
    from nerf_pl_amd.imageio_min import jpeg_parse
    for k, name in _decodable(expected):
        parsed = jpeg_parse(_path(name))
        coef = ops.jpeg_entropy_decode(parsed)
        assert len(coef) == len(parsed["components"])
        for c, a in zip(parsed["components"], coef):
            assert a.dtype == np.int16 and a.shape == (parsed["mcus_y"] * c[2], parsed["mcus_x"] * c[1], 64)
        got = numpy_decode(parsed, coef)
        want = expected["rgb_%d" % k]
        assert got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_damaged_files_raise_and_do_not_crash(lib, expected):
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.imageio_min import jpeg_parse

    def decode(data):
        return ops.jpeg_entropy_decode(jpeg_parse(data))
    for k, name in _decodable(expected):
        data = open(_path(name), "rb").read()
        for cut in (len(data) // 3, 2 * len(data) // 3):
            with pytest.raises((ValueError, NerfHipError)):
                decode(data[:cut])
            # ... and with the end-of-image marker put back behind the cut, so that the parser accepts the file and the C decoder
            # meets the truncated scan
            if cut > data.index(b"\xff\xda") + 14:
                body = data[:cut - 1] if data[cut - 1] == 0xff else data[:cut]
                with pytest.raises(NerfHipError, match="damaged"):
                    decode(body + b"\xff\xd9")
    # a Huffman table zeroed: the counts and symbols of the first DC table
    data = bytearray(open(_path("q90_420_61x45"), "rb").read())
    at = data.index(b"\xff\xc4") + 5
    data[at:at + 16 + 12] = bytes(28)
    with pytest.raises((ValueError, NerfHipError)):
        decode(bytes(data))
    # over-subscribed code lengths (three codes of length 1) reach the C side intact and are refused there
    parsed = jpeg_parse(_path("q90_420_61x45"))
    counts, symbols = parsed["huffman"][(1, 0)]
    counts = counts.copy()
    counts[0] = 3
    parsed["huffman"][(1, 0)] = (counts, np.concatenate([symbols, symbols[:3]]))
    with pytest.raises(NerfHipError, match="damaged"):
        ops.jpeg_entropy_decode(parsed)
    # a table the scan names but the file does not define
    parsed = jpeg_parse(_path("q90_420_61x45"))
    del parsed["huffman"][(1, 1)]
    with pytest.raises(NerfHipError, match="damaged"):
        ops.jpeg_entropy_decode(parsed)
    # a wrong restart marker number
    parsed = jpeg_parse(_path("q85_420_61x45_restart3"))
    scan = bytearray(parsed["scan"])
    scan[scan.index(b"\xff\xd1") + 1] = 0xd5
    parsed["scan"] = bytes(scan)
    with pytest.raises(NerfHipError, match="damaged"):
        ops.jpeg_entropy_decode(parsed)
    # random bytes as a scan: an error or garbage coefficients, never a crash
    rng = np.random.default_rng(0)
    for i in range(20):
        parsed = jpeg_parse(_path("q90_420_61x45"))
        noise = rng.integers(0, 255, rng.integers(1, 400), dtype=np.uint8).tobytes()      # (no 0xff: no markers)
        parsed["scan"] = noise
        try:
            ops.jpeg_entropy_decode(parsed)
        except NerfHipError:
            pass


def test_entry_point_validates_arguments(lib):
    from nerf_pl_amd import ops
    from nerf_pl_amd.imageio_min import jpeg_parse
    parsed = jpeg_parse(_path("q90_420_8x8"))
    scan = np.frombuffer(parsed["scan"], np.uint8)
    comp = np.array([[2, 2, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1]], np.int32)
    table = np.zeros((8, 272), np.uint8)
    mask = 0
    for (tc, th), (counts, symbols) in parsed["huffman"].items():
        table[4 * tc + th, :16], table[4 * tc + th, 16:16 + len(symbols)] = counts, symbols
        mask |= 1 << (4 * tc + th)
    coef = [np.zeros((4, 64), np.int16), np.zeros((1, 64), np.int16), np.zeros((1, 64), np.int16)]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in coef])
    caps = (ctypes.c_int64 * 3)(4, 1, 1)
    f = lib.nerfhip_jpeg_entropy_decode
    good = (scan.ctypes.data, len(scan), 3, comp.ctypes.data, table.ctypes.data, mask, 1, 1, 0, ptrs, caps)
    assert f(*good) == 0
    assert np.array_equal(np.concatenate([c.reshape(-1) for c in coef]),
                          np.concatenate([c.reshape(-1) for c in ops.jpeg_entropy_decode(parsed)]))

    def with_(i, v):
        a = list(good)
        a[i] = v
        return f(*a)
    assert with_(0, None) == E_BADARG and with_(3, None) == E_BADARG and with_(4, None) == E_BADARG
    assert with_(9, None) == E_BADARG and with_(10, None) == E_BADARG
    assert with_(1, 0) == E_BADARG and with_(1, -5) == E_BADARG
    assert with_(2, 0) == E_BADARG and with_(2, 2) == E_BADARG and with_(2, 4) == E_BADARG
    assert with_(6, 0) == E_BADARG and with_(7, 0) == E_BADARG and with_(8, -1) == E_BADARG
    assert with_(10, (ctypes.c_int64 * 3)(3, 1, 1)) == E_BADARG                   # too small an output for the luma blocks
    assert with_(9, (ctypes.c_void_p * 3)(coef[0].ctypes.data, None, coef[2].ctypes.data)) == E_BADARG
    bad = comp.copy()
    bad[0, 0] = 3
    assert with_(3, bad.ctypes.data) == E_BADARG
    assert with_(5, mask & ~1) == E_DATA                                          # DC table 0 undefined
    assert with_(1, len(scan) // 2) == E_DATA                                     # half the scan
    assert b"damaged" in lib.nerfhip_error_string(E_DATA)
    # the device entry points refuse bad arguments before anything is launched
    d = lib.nerfhip_jpeg_decode
    fake = ctypes.c_void_p(0x10000)
    assert d(None, None, None, None, None, None, 0, 8, 8, 3, 2, 2, None) == 0
    assert d(None, None, None, None, None, None, 1, 8, 8, 3, 2, 2, None) == E_BADARG
    assert d(fake, None, None, fake, fake, fake, 1, 8, 8, 3, 2, 2, None) == E_BADARG       # three components, one array
    assert d(fake, fake, fake, fake, fake, fake, 1, 8, 8, 3, 1, 2, None) == E_BADARG       # 1x2 sampling
    assert d(fake, fake, fake, fake, fake, fake, 1, 8, 8, 4, 1, 1, None) == E_BADARG
    assert d(fake, None, None, fake, fake, fake, 1, 8, 8, 1, 2, 1, None) == E_BADARG
    assert d(fake, fake, fake, fake, fake, fake, 1, 0, 8, 3, 1, 1, None) == E_BADARG
    assert d(ctypes.c_void_p(0x10002), fake, fake, fake, fake, fake, 1, 8, 8, 3, 1, 1, None) == -3
    assert lib.nerfhip_jpeg_planes_bytes(45, 61, 3, 2, 2) == 64 * 48 + 2 * 32 * 24
    assert lib.nerfhip_jpeg_planes_bytes(45, 61, 1, 1, 1) == 64 * 48 and lib.nerfhip_jpeg_planes_bytes(45, 61, 3, 1, 2) == 0


def test_ops_refuse_the_cpu():
    import torch
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    with pytest.raises(NerfHipError, match="no CPU fallback"):
        ops.decode_jpeg_batch([torch.zeros(1, 1, 64, dtype=torch.int16)], torch.ones(1, 1, 64, dtype=torch.int16), 8, 8)

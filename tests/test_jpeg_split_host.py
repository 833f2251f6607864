"""CPU: the self-synchronising entropy decoder of csrc/jpeg_entropy.hip through its host twin, nerfhip_jpeg_entropy_decode_split,
which runs the device decoder's four steps (prepare, synchronise, offsets, emit) with the same per-symbol code over the same
subsequences on the CPU.  Reference: the sequential host decoder nerfhip_jpeg_entropy_decode, coefficient for coefficient, on the
files of tests/golden/jpeg_mini and on the streams of tests/tools/jpeg_synth.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEGS = os.path.join(ROOT, "tests", "golden", "jpeg_mini")
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
E_BADARG, E_ALIGN, E_DATA = -1, -3, -4
SUBSEQ_BITS = (32, 64, 256, 1024)


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


def _fixtures():
    from nerf_pl_amd.imageio_min import jpeg_parse
    out = []
    for f in sorted(os.listdir(JPEGS)):
        if f.endswith(".jpg") and "progressive" not in f:
            p = jpeg_parse(os.path.join(JPEGS, f))
            p["name"] = f
            out.append(p)
    return out


@pytest.fixture(scope="module")
def standard():
    from nerf_pl_amd.imageio_min import jpeg_parse
    return jpeg_parse(os.path.join(JPEGS, "q90_420_61x45.jpg"))["huffman"]


def _equal(got, want, i=0):
    return len(got) == len(want) and all(np.array_equal(g[i], w) for g, w in zip(got, want))


def test_synthetic_streams_decode_to_their_input_with_the_sequential_decoder(lib, standard):
    """the test-side encoder first: the existing decoder must give it its own input back"""
    import jpeg_synth
    from nerf_pl_amd import ops
    cases = jpeg_synth.edge_cases(standard)
    assert len(cases) >= 8
    for name, parsed, coef in cases:
        got = ops.jpeg_entropy_decode(parsed)
        assert _equal([g[None] for g in got], coef), name
    by_name = {n: p for n, p, _ in cases}
    assert b"\xff\x00\xff\x00\xff\x00" in by_name["ff_runs"]["scan"]
    rst = [b for a, b in zip(by_name["restart1_wraps"]["scan"], by_name["restart1_wraps"]["scan"][1:]) if a == 0xff and 0xd0 <= b <= 0xd7]
    assert rst == [0xd0 + (i & 7) for i in range(11)]
    assert jpeg_synth.codes(*jpeg_synth.DEEP_AC)[0x0a] == "1" * 15 + "0"


def test_split_equals_sequential_on_every_fixture(lib):
    from nerf_pl_amd import ops
    files = _fixtures()
    assert len(files) >= 12
    for parsed in files:
        want = ops.jpeg_entropy_decode(parsed)
        for bits in SUBSEQ_BITS:
            got = ops.jpeg_entropy_decode_split([parsed], bits)
            assert _equal(got, want), (parsed["name"], bits)


def test_split_equals_sequential_on_synthetic_streams(lib, standard):
    import jpeg_synth
    from nerf_pl_amd import ops
    for name, parsed, coef in jpeg_synth.edge_cases(standard):
        for bits in SUBSEQ_BITS + (4096,):
            got = ops.jpeg_entropy_decode_split([parsed], bits)
            assert _equal(got, coef), (name, bits)


def test_long_chains_cross_workgroups(lib, standard):
    """at 32 bits per subsequence the dense stream fills several workgroups of 256 subsequences and needs rounds between them"""
    import jpeg_synth
    from nerf_pl_amd import ops
    name, parsed, coef = [c for c in jpeg_synth.edge_cases(standard) if c[0] == "dense"][0]
    assert len(parsed["scan"]) * 8 // 32 > 3 * 256
    got, status, rounds = ops.jpeg_entropy_decode_split([parsed], 32, return_status=True)
    assert status.tolist() == [0] and rounds >= 1 and _equal(got, coef)
    assert lib.nerfhip_jpeg_entropy_workgroups(len(parsed["scan"]), 1, 32) > 3


def test_batches_keep_their_images_apart(lib):
    from nerf_pl_amd import ops
    by_name = {p["name"]: p for p in _fixtures()}
    for group in (["q90_420_61x45.jpg", "q75_420_61x45_optimized.jpg", "q85_420_61x45_restart3.jpg"],
                  ["q30_420_64x48.jpg", "q50_420_64x48_restart1.jpg"]):
        for bits in (32, 1024):
            got = ops.jpeg_entropy_decode_split([by_name[n] for n in group], bits)
            for i, n in enumerate(group):
                assert _equal(got, ops.jpeg_entropy_decode(by_name[n]), i), (n, bits)


def test_damaged_streams_are_refused_and_spare_their_neighbours(lib, standard):
    import jpeg_synth
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    cases = jpeg_synth.damaged_cases(standard)
    assert {n for n, _ in cases} >= {"truncated_half", "wrong_restart_number", "missing_restart", "no_prefix_code", "invalid_code"}
    for name, parsed in cases:
        with pytest.raises(NerfHipError, match="damaged"):
            ops.jpeg_entropy_decode(parsed)                                       # the reference refuses it
        for bits in SUBSEQ_BITS:
            got, status, _ = ops.jpeg_entropy_decode_split([parsed], bits, return_status=True)
            assert status.tolist() == [E_DATA], (name, bits)
            with pytest.raises(NerfHipError, match=name):
                ops.jpeg_entropy_decode_split([parsed], bits)
    # the damaged files of the sequential decoder's own test: truncated fixtures with the end marker put back
    from nerf_pl_amd.imageio_min import jpeg_parse
    for f in ("q90_420_61x45", "q85_420_61x45_restart3", "q90_grey_37x29"):
        data = open(os.path.join(JPEGS, f + ".jpg"), "rb").read()
        for cut in (len(data) // 3, 2 * len(data) // 3):
            if cut > data.index(b"\xff\xda") + 14:
                body = data[:cut - 1] if data[cut - 1] == 0xff else data[:cut]
                parsed = jpeg_parse(body + b"\xff\xd9")
                for bits in (32, 1024):
                    assert ops.jpeg_entropy_decode_split([parsed], bits, return_status=True)[1].tolist() == [E_DATA], (f, cut, bits)
    # in a batch of three the other two decode
    good = [c for c in jpeg_synth.edge_cases(standard) if c[0] == "dense"][0]
    bad = dict(good[1], name="cut", scan=good[1]["scan"][:200])
    got, status, _ = ops.jpeg_entropy_decode_split([good[1], bad, good[1]], 32, return_status=True)
    assert status.tolist() == [0, E_DATA, 0] and _equal(got, good[2], 0) and _equal(got, good[2], 2)
    # random bytes as a scan: an error or garbage, never a crash
    rng = np.random.default_rng(0)
    for i in range(20):
        noise = rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes()
        status = ops.jpeg_entropy_decode_split([dict(good[1], scan=noise)], 32 << (i % 4), return_status=True)[1]
        assert status[0] in (0, E_DATA)


def test_split_answers_like_the_sequential_decoder_on_noise(lib, standard):
    """random scans (markers and stuffing included): both decoders accept or refuse together, with equal coefficients"""
    import jpeg_synth
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    good = [c for c in jpeg_synth.edge_cases(standard) if c[0] == "restart5"][0][1]
    rng = np.random.default_rng(3)
    seen = set()
    for i in range(60):
        scan = bytearray(good["scan"])
        for _ in range(int(rng.integers(1, 4))):
            scan[int(rng.integers(0, len(scan)))] = int(rng.choice([0xff, 0x00, 0xd0, 0xd3, 0xd9, int(rng.integers(0, 256))]))
        parsed = dict(good, scan=bytes(scan))
        try:
            want = ops.jpeg_entropy_decode(parsed)
        except NerfHipError:
            want = None
        got, status, _ = ops.jpeg_entropy_decode_split([parsed], 64, return_status=True)
        assert (status[0] == 0) == (want is not None), i
        if want is not None:
            assert _equal(got, want), i
        seen.add(want is not None)
    assert seen == {True, False}


def test_entry_point_validates_arguments(lib, standard):
    import jpeg_synth
    from nerf_pl_amd import _lib, ops
    parsed = [c for c in jpeg_synth.edge_cases(standard) if c[0] == "restart5"][0][1]
    arrays = ops._jpeg_batch_arrays("test", [parsed], 64)
    nbytes = lib.nerfhip_jpeg_entropy_workspace_bytes(1, arrays[7], arrays[8], 64)
    assert nbytes > 0 and nbytes % 256 == 0
    raw = np.zeros(nbytes + 256, np.uint8)
    ws = raw[(-raw.ctypes.data) % 256:][:nbytes]
    status, progress = np.zeros(1, np.int32), np.zeros(1, np.int32)
    coef = [np.zeros((1, 5, 7, 64), np.int16) for _ in range(3)]
    f = lib.nerfhip_jpeg_entropy_decode_split

    def call(coefs=(0, 1, 2), **fields):
        for a in coef:
            a[:] = 0
        b = ops._jpeg_batch_struct(lambda a: a.ctypes.data, arrays, fields.pop("subseq_bits", 64), ws, status, progress)
        for k, v in fields.items():
            setattr(b, k, v)
        return f(ctypes.addressof(b), *[coef[c].ctypes.data if c in coefs else None for c in range(3)])
    assert call() == 0 and status[0] == 0 and _equal(coef, ops.jpeg_entropy_decode(parsed))
    assert f(None, coef[0].ctypes.data, coef[1].ctypes.data, coef[2].ctypes.data) == E_BADARG
    for field in ("scans", "offsets", "huffman", "huffman_masks", "restart_intervals", "workspace", "status", "progress"):
        assert call(**{field: None}) == E_BADARG, field
    assert call(coefs=(1, 2)) == E_BADARG and call(coefs=(0, 1)) == E_BADARG
    for bits in (0, 16, 48, 31, 4128, 8192, -32):
        assert call(subseq_bits=bits) == E_BADARG, bits
        assert lib.nerfhip_jpeg_entropy_workspace_bytes(1, arrays[7], arrays[8], bits) == 0
    assert call(n_images=0) == E_BADARG and call(n_comp=2) == E_BADARG and call(mcus_x=0) == E_BADARG and call(mcus_y=-1) == E_BADARG
    assert call(max_scan_bytes=0) == E_BADARG and call(max_intervals=0) == E_BADARG and call(total_bytes=0) == E_BADARG
    assert call(max_scan_bytes=(1 << 28) + 1) == E_BADARG
    assert call(workspace=ws.ctypes.data + 8) == E_ALIGN and call(offsets=arrays[1].ctypes.data + 4) == E_ALIGN
    # sizes the image exceeds are the image's error, found before any of its bytes is read
    assert call(max_intervals=arrays[8] - 1) == 0 and status[0] == E_BADARG
    assert call(max_scan_bytes=arrays[7] - 1) == 0 and status[0] == E_BADARG
    assert call(total_bytes=arrays[7] - 1) == 0 and status[0] == E_BADARG
    assert call() == 0 and status[0] == 0
    # the device entry points refuse the same before anything is launched (no GPU is touched)
    b = ops._jpeg_batch_struct(lambda a: a.ctypes.data, arrays, 48, ws, status, progress)
    assert lib.nerfhip_jpeg_entropy_sync(ctypes.addressof(b), 4, None) == E_BADARG
    assert lib.nerfhip_jpeg_entropy_rounds(ctypes.addressof(b), 1, 4, None) == E_BADARG
    assert lib.nerfhip_jpeg_entropy_emit(ctypes.addressof(b), None, None, None, None) == E_BADARG
    b.subseq_bits = 64
    assert lib.nerfhip_jpeg_entropy_sync(ctypes.addressof(b), 65, None) == E_BADARG
    assert lib.nerfhip_jpeg_entropy_rounds(ctypes.addressof(b), 0, 1, None) == E_BADARG
    assert lib.nerfhip_jpeg_entropy_emit(ctypes.addressof(b), None, None, None, None) == E_BADARG
    assert lib.nerfhip_jpeg_entropy_workgroups(arrays[7], arrays[8], 48) == 0


def test_python_wrappers_refuse_what_they_cannot_batch(lib, standard):
    import jpeg_synth
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    cases = {n: p for n, p, _ in jpeg_synth.edge_cases(standard)}
    with pytest.raises(NerfHipError, match="k63_no_eob.*restart5|restart5.*k63_no_eob"):
        ops.jpeg_entropy_decode_split([cases["k63_no_eob"], cases["restart5"]], 64)
    with pytest.raises(NerfHipError, match="subseq_bits"):
        ops.jpeg_entropy_decode_split([cases["dense"]], 48)
    with pytest.raises(NerfHipError, match="no CPU fallback"):
        ops.jpeg_entropy_decode_batch([cases["dense"]], "cpu")

"""CPU: the device inflate's host twin (nerfhip_inflate_host: the kernel's per-symbol code, table builder and copy steps with the
lanes in lockstep) against the machine's zlib over the whole corpus of tests/inflate_streams.py, and the PNG container split
(imageio_min.png_idat).  The rule: status == 0 <=> zlib.decompress succeeds with exactly out_bytes bytes, and then the bytes are
equal."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_streams  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E_BADARG, E_ALIGN, E_DATA = -1, -3, -4


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def corpus():
    return inflate_streams.corpus()


def _png_files():
    out = []
    for base, _, files in os.walk(GOLDEN):
        out += [os.path.join(base, f) for f in sorted(files) if f.endswith(".png")]
    return sorted(out)


def check_batch(batch, out, status):
    for k, c in enumerate(batch):
        if c.expect is None:
            assert status[k] == E_DATA, (c.name, int(status[k]))
        else:
            assert status[k] == 0, (c.name, int(status[k]))
            assert out[k].tobytes() == c.expect, c.name


def test_corpus_covers_what_it_promises(corpus):
    groups = {g: [c for c in corpus if c.group == g] for g in ("zlib", "hand", "refused", "truncated", "mutated")}
    assert len(groups["zlib"]) >= 140 and len(groups["hand"]) >= 12 and len(groups["refused"]) >= 30
    assert len(groups["truncated"]) == 6 * 16 and len(groups["mutated"]) == 6 * 400
    sizes = {c.out_bytes for c in groups["zlib"]}
    assert {0, 1, 257, 32767, 32768, 32769, 65535, 200000} <= sizes
    # what the issue left open, as zlib 1.2.11 answers it: recorded here so that a zlib that answers differently shows
    by_name = {c.name: c for c in corpus}
    assert by_name["dynamic: the unassigned code of a one-code distance set"].expect is None
    assert by_name["dynamic: incomplete code-length code"].expect is None
    assert by_name["dynamic: only an end-of-block code of one bit"].expect == b""


def test_whole_corpus_in_mixed_batches(lib, corpus):
    from nerf_pl_amd import ops
    seen = 0
    for batch in inflate_streams.batches(corpus):
        out, status = ops.inflate_host([c.stream for c in batch], batch[0].out_bytes, return_status=True)
        check_batch(batch, out, status)
        seen += len(batch)
    assert seen == len(corpus)
    mixed = [b for b in inflate_streams.batches(corpus) if {c.expect is None for c in b} == {True, False}]
    assert len(mixed) >= 10                                    # good and damaged streams did share batches


def test_every_stream_alone_matches_its_verdict_in_a_batch(lib, corpus):
    from nerf_pl_amd import ops
    for c in [c for c in corpus if c.group in ("hand", "refused")]:
        out, status = ops.inflate_host([c.stream], c.out_bytes, return_status=True)
        check_batch([c], out, status)


def test_wrong_output_size_is_data(lib, corpus):
    from nerf_pl_amd import ops
    for c in [c for c in corpus if c.group in ("zlib", "hand")][::7]:
        for n in (c.out_bytes + 1, c.out_bytes - 1, 0):
            if n < 0 or n == c.out_bytes:
                continue
            _, status = ops.inflate_host([c.stream], n, return_status=True)
            assert status[0] == E_DATA, (c.name, n)


def _call(lib, data, offsets, total, n, out, out_bytes, stride, status):
    return lib.nerfhip_inflate_host(data.ctypes.data, offsets.ctypes.data, total, n, out.ctypes.data, out_bytes, stride, status.ctypes.data)


@pytest.mark.parametrize("shift", [0, 1, 5, 15])
def test_guards_and_stride_gap_untouched(lib, corpus, shift):
    """Nothing outside [i * stride, i * stride + out_bytes) is written: good streams, damaged ones and ones that hold more bytes
    than out_bytes, at output addresses of every alignment class."""
    n_out = inflate_streams.N
    picks = [c for c in corpus if c.out_bytes == n_out and c.group == "zlib"][:6] + [c for c in corpus if c.group == "mutated"][:40:4] \
        + [c for c in corpus if c.group == "truncated"][:16:3]
    longer = zlib.compress(inflate_streams.random_bytes(n_out + 700, 5), 6)      # produces more than out_bytes
    streams = [c.stream for c in picks] + [longer]
    data = np.frombuffer(b"".join(streams), np.uint8)
    offsets = np.zeros(len(streams) + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in streams])
    stride, guard = n_out + 37, 4096
    buf = np.full(guard + shift + len(streams) * stride + guard, 0xa5, np.uint8)
    base = (-buf.ctypes.data) % 16 + shift
    out = buf[base + guard - 16:]
    status = np.full(len(streams), 77, np.int32)
    assert _call(lib, data, offsets, data.size, len(streams), out, n_out, stride, status) == 0
    region = out[:len(streams) * stride].reshape(len(streams), stride)
    for k, c in enumerate(picks):
        assert status[k] == (0 if c.expect is not None else E_DATA), c.name
        if c.expect is not None:
            assert region[k, :n_out].tobytes() == c.expect, c.name
    assert status[-1] == E_DATA
    assert (region[:, n_out:] == 0xa5).all()                   # the gap between the rows
    assert (buf[:base + guard - 16] == 0xa5).all() and (out[len(streams) * stride:] == 0xa5).all()


def test_bad_offsets_are_per_stream(lib, corpus):
    good = next(c for c in corpus if c.name == "distance 3 length 258")
    data = np.frombuffer(good.stream * 3, np.uint8)
    L = len(good.stream)
    offsets = np.array([0, L, L - 1, 3 * L + 1, 3 * L + 1], np.int64)       # stream 1 runs backwards, stream 2 leaves the data
    out = np.zeros((4, good.out_bytes), np.uint8)
    status = np.zeros(4, np.int32)
    assert _call(lib, data, offsets, data.size, 4, out, good.out_bytes, good.out_bytes, status) == 0
    assert status.tolist() == [0, E_BADARG, E_BADARG, E_BADARG]
    assert out[0].tobytes() == good.expect and not out[1:].any()


def test_argument_checks_without_a_gpu(lib):
    data, out = np.zeros(16, np.uint8), np.zeros(64, np.uint8)
    offsets, status = np.zeros(4, np.int64), np.zeros(4, np.int32)
    args = dict(data=data.ctypes.data, offsets=offsets.ctypes.data, total=16, n=1, out=out.ctypes.data, out_bytes=8, stride=8,
                status=status.ctypes.data)

    def both(**kw):
        a = dict(args, **kw)
        host = lib.nerfhip_inflate_host(a["data"], a["offsets"], a["total"], a["n"], a["out"], a["out_bytes"], a["stride"], a["status"])
        device = lib.nerfhip_inflate(a["data"], a["offsets"], a["total"], a["n"], a["out"], a["out_bytes"], a["stride"], a["status"], None)
        assert host == device                                  # the device entry validates before it launches anything
        return host
    assert both(n=0) == 0
    assert both(n=0, data=None, offsets=None, out=None, status=None) == 0
    for bad in (dict(n=-1), dict(n=65536), dict(data=None), dict(offsets=None), dict(out=None), dict(status=None), dict(total=-1),
                dict(out_bytes=-1), dict(stride=7)):
        assert both(**bad) == E_BADARG, bad
    assert both(offsets=offsets.ctypes.data + 4) == E_ALIGN
    assert both(status=status.ctypes.data + 2) == E_ALIGN
    assert lib.nerfhip_abi_version() == 3


def test_ops_raises_naming_every_damaged_stream(lib, corpus):
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    good = next(c for c in corpus if c.name == "distance 1 length 258")
    bad = good.stream[:-1]
    with pytest.raises(NerfHipError) as e:
        ops.inflate_host([good.stream, bad, good.stream, bad], good.out_bytes)
    assert "stream 1 of the batch" in str(e.value) and "stream 3 of the batch" in str(e.value) and "stream 0" not in str(e.value)
    with pytest.raises(NerfHipError) as e:
        ops.inflate_host([bad, good.stream], good.out_bytes, names=["a.png", "b.png"])
    assert "a.png" in str(e.value) and "b.png" not in str(e.value)
    assert ops.inflate_host([], 5).shape == (0, 5)


def _split_idat(data, parts=3):
    """The same PNG with its IDAT data in `parts` chunks."""
    pos, out, idat = 8, [data[:8]], b""
    chunks = []
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        chunks.append((tag, data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    for tag, body in chunks:
        if tag == b"IDAT":
            idat += body
    done = False
    for tag, body in chunks:
        if tag == b"IDAT":
            if not done:
                cuts = [len(idat) * k // parts for k in range(parts + 1)]
                for a, b in zip(cuts, cuts[1:]):
                    out.append(struct.pack(">I", b - a) + b"IDAT" + idat[a:b] + struct.pack(">I", zlib.crc32(b"IDAT" + idat[a:b]) & 0xffffffff))
                done = True
            continue
        out.append(struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff))
    return b"".join(out), idat


def test_png_idat_joins_chunks_and_png_inflate_is_unchanged(lib):
    from nerf_pl_amd import ops
    from nerf_pl_amd.imageio_min import png_idat, png_inflate
    files = _png_files()
    assert len(files) >= 5
    for path in files:
        data = open(path, "rb").read()
        w, h, ch, stream = png_idat(path)
        assert png_idat(data) == (w, h, ch, stream)
        raw = zlib.decompress(stream)
        assert png_inflate(path) == (w, h, ch, raw) and len(raw) == h * (1 + w * ch)
        split, joined = _split_idat(data)
        assert split.count(b"IDAT") >= 3 and joined == stream
        assert png_idat(split) == (w, h, ch, stream)
        assert png_inflate(split) == (w, h, ch, raw)
        assert ops.inflate_host([stream], len(raw))[0].tobytes() == raw
    with pytest.raises(ValueError, match="not a PNG file"):
        png_idat(b"\xff\xd8 not a png")


@pytest.mark.parametrize("cls,kw", [("BlenderDataset", {}), ("LLFFDataset", {})])
def test_loader_option_is_validated_before_anything_else(cls, kw):
    from nerf_pl_amd import datasets
    with pytest.raises(ValueError, match='png_inflate must be "host" or "gpu"'):
        getattr(datasets, cls)("/nonexistent", png_inflate="device", **kw)

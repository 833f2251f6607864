"""The zlib streams the inflate tests share (tests/test_inflate_host.py, tests/test_gpu_inflate.py, tools/inflate_sanitize.py).

Every case is (name, stream, out_bytes, expect, group): `expect` is what the machine's zlib says — zlib.decompress(stream) where it
succeeds with exactly out_bytes bytes, else None — and is recorded here, once.  The rule every decoder is held to:
status == 0 <=> expect is not None, and then the bytes are equal.

Groups: "zlib" (streams zlib wrote: levels, strategies, window sizes, flushes, seam sizes), "hand" (streams from the bit writer
below that zlib accepts), "refused" (hand-made streams zlib refuses), "truncated" and "mutated" (six zlib streams cut short and
with single bytes changed).  The hand-made lists also say what verdict their author intended; building the corpus asserts that
zlib agrees, so a mistake in the bit writer shows here and not as a decoder failure."""
import collections
import functools
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Case = collections.namedtuple("Case", "name stream out_bytes expect group")

FRAME = 96                                  # the procedural frame: 96 x 96 RGBA
N = FRAME * (1 + 4 * FRAME)                 # its filtered scanlines: the size most cases share, so that they batch together


def verdict(stream, out_bytes):
    try:
        raw = zlib.decompress(bytes(stream))
    except zlib.error:
        return None
    return raw if len(raw) == out_bytes else None


# ---- data --------------------------------------------------------------------------------------------------------------------------
def random_bytes(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def fixture_scanlines(n=N):
    """The filtered scanlines of the blender_mini training frames, one after the other, repeated or cut to n bytes."""
    from nerf_pl_amd.imageio_min import png_inflate
    scene = os.path.join(ROOT, "tests", "golden", "blender_mini", "train")
    raw = b"".join(png_inflate(os.path.join(scene, f))[3] for f in sorted(os.listdir(scene)) if f.endswith(".png"))
    return (raw * (n // len(raw) + 1))[:n]


def procedural_scanlines(size=FRAME, seed=2):
    """A Blender-like RGBA frame (transparent background, a shaded disc, a little noise), Sub-filtered: size * (1 + 4 * size) bytes."""
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    r = np.hypot(x - size / 2, y - size / 2) / (size / 2)
    inside = r < 0.8
    rng = np.random.default_rng(seed)
    img = np.zeros((size, size, 4), np.uint8)
    shade = np.clip(255 * (1 - r), 0, 255)
    img[..., 0] = np.where(inside, shade, 0)
    img[..., 1] = np.where(inside, np.clip(shade * 0.6 + 3 * rng.standard_normal((size, size)), 0, 255), 0)
    img[..., 2] = np.where(inside, (x * 2) % 256, 0)
    img[..., 3] = np.where(inside, 255, 0)
    rows = img.reshape(size, 4 * size).astype(np.int32)
    sub = rows.copy()
    sub[:, 4:] -= rows[:, :-4]
    out = np.empty((size, 1 + 4 * size), np.uint8)
    out[:, 0] = 1
    out[:, 1:] = (sub & 255).astype(np.uint8)
    return out.tobytes()


def repetitive(n, seed=3):
    """Compressible data with matches at every distance up to the window: random picks among a few long phrases."""
    rng = np.random.default_rng(seed)
    phrases = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in (3, 17, 300, 5000, 40000)]
    out = bytearray()
    while len(out) < n:
        p = phrases[int(rng.integers(0, len(phrases)))]
        a = int(rng.integers(0, len(p)))
        out += p[a:a + int(rng.integers(1, 600))]
    return bytes(out[:n])


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flushes=()):
    """zlib's stream for `data`; flushes: (fraction of the data, flush mode) in ascending order."""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    out, at = [], 0
    for frac, mode in flushes:
        upto = int(len(data) * frac)
        out.append(co.compress(data[at:upto]))
        out.append(co.flush(mode))
        at = upto
    out.append(co.compress(data[at:]))
    out.append(co.flush())
    return b"".join(out)


def zlib_cases():
    out = []
    kinds = (("random", random_bytes(N)), ("fixture", fixture_scanlines()), ("frame", procedural_scanlines()))
    strategies = (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman", zlib.Z_HUFFMAN_ONLY),
                  ("filtered", zlib.Z_FILTERED))
    for kind, data in kinds:
        for level in (0, 1, 6, 9):
            for sname, strategy in strategies:
                for wbits in (9, 15):
                    out.append(("%s level %d %s wbits %d" % (kind, level, sname, wbits), deflate(data, level, strategy, wbits), len(data)))
        flushes = ((0.0, zlib.Z_SYNC_FLUSH), (0.3, zlib.Z_SYNC_FLUSH), (0.3, zlib.Z_FULL_FLUSH), (0.7, zlib.Z_FULL_FLUSH), (1.0, zlib.Z_SYNC_FLUSH))
        out.append(("%s with flushes" % kind, deflate(data, 6, flushes=flushes), len(data)))
        out.append(("%s level 0 with flushes" % kind, deflate(data, 0, flushes=flushes), len(data)))
    for n in (0, 1, 257, 32767, 32768, 32769):
        for level in (0, 6):
            out.append(("repetitive %d bytes level %d" % (n, level), deflate(repetitive(n), level), n))
        out.append(("random %d bytes fixed" % n, deflate(random_bytes(n, 7), 6, zlib.Z_FIXED), n))
    big = repetitive(200000)
    out.append(("repetitive 200000 bytes level 6", deflate(big, 6), len(big)))
    out.append(("repetitive 200000 bytes level 1 wbits 9", deflate(big, 1, wbits=9), len(big)))
    out.append(("one stored block of 65535 bytes", deflate(random_bytes(65535, 8), 0), 65535))
    return out


# ---- the bit writer ------------------------------------------------------------------------------------------------------------------
class Bits:
    """Deflate's bit order: values from the low end of each byte, Huffman codes from their first bit."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, bits):
        self.put(int(format(code, "0%db" % bits)[::-1], 2) if bits else 0, bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        self.align()
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
CL_DEFAULT = [4] * 13 + [5] * 6             # a complete code over all 19 code-length symbols


def canon(lens):
    """Canonical codes of the lengths (RFC 1951 3.2.2); an over-subscribed set simply runs out of its bits."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] & ((1 << l) - 1) if l else 0)
        if l:
            nxt[l] += 1
    return out


class Block:
    """One Huffman block: header, then symbols by the block's codes."""

    def __init__(self, bw, final, ll=None, dl=None, **header):
        self.bw = bw
        self.ll = FIXED_LL if ll is None else ll
        self.dl = FIXED_D if dl is None else dl
        bw.put(1 if final else 0, 1)
        if ll is None:
            bw.put(1, 2)
        else:
            self.dynamic_header(**header)
        self.llc, self.dc = canon(self.ll), canon(self.dl)

    def dynamic_header(self, cl_seq=None, hlit_field=None, hdist_field=None, cl_lens=None):
        bw = self.bw
        bw.put(2, 2)
        bw.put(len(self.ll) - 257 if hlit_field is None else hlit_field, 5)
        bw.put(len(self.dl) - 1 if hdist_field is None else hdist_field, 5)
        cl = CL_DEFAULT if cl_lens is None else cl_lens
        bw.put(19 - 4, 4)
        for s in CL_ORDER:
            bw.put(cl[s], 3)
        codes = canon(cl)
        for item in ([(l,) for l in list(self.ll) + list(self.dl)] if cl_seq is None else cl_seq):
            bw.code(codes[item[0]], cl[item[0]])
            if item[0] >= 16:
                bw.put(item[1], {16: 2, 17: 3, 18: 7}[item[0]])

    def sym(self, s):
        self.bw.code(self.llc[s], self.ll[s])

    def lits(self, data):
        for v in data:
            self.sym(v)

    def dist_sym(self, ds, extra=0, code=None):
        self.bw.code(self.dc[ds] if code is None else code, self.dl[ds])
        if ds < 30:
            self.bw.put(extra, DIST_EXTRA[ds])

    def match(self, length, dist, len_sym=None):
        k = max(i for i in range(29) if LEN_BASE[i] <= length) if len_sym is None else len_sym - 257
        self.sym(257 + k)
        self.bw.put(length - LEN_BASE[k], LEN_EXTRA[k])
        ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.dist_sym(ds, dist - DIST_BASE[ds])

    def end(self):
        self.sym(256)


def expand(tokens):
    """What the tokens stand for; a reference behind the first byte (refused streams only) reads zeros."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]] if t[1] <= len(out) else 0)
        else:
            out.append(t)
    return bytes(out)


def wrap(deflated, output, header=b"\x78\x9c", adler=None, tail=b""):
    a = zlib.adler32(output) if adler is None else adler
    return header + deflated + (a.to_bytes(4, "big") if a >= 0 else b"") + tail


def fixed_stream(tokens, final=True, prefix=None, **kw):
    """One fixed block of literals and (length, distance) matches, wrapped."""
    bw = Bits()
    if prefix:
        prefix(bw)
    b = Block(bw, final)
    for t in tokens:
        if isinstance(t, tuple):
            b.match(*t)
        else:
            b.sym(t)
    b.end()
    return wrap(bw.bytes(), expand([t[:2] if isinstance(t, tuple) else t for t in tokens]), **kw)


def dynamic_stream(ll, dl, body, output, **header):
    bw = Bits()
    b = Block(bw, True, ll, dl, **header)
    body(b)
    return wrap(bw.bytes(), output)


SMALL_LL = [0] * 97 + [1, 2] + [0] * 157 + [2]          # 'a' 1 bit, 'b' and end-of-block 2 bits: complete, HLIT = 257
MATCH_LL = [0] * 97 + [1, 2] + [0] * 157 + [3, 3]       # 'a', 'b', end-of-block, length 3


def hand_cases():
    """(name, stream, out_bytes, intended: True accepted / False refused / None not known in advance)"""
    lits = list(random_bytes(32768, 11))
    out = []

    def add(name, stream, n, intended):
        out.append((name, stream, n, intended))

    far = lits + [(258, 32768)]
    add("distance 32768 length 258 after 32768 literals", fixed_stream(far), 32768 + 258, True)
    add("distance 1 length 258", fixed_stream([65, (258, 1)]), 259, True)
    add("distance 3 length 258", fixed_stream([65, 66, 67, (258, 3)]), 261, True)
    add("length code 284 with extra 31", fixed_stream([65, (258, 1, 284)]), 259, True)

    def empty_stored(bw):
        bw.put(0, 3)
        bw.raw(b"\x00\x00\xff\xff")
    add("empty stored block, then a fixed block", fixed_stream([1, 2, 3, (5, 2)], prefix=empty_stored), 8, True)
    add("dynamic: one one-bit distance code", dynamic_stream(MATCH_LL, [1], lambda b: (b.lits(b"ab"), b.match(3, 1), b.end()), b"abbbb"), 5, True)
    add("dynamic: no distance code, literals only", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"abba"), b.end()), b"abba"), 4, True)
    add("dynamic: only an end-of-block code of one bit", dynamic_stream([0] * 256 + [1], [0], lambda b: b.end(), b""), 0, None)
    full_ll, full_d = [8] * 226 + [9] * 60, [4, 4] + [5] * 28

    def full_body(b):
        b.lits(bytes(range(256)))
        b.match(258, 256)
        b.match(10, 1)
        b.end()
    add("dynamic: HLIT 286 and HDIST 30", dynamic_stream(full_ll, full_d, full_body, expand(list(range(256)) + [(258, 256), (10, 1)])), 524, True)
    add("header 08 1d in front of a distance of 32768", fixed_stream(far, header=b"\x08\x1d"), 32768 + 258, True)
    add("bytes behind the Adler-32", fixed_stream([1, 2, 3], tail=b"trailing \x00\xff bytes"), 3, True)
    # SMALL_LL and one distance length of 0 as runs: 97 zeros, 1, 2, 157 zeros (138 + 10 + 9), 2, 0
    repeats = [(18, 86), (1,), (2,), (18, 127), (17, 7), (17, 6), (2,), (0,)]
    add("dynamic: lengths written with repeats 17 and 18", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"ab"), b.end()), b"ab", cl_seq=repeats), 2, True)
    ll16 = [0] * 97 + [3, 3, 3, 3, 2] + [0] * 154 + [2]      # 'a'..'d' 3 bits, 'e' and end-of-block 2 bits
    rep16 = [(18, 86), (3,), (16, 0), (2,), (18, 127), (18, 5), (2,), (0,)]
    add("dynamic: a repeat of the previous length", dynamic_stream(ll16, [0], lambda b: (b.lits(b"abcde"), b.end()), b"abcde", cl_seq=rep16), 5, True)

    # ---- refused
    add("distance 32768 after 32767 bytes", fixed_stream(lits[:32767] + [(258, 32768)]), 32767 + 258, False)
    add("a match before any output", fixed_stream([(3, 1)]), 3, False)
    for s in (286, 287):
        bw = Bits()
        b = Block(bw, True)
        b.lits(b"ab")
        b.sym(s)
        b.end()
        add("literal/length symbol %d" % s, wrap(bw.bytes(), b"ab"), 2, False)
    for ds in (30, 31):
        bw = Bits()
        b = Block(bw, True)
        b.lits(b"abcd")
        b.sym(257)
        b.dist_sym(ds)
        b.end()
        add("distance symbol %d" % ds, wrap(bw.bytes(), b"abcdabc"), 7, False)
    bw = Bits()
    bw.put(1 | 3 << 1, 3)
    add("block type 3", wrap(bw.bytes(), b""), 0, False)
    add("stored block: LEN and NLEN disagree", wrap(b"\x01\x03\x00\xfd\xff" + b"abc", b"abc"), 3, False)
    add("stored block: cut short", b"\x78\x9c\x01\x10\x00\xef\xff" + b"only ten b", 16, False)
    add("wrong Adler-32", fixed_stream([1, 2, 3], adler=zlib.adler32(b"\x01\x02\x03") ^ 0x10000), 3, False)
    add("no Adler-32", fixed_stream([1, 2, 3], adler=-1), 3, False)
    add("half an Adler-32", fixed_stream([1, 2, 3])[:-2], 3, False)
    add("no final block", fixed_stream([1, 2, 3], final=False), 3, False)
    for h in (b"\x88\x1c", b"\x79\x9c", b"\x78\x20", b"\x78\xbb"):
        add("header %s" % h.hex(), fixed_stream([1, 2, 3], header=h), 3, False)
    add("dynamic: no end-of-block code", dynamic_stream([0] * 97 + [1, 1] + [0] * 158, [0], lambda b: b.lits(b"ab"), b"ab"), 2, False)
    add("dynamic: over-subscribed literal/length set", dynamic_stream([0] * 97 + [1, 1] + [0] * 157 + [1], [0], lambda b: b.lits(b"a"), b"a"), 1, False)
    add("dynamic: incomplete literal/length set", dynamic_stream([0] * 97 + [2, 2] + [0] * 157 + [2], [0], lambda b: (b.lits(b"a"), b.end()), b"a"), 1, False)
    add("dynamic: incomplete distance set of two codes", dynamic_stream(MATCH_LL, [2, 2], lambda b: (b.lits(b"a"), b.end()), b"a"), 1, False)
    add("dynamic: over-subscribed distance set", dynamic_stream(MATCH_LL, [1, 1, 1], lambda b: (b.lits(b"a"), b.end()), b"a"), 1, False)
    add("dynamic: repeat 16 first", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"a"), b.end()), b"a", cl_seq=[(16, 0)] + [(l,) for l in SMALL_LL[3:]] + [(0,)]), 1, False)
    add("dynamic: a repeat past HLIT + HDIST", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"a"), b.end()), b"a", cl_seq=[(l,) for l in SMALL_LL] + [(17, 0)]), 1, False)
    add("dynamic: HLIT 288", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"a"), b.end()), b"a", hlit_field=31), 1, False)
    add("dynamic: HDIST 31", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"a"), b.end()), b"a", hdist_field=30), 1, False)
    add("dynamic: HDIST 32", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"a"), b.end()), b"a", hdist_field=31), 1, False)

    def unassigned(b):
        b.lits(b"ab")
        b.sym(257)
        b.dist_sym(0, code=1)
        b.end()
    add("dynamic: the unassigned code of a one-code distance set", dynamic_stream(MATCH_LL, [1], unassigned, b"abbbb"), 5, None)
    add("dynamic: a distance code where the block has none", dynamic_stream(MATCH_LL, [0], lambda b: (b.lits(b"ab"), b.sym(257), b.bw.put(0, 1), b.end()), b"abbbb"), 5, None)
    add("dynamic: incomplete code-length code", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"a"), b.end()), b"a", cl_lens=[4] * 13 + [5] * 5 + [0]), 1, None)
    add("dynamic: over-subscribed code-length code", dynamic_stream(SMALL_LL, [0], lambda b: (b.lits(b"a"), b.end()), b"a", cl_lens=[4] * 14 + [5] * 5), 1, None)
    add("an empty stream", b"", 0, False)
    add("a header and nothing else", b"\x78\x9c", 0, False)
    return out


def damaged_cases(valid):
    """Six of the valid zlib streams: every truncation at 16 evenly spaced lengths, 400 single-byte changes (fixed seed)."""
    picks = ["fixture level 6 default wbits 15", "fixture level 1 default wbits 9", "frame level 9 default wbits 15",
             "frame level 6 fixed wbits 15", "random level 0 default wbits 15", "frame with flushes"]
    by_name = {c[0]: c for c in valid}
    rng = np.random.default_rng(20)
    out = []
    for name in picks:
        _, stream, n = by_name[name]
        for k in range(16):
            cut = k * len(stream) // 16
            out.append(("%s cut at %d" % (name, cut), stream[:cut], n, "truncated"))
        for k in range(400):
            at, value = int(rng.integers(0, len(stream))), int(rng.integers(1, 256))
            changed = bytearray(stream)
            changed[at] ^= value
            out.append(("%s byte %d ^ %d" % (name, at, value), bytes(changed), n, "mutated"))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    cases = []
    valid = zlib_cases()
    for name, stream, n in valid:
        expect = verdict(stream, n)
        assert expect is not None, name
        cases.append(Case(name, stream, n, expect, "zlib"))
    for name, stream, n, intended in hand_cases():
        expect = verdict(stream, n)
        if intended is not None:
            assert (expect is not None) == intended, "zlib and the author of %r disagree" % name
        cases.append(Case(name, stream, n, expect, "hand" if expect is not None else "refused"))
    for name, stream, n, group in damaged_cases(valid):
        cases.append(Case(name, stream, n, verdict(stream, n), group))
    return tuple(cases)


def batches(cases, limit=64):
    """Lists of up to `limit` cases of one output size, good and damaged ones interleaved."""
    by_size = collections.OrderedDict()
    for c in cases:
        by_size.setdefault(c.out_bytes, []).append(c)
    for group in by_size.values():
        good = [c for c in group if c.expect is not None]
        bad = [c for c in group if c.expect is None]
        mixed = []
        while good or bad:
            if good:
                mixed.append(good.pop(0))
            mixed.extend(bad[:3])
            del bad[:3]
        for i in range(0, len(mixed), limit):
            yield mixed[i:i + limit]

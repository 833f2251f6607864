"""The PNG encoder of DESIGN.md §15 restated in numpy / plain Python.  The GPU path (csrc/png.hip + imageio_min.png_bytes_device)
must equal this byte for byte; that what this writes is a valid PNG is proved on the CPU (tests/test_png_host.py: Pillow,
zlib and imageio_min.png_inflate read it back).

  filter    per scanline all five PNG filters from the raw neighbours (bpp = channels, zeros above row 0); the smallest
            sum of (v < 128 ? v : 256 - v) wins, a tie goes to the lowest type
  strips    the filtered stream S is cut into strips of STRIP bytes; each is one dynamic-Huffman deflate block (BFINAL on
            the last), concatenated bit by bit
  tokens    maximal runs of equal bytes inside a strip; a run of L is a literal, (L-1) // 258 matches (258, distance 1) and for
            t = (L-1) % 258 a match (t, distance 1) if t >= 3 else t literals; then end-of-block
  lengths   `code_lengths` below, limit 15 for literals / lengths, 7 for the code-length alphabet; the one distance code has
            length 1 if the strip has a match, else 0
  header    HLIT = last used symbol - 256 (at least 0), HDIST = 0, HCLEN = last used entry of the permuted order (at least 4);
            the code-length sequence in the closed form of `cl_tokens`
  container signature, IHDR, one IDAT (78 01, the deflate bytes, Adler-32 of S), IEND
"""
import struct
import zlib

import numpy as np

STRIP = 8192          # K (NERFHIP_PNG_STRIP, ops.PNG_STRIP)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)      # RFC 1951 3.2.5


# ---------------------------------------------------------------------------------------------------------------- filter
def filter_stream(img):
    """(H, W), (H, W, 1|3|4) uint8 -> the filtered stream S as an (H, 1 + W*C) uint8 array."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    x = img.reshape(h, w * c).astype(np.int64)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, c:] = x[:-1, :-c]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255          # (5, H, W*C)
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                         # (5, H)
    best = np.argmin(cost, axis=0)                                                    # the first minimum: the lowest type
    out = np.empty((h, 1 + w * c), np.uint8)
    out[:, 0] = best
    out[:, 1:] = cand[best, np.arange(h)]
    return out


# ------------------------------------------------------------------------------------------------------------ code lengths
def code_lengths(counts, limit):
    """Length-limited Huffman lengths (a list as long as `counts`).
    Used symbols in ascending (count, symbol) order.  Plain Huffman by the two-queue merge: the two lightest of the leaf queue
    and the queue of merged nodes (in creation order); of equal weights the merged node goes first (a chain of Fibonacci counts
    then stays one chain whatever single counts stand beside it).  A leaf deeper than `limit` counts
    as `limit`.  While the Kraft sum exceeds 1 (by a whole number of 2^-limit): of the longest length below `limit` that is in
    use, one code becomes one longer and takes one code of length `limit` beside it.  The lengths go back to the symbols longest
    first in the ascending order.  One used symbol gets length 1."""
    counts = [int(c) for c in counts]
    order = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    lengths = [0] * len(counts)
    m = len(order)
    if m == 0:
        return lengths
    if m == 1:
        lengths[order[0][1]] = 1
        return lengths
    weight = [c for c, _ in order]
    parent = [0] * (2 * m - 1)
    leaf, node = 0, m
    while len(weight) < 2 * m - 1:
        nxt = len(weight)
        total = 0
        for _ in range(2):
            if leaf < m and (node >= nxt or weight[leaf] < weight[node]):
                x, leaf = leaf, leaf + 1
            else:
                x, node = node, node + 1
            total += weight[x]
            parent[x] = nxt
        weight.append(total)
    depth = [0] * (2 * m - 1)
    for k in range(2 * m - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    bl = [0] * (limit + 1)
    for k in range(m):
        bl[min(depth[k], limit)] += 1
    excess = sum(bl[b] << (limit - b) for b in range(1, limit + 1)) - (1 << limit)
    for _ in range(max(excess, 0)):
        bits = limit - 1
        while bl[bits] == 0:
            bits -= 1
        bl[bits] -= 1
        bl[bits + 1] += 2
        bl[limit] -= 1
    k = 0
    for bits in range(limit, 0, -1):
        for _ in range(bl[bits]):
            lengths[order[k][1]] = bits
            k += 1
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> codes with their bits reversed, ready for an LSB-first stream."""
    bl = [0] * 16
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            out[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return out


# ------------------------------------------------------------------------------------------------------------------ tokens
def runs_of(seq):
    """[(value, length)] of the maximal runs of equal values."""
    seq = np.asarray(seq)
    if seq.size == 0:
        return []
    starts = np.flatnonzero(np.concatenate([[True], seq[1:] != seq[:-1]]))
    return list(zip(seq[starts].tolist(), np.diff(np.concatenate([starts, [seq.size]])).tolist()))


def length_symbol(length):
    """match length 3..258 -> (symbol, extra bits, extra value)"""
    k = max(i for i, base in enumerate(LEN_BASE) if base <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def strip_tokens(strip):
    """-> [(symbol, extra bits, extra value)]: literals 0..255, matches 257..285 (all of distance 1), without end-of-block."""
    out = []
    for v, L in runs_of(strip):
        out.append((v, 0, 0))
        r = L - 1
        out += [length_symbol(258)] * (r // 258)
        t = r % 258
        out += [length_symbol(t)] if t >= 3 else [(v, 0, 0)] * t
    return out


def cl_tokens(seq):
    """The code-length sequence -> [(symbol 0..18, extra bits, extra value)]."""
    out = []
    for v, L in runs_of(seq):
        if v == 0:
            while L >= 138:
                out.append((18, 7, 127))
                L -= 138
            if L >= 11:
                out.append((18, 7, L - 11))
            elif L >= 3:
                out.append((17, 3, L - 3))
            else:
                out += [(0, 0, 0)] * L
        else:
            out.append((v, 0, 0))
            r = L - 1
            while r >= 6:
                out.append((16, 2, 3))
                r -= 6
            out += [(16, 2, r - 3)] if r >= 3 else [(v, 0, 0)] * r
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits

    def getvalue(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def deflate_strip(out, strip, final):
    """One dynamic-Huffman block for `strip` into the BitWriter."""
    tokens = strip_tokens(strip)
    hist = [0] * 286
    for sym, _, _ in tokens:
        hist[sym] += 1
    hist[256] = 1
    lit_len = code_lengths(hist, 15)
    n_lit = max(257, max(s for s in range(286) if lit_len[s]) + 1)
    has_match = any(lit_len[257:])
    seq = lit_len[:n_lit] + [1 if has_match else 0]
    cl = cl_tokens(seq)
    cl_hist = [0] * 19
    for sym, _, _ in cl:
        cl_hist[sym] += 1
    cl_len = code_lengths(cl_hist, 7)
    n_cl = max(4, max(i for i in range(19) if cl_len[CL_ORDER[i]]) + 1)
    lit_code, cl_code = canonical_codes(lit_len), canonical_codes(cl_len)
    out.put(1 if final else 0, 1)
    out.put(2, 2)
    out.put(n_lit - 257, 5)
    out.put(0, 5)
    out.put(n_cl - 4, 4)
    for i in range(n_cl):
        out.put(cl_len[CL_ORDER[i]], 3)
    for sym, eb, ev in cl:
        out.put(cl_code[sym], cl_len[sym])
        out.put(ev, eb)
    for sym, eb, ev in tokens:
        out.put(lit_code[sym], lit_len[sym])
        if sym > 256:
            out.put(ev, eb)
            out.put(0, 1)              # distance symbol 0 (distance 1), the one code of length 1
    out.put(lit_code[256], lit_len[256])


def deflate(stream, strip=STRIP):
    """bytes / uint8 array -> the raw deflate data of the strip-parallel encoder."""
    s = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else stream.reshape(-1)
    out = BitWriter()
    for first in range(0, s.size, strip):
        deflate_strip(out, s[first:first + strip], first + strip >= s.size)
    return out.getvalue()


def adler32(stream, strip=STRIP):
    """Adler-32 as the device forms it: per-strip sums of d and (n - j) d, combined modulo 65521."""
    s = np.asarray(stream, np.uint8).reshape(-1).astype(np.int64)
    n_all, a, b = s.size, 1, s.size % 65521
    for first in range(0, n_all, strip):
        d = s[first:first + strip]
        sa, sb = int(d.sum()), int(((d.size - np.arange(d.size)) * d).sum())
        a += sa
        b += sb + (n_all - first - d.size) * sa
    return (b % 65521) << 16 | (a % 65521)


# --------------------------------------------------------------------------------------------------------------- container
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def container(w, h, channels, deflate_bytes, adler):
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[channels], 0, 0, 0)
    idat = b"\x78\x01" + bytes(deflate_bytes) + struct.pack(">I", adler)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"")


def png_bytes(img, strip=STRIP):
    """(H, W) or (H, W, 1|3|4) uint8 -> the file contents."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    s = filter_stream(img)
    return container(w, h, c, deflate(s, strip), adler32(s, strip))


# ------------------------------------------------------------------------------------------------------------------- cases
RUN_EDGES = (2, 3, 4, 258, 259, 260, 261, 262, 517)      # run lengths of equal filtered bytes at the token rule's edges


def _noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def stripes(channels=1):
    """One row whose Sub-filtered form holds a run of exactly R zeros for every R in RUN_EDGES: runs of R + C equal bytes (they
    need not end with a pixel), their values alternating between 7 and 8, so that Sub leaves C bytes of 7, 1 or 255 and R zeros
    per run where None leaves 7 or 8 per byte; one more short run pads the row to whole pixels."""
    row = []
    for i, r in enumerate(RUN_EDGES):
        row += [7 + (i & 1)] * (r + channels)
    row += [15 - row[-1]] * (channels + -len(row) % channels)
    row = np.array(row, np.uint8)
    return row[None, :] if channels == 1 else row.reshape(1, -1, channels)


def image_cases(frames):
    """name -> image; `frames` is tests/golden/gif_mini/frames.npz as a dict.  C = 1, 3 and 4 throughout."""
    r96 = frames["render_96x96"]
    alpha = (255 * (r96.astype(np.int64).sum(axis=2) < 720)).astype(np.uint8)
    walk = (np.cumsum(np.random.RandomState(3).randint(-2, 3, (7, 1000, 3)) * (np.random.RandomState(4).rand(7, 1000, 3) < 0.2), axis=1)
            + 128).astype(np.uint8)
    cases = {
        "render_64x200": frames["render_64x200"], "render_96x96": r96, "gradient_48x64": frames["gradient_48x64"],
        "noise_67x117": frames["noise_67x117"],
        "render_96x96_grey": r96[:, :, 1].copy(), "render_96x96_rgba": np.dstack([r96, alpha]),
        "1x1_grey": _noise((1, 1), 1), "1x1_rgb": _noise((1, 1, 3), 2), "1x1_rgba": _noise((1, 1, 4), 3),
        "1x37_rgb": _noise((1, 37, 3), 4) >> 5, "41x1_rgba": _noise((41, 1, 4), 5) >> 6, "29x1_grey": _noise((29, 1), 6),
        "straddle_7x1000_rgb": walk,                                     # rows of 3001 bytes: strips end inside rows
        "stream_k_grey": _noise((1, STRIP - 1), 7) >> 6, "stream_kp1_grey": _noise((1, STRIP), 8) >> 6,
        "stream_kp1_rgba": _noise((1, STRIP // 4, 4), 9) >> 7, "stream_2kp1_grey": _noise((1, 2 * STRIP), 10) >> 6,
        "zeros_50x70_rgb": np.zeros((50, 70, 3), np.uint8), "zeros_20x30_rgba": np.zeros((20, 30, 4), np.uint8),
        "zeros_90x100_grey": np.zeros((90, 100), np.uint8),
        "full_50x70_rgb": np.full((50, 70, 3), 255, np.uint8), "full_20x30_grey": np.full((20, 30), 255, np.uint8),
        "full_33x21_rgba": np.full((33, 21, 4), 255, np.uint8),
        "stripes_grey": stripes(1), "stripes_rgb": stripes(3), "stripes_rgba": stripes(4),
        "noise_31x45_grey": _noise((31, 45), 11), "noise_19x23_rgba": _noise((19, 23, 4), 12),
    }
    return cases


def fibonacci_stream():
    """2,583 bytes: 16 byte values with the frequencies 1, 1, 2, 3, ..., 987 and no two equal bytes adjacent.  With the count of
    end-of-block the 17 symbols form one chain 16 deep: the 15-bit limit is hit inside one strip."""
    fib = [1, 1]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    # the values by descending frequency into positions 0, 2, 4, ... and then 1, 3, 5, ...: no value has more than half of the
    # positions (987 of 2,583), so none meets itself
    values = np.array([v for v in range(15, -1, -1) for _ in range(fib[v])], np.uint8)
    out = np.empty(values.size, np.uint8)
    half = (values.size + 1) // 2
    out[0::2], out[1::2] = values[:half], values[half:]
    assert out.size == 2583 and np.all(out[1:] != out[:-1])
    return out


def stream_cases():
    """name -> byte stream fed to the coder directly (never through the filter)."""
    edges = []
    for i, r in enumerate(RUN_EDGES):
        edges += [i + 1] * r + [200 + i]
    return {"fibonacci": fibonacci_stream(), "run_edges": np.array(edges, np.uint8),
            "one_byte": np.array([9], np.uint8), "zeros_2k": np.zeros(2 * STRIP, np.uint8),
            "noise_kp7": _noise(STRIP + 7, 13)}

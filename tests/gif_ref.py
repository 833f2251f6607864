"""The animated-GIF pipeline of DESIGN.md §13 restated in numpy, and a GIF decoder that shares no code with
`nerf_pl_amd.imageio_min.read_gif`.  The GPU path (csrc/gif.hip + imageio_min.gif_bytes) must equal this byte for byte; that
what this writes is a valid GIF is proved on the CPU (tests/test_gif_host.py: this decoder and Pillow read it back).

Everything is integer arithmetic:
  histogram   32 x 32 x 32 bins (r >> 3, g >> 3, b >> 3) per frame
  median cut  on the histogram; boxes always shrunk to their non-empty bins; split the most populated splittable box (tie: lowest
              index) along its longest axis (tie: r, g, b) after the first coordinate whose cumulative count reaches (n + 1) // 2,
              clamped so that the upper part is not empty; the lower part keeps the index, the upper part gets the next one
  index       the box holding the pixel's bin
  palette     (2 * sum + cnt) // (2 * cnt) of the true colours per entry, unused entries 0
  LZW         minimum code size 8, strips of STRIP pixels that each start with a clear code
"""
import struct

import numpy as np

STRIP = 3838          # K: 257 + K <= 4095, so a strip's decoder never assigns code 4095 and the table is never full
CLEAR, END, FIRST = 256, 257, 258


# ------------------------------------------------------------------------------------------------------------- quantiser
def histogram(frame):
    px = np.asarray(frame, np.uint8).reshape(-1, 3).astype(np.int64) >> 3
    return np.bincount((px[:, 0] << 10) | (px[:, 1] << 5) | px[:, 2], minlength=32768).reshape(32, 32, 32)


def _shrunk(hist, lo, hi):
    """The box lo..hi (inclusive) cut down to the non-empty bins it holds -> (lo, hi, n)."""
    sub = hist[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    new_lo, new_hi = [], []
    for ax in range(3):
        nz = np.flatnonzero(sub.sum(axis=tuple(a for a in range(3) if a != ax)))
        new_lo.append(lo[ax] + int(nz[0]))
        new_hi.append(lo[ax] + int(nz[-1]))
    return new_lo, new_hi, int(sub.sum())


def median_cut(hist):
    """-> [(lo, hi, n)] with lo / hi lists of three inclusive bin coordinates, at most 256 boxes."""
    boxes = [_shrunk(hist, [0, 0, 0], [31, 31, 31])]
    while len(boxes) < 256:
        best = -1
        for i, (lo, hi, n) in enumerate(boxes):
            if lo != hi and (best < 0 or n > boxes[best][2]):
                best = i
        if best < 0:
            break
        lo, hi, n = boxes[best]
        ext = [hi[a] - lo[a] for a in range(3)]
        ax = ext.index(max(ext))
        sub = hist[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        cum = np.cumsum(sub.sum(axis=tuple(a for a in range(3) if a != ax)))
        cut = lo[ax] + int(np.argmax(cum >= (n + 1) // 2))
        cut = min(cut, hi[ax] - 1)
        lower_hi, upper_lo = list(hi), list(lo)
        lower_hi[ax], upper_lo[ax] = cut, cut + 1
        boxes[best] = _shrunk(hist, lo, lower_hi)
        boxes.append(_shrunk(hist, upper_lo, hi))
    return boxes


def quantize(frame):
    """(H, W, 3) uint8 -> (indices (H*W,) uint8, palette (256, 3) uint8, number of boxes)."""
    frame = np.asarray(frame, np.uint8)
    px = frame.reshape(-1, 3)
    boxes = median_cut(histogram(frame))
    lut = np.zeros((32, 32, 32), np.uint8)
    for i, (lo, hi, _) in enumerate(boxes):
        lut[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = i
    idx = lut[px[:, 0] >> 3, px[:, 1] >> 3, px[:, 2] >> 3]
    cnt = np.bincount(idx, minlength=256).astype(np.int64)
    pal = np.zeros((256, 3), np.uint8)
    used = cnt > 0
    for c in range(3):
        s = np.bincount(idx, px[:, c], minlength=256).astype(np.int64)      # (float64 sums of bytes: exact below 2^53)
        pal[used, c] = ((2 * s[used] + cnt[used]) // (2 * cnt[used])).astype(np.uint8)
    return idx, pal, len(boxes)


# ------------------------------------------------------------------------------------------------------------------- LZW
def lzw_codes(indices, K=STRIP):
    """The code sequence of one frame -> (codes, widths) int64 arrays.  Emission m of a strip (m = 1 for the first colour code
    after the strip's clear code) is 9 bits wide until 256 + m reaches 512, then 10, ...: the decoder has assigned codes up to
    256 + m - 1 by then.  The clear code that starts the next strip (or the end code) counts as one more emission of the strip
    before it."""
    indices = np.asarray(indices, np.uint8).reshape(-1).tolist()
    assert 1 <= K <= 3838 and len(indices) > 0
    codes, widths = [CLEAR], [9]
    for start in range(0, len(indices), K):
        strip = indices[start:start + K]
        table, nxt, width = {}, FIRST, 9
        prefix = strip[0]
        for c in strip[1:]:
            key = (prefix << 8) | c
            hit = table.get(key)
            if hit is not None:
                prefix = hit
                continue
            codes.append(prefix)
            widths.append(width)
            table[key] = nxt
            nxt += 1
            if nxt > (1 << width):
                width += 1
            prefix = c
        codes.append(prefix)
        widths.append(width)
        nxt += 1                                  # the decoder assigns a code for this emission too
        if nxt > (1 << width):
            width += 1
        assert nxt <= 4096 and width <= 12
        codes.append(END if start + K >= len(indices) else CLEAR)
        widths.append(width)
    return np.array(codes, np.int64), np.array(widths, np.int64)


def pack_bits(codes, widths):
    """LSB-first packing -> bytes (the last byte zero-padded)."""
    off = np.concatenate([[0], np.cumsum(widths)])
    bits = np.zeros(-(-int(off[-1]) // 8) * 8, np.uint8)
    for j in range(12):
        m = widths > j
        bits[off[:-1][m] + j] = (codes[m] >> j) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def sub_blocks(data):
    """255-byte sub-blocks, each behind its length byte; without the terminating zero-length block."""
    out = bytearray()
    for i in range(0, len(data), 255):
        out.append(min(255, len(data) - i))
        out += data[i:i + 255]
    return bytes(out)


def lzw(indices, K=STRIP):
    """One frame's image data as it stands in the file between the minimum-code-size byte and the block terminator."""
    return sub_blocks(pack_bits(*lzw_codes(indices, K)))


def data_stride(H, W, K=STRIP):
    """Worst case of len(lzw(...)): every code 12 bits wide."""
    n = H * W
    raw = (12 * (n + -(-n // K) + 1) + 7) // 8
    return raw + -(-raw // 255)


# -------------------------------------------------------------------------------------------------------------- container
def header(W, H):
    return b"GIF89a" + struct.pack("<HHBBB", W, H, 0x70, 0, 0) + b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"


def frame_header(W, H, fps):
    return b"\x21\xf9\x04\x00" + struct.pack("<H", round(100 / fps)) + b"\x00\x00" + b"\x2c" + struct.pack("<HHHHB", 0, 0, W, H, 0x87)


def gif_bytes(frames, fps=30, K=STRIP):
    """(F, H, W, 3) uint8 (or a list of (H, W, 3)) -> the file."""
    frames = [np.asarray(f, np.uint8) for f in frames]
    H, W = frames[0].shape[:2]
    out = [header(W, H)]
    for f in frames:
        idx, pal, _ = quantize(f)
        out += [frame_header(W, H, fps), pal.tobytes(), b"\x08", lzw(idx, K), b"\x00"]
    out.append(b"\x3b")
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------- decoder
def _lzw_decode(data, min_size, npix):
    clear, end = 1 << min_size, (1 << min_size) + 1
    table = {i: bytes([i]) for i in range(clear)}
    out = bytearray()
    acc = nacc = pos = 0
    width, prev = min_size + 1, None
    while True:
        while nacc < width:
            if pos >= len(data):
                raise ValueError("LZW data ends without an end code")
            acc |= data[pos] << nacc
            nacc += 8
            pos += 1
        code = acc & ((1 << width) - 1)
        acc >>= width
        nacc -= width
        if code == clear:
            table = {i: bytes([i]) for i in range(clear)}
            width, prev = min_size + 1, None
            continue
        if code == end:
            break
        nxt = end + 1 + (len(table) - clear)
        if prev is None:
            if code >= clear:
                raise ValueError("first code after a clear is not a colour")
            entry = table[code]
        else:
            if code in table:
                entry = table[code]
            elif code == nxt and nxt < 4096:
                entry = prev + prev[:1]
            else:
                raise ValueError("invalid LZW code %d (next free %d)" % (code, nxt))
            if nxt < 4096:
                table[nxt] = prev + entry[:1]
                if nxt + 1 == (1 << width) and width < 12:
                    width += 1
        out += entry
        prev = entry
    if len(out) != npix:
        raise ValueError("LZW data holds %d pixels, the image has %d" % (len(out), npix))
    return np.frombuffer(bytes(out), np.uint8)


def decode_gif(data):
    """File contents -> dict: width, height, loop (None when there is no NETSCAPE2.0 block), frames = [dict(indices (h, w) uint8,
    palette (n, 3) uint8, delay in centiseconds, left, top, transparent index or None, disposal)]."""
    data = bytes(data)
    if data[:6] not in (b"GIF89a", b"GIF87a"):
        raise ValueError("not a GIF file")
    W, H, packed = struct.unpack("<HHB", data[6:11])
    pos = 13
    gpal = None
    if packed & 0x80:
        n = 2 << (packed & 7)
        gpal = np.frombuffer(data, np.uint8, 3 * n, pos).reshape(n, 3)
        pos += 3 * n
    res = {"width": W, "height": H, "loop": None, "frames": []}
    delay, transparent, disposal = 0, None, 0

    def blocks(pos):
        body = bytearray()
        while data[pos]:
            body += data[pos + 1:pos + 1 + data[pos]]
            pos += 1 + data[pos]
        return bytes(body), pos + 1

    while True:
        tag = data[pos]
        pos += 1
        if tag == 0x3b:
            break
        if tag == 0x21:
            label = data[pos]
            body, pos = blocks(pos + 1)
            if label == 0xf9:
                flags, delay, tr = struct.unpack("<BHB", body[:4])
                transparent = tr if flags & 1 else None
                disposal = (flags >> 2) & 7
            elif label == 0xff and body[:11] == b"NETSCAPE2.0" and body[11] == 1:
                res["loop"] = struct.unpack("<H", body[12:14])[0]
        elif tag == 0x2c:
            left, top, w, h, flags = struct.unpack("<HHHHB", data[pos:pos + 9])
            pos += 9
            if flags & 0x40:
                raise NotImplementedError("interlaced GIF")
            pal = gpal
            if flags & 0x80:
                n = 2 << (flags & 7)
                pal = np.frombuffer(data, np.uint8, 3 * n, pos).reshape(n, 3)
                pos += 3 * n
            min_size = data[pos]
            body, pos = blocks(pos + 1)
            res["frames"].append({"indices": _lzw_decode(body, min_size, w * h).reshape(h, w), "palette": pal, "delay": delay,
                                  "left": left, "top": top, "transparent": transparent, "disposal": disposal})
            delay, transparent, disposal = 0, None, 0
        else:
            raise ValueError("unknown block 0x%02x at byte %d" % (tag, pos - 1))
    return res


# ---------------------------------------------------------------------------------------------------------- test frames
def psnr_u8(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(10.0 * np.log10(255.0 ** 2 / np.mean(d * d)))


def render_like(H, W, seed=0):
    """A smooth shaded blob with a soft-edged texture on a white background: what a synthetic NeRF render looks like."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (x + 0.5) / W - 0.5, (y + 0.5) / H - 0.5
    r2 = (u * u + v * v) / 0.16
    inside = r2 < 1.0
    z = np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))
    ph = rng.uniform(0, 2 * np.pi, 3)
    col = np.stack([0.5 + 0.4 * np.sin(9 * u + 5 * v + ph[0]) * z, 0.45 + 0.35 * np.cos(7 * v - 3 * u + ph[1]),
                    0.3 + 0.6 * z * (0.5 + 0.5 * np.sin(13 * u * v + ph[2]))], axis=-1)
    col = col * (0.35 + 0.65 * z[..., None]) + rng.normal(0, 0.004, (H, W, 3))
    edge = np.clip((1.0 - r2) * 40.0, 0.0, 1.0)[..., None]
    img = np.where(inside[..., None], col * edge + (1.0 - edge), 1.0)
    return (np.clip(img, 0.0, 1.0) * 255.0).astype(np.uint8)


def bins_frame(n_bins, H, W, seed=0):
    """A frame whose pixels occupy exactly `n_bins` histogram bins (every bin at least once, the low 3 bits random)."""
    assert H * W >= n_bins
    rng = np.random.RandomState(seed)
    bins = rng.permutation(32768)[:n_bins]
    pick = np.concatenate([bins, bins[rng.randint(0, n_bins, H * W - n_bins)]])
    rng.shuffle(pick)
    px = np.stack([pick >> 10, (pick >> 5) & 31, pick & 31], axis=-1) * 8 + rng.randint(0, 8, (H * W, 3))
    return px.astype(np.uint8).reshape(H, W, 3)

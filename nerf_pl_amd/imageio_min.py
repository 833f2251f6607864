"""Image / depth writers of the reference's eval loop (eval.py:119-149) without its imageio / cv2 dependencies:
PNG (8-bit RGB or grey, zlib-deflated, filter 0), PFM (datasets/depth_utils.py:43-69 `save_pfm` / `read_pfm`, same bytes)
and the raw little-endian float32 dump of `--depth_format bytes` (eval.py:135-137); and the host half of scene loading
(nerf_pl_amd/datasets): the PNG container parser, the JPEG marker parser and Pillow's Lanczos taps.  Host-side, numpy only —
except the animated GIF of eval.py:145 at the end of the file, whose palettes and LZW data come from the GPU (csrc/gif.hip)
and whose container is written here, and the opt-in `png_bytes_device`, whose zlib data comes from the GPU (csrc/png.hip)."""
import math
import re
import struct
import sys
import zlib

import numpy as np


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def png_bytes(img, level=6):
    """(H, W, 3) or (H, W) uint8 -> PNG file contents."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8:
        raise ValueError("write_png expects uint8 (eval.py:139 converts with (img*255).astype(np.uint8))")
    if img.ndim == 2:
        color, ch = 0, 1
    elif img.ndim == 3 and img.shape[2] == 3:
        color, ch = 2, 3
    elif img.ndim == 3 and img.shape[2] == 4:
        color, ch = 6, 4
    else:
        raise ValueError("write_png expects (H, W), (H, W, 3) or (H, W, 4)")
    h, w = img.shape[:2]
    rows = np.empty((h, 1 + w * ch), dtype=np.uint8)
    rows[:, 0] = 0                                           # filter type 0 (None) on every scanline
    rows[:, 1:] = img.reshape(h, w * ch)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path, img, level=6):
    """imageio.imwrite(path, img_uint8) of eval.py:141."""
    with open(path, "wb") as f:
        f.write(png_bytes(img, level))


def read_png(path):
    """Decoder for the files write_png produces (8-bit, non-interlaced, filter 0-4) — used by the tests."""
    data = open(path, "rb").read() if isinstance(path, str) else path
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, color = hdr[:4]
    ch = {0: 1, 2: 3, 6: 4}[color]
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    if np.any(raw[:, 0] != 0):
        raise NotImplementedError("only filter 0 is decoded")
    out = raw[:, 1:].reshape(h, w, ch)
    return out[:, :, 0].copy() if ch == 1 else out.copy()


def png_idat(data):
    """PNG file contents (bytes, or a path) -> (w, h, channels, zlib stream): the IDAT chunks joined, not inflated (what
    ops.inflate_batch takes).  Only what ops.decode_png_batch takes is accepted: 8 bits per sample, no interlace, grey / RGB /
    RGBA."""
    if isinstance(data, str):
        with open(data, "rb") as f:
            data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError("PNG without IHDR")
    w, h, depth, color, _, _, interlace = hdr
    if depth != 8:
        raise ValueError("PNG bit depth %d is not supported (8 only)" % depth)
    if interlace != 0:
        raise ValueError("interlaced PNG is not supported")
    if color not in (0, 2, 6):
        raise ValueError("PNG colour type %d (%s) is not supported (grey, RGB, RGBA only)"
                         % (color, {3: "palette", 4: "grey + alpha"}.get(color, "unknown")))
    return w, h, {0: 1, 2: 3, 6: 4}[color], b"".join(idat)


def png_inflate(data):
    """PNG file contents (bytes, or a path) -> (w, h, channels, inflated IDAT stream).  The stream is h scanlines of
    1 filter byte + w * channels bytes, still filtered: the GPU reverses the filters (ops.decode_png_batch).  Only what that
    kernel takes is accepted: 8 bits per sample, no interlace, grey / RGB / RGBA."""
    w, h, ch, stream = png_idat(data)
    raw = zlib.decompress(stream)
    if len(raw) != h * (1 + w * ch):
        raise ValueError("PNG data holds %d bytes, %d x %d x %d needs %d" % (len(raw), h, w, ch, h * (1 + w * ch)))
    return w, h, ch, raw


def png_bytes_device(images):
    """(n, H, W) or (n, H, W, C) uint8 images ON THE DEVICE, C in (1, 3, 4) -> a list of n PNG file contents.
    Filter choice, deflate (8192-byte strips, run-length matches, one dynamic-Huffman block each) and Adler-32 are formed on the
    GPU (ops.png_filter, ops.png_deflate); one copy brings the data to the host and one the lengths and checksums; the
    container and its chunk CRC-32s are written here."""
    import torch

    from . import ops
    from ._lib import NerfHipError
    if torch.is_tensor(images) and images.dim() == 3:
        images = images.unsqueeze(3)
    streams = ops.png_filter(images)
    n, h, w, ch = images.shape
    if n == 0:
        return []
    meta = torch.empty((2, n), device=images.device, dtype=torch.int32)
    data, _, _ = ops.png_deflate(streams, meta=meta)
    meta = meta.cpu().numpy()
    lengths, adler = meta[0], meta[1]
    if np.any(lengths < 0):
        raise NerfHipError("png_deflate: a strip exceeded its worst-case size in image %d" % int(np.flatnonzero(lengths < 0)[0]))
    data = data[:, :int(lengths.max())].cpu().numpy()
    head = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0))
    tail = _chunk(b"IEND", b"")
    return [head + _chunk(b"IDAT", b"\x78\x01" + data[i, :lengths[i]].tobytes() + struct.pack(">I", int(adler[i]) & 0xffffffff)) + tail
            for i in range(n)]


def write_png_device(paths, images):
    """One file per image of `png_bytes_device(images)`: `paths` is a list of n names."""
    files = png_bytes_device(images)
    if len(paths) != len(files):
        raise ValueError("write_png_device: %d paths for %d images" % (len(paths), len(files)))
    for path, data in zip(paths, files):
        with open(path, "wb") as f:
            f.write(data)


# zigzag position -> natural (row-major) index of an 8 x 8 block
JPEG_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                        21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                        61, 54, 47, 55, 62, 63], np.int64)

_SOF_NAMES = {0xc1: "extended sequential DCT", 0xc2: "progressive DCT", 0xc3: "lossless", 0xc5: "differential sequential DCT",
              0xc6: "differential progressive DCT", 0xc7: "differential lossless", 0xc9: "arithmetic-coded sequential DCT",
              0xca: "arithmetic-coded progressive DCT", 0xcb: "arithmetic-coded lossless", 0xcd: "arithmetic-coded differential",
              0xce: "arithmetic-coded differential progressive", 0xcf: "arithmetic-coded differential lossless"}


def jpeg_parse(data):
    """JPEG file contents (bytes, or a path) -> dict: the counterpart of png_inflate.  Only what ops.jpeg_entropy_decode and
    ops.decode_jpeg_batch take is accepted — baseline sequential DCT (SOF0), 8 bits, Huffman-coded, one interleaved scan; one
    component, or three (YCbCr) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1 — anything else raises a ValueError that names
    the problem and the file.  Keys:
        width, height, restart_interval (MCUs, 0 = none), mcus_x, mcus_y
        components       [(id, h, v, quantisation table id, DC table id, AC table id)] in scan order
        quant            {id: (64,) uint16 in natural order}
        huffman          {(class, id): (counts (16,) uint8, symbols (n,) uint8)}, class 0 = DC, 1 = AC
        scan             the entropy-coded segment (bytes), stuffed zeros and RSTm markers still inside"""
    name = "JPEG data"
    if isinstance(data, str):
        name = data
        with open(data, "rb") as f:
            data = f.read()
    data = bytes(data)

    def bad(what):
        return ValueError("%s: %s" % (name, what))

    if data[:2] != b"\xff\xd8":
        raise bad("not a JPEG file")
    pos, n = 2, len(data)
    frame, quant, huffman, restart, adobe_transform = None, {}, {}, 0, None
    while True:
        while pos < n and data[pos] != 0xff:              # (garbage between segments is skipped, as libjpeg does)
            pos += 1
        while pos < n and data[pos] == 0xff:
            pos += 1
        if pos >= n:
            raise bad("truncated: the file ends before a scan starts")
        marker = data[pos]
        pos += 1
        if marker == 0xd8 or marker == 0x01 or 0xd0 <= marker <= 0xd7:
            continue
        if marker == 0xd9:
            raise bad("no scan before the end-of-image marker")
        if pos + 2 > n:
            raise bad("truncated inside a marker segment")
        length = struct.unpack(">H", data[pos:pos + 2])[0]
        if length < 2 or pos + length > n:
            raise bad("truncated inside a marker segment")
        body = data[pos + 2:pos + length]
        pos += length
        if marker == 0xc0:
            if frame is not None:
                raise bad("more than one frame header")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise bad("malformed frame header")
            depth, height, width, ncomp = struct.unpack(">BHHB", body[:6])
            if depth != 8:
                raise bad("%d-bit samples are not supported (8 only)" % depth)
            if height < 1 or width < 1:
                raise bad("empty image (%d x %d)" % (width, height))
            frame = (width, height, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i])
                                     for i in range(ncomp)])
        elif marker in _SOF_NAMES:
            depth = body[0] if body else 8
            raise bad("%s%s (SOF%d) is not supported (baseline sequential DCT only)"
                      % (_SOF_NAMES[marker], ", %d-bit" % depth if depth != 8 else "", marker - 0xc0))
        elif marker == 0xcc:
            raise bad("arithmetic coding is not supported")
        elif marker == 0xdb:
            at = 0
            while at < len(body):
                pq, tq = body[at] >> 4, body[at] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or at + 1 + size > len(body):
                    raise bad("malformed quantisation table")
                if pq:
                    raise bad("16-bit quantisation tables are not supported")
                table = np.zeros(64, np.uint16)
                table[JPEG_ZIGZAG] = np.frombuffer(body, np.uint8, 64, at + 1)
                quant[tq] = table
                at += 1 + size
        elif marker == 0xc4:
            at = 0
            while at < len(body):
                if at + 17 > len(body):
                    raise bad("malformed Huffman table")
                tc, th = body[at] >> 4, body[at] & 15
                counts = np.frombuffer(body, np.uint8, 16, at + 1).copy()
                total = int(counts.sum())
                if tc > 1 or th > 3 or total > 256 or at + 17 + total > len(body):
                    raise bad("malformed Huffman table")
                huffman[(tc, th)] = (counts, np.frombuffer(body, np.uint8, total, at + 17).copy())
                at += 17 + total
        elif marker == 0xdd:
            if len(body) != 2:
                raise bad("malformed restart interval")
            restart = struct.unpack(">H", body)[0]
        elif marker == 0xee and body[:5] == b"Adobe" and len(body) >= 12:
            adobe_transform = body[11]
        elif marker == 0xda:
            break
    if frame is None:
        raise bad("scan without a frame header")
    width, height, comps = frame
    if len(comps) not in (1, 3):
        raise bad("%d components are not supported (1, or 3 as YCbCr)" % len(comps))
    if len(comps) == 3 and (adobe_transform == 0 or [c[0] for c in comps] == [82, 71, 66]):
        raise bad("RGB-coded JPEG is not supported (YCbCr only)")
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise bad("malformed scan header")
    if body[0] != len(comps):
        raise bad("a scan of %d of the %d components (non-interleaved file) is not supported" % (body[0], len(comps)))
    ss, se, ahal = body[1 + 2 * body[0]:]
    if (ss, se, ahal) != (0, 63, 0):
        raise bad("spectral selection / successive approximation in a baseline scan")
    components = []
    for i, (cid, h, v, tq) in enumerate(comps):
        sid, tables = body[1 + 2 * i], body[2 + 2 * i]
        if sid != cid:
            raise bad("scan components out of frame order")
        td, ta = tables >> 4, tables & 15
        if td > 3 or ta > 3:
            raise bad("malformed scan header")
        if tq not in quant:
            raise bad("component %d names quantisation table %d, which the file does not define" % (cid, tq))
        components.append((cid, h, v, tq, td, ta))
    if len(components) == 1:
        components[0] = (components[0][0], 1, 1) + components[0][3:]      # one component: its factors do not matter
    else:
        factors = [(c[1], c[2]) for c in components]
        if factors[0] not in ((1, 1), (2, 1), (2, 2)) or factors[1:] != [(1, 1), (1, 1)]:
            raise bad("sampling factors %s are not supported (luma 1x1, 2x1 or 2x2 with chroma 1x1)"
                      % ", ".join("%dx%d" % f for f in factors))
    # the entropy-coded segment ends at the first marker that is neither a stuffed zero nor RSTm
    buf = np.frombuffer(data, np.uint8, offset=pos)
    ff = np.flatnonzero(buf[:-1] == 0xff) if len(buf) > 1 else np.zeros(0, np.int64)
    follow = buf[ff + 1]
    stop = ff[(follow != 0) & ((follow < 0xd0) | (follow > 0xd7)) & (follow != 0xff)]
    if len(stop) == 0:
        raise bad("truncated: the entropy-coded data is not terminated by a marker")
    end = int(stop[0])
    if buf[end + 1] != 0xd9:
        raise bad("more than one scan (marker 0x%02x follows the first) is not supported" % buf[end + 1])
    if end == 0:
        raise bad("empty scan")
    hs, vs = components[0][1], components[0][2]
    return {"width": width, "height": height, "components": components, "quant": quant, "huffman": huffman,
            "restart_interval": restart, "mcus_x": -(-width // (8 * hs)), "mcus_y": -(-height // (8 * vs)),
            "scan": data[pos:pos + end], "name": name}


LANCZOS_PRECISION_BITS = 32 - 8 - 2      # Pillow's fixed point: 8 bits of pixel, 2 of headroom for the negative lobes


def _lanczos(x):
    if not (-3.0 <= x < 3.0):
        return 0.0
    if x == 0.0:
        return 1.0
    a, b = x * math.pi, x / 3.0 * math.pi
    return (math.sin(a) / a) * (math.sin(b) / b)


def lanczos_taps(in_size, out_size):
    """Pillow's resampling coefficients of `Image.resize(..., Image.LANCZOS)` for one axis, in its 22-bit fixed point:
    (xmin (out,), count (out,), taps (out, ksize)) int32; output xx = clip8((2^21 + sum_j in[xmin + j] * taps[xx, j]) >> 22).
    Formed in double, scalar by scalar with the C library's sin, as Pillow forms them: the last bit decides a rounding."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    one = float(1 << LANCZOS_PRECISION_BITS)
    xmin = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    taps = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [_lanczos((x - center + 0.5) * ss) * ss for x in range(lo, hi)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], count[xx] = lo, hi - lo
        taps[xx, :hi - lo] = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]
    return xmin, count, taps


def save_pfm(filename, image, scale=1):
    """datasets/depth_utils.py:43-69: bottom-to-top float32 rows, header 'Pf' (grey) / 'PF' (colour), negative scale =
    little-endian."""
    image = np.flipud(image)
    if image.dtype.name != "float32":
        raise Exception("Image dtype must be float32.")
    if len(image.shape) == 3 and image.shape[2] == 3:
        color = True
    elif len(image.shape) == 2 or len(image.shape) == 3 and image.shape[2] == 1:
        color = False
    else:
        raise Exception("Image must have H x W x 3, H x W x 1 or H x W dimensions.")
    endian = image.dtype.byteorder
    if endian == "<" or endian == "=" and sys.byteorder == "little":
        scale = -scale
    with open(filename, "wb") as f:
        f.write(b"PF\n" if color else b"Pf\n")
        f.write(("%d %d\n" % (image.shape[1], image.shape[0])).encode("utf-8"))
        f.write(("%f\n" % scale).encode("utf-8"))
        f.write(np.ascontiguousarray(image).tobytes())


def read_pfm(filename):
    """datasets/depth_utils.py:5-40 -> (data, scale)."""
    with open(filename, "rb") as f:
        header = f.readline().decode("utf-8").rstrip()
        if header not in ("PF", "Pf"):
            raise Exception("Not a PFM file.")
        color = header == "PF"
        m = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
        if not m:
            raise Exception("Malformed PFM header.")
        width, height = map(int, m.groups())
        scale = float(f.readline().rstrip())
        endian = "<" if scale < 0 else ">"
        data = np.frombuffer(f.read(), dtype=endian + "f4")
    data = np.reshape(data, (height, width, 3) if color else (height, width))
    return np.flipud(data), abs(scale)


def depth_bytes(depth):
    """eval.py:135-137 (`--depth_format bytes`): the float32 depth map's raw bytes."""
    return np.ascontiguousarray(depth, dtype=np.float32).tobytes()


def jet_table():
    """The JET colour map as a (256, 3) uint8 table whose columns are in the order of the channels `visualize_depth` returns:
    the reference hands cv2's BGR image to PIL as if it were RGB (visualization.py:16-17), so column 0 is the map's BLUE,
    column 1 its green and column 2 its red.  v = (i + 1) / 256; r = clip(1.5 - |4v - 3|), g = clip(1.5 - |4v - 2|),
    b = clip(1.5 - |4v - 1|); bytes = round-half-even(255 c).  (Formed in float64, where every value before the rounding is
    exact.  Equality with the bytes of cv2.COLORMAP_JET is unverified: cv2 is no dependency; a table is an argument.)"""
    v = (np.arange(256, dtype=np.float64) + 1.0) / 256.0
    r, g, b = (np.clip(1.5 - np.abs(4.0 * v - k), 0.0, 1.0) for k in (3.0, 2.0, 1.0))
    return np.rint(255.0 * np.stack([b, g, r], axis=1)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- animated GIF (eval.py:145)
GIF_BATCH = 8          # frames quantised and LZW-coded per call: at 800 x 800 about 10 MB of device memory per frame


def _gif_header(w, h):
    """'GIF89a', the logical screen (no global colour table) and the NETSCAPE2.0 block for endless looping."""
    return b"GIF89a" + struct.pack("<HHBBB", w, h, 0x70, 0, 0) + b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"


def _gif_frame_header(w, h, fps):
    """Graphic control extension (delay in centiseconds, no transparency, no disposal) and the image descriptor of a full frame
    with a 256-entry local colour table."""
    return b"\x21\xf9\x04\x00" + struct.pack("<H", round(100 / fps)) + b"\x00\x00\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0x87)


class GifWriter:
    """The file of `imageio.mimsave(path, imgs, fps=fps)` piece by piece: `append` takes (n, H, W, 3) uint8 frames ON THE
    DEVICE, `getvalue` closes the file.  Per `append`: quantise and LZW-code on the GPU (ops.gif_quantize, ops.gif_lzw), read
    the n lengths, then the palettes and the data up to the longest length; every frame has its own palette, as imageio's writer
    gives it.  Nothing is kept on the device between calls."""

    def __init__(self, fps=30):
        if not fps > 0 or round(100 / fps) > 65535:
            raise ValueError("fps must be positive and give a delay below 65536 centiseconds, got %r" % (fps,))
        self.fps, self.size, self.pieces, self.n_frames = fps, None, [], 0

    def append(self, frames):
        from . import ops
        from ._lib import NerfHipError
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("GifWriter.append expects (n, H, W, 3) uint8 frames, got %s" % (tuple(frames.shape),))
        n, h, w = frames.shape[:3]
        if n == 0:
            return
        if self.size is None:
            self.size = (w, h)
            self.pieces.append(_gif_header(w, h))
        elif self.size != (w, h):
            raise ValueError("frames of %d x %d after frames of %d x %d" % ((w, h) + self.size))
        ws = ops.gif_workspace(n, h, w, frames.device)
        indices, palettes, _ = ops.gif_quantize(frames, ws)
        data, lengths = ops.gif_lzw(indices, h, w, ws)
        lengths = lengths.cpu().numpy()                                # the one read that decides how much data follows
        if (lengths < 0).any():
            raise NerfHipError("gif_lzw: a dictionary probe exceeded its bound in frame %d" % int(np.flatnonzero(lengths < 0)[0]))
        data = data[:, :int(lengths.max())].cpu().numpy()
        palettes = palettes.cpu().numpy()
        head = _gif_frame_header(w, h, self.fps)
        for i in range(n):
            self.pieces += [head, palettes[i].tobytes(), b"\x08", data[i, :lengths[i]].tobytes(), b"\x00"]
        self.n_frames += n

    def getvalue(self):
        if self.size is None:
            raise ValueError("a GIF needs at least one frame")
        return b"".join(self.pieces) + b"\x3b"


def gif_bytes(frames, fps=30, batch=GIF_BATCH):
    """(F, H, W, 3) uint8 frames on the device -> the animated GIF's file contents, `batch` frames per GPU call."""
    out = GifWriter(fps)
    for i in range(0, frames.shape[0], batch):
        out.append(frames[i:i + batch])
    return out.getvalue()


def write_gif(path, frames, fps=30):
    """imageio.mimsave(path, frames, fps=fps) of eval.py:145 for frames on the device."""
    data = gif_bytes(frames, fps)
    with open(path, "wb") as f:
        f.write(data)


def read_gif(data):
    """Decoder for GIF files (contents, or a path) of non-interlaced frames: {'width', 'height', 'loop' (None without a
    NETSCAPE2.0 block), 'palettes': [(n, 3) uint8], 'indices': [(h, w) uint8], 'delays': [centiseconds], 'offsets': [(left,
    top)]}.  Frames are returned as stored: no compositing, transparency or disposal."""
    if isinstance(data, str):
        with open(data, "rb") as f:
            data = f.read()
    buf = np.frombuffer(bytes(data), np.uint8)
    if bytes(buf[:6]) not in (b"GIF87a", b"GIF89a"):
        raise ValueError("not a GIF file")
    out = {"width": int(buf[6]) | int(buf[7]) << 8, "height": int(buf[8]) | int(buf[9]) << 8, "loop": None, "palettes": [],
           "indices": [], "delays": [], "offsets": []}
    pos = 13
    global_table = None
    if buf[10] & 0x80:
        n = 2 << (int(buf[10]) & 7)
        global_table = buf[pos:pos + 3 * n].reshape(n, 3).copy()
        pos += 3 * n

    def sub_blocks(pos):
        parts = []
        while buf[pos] != 0:
            parts.append(buf[pos + 1:pos + 1 + int(buf[pos])])
            pos += 1 + int(buf[pos])
        return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), pos + 1

    delay = 0
    while True:
        if pos >= len(buf):
            raise ValueError("GIF without a trailer")
        kind = int(buf[pos])
        pos += 1
        if kind == 0x3b:
            return out
        if kind == 0x21:
            label = int(buf[pos])
            body, pos = sub_blocks(pos + 1)
            if label == 0xf9 and len(body) >= 4:
                delay = int(body[1]) | int(body[2]) << 8
            elif label == 0xff and len(body) >= 14 and bytes(body[:11]) == b"NETSCAPE2.0" and body[11] == 1:
                out["loop"] = int(body[12]) | int(body[13]) << 8
            continue
        if kind != 0x2c:
            raise ValueError("unknown GIF block 0x%02x" % kind)
        left, top, w, h = (int(buf[pos + 2 * k]) | int(buf[pos + 2 * k + 1]) << 8 for k in range(4))
        flags = int(buf[pos + 8])
        pos += 9
        if flags & 0x40:
            raise ValueError("interlaced GIF frames are not supported")
        table = global_table
        if flags & 0x80:
            n = 2 << (flags & 7)
            table = buf[pos:pos + 3 * n].reshape(n, 3).copy()
            pos += 3 * n
        min_size = int(buf[pos])
        body, pos = sub_blocks(pos + 1)
        out["palettes"].append(table)
        out["indices"].append(_gif_lzw_decode(body, min_size, w * h).reshape(h, w))
        out["delays"].append(delay)
        out["offsets"].append((left, top))
        delay = 0


def _gif_lzw_decode(body, min_size, n_pixels):
    """Variable-width LZW of GIF: codes as (prefix code, last byte, length) arrays, strings written back to front."""
    if not 2 <= min_size <= 8:
        raise ValueError("LZW minimum code size %d" % min_size)
    clear = 1 << min_size
    prefix = np.zeros(4096, np.int32)
    last = np.zeros(4096, np.uint8)
    first = np.zeros(4096, np.uint8)
    length = np.ones(4096, np.int32)
    last[:clear] = first[:clear] = np.arange(clear)
    stream = int.from_bytes(body.tobytes(), "little")
    n_bits = 8 * len(body)
    out = np.zeros(n_pixels, np.uint8)
    at = bit = 0
    width, free, prev = min_size + 1, clear + 2, -1
    while True:
        if bit + width > n_bits:
            raise ValueError("LZW data ends before its end code")
        code = (stream >> bit) & ((1 << width) - 1)
        bit += width
        if bit > 1 << 16:                     # keep the shifts short
            stream >>= bit
            n_bits -= bit
            bit = 0
        if code == clear:
            width, free, prev = min_size + 1, clear + 2, -1
            continue
        if code == clear + 1:
            break
        if prev < 0:
            if code >= clear:
                raise ValueError("LZW: a string code directly after a clear code")
        else:
            if code > free or (code == free and free >= 4096):
                raise ValueError("LZW: code %d is not in the table" % code)
            if free < 4096:
                prefix[free], length[free], first[free] = prev, length[prev] + 1, first[prev]
                last[free] = first[prev] if code == free else first[code]
                free += 1
                if free == 1 << width and width < 12:
                    width += 1
        n = int(length[code])
        if at + n > n_pixels:
            raise ValueError("LZW data holds more pixels than the frame")
        c = code
        for k in range(at + n - 1, at - 1, -1):
            out[k] = last[c]
            c = prefix[c]
        at += n
        prev = code
    if at != n_pixels:
        raise ValueError("LZW data holds %d pixels, the frame has %d" % (at, n_pixels))
    return out

"""Image / depth writers of the reference's eval loop (eval.py:119-149) without its imageio / cv2 dependencies:
PNG (8-bit RGB or grey, zlib-deflated, filter 0), PFM (datasets/depth_utils.py:43-69 `save_pfm` / `read_pfm`, same bytes)
and the raw little-endian float32 dump of `--depth_format bytes` (eval.py:135-137); and the host half of scene loading
(nerf_pl_amd/datasets): the PNG container parser and Pillow's Lanczos taps.  Host-side, numpy only."""
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


def png_inflate(data):
    """PNG file contents (bytes, or a path) -> (w, h, channels, inflated IDAT stream).  The stream is h scanlines of
    1 filter byte + w * channels bytes, still filtered: the GPU reverses the filters (ops.decode_png_batch).  Only what that
    kernel takes is accepted: 8 bits per sample, no interlace, grey / RGB / RGBA."""
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
    ch = {0: 1, 2: 3, 6: 4}[color]
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (1 + w * ch):
        raise ValueError("PNG data holds %d bytes, %d x %d x %d needs %d" % (len(raw), h, w, ch, h * (1 + w * ch)))
    return w, h, ch, raw


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

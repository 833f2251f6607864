"""Test-side baseline JPEG entropy encoder: coefficient blocks + Huffman definitions -> the scan's bytes (stuffing, optional RSTm
markers) in the dict shape of nerf_pl_amd.imageio_min.jpeg_parse, as far as the entropy decoders read it.  It builds the streams
no small photo contains (runs of 0xFF bytes, ZRL chains, a coefficient at k = 63, extreme DC values, 16-bit codes, many restart
intervals) without Pillow and without new binary fixtures.  Not an encoder for images: no DCT, no quantisation, no file headers."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])

# one code of every length 1..16 (the all-ones code stays free, as the standard demands): the last symbol has a 16-bit code
DEEP_DC = (np.ones(16, np.uint8) * (np.arange(16) < 12), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], np.uint8))
DEEP_AC = (np.ones(16, np.uint8), np.array([0x01, 0x00, 0x02, 0x11, 0x03, 0xf0, 0x21, 0x04, 0x12, 0x31, 0x05, 0x41, 0x13, 0x06,
                                            0x51, 0x0a], np.uint8))


def codes(counts, symbols):
    """{symbol: bit string} of the canonical code"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(int(counts[length - 1])):
            out[int(symbols[k])] = format(code, "0%db" % length)
            code += 1
            k += 1
        code <<= 1
    return out


def _magnitude(v):
    """(size, bits) of a DC difference or AC coefficient"""
    if v == 0:
        return 0, ""
    size = int(abs(v)).bit_length()
    return size, format(v if v > 0 else v + (1 << size) - 1, "0%db" % size)


def block_bits(block, pred, dc, ac):
    """one block (64 values, natural order, DC absolute) -> bit string; dc, ac: codes()"""
    zz = [int(block[i]) for i in ZIGZAG]
    diff = ((zz[0] - pred + 32768) & 0xffff) - 32768           # the decoders keep DC sums modulo 2^16
    assert abs(diff) <= 2047, "a DC difference has at most 11 bits"
    size, extra = _magnitude(diff)
    bits = [dc[size], extra]
    run = 0
    for k in range(1, 64):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            bits.append(ac[0xf0])
            run -= 16
        size, extra = _magnitude(zz[k])
        bits += [ac[(run << 4) | size], extra]
        run = 0
    if run:
        bits.append(ac[0x00])
    return "".join(bits)


def pack(bits):
    """bit string -> bytes: padded with ones to a whole byte, a zero stuffed behind every 0xFF"""
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return raw.replace(b"\xff", b"\xff\x00")


def interval_bits(coef, components, huffman, mcus_x, first, last):
    """the bit string of MCUs [first, last): DC predictions start at 0"""
    tables = {key: codes(*value) for key, value in huffman.items()}
    pred = [0] * len(components)
    out = []
    for m in range(first, last):
        my, mx = divmod(m, mcus_x)
        for c, (_, h, v, _, td, ta) in enumerate(components):
            for yy in range(v):
                for xx in range(h):
                    block = coef[c][my * v + yy, mx * h + xx]
                    out.append(block_bits(block, pred[c], tables[(0, td)], tables[(1, ta)]))
                    pred[c] = int(block[0])
    return "".join(out)


def encode(coef, components, huffman, mcus_x, mcus_y, restart_interval=0, name="synthetic"):
    """coef: per component (blocks_y, blocks_x, 64) int16, natural order, DC values absolute; components: (id, h, v, tq, td, ta)
    rows; huffman: {(class, id): (counts[16], symbols)} -> the parsed-file dict the entropy decoders take"""
    n_mcu = mcus_x * mcus_y
    per = restart_interval if restart_interval > 0 else n_mcu
    scan = b""
    for i, first in enumerate(range(0, n_mcu, per)):
        if i:
            scan += bytes([0xff, 0xd0 + ((i - 1) & 7)])
        scan += pack(interval_bits(coef, components, huffman, mcus_x, first, min(first + per, n_mcu)))
    H, W = 8 * mcus_y * components[0][2], 8 * mcus_x * components[0][1]
    return {"name": name, "width": W, "height": H, "components": [tuple(c) for c in components], "huffman": dict(huffman),
            "mcus_x": mcus_x, "mcus_y": mcus_y, "restart_interval": int(restart_interval), "scan": scan}


# ---- the streams the decoders' tests share ------------------------------------------------------------------------------------------
C420 = [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]
C444 = [(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]
GREY = [(1, 1, 1, 0, 0, 0)]


def _empty(components, mcus_x, mcus_y):
    return [np.zeros((mcus_y * c[2], mcus_x * c[1], 64), np.int16) for c in components]


def _random(rng, components, mcus_x, mcus_y, density, amplitude=1023):
    coef = _empty(components, mcus_x, mcus_y)
    for a in coef:
        a[..., 1:] = rng.integers(-amplitude, amplitude + 1, a[..., 1:].shape) * (rng.random(a[..., 1:].shape) < density)
        a[..., 0] = np.cumsum(rng.integers(-300, 301, a.shape[:2]).reshape(-1)).reshape(a.shape[:2]) % 2000 - 1000
    return coef


def edge_cases(standard):
    """[(name, parsed dict, coefficient arrays)]; standard: the four standard tables, e.g. jpeg_parse(a fixture)["huffman"]"""
    rng = np.random.default_rng(11)
    deep = {(0, 0): DEEP_DC, (1, 0): DEEP_AC, (0, 1): DEEP_DC, (1, 1): DEEP_AC}
    out = []

    def add(name, coef, components, huffman, mx, my, restart=0):
        out.append((name, encode(coef, components, huffman, mx, my, restart, name=name), coef))
    # runs of 0xFF: run 15 / size 10 is the standard tables' last, 16-bit code (fifteen ones and a zero), 1023 is ten ones
    coef = _empty(C420, 3, 2)
    for a in coef:
        for k in (16, 32, 48):
            a[..., ZIGZAG[k]] = 1023
    add("ff_runs", coef, C420, standard, 3, 2)
    # ZRL chains: one coefficient far out, behind 61, 47 and 16 zeros
    coef = _empty(C420, 3, 2)
    coef[0][..., ZIGZAG[62]] = -3
    coef[1][..., ZIGZAG[48]] = 5
    coef[2][..., ZIGZAG[17]] = 1
    add("zrl_chains", coef, C420, standard, 3, 2)
    # a coefficient at k = 63: the block has no end-of-block code
    coef = _random(rng, C444, 4, 3, 0.2, 40)
    for a in coef:
        a[..., 63] = rng.integers(1, 9, a.shape[:2])
    add("k63_no_eob", coef, C444, standard, 4, 3)
    # DC differences of +-2047 and sums that leave int16
    coef = _empty(GREY, 8, 6)
    dc = np.cumsum(np.where(np.arange(48) < 30, 2047, -2047))
    coef[0][..., 0] = ((dc + 32768) % 65536 - 32768).reshape(6, 8)
    add("dc_wraps", coef, GREY, {(0, 0): standard[(0, 0)], (1, 0): standard[(1, 0)]}, 8, 6)
    # 16-bit codes: DC size 11 has a 12-bit code here, AC 0/10 a 16-bit one
    coef = _empty(C420, 3, 3)
    for a in coef:
        a[..., 0] = np.cumsum(np.tile([1500, -1500], a.shape[0] * a.shape[1])[:a.shape[0] * a.shape[1]]).reshape(a.shape[:2])
        a[..., 1] = 1023
        a[..., 8] = -513
        a[..., ZIGZAG[8]] = -1                     # run 5, size 1
        a[..., ZIGZAG[9]] = 33                     # run 0, size 6
    add("deep_codes", coef, C420, deep, 3, 3)
    # restart interval 1 and more than 8 intervals: the marker numbers wrap
    add("restart1_wraps", _random(rng, C420, 4, 3, 0.3, 200), C420, standard, 4, 3, restart=1)
    add("restart5", _random(rng, C444, 7, 5, 0.5), C444, standard, 7, 5, restart=5)
    # one block
    coef = _empty(GREY, 1, 1)
    coef[0][0, 0, :4] = [-7, 2, 0, 1]
    add("one_block", coef, GREY, {(0, 0): standard[(0, 0)], (1, 0): standard[(1, 0)]}, 1, 1)
    # dense enough for several workgroups of 32-bit subsequences
    add("dense", _random(rng, C420, 6, 5, 0.6), C420, standard, 6, 5)
    return out


def damaged_cases(standard):
    """[(name, parsed dict)]: every one is refused by the sequential decoder"""
    rng = np.random.default_rng(12)
    out = []
    coef = _random(rng, C420, 6, 5, 0.4)
    good = encode(coef, C420, standard, 6, 5, 4)

    def variant(name, **changes):
        p = dict(good, name=name)
        p.update(changes)
        out.append((name, p))
    variant("truncated_half", scan=good["scan"][:len(good["scan"]) // 2])
    variant("truncated_third", scan=good["scan"][:len(good["scan"]) // 3])
    scan = bytearray(good["scan"])
    scan[scan.index(b"\xff\xd1") + 1] = 0xd5
    variant("wrong_restart_number", scan=bytes(scan))
    at = good["scan"].index(b"\xff\xd2")
    variant("missing_restart", scan=good["scan"][:at] + good["scan"][at + 2:])
    at = good["scan"].rindex(b"\xff\xd6")             # 30 MCUs in 8 intervals: the 7th marker is the last
    variant("missing_last_restart", scan=good["scan"][:at])
    counts, symbols = standard[(1, 0)]
    counts = counts.copy()
    counts[0] = 3
    variant("no_prefix_code", huffman={**standard, (1, 0): (counts, np.concatenate([symbols, symbols[:3]]))})
    variant("missing_table", huffman={k: v for k, v in standard.items() if k != (1, 1)})
    # an invalid code where a block starts: twelve ones are no code of the deep DC table
    deep = {(0, 0): DEEP_DC, (1, 0): DEEP_AC, (0, 1): DEEP_DC, (1, 1): DEEP_AC}
    coef = _empty(C420, 3, 3)
    for a in coef:
        a[..., 1] = 3
    bits = interval_bits(coef, C420, deep, 3, 0, 4) + "1" * 16 + interval_bits(coef, C420, deep, 3, 4, 9)
    p = encode(coef, C420, deep, 3, 3, name="invalid_code")
    p["scan"] = pack(bits)
    out.append(("invalid_code", p))
    return out

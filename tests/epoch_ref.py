"""numpy restatement of `epoch_perm` (csrc/epoch_core.h), written from the header's description — not a call into the library.

key:   s = seed; a = splitmix64(s); s = a ^ epoch; rk[r] = splitmix64(s) >> 32, r = 0..5
E(v):  b = max(2, ceil(log2 n)) bits, v = L << wr | R with wr = b // 2, wl = b - wr; six rounds
       (L, R) <- (R, L ^ (fmix32(R + rk[r]) & (2^wl - 1))), the widths swapping after every round
perm:  v = E(p); while v >= n: v = E(v)
ranks: the j-th id of rank r of `world` is perm((j * world + r) mod n), ceil(n / world) of them
"""
import numpy as np

ROUNDS = 6
M64 = (1 << 64) - 1


def _splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def round_keys(seed, epoch, rounds=ROUNDS):
    s, a = _splitmix64(int(seed) & M64)
    s = a ^ (int(epoch) & M64)
    keys = []
    for _ in range(rounds):
        s, z = _splitmix64(s)
        keys.append(z >> 32)
    return keys


def _fmix32(h):
    h = h.astype(np.uint64)                      # 32-bit values in 64-bit lanes: every product is masked back to 32 bits
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def bits(n):
    return max(2, int(n - 1).bit_length())


def encrypt(keys, b, v):
    wr = b // 2
    wl = b - wr
    v = v.astype(np.uint64)
    L, R = v >> np.uint64(wr), v & np.uint64((1 << wr) - 1)
    for k in keys:
        f = _fmix32((R + np.uint64(k)) & np.uint64(0xFFFFFFFF)) & np.uint64((1 << wl) - 1)
        L, R = R, L ^ f
        wl, wr = wr, wl
    return (L << np.uint64(wr)) | R


def perm(seed, epoch, n, positions, rounds=ROUNDS):
    """ids of `positions` (any integer array with values in [0, n)) as int64"""
    p = np.asarray(positions, np.int64)
    if n == 1:
        return np.zeros(p.shape, np.int64)
    keys, b = round_keys(seed, epoch, rounds), bits(n)
    v = encrypt(keys, b, p.astype(np.uint64))
    while True:
        out = v >= np.uint64(n)
        if not out.any():
            return v.astype(np.int64)
        v[out] = encrypt(keys, b, v[out])


def rank_ids(seed, epoch, n, rank=0, world=1, first=0, count=None):
    share = (n + world - 1) // world
    if count is None:
        count = share - first
    j = np.arange(first, first + count, dtype=np.int64)
    return perm(seed, epoch, n, (j * world + rank) % n)

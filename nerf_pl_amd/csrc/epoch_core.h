// The epoch shuffle: a keyed bijection on [0, n) evaluated per position, the routine of the epoch kernels
// (epoch.hip) and of their host twin nerfhip_epoch_ids_host, from this one source.  Integer arithmetic only: the device and the
// host produce the same bits.  The function is public — tests/epoch_ref.py restates it in numpy from the text below, and a user
// can recompute which ray any step of any epoch saw.
//
// Key.  s = seed;  a = splitmix64(s);  s = a ^ epoch;  rk[r] = splitmix64(s) >> 32  for r = 0 .. 5, where splitmix64(s) is
//   s += 0x9E3779B97F4A7C15;  z = s;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
//   return z ^ z >> 31                                       (all mod 2^64; s keeps its new value between calls).
//
// Permutation.  epoch_perm(key, 1, 0) = 0.  Otherwise b = max(2, ceil(log2 n)) bits, split into a left half of wl = b - b / 2
// bits and a right half of wr = b / 2 bits: v = L << wr | R.  One encryption E(v) is six rounds r = 0 .. 5 of an alternating
// Feistel network,
//     (L, R) <- (R, L ^ (fmix32((uint32) R + rk[r]) & (2^wl - 1))),  then wl and wr swap,
// fmix32 being murmur3's finaliser  h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16  (mod 2^32);
// after the sixth round the widths are the initial ones again and E(v) = L << wr | R.  Every round is invertible, so E is a
// bijection on [0, 2^b).  epoch_perm(key, n, p) walks the cycle of E from p: v = E(p), and while v >= n, v = E(v).
//
// The walk ends.  E permutes [0, 2^b); the cycle through p in [0, n) comes back to p, which is < n, so it meets [0, n) again after
// at most (the 2^b - n values outside) + 1 steps.  That bound is the loop's limit: there is no unbounded loop.  2^b < 2 n (n > 2),
// so a step lands in [0, n) with probability above 1/2 and the expected number of encryptions is below 2.  Restricting a
// permutation to the first return into a subset is again a permutation: epoch_perm(key, n, .) is a bijection on [0, n).
#pragma once
#include "twin.h"

namespace nerfhip {

constexpr int kEpochRounds = 6;
constexpr uint64_t kEpochMaxN = (uint64_t)1 << 40;

struct EpochKey {
    uint32_t rk[kEpochRounds];
};

NH_TWIN_HD uint64_t epoch_splitmix64(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

NH_TWIN_HD EpochKey epoch_key(uint64_t seed, uint64_t epoch) {
    uint64_t s = seed;
    s = epoch_splitmix64(s) ^ epoch;
    EpochKey k;
#pragma unroll
    for (int r = 0; r < kEpochRounds; ++r) k.rk[r] = (uint32_t)(epoch_splitmix64(s) >> 32);
    return k;
}

NH_TWIN_HD uint32_t epoch_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// max(2, ceil(log2 n)) for 2 <= n <= 2^40
NH_TWIN_HD int epoch_bits(uint64_t n) {
    int b = 2;
    while (b < 40 && ((uint64_t)1 << b) < n) ++b;
    return b;
}

// one encryption of the b-bit value v (both halves are at most 20 bits wide)
NH_TWIN_HD uint64_t epoch_encrypt(const EpochKey& k, int b, uint64_t v) {
    int wr = b >> 1, wl = b - wr;
    uint32_t L = (uint32_t)(v >> wr), R = (uint32_t)v & ((1u << wr) - 1u);
#pragma unroll
    for (int r = 0; r < kEpochRounds; ++r) {
        const uint32_t f = epoch_fmix32(R + k.rk[r]) & ((1u << wl) - 1u);
        const uint32_t nr = L ^ f;
        L = R;
        R = nr;
        const int w = wl;
        wl = wr;
        wr = w;
    }
    return ((uint64_t)L << wr) | R;
}

// position p in [0, n) -> id in [0, n);  1 <= n <= 2^40
NH_TWIN_HD uint64_t epoch_perm(const EpochKey& k, uint64_t n, uint64_t p) {
    if (n == 1) return 0;
    const int b = epoch_bits(n);
    const uint64_t limit = ((uint64_t)1 << b) - n + 1;
    uint64_t v = p;
    for (uint64_t step = 0; step < limit; ++step) {
        v = epoch_encrypt(k, b, v);
        if (v < n) break;
    }
    return v;
}

// Ranks (torch's DistributedSampler): rank r of `world` owns ceil(n / world) positions, its j-th one is (j world + r) mod n — the
// wrap is the sampler's padding.
NH_TWIN_HD int64_t epoch_rank_share(int64_t n, int world) { return (n + world - 1) / world; }
NH_TWIN_HD uint64_t epoch_rank_id(const EpochKey& k, int64_t n, int rank, int world, int64_t j) {
    return epoch_perm(k, (uint64_t)n, (uint64_t)((j * world + rank) % n));
}

}  // namespace nerfhip

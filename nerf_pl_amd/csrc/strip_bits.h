// What the two strip coders (gif.hip: LZW, png.hip: deflate) share.  Both cut a stream into strips that are coded independently
// into their own fixed-size bit buffers (32-bit words, bits from the low end); a one-workgroup scan (block_scan.h) turns the strips'
// bit lengths into offsets, and a gather forms every output byte from the strip that holds its first bit and the following ones.
#pragma once
#include <hip/hip_runtime.h>

namespace nerfhip {

// How a full word leaves a BitWriter.  StoreWord: the writer owns the words (a strip written by one lane).  OrWord: several
// writers at different bit positions of zeroed shared words; OR only, so their order does not matter.
struct StoreWord { static __device__ __forceinline__ void flush(uint32_t* p, uint32_t v) { *p = v; } };
struct OrWord { static __device__ __forceinline__ void flush(uint32_t* p, uint32_t v) { atomicOr(p, v); } };

// A 64-bit accumulator in front of 32-bit words, bits from the low end: start at any bit of `base`, put, finish.
template <typename Flush>
struct BitWriter {
    uint32_t* words;
    unsigned long long acc;
    int nacc, nwords;
    __device__ __forceinline__ void start(uint32_t* base, int bit) {
        words = base;
        acc = 0;
        nacc = bit & 31;
        nwords = bit >> 5;
    }
    __device__ __forceinline__ void put(uint32_t v, int nb) {      // nb <= 32
        acc |= (unsigned long long)v << nacc;
        nacc += nb;
        if (nacc >= 32) {
            Flush::flush(&words[nwords++], (uint32_t)acc);
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc > 0) Flush::flush(&words[nwords], (uint32_t)acc);
    }
    __device__ __forceinline__ int bits() const { return nwords * 32 + nacc; }      // the position behind the last bit put
};

// The value of strip i in the scan of the bit lengths: its length, or 0 with *bad raised where its coder gave up (-1).
__device__ __forceinline__ int64_t strip_bits_or_flag(int32_t len, int* bad) {
    if (len < 0) atomicOr(bad, 1);
    return len < 0 ? 0 : len;
}

// The 8 bits at `bit` of the stream that the S strips first_strip .. first_strip + S - 1 form: off[s] is the first bit of strip s in
// the stream and len[s] its bit count (both indexed from the stream's first strip), its words start at bits + (first_strip + s) *
// strip_words.  Binary search for the last strip whose offset is <= bit, then the bits of that strip and the following ones (a
// strip may hold fewer than 8; empty ones are passed over); bits behind the last strip are zero.
__device__ __forceinline__ unsigned gather_byte(const int64_t* off, const int32_t* len, const uint32_t* bits, int64_t first_strip,
                                                int64_t S, int strip_words, int64_t bit) {
    int64_t lo = 0, hi = S - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= bit) lo = mid; else hi = mid - 1;
    }
    int64_t s = lo;
    int got = 0;
    unsigned v = 0;
    while (got < 8 && s < S) {
        const int64_t q = bit - off[s];
        const int avail = (int)(len[s] - q);
        if (avail <= 0) { ++s; continue; }
        const int take = avail < 8 - got ? avail : 8 - got;
        const uint32_t* words = bits + (first_strip + s) * strip_words;
        const int word = (int)(q >> 5), sh = (int)(q & 31);
        unsigned long long x = words[word];
        if (sh + take > 32) x |= (unsigned long long)words[word + 1] << 32;      // (then the strip has that word: avail > 32 - sh)
        v |= (unsigned)((x >> sh) & ((1u << take) - 1u)) << got;
        got += take;
        bit += take;
    }
    return v;
}

}  // namespace nerfhip

// What the two baseline-JPEG entropy decoders share (jpeg.hip: the sequential host walk; jpeg_entropy.hip: the self-synchronising
// split decoder, device kernels and host twin): the Huffman table layout, a bounds-checked bit fetch over a compacted segment, and
// the one-symbol step of the decoder state (bit position, block slot inside the MCU, zigzag index).  Plain arithmetic, no
// intrinsics: every function compiles for the host and for gfx950 alike.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define NH_HD __host__ __device__
#else
#define NH_HD
#endif

namespace nerfhip {
namespace jpeg {

// natural (row-major) index of the k-th coefficient in zigzag order
NH_HD inline int zigzag(int k) {
    constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k];
}

constexpr int kLook = 9;                 // bits resolved by one table lookup

struct HuffTable {
    bool present = false;
    uint16_t look[1 << kLook];           // (length << 8) | symbol for codes of up to kLook bits, 0 = longer or invalid
    int32_t maxcode[18];                 // largest code of each length (-1: none), canonical decoding for the longer ones
    int32_t valptr[17];
    int32_t mincode[17];
    uint8_t symbols[256];
};
static_assert(sizeof(HuffTable) % 4 == 0, "tables are staged in LDS dword by dword");

// counts[16] + symbols[256] -> decoding tables.  False when the counts describe no prefix code (over-subscribed or > 256 symbols).
NH_HD inline bool build_table(const uint8_t* def, HuffTable& t) {
    int total = 0;
    for (int l = 0; l < 16; ++l) total += def[l];
    if (total < 1 || total > 256) return false;
    for (int i = 0; i < 256; ++i) t.symbols[i] = def[16 + i];
    for (int i = 0; i < (1 << kLook); ++i) t.look[i] = 0;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = def[l - 1];
        t.valptr[l] = k;
        t.mincode[l] = code;
        if (code + n > (1 << l)) return false;
        for (int i = 0; i < n; ++i, ++k, ++code) {
            if (l <= kLook) {
                const int first = code << (kLook - l);
                for (int j = 0; j < (1 << (kLook - l)); ++j) t.look[first + j] = (uint16_t)((l << 8) | t.symbols[k]);
            }
        }
        t.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.present = true;
    return true;
}

// ---- the split decoder's view of one image ---------------------------------------------------------------------------------------
// The data bytes of a scan, stuffing and markers removed, as big-endian bit stream: `words` dwords of the buffer may be read.
struct Segment {
    const uint32_t* data;                // 4-byte aligned
    int64_t words;
};

// The 32 bits from bit position p (MSB first).  Bits at or behind `valid_end` read as zero, and no dword outside [0, words) is
// touched.  p >= 0.
NH_HD inline uint32_t fetch32(const Segment& s, int64_t p, int64_t valid_end) {
    if (p >= valid_end) return 0;
    const int64_t w = p >> 5;
    const uint32_t a = w < s.words ? s.data[w] : 0u, b = w + 1 < s.words ? s.data[w + 1] : 0u;
    // the bytes are in stream order, the machine is little-endian
    const uint64_t hi = ((a & 0xffu) << 24) | ((a & 0xff00u) << 8) | ((a >> 8) & 0xff00u) | (a >> 24);
    const uint64_t lo = ((b & 0xffu) << 24) | ((b & 0xff00u) << 8) | ((b >> 8) & 0xff00u) | (b >> 24);
    uint32_t v = (uint32_t)((((hi << 32) | lo) << (p & 31)) >> 32);
    const int64_t avail = valid_end - p;
    if (avail < 32) v &= ~0u << (32 - (int)avail);
    return v;
}

// One Huffman code at the top of `bits`: the symbol and its length, or length 0 for a code the table does not hold.
NH_HD inline int lookup(const HuffTable& t, uint32_t bits, int& len) {
    const uint32_t e = t.look[bits >> (32 - kLook)];
    if (e) {
        len = (int)(e >> 8);
        return (int)(e & 255);
    }
    const int32_t code16 = (int32_t)(bits >> 16);
    for (int l = kLook + 1; l <= 16; ++l) {
        const int32_t code = code16 >> (16 - l);
        if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l]) {
            len = l;
            return t.symbols[t.valptr[l] + code - t.mincode[l]];
        }
    }
    len = 0;
    return -1;
}

// s extra bits at the top of `bits` -> the signed value (libjpeg's EXTEND); s in 1..15
NH_HD inline int extend(uint32_t bits, int s) {
    const int v = (int)(bits >> (32 - s));
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The decoder state between two symbols.
struct State {
    int64_t p;                           // bit position inside the image's segment
    int slot;                            // block inside the MCU, which selects the component and so the tables
    int k;                               // next zigzag index: 0 = the block's DC symbol comes next
};

// What one symbol did.
struct Symbol {
    bool finished;                       // the symbol ended its block
    bool bad;                            // what the sequential decoder answers with NERFHIP_E_DATA: an invalid code, a DC size above
                                         // 11, an AC size above 10, a coefficient behind index 63
    bool has_value;                      // `value` belongs at zigzag index `at` (0: the DC difference)
    int at;
    int value;
};

// The tables of one image's blocks by slot, as 4-bit fields (an array indexed by the slot would live in scratch memory on the
// device): bits 4 * slot of dc_ids / ac_ids hold the index into `tables` (DC: 0..3, AC: 4..7).
struct SlotTables {
    const HuffTable* tables;             // the image's 8 tables
    uint32_t dc_ids, ac_ids;
    int n_slots;                         // blocks per MCU, 1..6
};

// One symbol from state `st`, which advances.  A symbol consumes 1..31 bits.  An invalid code (or a DC size above 11) skips one bit and
// leaves slot and k alone, so that a speculative walk goes on and falls into step; a run past index 63 ends the block.
NH_HD inline Symbol step(const Segment& seg, int64_t valid_end, const SlotTables& tb, State& st) {
    Symbol out = {false, false, false, 0, 0};
    const uint32_t bits = fetch32(seg, st.p, valid_end);
    int len;
    if (st.k == 0) {
        const int s = lookup(tb.tables[(tb.dc_ids >> (4 * st.slot)) & 15], bits, len);
        if (s < 0 || s > 11) {
            out.bad = true;
            st.p += 1;
            return out;
        }
        out.has_value = true;
        out.value = s ? extend(bits << len, s) : 0;
        st.p += len + s;
        st.k = 1;
        return out;
    }
    const int rs = lookup(tb.tables[(tb.ac_ids >> (4 * st.slot)) & 15], bits, len);
    if (rs < 0) {
        out.bad = true;
        st.p += 1;
        return out;
    }
    const int r = rs >> 4, s = rs & 15;
    st.p += len + s;
    if (s == 0) {
        if (r == 15) {
            st.k += 16;
            out.finished = st.k > 63;
        } else {
            out.finished = true;         // end of block
        }
    } else {
        st.k += r;
        if (st.k > 63 || s > 10) out.bad = true;
        if (st.k <= 63) {
            out.has_value = true;
            out.at = st.k;
            out.value = extend(bits << len, s);
            ++st.k;
        }
        out.finished = st.k > 63;
    }
    if (out.finished) {
        st.k = 0;
        st.slot = st.slot + 1 == tb.n_slots ? 0 : st.slot + 1;
    }
    return out;
}

// A subsequence's record: the state behind its last symbol and the blocks it finished, in one 64-bit word that is stored whole.
NH_HD inline uint64_t pack_record(const State& st, int blocks) {
    return (uint64_t)(uint32_t)st.p | ((uint64_t)st.slot << 32) | ((uint64_t)st.k << 35) | ((uint64_t)blocks << 41);
}
NH_HD inline State record_state(uint64_t r) {
    State st;
    st.p = (int64_t)(uint32_t)r;
    st.slot = (int)((r >> 32) & 7);
    st.k = (int)((r >> 35) & 63);
    return st;
}
NH_HD inline int record_blocks(uint64_t r) { return (int)(r >> 41); }

// Every symbol that starts before `end` (the subsequence's end, at most the interval's valid end), from `st`; returns the
// record.  At most end - st.p steps, as every symbol consumes a bit.
NH_HD inline uint64_t walk(const Segment& seg, int64_t end, int64_t valid_end, const SlotTables& tb, State st) {
    int blocks = 0;
    while (st.p < end) blocks += step(seg, valid_end, tb, st).finished ? 1 : 0;
    return pack_record(st, blocks);
}

// ---- byte classes of a raw scan (what BitReader::fill and the interval cut of the sequential decoder do, restated per byte) -------
enum ByteClass { kData = 0, kSkip = 1, kRestart = 2, kStop = 3 };

// kData: an entropy-coded byte.  kSkip: the stuffed 00 behind FF, or a restart marker's second byte.  kRestart: the FF of FF D0..D7.
// kStop: any other FF (another marker, FF FF, a lone FF at the end): the interval's data ends in front of it.
NH_HD inline int classify(const uint8_t* scan, int64_t n, int64_t i) {
    const int b = scan[i];
    if (b == 0xff) {
        if (i + 1 >= n) return kStop;
        const int next = scan[i + 1];
        return next == 0 ? kData : ((next >= 0xd0 && next <= 0xd7) ? kRestart : kStop);
    }
    if (i > 0 && scan[i - 1] == 0xff && (b == 0 || (b >= 0xd0 && b <= 0xd7))) return kSkip;
    return kData;
}

}  // namespace jpeg
}  // namespace nerfhip

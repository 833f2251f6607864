// Inflating one zlib stream (RFC 1950 / 1951) by 64 lanes that work in alternating phases, written once for both sides: the
// kernel of inflate.hip runs the phases on one wave with a barrier between them and `Core` in LDS, nerfhip_inflate_host runs the
// same functions on the host with the lanes in lockstep.  DESIGN.md §16 holds the algorithm and what bounds each loop.
//
//   refill        all lanes: the next kInBytes of the stream into `in` (bytes outside the stream read as zeros)
//   decode_batch  lane 0: headers and Huffman symbols -> up to kTokens tokens (literals; matches and stored runs) of up to
//                 kBatchBytes output bytes, each with its position; every value is validated before a token is written
//   place / copy  all lanes: the literals at once, then the matches and stored runs in order, into the ring
//   flush         all lanes: whole 16-byte pieces of the ring to the output, and their Adler-32 terms
//   build         all lanes: the two decoding tables of a block from its code lengths
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/nerfhip.h"

#define NHI_HD __host__ __device__ inline

namespace nerfhip {
namespace inflate {

constexpr int kLanes = 64;
constexpr int kRing = 1 << 16;            // the 32 KiB window, a batch's output and the unflushed tail, addressed modulo
constexpr int kRingMask = kRing - 1;
constexpr int kWindow = 32768;
constexpr int kInBytes = 4096;            // stream bytes staged at a time
constexpr int kStepBytes = 576;           // the most one step of lane 0 reads: a dynamic header, 17 + 57 + 316 * 14 bits = 563 bytes
constexpr int kRefillBelow = 2048;        // refill when fewer staged bytes than this lie ahead
constexpr int kTokens = 256;
constexpr int kBatchBytes = 16384;
constexpr int kMaxMatch = 258;
constexpr uint32_t kAdlerMod = 65521;
constexpr int64_t kMaxStream = (int64_t)1 << 27;      // bit positions, a step's overshoot included, stay below 2^31
// a flush covers the batch and fewer than 16 bytes kept back: a lane's weighted Adler sum must fit 32 bits
constexpr int kFlushMost = kBatchBytes + 16;
static_assert((uint64_t)255 * kFlushMost * (kFlushMost / kLanes + 48) < ((uint64_t)1 << 32), "a lane's Adler sums must fit 32 bits");
static_assert(kWindow + kBatchBytes + 16 <= kRing, "a batch must not overwrite the window or the unflushed tail");
static_assert(kStepBytes < kRefillBelow && kRefillBelow < kInBytes, "a refill must leave room for a step");

enum Mode { kZlibHeader, kBlockHeader, kStored, kCodes, kBuildFixed, kBuildDynamic, kTrailer, kDone };
enum Kind { kLiteral = 0, kMatch = 1, kRun = 2 };

template <int NSYM, int FB>
struct Huff {
    static constexpr int n_sym = NSYM, fast_bits = FB;
    uint16_t count[16];                   // codes of each length
    uint16_t symbol[NSYM];                // the symbols in canonical order
    uint16_t fast[1 << FB];               // the next FB bits -> length << 9 | symbol, 0: longer than FB bits, or no code
};

struct Copy {
    uint32_t kind_len;                    // kind << 30 | length
    uint32_t from;                        // match: distance; run: the stream byte it starts at
    uint32_t pos;                         // output position inside the batch
    uint32_t pad;
};

struct Core {
    alignas(16) uint8_t ring[kRing];
    alignas(16) uint32_t in[kInBytes / 4 + 2];
    alignas(16) Copy copy[kTokens];       // the batch's matches and runs, in order
    uint32_t lits[kTokens];               // the batch's literals: position inside the batch << 8 | byte
    uint32_t part_a[kLanes], part_b[kLanes];
    Huff<288, 10> lit;
    Huff<32, 9> dist;
    Huff<19, 1> cl;
    uint8_t lens[320];
    uint8_t cl_lens[20];
    int64_t out_pos;                      // bytes resolved into the ring
    int64_t flushed;                      // bytes stored to the output
    int32_t in_base;                      // the stream byte in[0] starts at
    int32_t bitpos, mode, last, stored_left, status;
    int32_t nlit, nseq, batch_bytes, hlit, hdist;
    int32_t flush_to_final;               // the coming flush is the last one
    int32_t finished;
    uint32_t adler_want, a, b;
};

struct Stream {
    const uint8_t* data;                  // the stream's first byte
    int64_t nbytes;
    uint8_t* out;                         // the stream's first output byte
    int64_t out_bytes;
    int mis;                              // out's address modulo 16: the ring is addressed by (mis + position), so that 16-byte
};                                        // aligned output addresses are 16-byte aligned ring addresses

NHI_HD void init(Core& c, int lane) {
    if (lane != 0) return;
    c.out_pos = c.flushed = 0;
    c.in_base = -kInBytes;                // nothing staged
    c.bitpos = 0;
    c.mode = kZlibHeader;
    c.last = c.stored_left = c.status = 0;
    c.nlit = c.nseq = c.batch_bytes = c.hlit = c.hdist = 0;
    c.flush_to_final = c.finished = 0;
    c.adler_want = 0;
    c.a = 1;
    c.b = 0;
}

// ---- the staged input ------------------------------------------------------------------------------------------------------------
NHI_HD bool need_refill(const Core& c) { return (c.bitpos >> 3) - c.in_base + kRefillBelow > kInBytes; }

// the 4 stream bytes at p (address 4-byte aligned); bytes outside [0, n) are zeros and are not read
NHI_HD uint32_t load_word(const uint8_t* data, int64_t n, int64_t p) {
    if (p >= 0 && p + 4 <= n) return *(const uint32_t*)(data + p);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (p + k >= 0 && p + k < n) v |= (uint32_t)data[p + k] << (8 * k);
    return v;
}

NHI_HD void refill(Core& c, const Stream& s, int lane) {
    const int32_t start = c.bitpos >> 3;
    const int32_t base = start - (int32_t)(((uintptr_t)s.data + (uintptr_t)start) & 3);
    for (int w = lane; w < kInBytes / 4 + 2; w += kLanes) c.in[w] = load_word(s.data, s.nbytes, (int64_t)base + 4 * w);
    if (lane == kLanes - 1) c.in_base = base;            // (the loads above do not read it)
}

// the 32 bits at bit position `bitpos`, which a step keeps inside the staged bytes
NHI_HD uint32_t peek(const Core& c, int32_t bitpos) {
    const uint32_t rel = (uint32_t)(bitpos - 8 * c.in_base);
    const uint32_t w = rel >> 5, sh = rel & 31;
    const uint64_t two = (uint64_t)c.in[w + 1] << 32 | c.in[w];
    return (uint32_t)(two >> sh);
}

// ---- canonical codes -------------------------------------------------------------------------------------------------------------
// The symbol whose code the low bits of `bits` start with (the code's first bit is bit 0), its length in `len`; -1: no code of up
// to 15 bits matches (an unassigned code of an incomplete set).
template <typename H>
NHI_HD int decode_slow(const H& h, uint32_t bits, int& len) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int count = h.count[l];
        if (code - count < first) {
            const int at = index + (code - first);
            len = l;
            return at >= 0 && at < H::n_sym ? h.symbol[at] : -1;
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

template <typename H>
NHI_HD int decode(const H& h, uint32_t bits, int& len) {
    const uint32_t e = h.fast[bits & ((1u << H::fast_bits) - 1u)];
    if (e) {
        len = (int)(e >> 9);
        return (int)(e & 511);
    }
    return decode_slow(h, bits, len);
}

// codes of length l among lens[0 .. n)
template <typename H>
NHI_HD void count_pass(H& h, const uint8_t* lens, int n, int l) {
    int cnt = 0;
    for (int s = 0; s < n; ++s) cnt += lens[s] == l ? 1 : 0;
    h.count[l] = (uint16_t)cnt;
}

// What zlib's inflate_table accepts: not over-subscribed; incomplete only as the single code of one bit (never for the
// code-length code); no code at all passes here and fails at the first symbol.
template <typename H>
NHI_HD bool accept(const H& h, bool code_length_code) {
    int left = 1, max = 0;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - h.count[l];
        if (left < 0) return false;
        if (h.count[l]) max = l;
    }
    if (max == 0) return true;
    return !(left > 0 && (code_length_code || max != 1));
}

// the symbols of length l to their place in canonical order (an accepted set has at most n <= n_sym codes)
template <typename H>
NHI_HD void place_pass(H& h, const uint8_t* lens, int n, int l) {
    int at = 0;
    for (int k = 1; k < l; ++k) at += h.count[k];
    for (int s = 0; s < n; ++s)
        if (lens[s] == l && at < H::n_sym) h.symbol[at++] = (uint16_t)s;
}

template <typename H>
NHI_HD void fast_pass(H& h, int lane, int lanes) {
    for (int e = lane; e < (1 << H::fast_bits); e += lanes) {
        int len = 0;
        const int sym = decode_slow(h, (uint32_t)e, len);
        h.fast[e] = (sym >= 0 && len <= H::fast_bits) ? (uint16_t)(len << 9 | sym) : (uint16_t)0;
    }
}

// The tables of the block whose lengths stand in c.lens: phase 0 .. 4, a barrier behind each.
constexpr int kBuildPhases = 5;
NHI_HD void build_phase(Core& c, int phase, int lane) {
    if (phase == 0) {
        if (c.mode == kBuildFixed)
            for (int i = lane; i < 320; i += kLanes) c.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
        if (c.mode == kBuildFixed && lane == 0) {
            c.hlit = 288;
            c.hdist = 32;
        }
    } else if (phase == 1) {
        if (lane < 16) count_pass(c.lit, c.lens, c.hlit, lane);
        else if (lane < 32) count_pass(c.dist, c.lens + c.hlit, c.hdist, lane - 16);
    } else if (phase == 2) {
        if (lane == 0 && !(accept(c.lit, false) && accept(c.dist, false))) c.status = NERFHIP_E_DATA;
    } else if (phase == 3) {
        if (c.status != 0) return;
        if (lane >= 1 && lane < 16) place_pass(c.lit, c.lens, c.hlit, lane);
        else if (lane >= 17 && lane < 32) place_pass(c.dist, c.lens + c.hlit, c.hdist, lane - 16);
    } else {
        if (c.status != 0) return;
        fast_pass(c.lit, lane, kLanes);
        fast_pass(c.dist, lane, kLanes);
        if (lane == 0) c.mode = kCodes;   // (read again only behind the barrier)
    }
}

// ---- lane 0: the sequential part -------------------------------------------------------------------------------------------------
// The header of a dynamic block behind its three type bits: the counts, the code-length code (built by this lane alone), the
// code lengths into c.lens.  Reads at most 14 + 57 + 316 * 14 bits.
NHI_HD int read_dynamic(Core& c, int32_t& bitpos) {
    uint32_t w = peek(c, bitpos);
    const int hlit = (int)(w & 31) + 257, hdist = (int)((w >> 5) & 31) + 1, hclen = (int)((w >> 10) & 15) + 4;
    bitpos += 14;
    if (hlit > 286 || hdist > 30) return NERFHIP_E_DATA;
    const uint64_t order_lo = 0x022caa324e804a30ull;     // 16 17 18 0 8 7 9 6 10 5 11 4, five bits each from the low end
    const uint64_t order_hi = 0x00000003c2e1346cull;     // 12 3 13 2 14 1 15
    for (int i = 0; i < 19; ++i) c.cl_lens[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        const int sym = (int)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31);
        c.cl_lens[sym < 19 ? sym : 0] = (uint8_t)(peek(c, bitpos) & 7);
        bitpos += 3;
    }
    for (int l = 0; l < 16; ++l) count_pass(c.cl, c.cl_lens, 19, l);
    if (!accept(c.cl, true)) return NERFHIP_E_DATA;
    for (int l = 1; l < 16; ++l) place_pass(c.cl, c.cl_lens, 19, l);
    const int total = hlit + hdist;
    int have = 0;
    while (have < total) {                               // every round adds at least one length
        w = peek(c, bitpos);
        int l = 0;
        const int sym = decode_slow(c.cl, w, l);
        if (sym < 0) return NERFHIP_E_DATA;
        bitpos += l;
        w >>= l;
        if (sym < 16) {
            c.lens[have++] = (uint8_t)sym;
            continue;
        }
        int prev = 0, rep;
        if (sym == 16) {
            if (have == 0) return NERFHIP_E_DATA;
            prev = c.lens[have - 1];
            rep = 3 + (int)(w & 3);
            bitpos += 2;
        } else if (sym == 17) {
            rep = 3 + (int)(w & 7);
            bitpos += 3;
        } else {
            rep = 11 + (int)(w & 127);
            bitpos += 7;
        }
        if (have + rep > total) return NERFHIP_E_DATA;
        for (; rep > 0; --rep) c.lens[have++] = (uint8_t)prev;
    }
    if (c.lens[256] == 0) return NERFHIP_E_DATA;         // no end-of-block code
    c.hlit = hlit;
    c.hdist = hdist;
    return 0;
}

// Steps until the batch is full, the staged bytes run low, tables are to be built, or the stream ends.  Every step consumes at
// least one bit; the caller has refilled, so at least one step runs.  Inside a Huffman block the bits come from a 64-bit
// register that is topped up a word at a time, so a literal costs one table read.
NHI_HD void decode_batch(Core& c, const Stream& s) {
    int32_t bitpos = c.bitpos, mode = c.mode, status = c.status, nlit = 0, nseq = 0, bytes = 0;
    const int32_t in_base = c.in_base, nbits = (int32_t)(8 * s.nbytes);       // (a stream has at most 2^27 bytes)
    const int64_t out_pos = c.out_pos, left = s.out_bytes - out_pos;
    // what limits a token, as 32-bit numbers: the output still to come and the bytes produced, both cut off far above a batch
    const int32_t cap = (int32_t)(left < (1 << 20) ? left : (1 << 20)), have = (int32_t)(out_pos < (1 << 20) ? out_pos : (1 << 20));
    while (status == 0 && mode != kDone && mode != kBuildFixed && mode != kBuildDynamic) {
        if ((bitpos >> 3) - in_base + kStepBytes > kInBytes) break;
        if (nlit + nseq == kTokens || bytes + kMaxMatch > kBatchBytes) break;
        if (mode == kCodes) {
            const uint32_t rel = (uint32_t)(bitpos - 8 * in_base);
            uint32_t word = rel >> 5;
            uint64_t buf = ((uint64_t)c.in[word + 1] << 32 | c.in[word]) >> (rel & 31);
            int cnt = 64 - (int)(rel & 31);
            word += 2;
            while (status == 0 && mode == kCodes) {      // the same two conditions as above, per token
                if ((bitpos >> 3) - in_base + kStepBytes > kInBytes) break;
                if (nlit + nseq == kTokens || bytes + kMaxMatch > kBatchBytes) break;
                if (cnt < 32) {                          // (word stays below the step bound's (kInBytes - kStepBytes) / 4 + 4)
                    buf |= (uint64_t)c.in[word++] << cnt;
                    cnt += 32;
                }
                int l = 0;
                const int sym = decode(c.lit, (uint32_t)buf, l);
                if (sym < 0 || sym >= 286) {
                    status = NERFHIP_E_DATA;
                } else if (sym < 256) {
                    if (bytes + 1 > cap) status = NERFHIP_E_DATA;
                    else c.lits[nlit++] = (uint32_t)bytes++ << 8 | (uint32_t)sym;
                } else if (sym == 256) {
                    mode = c.last ? kTrailer : kBlockHeader;
                } else {                                 // 15 bits of code and 5 of extra are there
                    const int k = sym - 257;
                    const int lext = k < 8 || k == 28 ? 0 : (k >> 2) - 1;
                    const int len = (k < 8 ? 3 + k : k == 28 ? 258 : 3 + ((4 + (k & 3)) << lext)) + (int)((uint32_t)(buf >> l) & ((1u << lext) - 1u));
                    l += lext;
                    buf >>= l;
                    cnt -= l;
                    bitpos += l;
                    if (cnt < 32) {
                        buf |= (uint64_t)c.in[word++] << cnt;
                        cnt += 32;
                    }
                    l = 0;
                    const int ds = decode(c.dist, (uint32_t)buf, l);
                    if (ds < 0 || ds >= 30) {
                        status = NERFHIP_E_DATA;
                    } else {                             // 15 + 13 bits are there
                        const int dext = ds < 4 ? 0 : (ds >> 1) - 1;
                        const int dist = (ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << dext)) + (int)((uint32_t)(buf >> l) & ((1u << dext) - 1u));
                        l += dext;
                        // the distance is at most 32768 by its code; only the bytes produced so far limit it further
                        if (dist > have + bytes || bytes + len > cap) {
                            status = NERFHIP_E_DATA;
                        } else {
                            c.copy[nseq++] = Copy{(uint32_t)kMatch << 30 | (uint32_t)len, (uint32_t)dist, (uint32_t)bytes, 0};
                            bytes += len;
                        }
                    }
                }
                buf >>= l;                               // (l is 0 where no code matched)
                cnt -= l;
                bitpos += l;
                if (bitpos > nbits) status = NERFHIP_E_DATA;
            }
            continue;
        }
        uint32_t w = peek(c, bitpos);
        if (mode == kZlibHeader) {
            const uint32_t cmf = w & 255, flg = (w >> 8) & 255;
            bitpos += 16;
            if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) status = NERFHIP_E_DATA;
            mode = kBlockHeader;
        } else if (mode == kBlockHeader) {
            c.last = (int32_t)(w & 1);
            const int type = (int)((w >> 1) & 3);
            bitpos += 3;
            if (type == 0) {
                bitpos = (bitpos + 7) & ~7;
                w = peek(c, bitpos);
                bitpos += 32;
                const int32_t len = (int32_t)(w & 0xffff);
                if ((w >> 16) != (~w & 0xffff) || (bitpos >> 3) + (int64_t)len > s.nbytes) status = NERFHIP_E_DATA;
                c.stored_left = len;
                mode = len > 0 ? kStored : (c.last ? kTrailer : kBlockHeader);
            } else if (type == 1) {
                mode = kBuildFixed;
            } else if (type == 2) {
                status = read_dynamic(c, bitpos);
                mode = kBuildDynamic;
            } else {
                status = NERFHIP_E_DATA;
            }
        } else if (mode == kStored) {
            const int32_t room = kBatchBytes - bytes, n = c.stored_left < room ? c.stored_left : room;       // n >= 1
            if (bytes + n > cap) {
                status = NERFHIP_E_DATA;
            } else {
                c.copy[nseq++] = Copy{(uint32_t)kRun << 30 | (uint32_t)n, (uint32_t)(bitpos >> 3), (uint32_t)bytes, 0};
                bytes += n;
                bitpos += 8 * n;
                c.stored_left -= n;
                if (c.stored_left == 0) mode = c.last ? kTrailer : kBlockHeader;
            }
        } else {                                         // kTrailer
            bitpos = (bitpos + 7) & ~7;
            w = peek(c, bitpos);
            bitpos += 32;
            c.adler_want = (w & 255) << 24 | ((w >> 8) & 255) << 16 | ((w >> 16) & 255) << 8 | (w >> 24);
            mode = kDone;
        }
        if (bitpos > nbits) status = NERFHIP_E_DATA;     // the step read bits the stream does not have
    }
    c.bitpos = bitpos;
    c.mode = mode;
    c.status = status;
    c.nlit = nlit;
    c.nseq = nseq;
    c.batch_bytes = bytes;
    c.flush_to_final = mode == kDone && status == 0;
}

// ---- all lanes: tokens -> ring ---------------------------------------------------------------------------------------------------
NHI_HD void place_literals(Core& c, const Stream& s, int lane) {
    const int64_t base = s.mis + c.out_pos;
    for (int t = lane; t < c.nlit; t += kLanes) {
        const uint32_t lit = c.lits[t];
        c.ring[(base + (lit >> 8)) & kRingMask] = (uint8_t)lit;
    }
}

// match or run i of the batch; the ones before it are in the ring, whose position `base` = mis + out_pos holds the batch's first
// byte.  A match reads only bytes in front of its first one (an overlapping copy repeats its first `dist` bytes), so its lanes do
// not depend on each other.
NHI_HD void copy_token(Core& c, const Stream& s, int64_t base, int i, int lane) {
    const Copy t = c.copy[i];
    const int len = (int)(t.kind_len & 0xffff);
    const int64_t dst = base + t.pos;
    if ((t.kind_len >> 30) == kMatch) {
        const int dist = (int)t.from;
        const int64_t src = dst - dist;
        for (int j = lane; j < len; j += kLanes) c.ring[(dst + j) & kRingMask] = c.ring[(src + (dist >= len ? j : j % dist)) & kRingMask];
    } else {
        const uint8_t* src = s.data + t.from;            // decode_batch checked that the run lies inside the stream
        for (int j = lane; j < len; j += kLanes) c.ring[(dst + j) & kRingMask] = src[j];
    }
}

// ---- all lanes: ring -> output -----------------------------------------------------------------------------------------------------
// The bytes [flushed, upto) go out: upto is everything on the last flush, else the last position whose address is a multiple of
// 16.  Single bytes up to the first such address and behind the last, 16-byte pieces between.  Every lane leaves the Adler terms
// of its bytes: sum d and sum (upto - position) d, below 65521.
NHI_HD int64_t flush_end(const Core& c, const Stream& s) {
    const int64_t produced = c.out_pos + c.batch_bytes;
    if (c.flush_to_final) return produced;
    const int64_t upto = ((s.mis + produced) & ~(int64_t)15) - s.mis;
    return upto > c.flushed ? upto : c.flushed;
}

NHI_HD void flush(Core& c, const Stream& s, int lane) {
    const int64_t from = c.flushed, upto = flush_end(c, s);
    int64_t v0 = ((s.mis + from + 15) & ~(int64_t)15) - s.mis, v1 = ((s.mis + upto) & ~(int64_t)15) - s.mis;
    if (v0 > upto) v0 = upto;
    if (v1 < v0) v1 = v0;
    uint32_t sa = 0, sb = 0;
    for (int64_t o = from + lane; o < v0; o += kLanes) {
        const uint32_t d = c.ring[(s.mis + o) & kRingMask];
        s.out[o] = (uint8_t)d;
        sa += d;
        sb += (uint32_t)(upto - o) * d;
    }
    for (int64_t o = v0 + 16 * (int64_t)lane; o < v1; o += 16 * kLanes) {
        const uint4 q = *(const uint4*)&c.ring[(s.mis + o) & kRingMask];
        *(uint4*)(s.out + o) = q;
        const uint32_t words[4] = {q.x, q.y, q.z, q.w};
        for (int k = 0; k < 16; ++k) {
            const uint32_t d = (words[k >> 2] >> (8 * (k & 3))) & 255;
            sa += d;
            sb += (uint32_t)(upto - o - k) * d;
        }
    }
    for (int64_t o = v1 + lane; o < upto; o += kLanes) {
        const uint32_t d = c.ring[(s.mis + o) & kRingMask];
        s.out[o] = (uint8_t)d;
        sa += d;
        sb += (uint32_t)(upto - o) * d;
    }
    c.part_a[lane] = sa % kAdlerMod;
    c.part_b[lane] = sb % kAdlerMod;
}

// lane 0 behind the flush: a' = a + sum d, b' = b + n a + sum (n - j) d over the n bytes that went out; the verdict at the end
NHI_HD void after_flush(Core& c, const Stream& s) {
    const int64_t upto = flush_end(c, s);
    uint64_t sa = 0, sb = 0;
    for (int l = 0; l < kLanes; ++l) {
        sa += c.part_a[l];
        sb += c.part_b[l];
    }
    const uint64_t n = (uint64_t)(upto - c.flushed);     // below 2^15
    c.b = (uint32_t)((c.b + n * c.a + sb) % kAdlerMod);
    c.a = (uint32_t)((c.a + sa) % kAdlerMod);
    c.flushed = upto;
    c.out_pos += c.batch_bytes;
    c.batch_bytes = 0;
    if (c.status != 0) {
        c.finished = 1;
    } else if (c.mode == kDone) {
        if (c.out_pos != s.out_bytes || (c.b << 16 | c.a) != c.adler_want) c.status = NERFHIP_E_DATA;
        c.finished = 1;
    }
}

// 0, or NERFHIP_E_BADARG for offsets that are not increasing inside total_bytes or a stream longer than kMaxStream
NHI_HD int check_stream(const int64_t* offsets, int64_t total_bytes, int i) {
    const int64_t o0 = offsets[i], o1 = offsets[i + 1];
    return (o0 < 0 || o1 < o0 || o1 > total_bytes || o1 - o0 > kMaxStream) ? NERFHIP_E_BADARG : 0;
}

}  // namespace inflate
}  // namespace nerfhip

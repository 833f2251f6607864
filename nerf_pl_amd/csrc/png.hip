// The PNG file of the reference's eval loop (eval.py:138 `imageio.imwrite('{i:03d}.png')`) encoded on the device: per scanline
// the filter of the smallest absolute sum, the filtered stream cut into strips that each become one dynamic-Huffman deflate
// block of literals and distance-1 matches, and the stream's Adler-32.  The exact definition, the strip length and the byte
// layout of the result: DESIGN.md §15 and include/nerfhip.h; tests/png_ref.py restates it in numpy.  The host writes the
// container (signature, chunks, CRC-32) around the data.  The bit writer, the scan of the strips' bit lengths and the gather of
// the bytes are the ones gif.hip has: strip_bits.h, block_scan.h.
#include "block_scan.h"
#include "common.h"
#include "png_huff.h"
#include "strip_bits.h"

namespace {

using nerfhip::block_excl_scan;
using nerfhip::carve;
using nerfhip::HuffScratch;
using StripBits = nerfhip::BitWriter<nerfhip::OrWord>;      // into the strip's zeroed words in LDS, several threads at once

constexpr int kBlock = 256;                       // threads of the filter, strip and gather kernels
constexpr int kScanBlock = 1024;                  // the one workgroup per stream that scans strip lengths
constexpr int kStrip = NERFHIP_PNG_STRIP;
constexpr int kChunk = kStrip / kBlock;           // consecutive bytes per thread of the strip kernel
constexpr int kLit = 286, kCl = 19;
constexpr uint32_t kAdler = 65521;
// A strip's bits: 17 of block header, 19 x 3 of code-length code lengths, at most 287 code-length symbols of at most 7 + 7 bits,
// at most 15 bits per byte (a match costs at most 15 + 5 + 1 bits and stands for 3 bytes or more), 15 of end-of-block.
constexpr int kHeadBits = 17 + 3 * kCl + (kLit + 1) * 14 + 15;
constexpr int kStripBits = kHeadBits + 15 * kStrip;
constexpr int kStripWords = (kStripBits + 31) / 32;

static_assert(kStrip % kBlock == 0, "a strip is a whole number of bytes per thread");
static_assert(kStrip <= 32767, "positions in a strip are kept in 16 bits");
// Adler-32 per thread: sum d <= 255 * kChunk, sum (n - j) d <= 255 * kStrip * kChunk < 2^32; both are reduced below 65521 before
// the workgroup adds kBlock of them in 32 bits.
static_assert((uint64_t)255 * kStrip * kChunk < ((uint64_t)1 << 32), "a thread's Adler sums must fit 32 bits");

__constant__ unsigned char kClOrder[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__host__ __device__ inline int64_t strips_of(int64_t bytes) { return (bytes + kStrip - 1) / kStrip; }

struct PngWs {
    int32_t* bitlen;       // (n, S) bits of each strip, -1: its bit buffer would not hold them
    int64_t* off;          // (n, S) first bit of each strip in the stream's deflate data
    int64_t* total;        // (n) bits of the stream's deflate data
    uint32_t* sum_a;       // (n, S) sum d of the strip's bytes, below 65521
    uint32_t* sum_b;       // (n, S) sum (count - j) d, below 65521
    uint32_t* bits;        // (n, S, kStripWords)
};

__host__ __device__ inline PngWs png_ws(void* base, int64_t n, int64_t bytes, size_t* size) {
    const int64_t S = strips_of(bytes);
    char* p = (char*)base;
    PngWs w;
    w.bitlen = carve<int32_t>(p, (size_t)n * S);
    w.off = carve<int64_t>(p, (size_t)n * S);
    w.total = carve<int64_t>(p, (size_t)n);
    w.sum_a = carve<uint32_t>(p, (size_t)n * S);
    w.sum_b = carve<uint32_t>(p, (size_t)n * S);
    w.bits = carve<uint32_t>(p, (size_t)n * S * kStripWords);
    if (size) *size = (size_t)(p - (char*)base);
    return w;
}

__host__ __device__ inline int64_t data_stride(int64_t bytes) { return (strips_of(bytes) * kHeadBits + 15 * bytes + 7) / 8; }

// ---- filter ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filtered(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255;
}

__device__ __forceinline__ int cost_of(int v) { return v < 128 ? v : 256 - v; }

// One wave per scanline: the five sums in one pass over the row and its predecessor, then the winner is formed again and stored.
__global__ void __launch_bounds__(kBlock) png_filter_rows(const unsigned char* __restrict__ images, int H, int64_t row_bytes, int bpp,
                                                         unsigned char* __restrict__ streams) {
    const int lane = threadIdx.x & 63;
    const int64_t y = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (y >= H) return;                                   // (whole waves leave: the shuffles below see full waves)
    const int64_t img = blockIdx.y;
    const unsigned char* cur = images + (img * H + y) * row_bytes;
    const unsigned char* up = cur - row_bytes;
    const bool has_up = y > 0;
    unsigned sum[5] = {0, 0, 0, 0, 0};
    for (int64_t i = lane; i < row_bytes; i += 64) {
        const int x = cur[i];
        const int a = i >= bpp ? cur[i - bpp] : 0;
        const int b = has_up ? up[i] : 0;
        const int c = (has_up && i >= bpp) ? up[i - bpp] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) sum[t] += (unsigned)cost_of(filtered(t, x, a, b, c));
    }
    int best = 0;
    unsigned long long best_sum = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        unsigned long long s = sum[t];                    // at most 128 * row_bytes < 2^38 in all, per lane 1/64 of it: below 2^32
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (t == 0 || s < best_sum) {
            best = t;
            best_sum = s;
        }
    }
    unsigned char* out = streams + (img * H + y) * (row_bytes + 1);
    if (lane == 0) out[0] = (unsigned char)best;
    for (int64_t i = lane; i < row_bytes; i += 64) {
        const int a = i >= bpp ? cur[i - bpp] : 0;
        const int b = has_up ? up[i] : 0;
        const int c = (has_up && i >= bpp) ? up[i - bpp] : 0;
        out[1 + i] = (unsigned char)filtered(best, cur[i], a, b, c);
    }
}

// ---- deflate -----------------------------------------------------------------------------------------------------------------
struct StripState {
    unsigned char bytes[kStrip];
    uint32_t bits[kStripWords];
    uint32_t hist[kLit];
    uint32_t cl_hist[kCl];
    uint16_t code[kLit];               // bit-reversed canonical codes
    uint16_t next_code[16];
    unsigned char len[kLit + 2];       // literal/length lengths, then the one distance length: the code-length sequence
    unsigned char cl_len[kCl], cl_code[kCl];
    short last_start[kBlock], first_start[kBlock];      // per thread: the last / first run start among its bytes
    short wave_max[kBlock / 64], wave_min[kBlock / 64];
    uint32_t sum_a, sum_b;
    int used, head_bits;
    HuffScratch huff;
};

// The tokens of bytes [c0, c1) of a strip of n bytes in the closed form of DESIGN.md §15 step 3.  `start` is the first byte of
// the run that holds c0, `next` the first run start at or behind c1 (n if none).  f(symbol, extra bits, extra value): a literal
// has its value as symbol; a match (distance 1) its length symbol 257..285.
template <typename F>
__device__ __forceinline__ void for_tokens(const unsigned char* bytes, int c0, int c1, int start, int next, F f) {
    int p = start, e = c0;
    for (int j = c0; j < c1; ++j) {
        if (j == e) {                                      // the end of the run that holds j
            if (j > c0 || j == start) p = j;
            const int v = bytes[j];
            e = j + 1;
            while (e < c1 && bytes[e] == v) ++e;
            if (e == c1) e = next;
        }
        const int o = j - p;
        if (o == 0) {
            f((int)bytes[j], 0, 0);
            continue;
        }
        const int q = o - 1, r = e - p - 1, full = r / 258 * 258;
        int len;
        if (q < full) {
            if (q % 258) continue;
            len = 258;
        } else if (r - full >= 3) {
            if (q != full) continue;
            len = r - full;
        } else {
            f((int)bytes[j], 0, 0);
            continue;
        }
        const int l = len - 3;
        if (len == 258) {
            f(285, 0, 0);
        } else if (l < 8) {
            f(257 + l, 0, 0);
        } else {
            const int x = 29 - __clz(l);                   // floor(log2 l) - 2 extra bits
            f(261 + 4 * x + ((l >> x) & 3), x, l & ((1 << x) - 1));
        }
    }
}

// The code-length sequence in the closed form of step 4: a run of L zeros is 18(138) while L >= 138, then 18(L) for L >= 11,
// 17(L) for L >= 3, else L zeros; a run of L equal lengths v is v, then 16(6) while 6 or more remain, 16(r) for r >= 3, else r
// times v.  f(symbol, extra bits, extra value).
template <typename F>
__device__ __forceinline__ void for_cl_tokens(const unsigned char* seq, int n, F f) {
    for (int i = 0; i < n;) {
        const int v = seq[i];
        int L = 1;
        while (i + L < n && seq[i + L] == v) ++L;
        i += L;
        if (v == 0) {
            for (; L >= 138; L -= 138) f(18, 7, 127);
            if (L >= 11) f(18, 7, L - 11);
            else if (L >= 3) f(17, 3, L - 3);
            else for (; L > 0; --L) f(0, 0, 0);
        } else {
            f(v, 0, 0);
            int r = L - 1;
            for (; r >= 6; r -= 6) f(16, 2, 3);
            if (r >= 3) f(16, 2, r - 3);
            else for (; r > 0; --r) f(v, 0, 0);
        }
    }
}

__device__ __forceinline__ uint32_t reversed(uint32_t code, int len) { return __brev(code) >> (32 - len); }

// One workgroup per strip: run starts, tokens and their histogram, code lengths, the block header, the token bits, the strip's
// Adler sums.  Thread 0 does what is sequential (two-queue merge, header) on LDS arrays.
__global__ void __launch_bounds__(kBlock) png_strip(const unsigned char* __restrict__ streams, int64_t stream_bytes, int64_t S, PngWs w) {
    __shared__ StripState st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t img = blockIdx.y, s = blockIdx.x, g = img * S + s;
    const int64_t first = s * kStrip;
    const int n = (int)(stream_bytes - first < kStrip ? stream_bytes - first : kStrip);
    const unsigned char* in = streams + img * stream_bytes + first;
    const int c0 = tid * kChunk < n ? tid * kChunk : n, c1 = c0 + kChunk < n ? c0 + kChunk : n;

    for (int i = tid; i < kStripWords; i += kBlock) st.bits[i] = 0;
    for (int i = tid; i < kLit; i += kBlock) st.hist[i] = 0;
    if (tid < kCl) st.cl_hist[tid] = 0;
    if (tid == 0) st.sum_a = st.sum_b = 0, st.used = 0;
    uint32_t a = 0, b = 0;
    for (int j = c0; j < c1; ++j) {
        const uint32_t d = in[j];
        st.bytes[j] = (unsigned char)d;
        a += d;
        b += (uint32_t)(n - j) * d;
    }
    __syncthreads();
    if (c0 < c1) {
        atomicAdd(&st.sum_a, a % kAdler);
        atomicAdd(&st.sum_b, b % kAdler);
    }
    // run starts: byte 0 and every byte that differs from the one before it
    int last = -1, head = n;
    for (int j = c0; j < c1; ++j)
        if (j == 0 || st.bytes[j] != st.bytes[j - 1]) {
            if (head == n) head = j;
            last = j;
        }
    int pm = last, sm = head;                              // inclusive prefix maximum / suffix minimum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(pm, o, 64), u = __shfl_down(sm, o, 64);
        if (lane >= o) pm = t > pm ? t : pm;
        if (lane + o < 64) sm = u < sm ? u : sm;
    }
    if (lane == 63) st.wave_max[wave] = (short)pm;
    if (lane == 0) st.wave_min[wave] = (short)sm;
    int start = __shfl_up(pm, 1, 64), next = __shfl_down(sm, 1, 64);
    if (lane == 0) start = -1;
    if (lane == 63) next = n;
    __syncthreads();
    for (int k = 0; k < kBlock / 64; ++k) {
        if (k < wave && st.wave_max[k] > start) start = st.wave_max[k];
        if (k > wave && st.wave_min[k] < next) next = st.wave_min[k];
    }
    if (head == c0) start = c0;                            // (the run that holds c0 starts there)
    if (start < 0) start = 0;                              // (only a thread without bytes)

    for_tokens(st.bytes, c0, c1, start, next, [&](int sym, int, int) { atomicAdd(&st.hist[sym], 1u); });
    if (tid == 0) atomicAdd(&st.hist[256], 1u);
    __syncthreads();

    // step 4: literal/length code lengths.  The ranks are one symbol per thread, the merge is thread 0's.
    for (int i = tid; i < kLit; i += kBlock)
        if (st.hist[i]) {
            st.huff.order[nerfhip::huff_rank(st.hist, kLit, i)] = (uint16_t)i;
            atomicAdd(&st.used, 1);
        }
    __syncthreads();
    if (tid == 0) {
        nerfhip::huff_from_order(st.hist, kLit, st.used, 15, st.len, st.huff);
        int n_lit = kLit, matches = 0;
        while (n_lit > 257 && st.len[n_lit - 1] == 0) --n_lit;
        for (int i = 257; i < kLit; ++i) matches |= st.len[i];
        st.len[n_lit] = matches ? 1 : 0;                   // the one distance code: symbol 0, or "all literals"
        const int n_seq = n_lit + 1;
        for_cl_tokens(st.len, n_seq, [&](int sym, int, int) { ++st.cl_hist[sym]; });
        nerfhip::huff_lengths(st.cl_hist, kCl, 7, st.cl_len, st.huff);
        int n_cl = kCl;
        while (n_cl > 4 && st.cl_len[kClOrder[n_cl - 1]] == 0) --n_cl;
        // canonical codes (RFC 1951 3.2.2), stored bit-reversed: Huffman codes go into the stream from their top bit
        for (int pass = 0; pass < 2; ++pass) {
            const unsigned char* len = pass ? st.len : st.cl_len;
            const int count = pass ? n_lit : kCl;
            for (int i = 0; i < 16; ++i) st.next_code[i] = 0;
            for (int i = 0; i < count; ++i) ++st.next_code[len[i]];
            uint32_t code = 0, prev = 0;
            for (int i = 1; i < 16; ++i) {
                code = (code + prev) << 1;
                prev = st.next_code[i];
                st.next_code[i] = (uint16_t)code;
            }
            for (int i = 0; i < count; ++i) {
                const int l = len[i];
                if (l == 0) continue;
                const uint32_t c = reversed(st.next_code[l]++, l);
                if (pass) st.code[i] = (uint16_t)c; else st.cl_code[i] = (unsigned char)c;
            }
        }
        StripBits out;
        out.start(st.bits, 0);
        out.put(s + 1 == S ? 1u : 0u, 1);
        out.put(2, 2);
        out.put((uint32_t)(n_lit - 257), 5);
        out.put(0, 5);
        out.put((uint32_t)(n_cl - 4), 4);
        for (int i = 0; i < n_cl; ++i) out.put(st.cl_len[kClOrder[i]], 3);
        for_cl_tokens(st.len, n_seq, [&](int sym, int eb, int ev) {
            out.put((uint32_t)st.cl_code[sym] | (uint32_t)ev << st.cl_len[sym], st.cl_len[sym] + eb);
        });
        out.finish();
        st.head_bits = out.bits();
    }
    __syncthreads();

    int mine = 0;
    for_tokens(st.bytes, c0, c1, start, next, [&](int sym, int eb, int) { mine += st.len[sym] + (sym > 256 ? eb + 1 : 0); });
    int tokens;
    const int before = block_excl_scan<kBlock>(mine, tokens);
    const int total = st.head_bits + tokens + st.len[256];
    if (total <= kStripBits) {                             // (always: kStripBits is the derived worst case)
        StripBits out;
        out.start(st.bits, st.head_bits + before);
        for_tokens(st.bytes, c0, c1, start, next, [&](int sym, int eb, int ev) {
            const int l = st.len[sym];
            if (sym > 256) out.put((uint32_t)st.code[sym] | (uint32_t)ev << l, l + eb + 1);      // + the 1-bit distance code 0
            else out.put(st.code[sym], l);
        });
        out.finish();
        if (tid == 0) {
            out.start(st.bits, st.head_bits + tokens);
            out.put(st.code[256], st.len[256]);
            out.finish();
        }
    }
    __syncthreads();
    if (total <= kStripBits) {
        uint32_t* dst = w.bits + g * kStripWords;
        for (int i = tid; i < (total + 31) / 32; i += kBlock) dst[i] = st.bits[i];
    }
    if (tid == 0) {
        w.bitlen[g] = total <= kStripBits ? total : -1;
        w.sum_a[g] = st.sum_a % kAdler;
        w.sum_b[g] = st.sum_b % kAdler;
    }
}

// One workgroup per stream: exclusive scan of the strips' bit lengths, the byte length, and the Adler-32.  With strip s of n_s
// bytes at offset o_s in a stream of N bytes: a = 1 + sum A_s, b = N + sum (B_s + (N - o_s - n_s) A_s), both modulo 65521; each
// term is below 65521 + 65521^2 < 2^33 and there are fewer than 2^31 / 8192 strips: the 64-bit sums stay below 2^52.
__global__ void __launch_bounds__(kScanBlock) png_scan(int64_t stream_bytes, int64_t S, PngWs w, int32_t* __restrict__ lengths,
                                                       uint32_t* __restrict__ adler) {
    __shared__ int bad;
    const int64_t f = blockIdx.x;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    unsigned long long sa = 0, sb = 0;
    const int64_t bits = nerfhip::block_offsets_scan<kScanBlock>(
        S, w.off + f * S, [&](int64_t i) { return nerfhip::strip_bits_or_flag(w.bitlen[f * S + i], &bad); },
        [&](int64_t i) {                                    // the pass's Adler terms, summed over the workgroup
            unsigned long long ta = 0, tb = 0, all;
            if (i < S) {
                const int64_t end = (i + 1) * kStrip < stream_bytes ? (i + 1) * kStrip : stream_bytes;
                ta = w.sum_a[f * S + i];
                tb = w.sum_b[f * S + i] + (unsigned long long)((stream_bytes - end) % kAdler) * ta;
            }
            block_excl_scan<kScanBlock>(ta, all);
            sa += all;
            block_excl_scan<kScanBlock>(tb, all);
            sb += all;
        });
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t n = (bits + 7) / 8;
        w.total[f] = bits;
        lengths[f] = (bad || n > 0x7fffffff) ? -1 : (int32_t)n;
        const uint32_t lo = (uint32_t)((1 + sa) % kAdler), hi = (uint32_t)(((unsigned long long)(stream_bytes % kAdler) + sb) % kAdler);
        adler[f] = hi << 16 | lo;
    }
}

// Gather: one thread per byte of the stream's deflate data: gather_byte (strip_bits.h) of its first bit; the bits behind the
// last strip are zero.  No byte has two writers.
__global__ void __launch_bounds__(kBlock) png_gather(int64_t S, int64_t stride, PngWs w, const int32_t* __restrict__ lengths,
                                                     unsigned char* __restrict__ data) {
    const int64_t f = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (int64_t)lengths[f] || p >= stride) return;      // (-1: the stream failed, nothing is written)
    data[f * stride + p] = (unsigned char)nerfhip::gather_byte(w.off + f * S, w.bitlen + f * S, w.bits, f * S, S, kStripWords, 8 * p);
}

bool stream_ok(int n, int64_t stream_bytes) { return n >= 0 && n <= 65535 && stream_bytes >= 1 && stream_bytes < ((int64_t)1 << 31); }

}  // namespace

extern "C" size_t nerfhip_png_workspace_bytes(int n, int64_t stream_bytes) {
    if (n <= 0 || !stream_ok(n, stream_bytes)) return 0;
    size_t bytes = 0;
    png_ws(nullptr, n, stream_bytes, &bytes);
    return bytes;
}

extern "C" size_t nerfhip_png_data_stride(int64_t stream_bytes) {
    if (!stream_ok(1, stream_bytes)) return 0;
    return (size_t)data_stride(stream_bytes);
}

extern "C" int nerfhip_png_filter(const uint8_t* images, int n, int H, int W, int C, uint8_t* streams, nerfhip_stream_t stream) {
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(C == 1 || C == 3 || C == 4);
    NERFHIP_CHECK_ARG(H >= 1 && W >= 1);
    NERFHIP_CHECK_ARG(stream_ok(n, (int64_t)H * (1 + (int64_t)W * C)));
    NERFHIP_CHECK_ARG(images && streams);
    const unsigned rows = (unsigned)(((int64_t)H + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL(png_filter_rows, dim3(rows, n), dim3(kBlock), 0, (hipStream_t)stream, images, H, (int64_t)W * C, C, streams);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_png_deflate(const uint8_t* streams, int n, int64_t stream_bytes, uint8_t* data, int32_t* lengths,
                                   uint32_t* adler, void* workspace, nerfhip_stream_t stream) {
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(stream_ok(n, stream_bytes));
    NERFHIP_CHECK_ARG(streams && data && lengths && adler && workspace);
    if ((uintptr_t)workspace % 8 != 0) return NERFHIP_E_ALIGN;
    const int64_t S = strips_of(stream_bytes), stride = data_stride(stream_bytes);
    const PngWs w = png_ws(workspace, n, stream_bytes, nullptr);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(png_strip, dim3((unsigned)S, n), dim3(kBlock), 0, s, streams, stream_bytes, S, w);
    hipLaunchKernelGGL(png_scan, dim3(n), dim3(kScanBlock), 0, s, stream_bytes, S, w, lengths, adler);
    hipLaunchKernelGGL(png_gather, dim3((unsigned)((stride + kBlock - 1) / kBlock), n), dim3(kBlock), 0, s, S, stride, w, lengths, data);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_png_code_lengths(const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths) {
    NERFHIP_CHECK_ARG(counts && lengths);
    NERFHIP_CHECK_ARG(n_symbols >= 1 && n_symbols <= nerfhip::kHuffMaxSymbols && limit >= 1 && limit <= nerfhip::kHuffMaxLimit);
    NERFHIP_CHECK_ARG(n_symbols <= (1 << limit));
    HuffScratch scratch;
    nerfhip::huff_lengths(counts, n_symbols, limit, lengths, scratch);
    return 0;
}

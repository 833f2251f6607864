// The animated GIF of the reference's eval loop (eval.py:145 `imageio.mimsave`) formed on the device: per frame a 256-colour
// median cut over a 32 x 32 x 32 histogram, the index image and its palette, and the LZW code stream cut into strips that each
// start with a clear code, so that every strip is encoded by its own lane.  The exact integer definition, the strip length and
// the byte layout of the result: DESIGN.md §13 and include/nerfhip.h.  The host writes the container around the data.  The bit
// writer, the scan of the strips' bit lengths and the gather of the bytes are the ones png.hip has: strip_bits.h, block_scan.h.
#include "block_scan.h"
#include "common.h"
#include "strip_bits.h"

namespace {

using nerfhip::carve;

constexpr int kBlock = 256;              // threads of the per-pixel and per-byte kernels
constexpr int kRun = 16;                 // consecutive pixels per thread of the per-pixel kernels
constexpr int kCutBlock = 1024;          // the one workgroup per frame that cuts boxes and scans strip lengths
constexpr int kBins = 32768;
constexpr int kStrip = NERFHIP_GIF_STRIP;
constexpr int kTable = 8192;             // hash slots per strip: at most kStrip - 1 = 3837 entries, load < 1/2
constexpr int kStripWords = 1440;        // 32-bit words per strip's bits: kStrip + 2 codes of at most 12 bits = 46080 bits
constexpr int64_t kMaxPixels = (int64_t)1 << 26;
constexpr uint32_t kEmpty = 0xffffffffu; // (key << 12 | code) never has all bits set: a code's prefix is below the code

static_assert(257 + kStrip <= 4095, "a strip must never fill the code table");
static_assert((kStrip + 2) * 12 <= kStripWords * 32, "strip bit buffer too small");
static_assert(2 * (kStrip - 1) < kTable, "hash load must stay under one half");

__host__ __device__ inline int64_t strips_of(int64_t hw) { return (hw + kStrip - 1) / kStrip; }

struct GifWs {
    uint32_t* hist;                 // (F, 32768) pixel counts per bin        } zeroed together by quantize
    unsigned long long* sums;       // (F, 256, 4) r, g, b sums and count     }
    unsigned char* lut;             // (F, 32768) bin -> palette index        }
    int32_t* bitlen;                // (F, S) bits of each strip, -1: its probe bound was hit
    int64_t* off;                   // (F, S) first bit of each strip in the frame's stream
    int64_t* total;                 // (F) bits of the frame's stream
    uint32_t* table;                // (F, S, kTable) hash slots, set to kEmpty by lzw
    uint32_t* bits;                 // (F, S, kStripWords)
};

__host__ __device__ inline GifWs gif_ws(void* base, int64_t F, int64_t hw, size_t* bytes) {
    const int64_t S = strips_of(hw);
    char* p = (char*)base;
    GifWs w;
    w.hist = carve<uint32_t>(p, (size_t)F * kBins);
    w.sums = carve<unsigned long long>(p, (size_t)F * 256 * 4);
    w.lut = carve<unsigned char>(p, (size_t)F * kBins);
    w.bitlen = carve<int32_t>(p, (size_t)F * S);
    w.off = carve<int64_t>(p, (size_t)F * S);
    w.total = carve<int64_t>(p, (size_t)F);
    w.table = carve<uint32_t>(p, (size_t)F * S * kTable);
    w.bits = carve<uint32_t>(p, (size_t)F * S * kStripWords);
    if (bytes) *bytes = (size_t)(p - (char*)base);
    return w;
}

__host__ __device__ inline int64_t data_stride(int64_t hw) {
    const int64_t raw = (12 * (hw + strips_of(hw) + 1) + 7) / 8;
    return raw + (raw + 254) / 255;
}

__device__ __forceinline__ int bin_of(const unsigned char* p) { return (p[0] >> 3) << 10 | (p[1] >> 3) << 5 | (p[2] >> 3); }

// ---- quantiser ---------------------------------------------------------------------------------------------------------------
// Histogram: a thread walks kRun consecutive pixels and issues one atomic per run of equal bins (a white background is one).
__global__ void __launch_bounds__(kBlock) gif_hist(const unsigned char* __restrict__ frames, int64_t hw, GifWs w) {
    const int64_t f = blockIdx.y;
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRun;
    if (first >= hw) return;
    const int64_t last = first + kRun < hw ? first + kRun : hw;
    const unsigned char* px = frames + f * hw * 3;
    uint32_t* hist = w.hist + f * kBins;
    int cur = bin_of(px + first * 3);
    uint32_t n = 1;
    for (int64_t i = first + 1; i < last; ++i) {
        const int b = bin_of(px + i * 3);
        if (b != cur) {
            atomicAdd(hist + cur, n);
            cur = b;
            n = 0;
        }
        ++n;
    }
    atomicAdd(hist + cur, n);
}

struct CutState {
    unsigned char lo[256][3], hi[256][3];
    uint32_t n[256];
    uint32_t marg[32];     // pixel count per coordinate of the cut axis
    uint32_t mask[2][32];  // per coordinate of the cut axis: occupied coordinates of the two other axes (in r, g, b order)
    int nbox, sel, axis;
};

// Fills marg / mask of box b for `axis` from the frame's histogram (all threads; the caller zeroed them and synchronises after).
__device__ __forceinline__ void cut_survey(const uint32_t* __restrict__ hist, CutState& st, int b, int axis) {
    const int l0 = st.lo[b][0], l1 = st.lo[b][1], l2 = st.lo[b][2];
    const int d1 = st.hi[b][1] - l1 + 1, d2 = st.hi[b][2] - l2 + 1;
    const int vol = (st.hi[b][0] - l0 + 1) * d1 * d2;
    for (int v = threadIdx.x; v < vol; v += kCutBlock) {
        int c[3];
        c[2] = l2 + v % d2;
        c[1] = l1 + (v / d2) % d1;
        c[0] = l0 + v / (d1 * d2);
        const uint32_t cnt = hist[c[0] << 10 | c[1] << 5 | c[2]];
        if (cnt == 0) continue;
        const int a = axis == 0 ? c[0] : axis == 1 ? c[1] : c[2];
        const int o1 = axis == 0 ? c[1] : c[0], o2 = axis == 2 ? c[1] : c[2];
        atomicAdd(&st.marg[a], cnt);
        atomicOr(&st.mask[0][a], 1u << o1);
        atomicOr(&st.mask[1][a], 1u << o2);
    }
}

// Thread 0: box `b` := the part of the surveyed box with cut-axis coordinates c_lo..c_hi, shrunk to its occupied bins.
__device__ void cut_assign(CutState& st, int b, int axis, int c_lo, int c_hi) {
    uint32_t n = 0, m1 = 0, m2 = 0;
    int first = -1, last = -1;
    for (int c = c_lo; c <= c_hi; ++c) {
        if (st.marg[c] == 0) continue;
        if (first < 0) first = c;
        last = c;
        n += st.marg[c];
        m1 |= st.mask[0][c];
        m2 |= st.mask[1][c];
    }
    if (first < 0) {          // (cannot happen: both parts of a shrunk box hold pixels; keeps every coordinate in range anyway)
        first = last = c_lo;
        m1 = m2 = 1;
    }
    const int o1 = axis == 0 ? 1 : 0, o2 = axis == 2 ? 1 : 2;
    st.lo[b][axis] = (unsigned char)first;
    st.hi[b][axis] = (unsigned char)last;
    st.lo[b][o1] = (unsigned char)(__ffs(m1) - 1);
    st.hi[b][o1] = (unsigned char)(31 - __clz(m1));
    st.lo[b][o2] = (unsigned char)(__ffs(m2) - 1);
    st.hi[b][o2] = (unsigned char)(31 - __clz(m2));
    st.n[b] = n;
}

// One workgroup per frame: the sequential cut.  Every decision is taken by thread 0 from exact integer marginals that all
// threads gather; the loop's exits read shared words behind a barrier, so they are uniform.
__global__ void __launch_bounds__(kCutBlock) gif_cut(GifWs w, int32_t* __restrict__ box_counts) {
    __shared__ CutState st;
    const int64_t f = blockIdx.x;
    const uint32_t* hist = w.hist + f * kBins;
    const int tid = threadIdx.x;
    if (tid < 32) st.marg[tid] = st.mask[0][tid] = st.mask[1][tid] = 0;
    if (tid == 0) {
        for (int a = 0; a < 3; ++a) { st.lo[0][a] = 0; st.hi[0][a] = 31; }
        st.nbox = 1;
    }
    __syncthreads();
    cut_survey(hist, st, 0, 0);
    __syncthreads();
    if (tid == 0) cut_assign(st, 0, 0, 0, 31);
    for (;;) {
        __syncthreads();
        const int nbox = st.nbox;
        if (nbox >= 256) break;
        if (tid < 64) {          // the most populated box that spans more than one bin; ties to the lowest index
            unsigned long long key = 0;
            for (int i = tid; i < nbox; i += 64) {
                const bool span = st.hi[i][0] > st.lo[i][0] || st.hi[i][1] > st.lo[i][1] || st.hi[i][2] > st.lo[i][2];
                const unsigned long long k = span ? ((unsigned long long)st.n[i] << 9 | (unsigned)(511 - i)) : 0ull;
                key = k > key ? k : key;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long t = __shfl_xor(key, o, 64);
                key = t > key ? t : key;
            }
            if (tid == 0) {
                const int b = key ? 511 - (int)(key & 511) : -1;
                st.sel = b;
                if (b >= 0) {
                    const int e0 = st.hi[b][0] - st.lo[b][0], e1 = st.hi[b][1] - st.lo[b][1], e2 = st.hi[b][2] - st.lo[b][2];
                    st.axis = (e0 >= e1 && e0 >= e2) ? 0 : (e1 >= e2 ? 1 : 2);
                }
            }
        }
        if (tid >= 64 && tid < 96) st.marg[tid - 64] = st.mask[0][tid - 64] = st.mask[1][tid - 64] = 0;
        __syncthreads();
        const int b = st.sel, axis = st.axis;
        if (b < 0) break;
        cut_survey(hist, st, b, axis);
        __syncthreads();
        if (tid == 0) {
            const int lo = st.lo[b][axis], hi = st.hi[b][axis];
            const uint32_t half = st.n[b] / 2 + (st.n[b] & 1);
            uint32_t cum = 0;
            int cut = hi - 1;
            for (int c = lo; c < hi; ++c) {
                cum += st.marg[c];
                if (cum >= half) { cut = c; break; }
            }
            cut_assign(st, nbox, axis, cut + 1, hi);      // (reads marg / mask only: the order of the two does not matter)
            cut_assign(st, b, axis, lo, cut);
            st.nbox = nbox + 1;
        }
    }
    const int nbox = st.nbox;
    if (tid == 0) box_counts[f] = nbox;
    unsigned char* lut = w.lut + f * kBins;
    for (int i = 0; i < nbox; ++i) {          // boxes are disjoint: every bin is written at most once
        const int l0 = st.lo[i][0], l1 = st.lo[i][1], l2 = st.lo[i][2];
        const int d1 = st.hi[i][1] - l1 + 1, d2 = st.hi[i][2] - l2 + 1;
        const int vol = (st.hi[i][0] - l0 + 1) * d1 * d2;
        for (int v = tid; v < vol; v += kCutBlock)
            lut[(l0 + v / (d1 * d2)) << 10 | (l1 + (v / d2) % d1) << 5 | (l2 + v % d2)] = (unsigned char)i;
    }
}

// Index image and the per-entry colour sums in one pass: workgroup-private sums in LDS (4096 pixels: below 2^32), one 64-bit
// atomic per touched entry and workgroup.
__global__ void __launch_bounds__(kBlock) gif_map(const unsigned char* __restrict__ frames, int64_t hw, GifWs w,
                                                  unsigned char* __restrict__ indices) {
    __shared__ uint32_t acc[256][4];
    const int64_t f = blockIdx.y;
    for (int k = 0; k < 4; ++k) acc[threadIdx.x][k] = 0;
    __syncthreads();
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRun;
    if (first < hw) {
        const int64_t last = first + kRun < hw ? first + kRun : hw;
        const unsigned char* px = frames + f * hw * 3;
        const unsigned char* lut = w.lut + f * kBins;
        unsigned char* out = indices + f * hw;
        int cur = -1;
        uint32_t s0 = 0, s1 = 0, s2 = 0, n = 0;
        for (int64_t i = first; i < last; ++i) {
            const unsigned char* p = px + i * 3;
            const int e = lut[bin_of(p)];
            out[i] = (unsigned char)e;
            if (e != cur) {
                if (n) {
                    atomicAdd(&acc[cur][0], s0);
                    atomicAdd(&acc[cur][1], s1);
                    atomicAdd(&acc[cur][2], s2);
                    atomicAdd(&acc[cur][3], n);
                }
                cur = e;
                s0 = s1 = s2 = n = 0;
            }
            s0 += p[0];
            s1 += p[1];
            s2 += p[2];
            ++n;
        }
        atomicAdd(&acc[cur][0], s0);
        atomicAdd(&acc[cur][1], s1);
        atomicAdd(&acc[cur][2], s2);
        atomicAdd(&acc[cur][3], n);
    }
    __syncthreads();
    if (acc[threadIdx.x][3]) {
        unsigned long long* sums = w.sums + (f * 256 + threadIdx.x) * 4;
        for (int k = 0; k < 4; ++k) atomicAdd(sums + k, (unsigned long long)acc[threadIdx.x][k]);
    }
}

__global__ void __launch_bounds__(kBlock) gif_palette(GifWs w, unsigned char* __restrict__ palettes) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // (frame, entry): the grid is exactly F blocks of 256
    const unsigned long long* s = w.sums + e * 4;
    const unsigned long long cnt = s[3];
    for (int k = 0; k < 3; ++k) palettes[e * 3 + k] = cnt ? (unsigned char)((2 * s[k] + cnt) / (2 * cnt)) : (unsigned char)0;
}

// ---- LZW ---------------------------------------------------------------------------------------------------------------------
// One strip per lane.  The dictionary is an open-addressing hash over (prefix << 8 | byte) in the strip's own kTable slots; a
// strip adds at most kStrip - 1 entries, so a free slot always exists, and the explicit probe bound only turns a broken
// invariant into bitlen = -1 instead of a spin.  The strip's last emission is the clear code of the next strip (the end code
// after the last one): its width belongs to this strip's dictionary state.
__global__ void __launch_bounds__(64) gif_strips(const unsigned char* __restrict__ indices, int64_t hw, int64_t S, int64_t n_strips,
                                                 GifWs w) {
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= n_strips) return;
    const int64_t f = g / S, s = g % S;
    const int64_t start = s * kStrip;
    const int count = (int)(hw - start < kStrip ? hw - start : kStrip);
    const unsigned char* in = indices + f * hw + start;
    uint32_t* table = w.table + g * kTable;
    nerfhip::BitWriter<nerfhip::StoreWord> out;      // the strip's words are this lane's alone
    out.start(w.bits + g * kStripWords, 0);
    int next = 258, width = 9;
    if (s == 0) out.put(256, 9);
    int prefix = in[0];
    for (int i = 1; i < count; ++i) {
        const int c = in[i];
        const uint32_t key = (uint32_t)prefix << 8 | (uint32_t)c;
        uint32_t h = (key * 2654435761u) >> 19;
        int hit = -1, probes = 0;
        for (; probes < kTable; ++probes) {
            const uint32_t e = table[h];
            if (e == kEmpty) break;
            if ((e >> 12) == key) { hit = (int)(e & 0xfff); break; }
            h = (h + 1) & (kTable - 1);
        }
        if (probes == kTable) {
            w.bitlen[g] = -1;
            return;
        }
        if (hit >= 0) {
            prefix = hit;
            continue;
        }
        out.put(prefix, width);
        table[h] = key << 12 | (uint32_t)next;
        ++next;
        if (next > (1 << width)) ++width;
        prefix = c;
    }
    out.put(prefix, width);
    ++next;                                   // the decoder assigns a code for this emission too
    if (next > (1 << width)) ++width;
    out.put(s + 1 == S ? 257 : 256, width);
    out.finish();
    w.bitlen[g] = out.bits();
}

// One workgroup per frame: exclusive scan of the strips' bit lengths, the frame's total and the length of its sub-blocked data.
__global__ void __launch_bounds__(kCutBlock) gif_scan(int64_t S, GifWs w, int32_t* __restrict__ lengths) {
    __shared__ int bad;
    const int64_t f = blockIdx.x;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const int64_t bits = nerfhip::block_offsets_scan<kCutBlock>(
        S, w.off + f * S, [&](int64_t i) { return nerfhip::strip_bits_or_flag(w.bitlen[f * S + i], &bad); });
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t n = (bits + 7) / 8;
        w.total[f] = bits;
        lengths[f] = bad ? -1 : (int32_t)(n + (n + 254) / 255);
    }
}

// Gather: one thread per byte of the frame's sub-blocked data.  A length byte stands at every 256th position; a data byte is
// gather_byte (strip_bits.h) of its position in the frame's stream.  No byte has two writers.
__global__ void __launch_bounds__(kBlock) gif_gather(int64_t S, int64_t stride, GifWs w, const int32_t* __restrict__ lengths,
                                                     unsigned char* __restrict__ data) {
    const int64_t f = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (int64_t)lengths[f] || p >= stride) return;      // (-1: the frame failed, nothing is written)
    const int64_t total = w.total[f], n = (total + 7) / 8;
    unsigned v;
    if ((p & 255) == 0) {
        const int64_t left = n - 255 * (p >> 8);
        v = left < 255 ? (unsigned)left : 255u;
    } else {
        const int64_t bit = 8 * (255 * (p >> 8) + (p & 255) - 1);
        v = nerfhip::gather_byte(w.off + f * S, w.bitlen + f * S, w.bits, f * S, S, kStripWords, bit);
    }
    data[f * stride + p] = (unsigned char)v;
}

int check_shape(int F, int H, int W) {
    if (F < 0 || F > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535) return NERFHIP_E_BADARG;
    if ((int64_t)H * W > kMaxPixels) return NERFHIP_E_BADARG;
    return 0;
}

}  // namespace

extern "C" size_t nerfhip_gif_workspace_bytes(int F, int H, int W) {
    if (F <= 0 || check_shape(F, H, W) != 0) return 0;
    size_t bytes = 0;
    gif_ws(nullptr, F, (int64_t)H * W, &bytes);
    return bytes;
}

extern "C" size_t nerfhip_gif_data_stride(int H, int W) {
    if (check_shape(1, H, W) != 0) return 0;
    return (size_t)data_stride((int64_t)H * W);
}

extern "C" int nerfhip_gif_quantize(const uint8_t* frames, int F, int H, int W, uint8_t* indices, uint8_t* palettes,
                                    int32_t* box_counts, void* workspace, nerfhip_stream_t stream) {
    if (F == 0) return 0;
    NERFHIP_CHECK_ARG(check_shape(F, H, W) == 0);
    NERFHIP_CHECK_ARG(frames && indices && palettes && box_counts && workspace);
    if ((uintptr_t)workspace % 8 != 0) return NERFHIP_E_ALIGN;
    const int64_t hw = (int64_t)H * W;
    const GifWs w = gif_ws(workspace, F, hw, nullptr);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(w.hist, 0, (size_t)((char*)w.bitlen - (char*)w.hist), s);      // hist, sums, lut
    if (e != hipSuccess) return (int)e;
    const unsigned px_blocks = (unsigned)((hw + (int64_t)kBlock * kRun - 1) / ((int64_t)kBlock * kRun));
    hipLaunchKernelGGL(gif_hist, dim3(px_blocks, F), dim3(kBlock), 0, s, frames, hw, w);
    hipLaunchKernelGGL(gif_cut, dim3(F), dim3(kCutBlock), 0, s, w, box_counts);
    hipLaunchKernelGGL(gif_map, dim3(px_blocks, F), dim3(kBlock), 0, s, frames, hw, w, indices);
    hipLaunchKernelGGL(gif_palette, dim3(F), dim3(kBlock), 0, s, w, palettes);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_gif_lzw(const uint8_t* indices, int F, int H, int W, uint8_t* data, int32_t* lengths, void* workspace,
                               nerfhip_stream_t stream) {
    if (F == 0) return 0;
    NERFHIP_CHECK_ARG(check_shape(F, H, W) == 0);
    NERFHIP_CHECK_ARG(indices && data && lengths && workspace);
    if ((uintptr_t)workspace % 8 != 0) return NERFHIP_E_ALIGN;
    const int64_t hw = (int64_t)H * W, S = strips_of(hw), n_strips = S * F, stride = data_stride(hw);
    const GifWs w = gif_ws(workspace, F, hw, nullptr);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(w.table, 0xff, (size_t)n_strips * kTable * 4, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(gif_strips, dim3((unsigned)((n_strips + 63) / 64)), dim3(64), 0, s, indices, hw, S, n_strips, w);
    hipLaunchKernelGGL(gif_scan, dim3(F), dim3(kCutBlock), 0, s, S, w, lengths);
    hipLaunchKernelGGL(gif_gather, dim3((unsigned)((stride + kBlock - 1) / kBlock), F), dim3(kBlock), 0, s, S, stride, w, lengths, data);
    return nerfhip_launch_status();
}

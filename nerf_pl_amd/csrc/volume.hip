// The Unity volume file (extract_mesh.ipynb, cell "Generate .vol file for volume rendering in Unity"): quantise rgb-sigma to
// RGBA bytes and keep, in index order, the lattice points whose alpha is positive.  One thread per point; the only cross-block
// communication is the block-total scan (one workgroup, block_scan.h's offsets scan) between two launches.  Passes and byte
// counts: DESIGN.md, volume export.
#include <math.h>

#include "block_scan.h"
#include "common.h"

namespace {

using nerfhip::block_excl_scan;
using nerfhip::carve;

constexpr int kBlock = 256;        // threads of the two per-point kernels (4 waves)
constexpr int kScanBlock = 1024;   // the single workgroup that scans the block totals

struct VolWs {
    int64_t* base;     // (1) the cursor's value before this call: where this call's first record goes
    int64_t* off;      // (nb) exclusive block offsets
    int32_t* blk;      // (nb) kept points per block
};

inline int64_t vol_blocks(int64_t n) { return (n + kBlock - 1) / kBlock; }

inline VolWs vol_ws(void* base, int64_t n, size_t* bytes) {
    const int64_t nb = vol_blocks(n);
    char* p = (char*)base;
    VolWs w;
    w.base = carve<int64_t>(p, 1);
    w.off = carve<int64_t>(p, nb);
    w.blk = carve<int32_t>(p, nb);
    if (bytes) *bytes = (size_t)(p - (char*)base);
    return w;
}

__device__ __forceinline__ uint32_t to_byte(float x) {    // trunc toward zero, clamped to 0..255 (NaN -> 0)
    if (!(x >= 1.0f)) return 0u;
    return x >= 255.0f ? 255u : (uint32_t)x;
}

// One point of the notebook's pack.  sigma <= 0, -0.0 and NaN are dropped without the exponential: np.maximum(sigma, 0) makes
// c * sigma a (signed) zero or NaN there, so 1 - exp(.) is 0 or NaN and `a > 0` is false whatever c is.
__device__ __forceinline__ bool vol_point(const float4 v, float neg_cell, uint32_t& word) {
    if (!(v.w > 0.0f)) return false;
    const float t = nh_mul(neg_cell, v.w);
    const float e = (float)exp((double)t);             // fp64 exp rounded once: independent of the device's fp32 expf
    const float a = nh_sub(1.0f, e);
    if (!(a > 0.0f)) return false;
    word = to_byte(nh_mul(v.x, 255.0f)) << 24 | to_byte(nh_mul(v.y, 255.0f)) << 16 | to_byte(nh_mul(v.z, 255.0f)) << 8 |
           to_byte(nh_mul(a, 255.0f));
    return true;
}

// Pass 1: kept points per block.
__global__ void __launch_bounds__(kBlock) vol_count(const float4* __restrict__ rgbsigma, int64_t n, float neg_cell, VolWs w) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t word;
    const int keep = i < n && vol_point(rgbsigma[i], neg_cell, word);
    int tot;
    block_excl_scan<kBlock>(keep, tot);
    if (threadIdx.x == 0) w.blk[blockIdx.x] = tot;
}

// One workgroup: exclusive offsets of the block totals; the device cursor is read (-> *w.base) and advanced by the call's count.
__global__ void __launch_bounds__(kScanBlock) vol_scan(int64_t nb, VolWs w, int64_t* __restrict__ cursor) {
    const int64_t kept = nerfhip::block_offsets_scan<kScanBlock>(nb, w.off, [&](int64_t i) { return w.blk[i]; });
    if (threadIdx.x == 0) {
        const int64_t c = *cursor;
        *w.base = c;
        *cursor = c + kept;
    }
}

// Pass 2: the records.  A block that keeps nothing (most of a trained scene) returns before it reads its points again.
__global__ void __launch_bounds__(kBlock) vol_emit(const float4* __restrict__ rgbsigma, int64_t n, int64_t first_index, float neg_cell,
                                                   VolWs w, uint2* __restrict__ records, int64_t capacity) {
    if (w.blk[blockIdx.x] == 0) return;                 // uniform over the block
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t word = 0;
    const int keep = i < n && vol_point(rgbsigma[i], neg_cell, word);
    int tot;
    const int ex = block_excl_scan<kBlock>(keep, tot);
    if (!keep) return;
    const int64_t pos = *w.base + w.off[blockIdx.x] + ex;
    if (pos < 0 || pos >= capacity) return;             // overflow: the caller sees it in the cursor
    records[pos] = make_uint2((uint32_t)(first_index + i), word);
}

inline bool vol_n_ok(int64_t n) { return n >= 0 && n <= ((int64_t)1 << 32); }

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" size_t nerfhip_vol_workspace_bytes(int64_t n) {
    if (!vol_n_ok(n)) return 0;
    size_t bytes = 0;
    vol_ws(nullptr, n, &bytes);
    return bytes;
}

extern "C" int nerfhip_vol_pack(const float* rgbsigma, int64_t n, int64_t first_index, float neg_cell, void* workspace,
                                uint32_t* records, int64_t capacity, int64_t* cursor, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(vol_n_ok(n) && capacity >= 0 && first_index >= 0 && first_index <= ((int64_t)1 << 32) - n);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rgbsigma && workspace && records && cursor);
    if ((((uintptr_t)rgbsigma) & 15) || (((uintptr_t)records) & 7) || (((uintptr_t)workspace) & 7) || (((uintptr_t)cursor) & 7))
        return NERFHIP_E_ALIGN;
    const VolWs w = vol_ws(workspace, n, nullptr);
    const unsigned nb = (unsigned)vol_blocks(n);        // <= 2^24
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vol_count, dim3(nb), dim3(kBlock), 0, s, (const float4*)rgbsigma, n, neg_cell, w);
    hipLaunchKernelGGL(vol_scan, dim3(1), dim3(kScanBlock), 0, s, (int64_t)nb, w, cursor);
    hipLaunchKernelGGL(vol_emit, dim3(nb), dim3(kBlock), 0, s, (const float4*)rgbsigma, n, first_index, neg_cell, w,
                       (uint2*)records, capacity);
    return nerfhip_launch_status();
}

// Empty-space skipping at eval: the occupancy bitfield of a sigma lattice, the per-ray cull against it, the
// stable compaction of the rays that hit and the scatter of their rendered values back into full-size outputs.
//
//   occupancy_build   sigma (N,N,N) -> one bit per cell: cell rule, three separable dilation passes on bytes, 32 cells per word
//   cull_rays         one thread per ray: occupancy_core.h's walk (shared with nerfhip_cull_rays_host)
//   cull_compact      hits per block -> one-workgroup scan of the block totals (block_scan.h, as mesh.hip) -> slot / index / rows
//   cull_scatter      compact value at slot[i], or the background
//
// Every launch is one thread per cell, word or ray in 256-thread blocks; nothing allocates, nothing synchronises.
#include "block_scan.h"
#include "common.h"
#include "occupancy_core.h"
#include "twin_launch.h"

namespace {

using nerfhip::block_excl_scan;
using nerfhip::blocks_of;
using nerfhip::carve;
using nerfhip::kMaxRays;
using nerfhip::misaligned;
using nerfhip::OccGrid;
using nerfhip::OccVerdict;

constexpr int kBlock = nerfhip::kItemBlock;
constexpr int kMaxN = 1025;            // M <= 1024: a cell's bit index fits 30 bits

// ---- bitfield -----------------------------------------------------------------------------------------------------------------
struct BuildWs {
    uint8_t* a;    // (M^3) one byte per cell
    uint8_t* b;    // (M^3) the other side of the dilation's ping-pong
};

inline BuildWs build_ws(void* base, int64_t M, size_t* bytes) {
    char* p = (char*)base;
    BuildWs w;
    w.a = carve<uint8_t>(p, (size_t)(M * M * M));
    w.b = carve<uint8_t>(p, (size_t)(M * M * M));
    if (bytes) *bytes = (size_t)(p - (char*)base);
    return w;
}

// A cell is occupied iff one of its 8 corners is > threshold or NaN: !(v <= threshold).
__global__ void __launch_bounds__(kBlock) occ_cells(const float* __restrict__ sigma, int N, float threshold, uint8_t* __restrict__ cells) {
    const int M = N - 1;
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= (uint32_t)M * M * M) return;
    const uint32_t iz = c % M, row = c / M, ix = row % M, iy = row / M;
    const float* p = sigma + ((size_t)iy * N + ix) * N + iz;
    bool occ = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float v = p[((size_t)(k >> 2) * N + ((k >> 1) & 1)) * N + (k & 1)];
        occ = occ || !(v <= threshold);
    }
    cells[c] = occ;
}

// One axis of the Chebyshev dilation: a cell is set iff a cell within r of it along the axis (stride in cells, clipped) is.
__global__ void __launch_bounds__(kBlock) occ_dilate(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int M, int r, int axis) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= (uint32_t)M * M * M) return;
    const int iz = c % M, row = c / M, ix = row % M, iy = row / M;
    const int i = axis == 0 ? iz : axis == 1 ? ix : iy;
    const int64_t stride = axis == 0 ? 1 : axis == 1 ? M : (int64_t)M * M;
    const int first = max(i - r, 0), last = min(i + r, M - 1);
    uint8_t v = 0;
    for (int k = first; k <= last && !v; ++k) v = in[(int64_t)c + (int64_t)(k - i) * stride];
    out[c] = v;
}

__global__ void __launch_bounds__(kBlock) occ_pack(const uint8_t* __restrict__ cells, uint32_t n_cells, uint32_t n_words, uint32_t* __restrict__ words) {
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    if (w >= n_words) return;
    uint32_t bits = 0;
    for (uint32_t k = 0; k < 32; ++k) {
        const uint32_t c = w * 32 + k;
        if (c < n_cells && cells[c]) bits |= 1u << k;
    }
    words[w] = bits;
}

// ---- cull ---------------------------------------------------------------------------------------------------------------------
struct CullItem {
    const float4* rays;
    OccGrid g;
    uint8_t* hit;
    float *t0, *t1;
    __host__ __device__ void operator()(int64_t i) const {
        float ray[8];
        nerfhip::load_ray(rays, i, ray);
        const OccVerdict v = nerfhip::occ_cull_ray(g, ray);
        hit[i] = v.hit;
        t0[i] = v.t0;
        t1[i] = v.t1;
    }
};

__global__ void __launch_bounds__(kBlock) cull_rays(const float4* __restrict__ rays, int64_t n, OccGrid g, uint8_t* __restrict__ hit,
                                                    float* __restrict__ t0, float* __restrict__ t1) {
    const int64_t i = nerfhip::item_index();
    if (i < n) CullItem{rays, g, hit, t0, t1}(i);
}

// M >= 1, lo < hi on every axis, everything finite; fills g (words stay the caller's)
inline bool make_grid(const void* words, int M, const float* ranges, OccGrid& g) {
    if (M < 1 || M > kMaxN - 1 || !ranges) return false;
    g.words = (const uint32_t*)words;
    g.M = M;
    for (int a = 0; a < 3; ++a) {
        const float lo = ranges[2 * a], hi = ranges[2 * a + 1];
        if (!(lo < hi) || !nerfhip::finite_f32(lo) || !nerfhip::finite_f32(hi)) return false;
        g.lo[a] = lo;
        g.hi[a] = hi;
        g.h[a] = (hi - lo) / (float)M;
        if (!(g.h[a] > 0.0f) || !nerfhip::finite_f32(g.h[a])) return false;
    }
    return true;
}

inline int cull_args(const float* rays, int64_t n, const int32_t* words, int M, const float* ranges, uint8_t* hit, float* t0, float* t1,
                     OccGrid& g) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays);
    NERFHIP_CHECK_ARG(make_grid(words, M, ranges, g));
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rays && words && hit && t0 && t1);
    if (misaligned(rays, 16) || misaligned(words, 4) || misaligned(t0, 4) || misaligned(t1, 4)) return NERFHIP_E_ALIGN;
    return 0;
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------
struct CompactWs {
    int64_t* off;      // (nb) exclusive block offsets
    int32_t* blk;      // (nb) hits per block
};

inline CompactWs compact_ws(void* base, int64_t n, size_t* bytes) {
    const int64_t nb = (n + kBlock - 1) / kBlock;
    char* p = (char*)base;
    CompactWs w;
    w.off = carve<int64_t>(p, (size_t)nb);
    w.blk = carve<int32_t>(p, (size_t)nb);
    if (bytes) *bytes = (size_t)(p - (char*)base);
    return w;
}

__global__ void __launch_bounds__(kBlock) compact_count(const uint8_t* __restrict__ hit, int64_t n, CompactWs w) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int keep = i < n && hit[i] != 0;
    int tot;
    block_excl_scan<kBlock>(keep, tot);
    if (threadIdx.x == 0) w.blk[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kBlock) compact_scan(int64_t nb, CompactWs w, int32_t* __restrict__ n_hit) {
    const int64_t kept = nerfhip::block_offsets_scan<kBlock>(nb, w.off, [&](int64_t i) { return w.blk[i]; });
    if (threadIdx.x == 0) *n_hit = (int32_t)kept;
}

__global__ void __launch_bounds__(kBlock) compact_emit(const uint8_t* __restrict__ hit, const float4* __restrict__ rays,
                                                       const float* __restrict__ t0, const float* __restrict__ t1, int64_t n, CompactWs w,
                                                       int32_t* __restrict__ slot, int32_t* __restrict__ index,
                                                       float4* __restrict__ rays_out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int keep = i < n && hit[i] != 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(keep, tot);
    if (i >= n) return;
    const int64_t pos = w.off[blockIdx.x] + ex;        // < n: the rank of a hit among the hits in front of it
    slot[i] = keep ? (int32_t)pos : -1;
    if (!keep) return;
    index[pos] = (int32_t)i;
    float4 b = rays[2 * i + 1];
    if (t0) b.z = t0[i];                                // a null t0 / t1 keeps the row's own near / far
    if (t1) b.w = t1[i];
    rays_out[2 * pos] = rays[2 * i];
    rays_out[2 * pos + 1] = b;
}

// ---- scatter ------------------------------------------------------------------------------------------------------------------
struct ScatterArgs {
    const float* rgb;          // (n_compact, 3)
    float* rgb_out;            // (n, 3)
    const float* scalar[3];    // (n_compact): depth and the two opacities
    float* scalar_out[3];      // (n)
};

__global__ void __launch_bounds__(kBlock) cull_scatter(const int32_t* __restrict__ slot, int64_t n, int64_t n_compact, float bg,
                                                       ScatterArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t s = slot[i];
    const bool have = s >= 0 && s < n_compact;
    if (a.rgb_out) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.rgb_out[3 * i + k] = have ? a.rgb[3 * s + k] : bg;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (a.scalar_out[k]) a.scalar_out[k][i] = have ? a.scalar[k][s] : 0.0f;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" size_t nerfhip_occupancy_workspace_bytes(int N) {
    if (N < 2 || N > kMaxN) return 0;
    size_t bytes = 0;
    build_ws(nullptr, N - 1, &bytes);
    return bytes;
}

extern "C" int nerfhip_occupancy_build(const float* sigma, int N, float threshold, int dilate, int32_t* words, void* workspace,
                                       nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(N >= 2 && N <= kMaxN && dilate >= 0 && sigma && words && workspace);
    if (misaligned(sigma, 4) || misaligned(words, 4)) return NERFHIP_E_ALIGN;
    const int M = N - 1;
    const uint32_t n_cells = (uint32_t)M * M * M, n_words = (n_cells + 31) / 32;
    const BuildWs w = build_ws(workspace, M, nullptr);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(occ_cells, dim3(blocks_of(n_cells)), dim3(kBlock), 0, s, sigma, N, threshold, w.a);
    const uint8_t* cells = w.a;
    if (dilate > 0) {
        const int r = dilate < M ? dilate : M;          // r >= M fills the grid's extent along the axis already
        hipLaunchKernelGGL(occ_dilate, dim3(blocks_of(n_cells)), dim3(kBlock), 0, s, (const uint8_t*)w.a, w.b, M, r, 0);
        hipLaunchKernelGGL(occ_dilate, dim3(blocks_of(n_cells)), dim3(kBlock), 0, s, (const uint8_t*)w.b, w.a, M, r, 1);
        hipLaunchKernelGGL(occ_dilate, dim3(blocks_of(n_cells)), dim3(kBlock), 0, s, (const uint8_t*)w.a, w.b, M, r, 2);
        cells = w.b;
    }
    hipLaunchKernelGGL(occ_pack, dim3(blocks_of(n_words)), dim3(kBlock), 0, s, cells, n_cells, n_words, (uint32_t*)words);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_cull_rays(const float* rays, int64_t n, const int32_t* words, int M, const float* ranges_host, uint8_t* hit,
                                 float* t0, float* t1, nerfhip_stream_t stream) {
    OccGrid g;
    const int e = cull_args(rays, n, words, M, ranges_host, hit, t0, t1, g);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(cull_rays, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, (const float4*)rays, n, g, hit, t0, t1);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_cull_rays_host(const float* rays, int64_t n, const int32_t* words, int M, const float* ranges_host, uint8_t* hit,
                                      float* t0, float* t1) {
    OccGrid g;
    const int e = cull_args(rays, n, words, M, ranges_host, hit, t0, t1, g);
    if (e || n == 0) return e;
    nerfhip::host_items(n, CullItem{(const float4*)rays, g, hit, t0, t1});
    return 0;
}

extern "C" size_t nerfhip_cull_compact_workspace_bytes(int64_t n) {
    if (n < 0 || n > kMaxRays) return 0;
    size_t bytes = 0;
    compact_ws(nullptr, n, &bytes);
    return bytes;
}

extern "C" int nerfhip_cull_compact(const uint8_t* hit, const float* rays, const float* t0, const float* t1, int64_t n, int32_t* slot,
                                    int32_t* index, float* rays_out, int32_t* n_hit, void* workspace, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays && n_hit);
    if (misaligned(n_hit, 4)) return NERFHIP_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        CompactWs none{nullptr, nullptr};
        hipLaunchKernelGGL(compact_scan, dim3(1), dim3(kBlock), 0, s, (int64_t)0, none, n_hit);    // *n_hit = 0
        return nerfhip_launch_status();
    }
    NERFHIP_CHECK_ARG(hit && rays && slot && index && rays_out && workspace);
    if (misaligned(rays, 16) || misaligned(rays_out, 16) || misaligned(workspace, 8) || misaligned(t0, 4) || misaligned(t1, 4) ||
        misaligned(slot, 4) || misaligned(index, 4))
        return NERFHIP_E_ALIGN;
    const CompactWs w = compact_ws(workspace, n, nullptr);
    const unsigned nb = blocks_of(n);
    hipLaunchKernelGGL(compact_count, dim3(nb), dim3(kBlock), 0, s, hit, n, w);
    hipLaunchKernelGGL(compact_scan, dim3(1), dim3(kBlock), 0, s, (int64_t)nb, w, n_hit);
    hipLaunchKernelGGL(compact_emit, dim3(nb), dim3(kBlock), 0, s, hit, (const float4*)rays, t0, t1, n, w, slot, index,
                       (float4*)rays_out);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_cull_scatter(const int32_t* slot, int64_t n, int64_t n_compact, int white_back, const float* rgb, float* rgb_out,
                                    const float* depth, float* depth_out, const float* opacity_a, float* opacity_a_out,
                                    const float* opacity_b, float* opacity_b_out, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays && n_compact >= 0 && n_compact <= n);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(slot);
    ScatterArgs a{rgb, rgb_out, {depth, opacity_a, opacity_b}, {depth_out, opacity_a_out, opacity_b_out}};
    // an output without its compact source is refused unless nothing was rendered (then every row is the background)
    NERFHIP_CHECK_ARG(!(rgb_out && !rgb && n_compact > 0));
    for (int k = 0; k < 3; ++k) NERFHIP_CHECK_ARG(!(a.scalar_out[k] && !a.scalar[k] && n_compact > 0));
    if (misaligned(slot, 4)) return NERFHIP_E_ALIGN;
    hipLaunchKernelGGL(cull_scatter, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, slot, n, n_compact,
                       white_back ? 1.0f : 0.0f, a);
    return nerfhip_launch_status();
}

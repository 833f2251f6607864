// The baked RGBA volume on the device: the lattice of a .vol file in 8^3-point bricks, the bitfield of its
// occupied cell bricks and the ray march through both.
//
//   baked_scatter      clear, then one thread per (index, RGBA) record of the file -> its point of the bricked volume
//   baked_from_dense   one thread per point of the bricked volume <- the dense (N,N,N,4) lattice (padding points: zero)
//   baked_bricks       one wave per word of the bitfield: 32 cell bricks, each the 9^3 points (clipped) its cells touch
//   baked_render       one thread per ray: baked_core.h's march (shared with nerfhip_baked_render_host)
//
// Nothing allocates, nothing synchronises; no texture objects, no LDS, no scratch.
#include "common.h"
#include "baked_core.h"
#include "twin_launch.h"

namespace {

using nerfhip::BakedPixel;
using nerfhip::BakedVol;
using nerfhip::baked_point_index;
using nerfhip::blocks_of;
using nerfhip::finite_f32;
using nerfhip::kMaxRays;
using nerfhip::misaligned;

constexpr int kBlock = nerfhip::kItemBlock;
constexpr int kWave = 64;
constexpr int kMaxN = 1625;                    // N^3 < 2^32: the file's point index is a uint32

inline bool lattice_ok(int N) { return N >= 2 && N <= kMaxN; }
inline int64_t point_bricks(int N) { return (N + 7) / 8; }
inline int64_t cell_bricks(int N) { return (N - 1 + 7) / 8; }
inline int64_t bricked_points(int N) { return point_bricks(N) * point_bricks(N) * point_bricks(N) * 512; }

// ---- build --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) baked_clear(uint4* __restrict__ dst, int64_t n16, int32_t* __restrict__ n_bad) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) *n_bad = 0;
    if (i < n16) dst[i] = make_uint4(0u, 0u, 0u, 0u);
}

// record = (i, R << 24 | G << 16 | B << 8 | A) with i = iy N^2 + ix N + iz; an index outside the lattice is counted, not stored
__global__ void __launch_bounds__(kBlock) baked_scatter(const uint2* __restrict__ records, int64_t K, uint32_t N, uint32_t NB,
                                                        uint32_t* __restrict__ points, int32_t* __restrict__ n_bad) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= K) return;
    const uint2 rec = records[k];
    if ((uint64_t)rec.x >= (uint64_t)N * N * N) {
        atomicAdd(n_bad, 1);
        return;
    }
    const uint32_t iz = rec.x % N, row = rec.x / N, ix = row % N, iy = row / N;
    points[baked_point_index((int)NB, iy, ix, iz)] = __builtin_bswap32(rec.y);    // R, G, B, A in memory order
}

__global__ void __launch_bounds__(kBlock) baked_permute(const uint32_t* __restrict__ dense, uint32_t N, uint32_t NB, int64_t n_points,
                                                        uint32_t* __restrict__ points) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_points) return;
    const uint64_t brick = (uint64_t)p >> 9;
    const uint32_t local = (uint32_t)p & 511u;
    const uint32_t bz = (uint32_t)(brick % NB), brow = (uint32_t)(brick / NB), bx = brow % NB, by = brow / NB;
    const uint32_t iy = by * 8 + (local >> 6), ix = bx * 8 + ((local >> 3) & 7u), iz = bz * 8 + (local & 7u);
    const bool inside = iy < N && ix < N && iz < N;
    points[p] = inside ? dense[((uint64_t)iy * N + ix) * N + iz] : 0u;
}

// Cell brick c = (by MB + bx) MB + bz is occupied iff a lattice point with every index in [8 b, 8 b + 8], clipped to the lattice,
// has A > 0.  One wave per word: its 32 bricks one after another, the brick's points strided over the lanes.
__global__ void __launch_bounds__(kWave) baked_bricks(const uint32_t* __restrict__ points, int N, int NB, int MB, uint32_t n_bricks,
                                                      uint32_t* __restrict__ words) {
    const uint32_t word = blockIdx.x;
    const int lane = threadIdx.x;
    uint32_t bits = 0;
    for (uint32_t j = 0; j < 32; ++j) {
        const uint32_t c = word * 32 + j;
        if (c >= n_bricks) break;
        const int bz = (int)(c % (uint32_t)MB), brow = (int)(c / (uint32_t)MB), bx = brow % MB, by = brow / MB;
        bool found = false;
        for (int q = lane; q < 729; q += kWave) {
            const int iy = by * 8 + q / 81, ix = bx * 8 + (q / 9) % 9, iz = bz * 8 + q % 9;
            if (iy < N && ix < N && iz < N)
                found = found || (points[baked_point_index(NB, (uint32_t)iy, (uint32_t)ix, (uint32_t)iz)] >> 24) != 0u;
        }
        if (__any(found)) bits |= 1u << j;
    }
    if (lane == 0) words[word] = bits;
}

// ---- render -------------------------------------------------------------------------------------------------------------------
struct RenderItem {
    const float4* rays;
    BakedVol v;
    float *rgb, *depth, *opacity;    // each may be null
    __host__ __device__ void operator()(int64_t i) const {
        float ray[8];
        nerfhip::load_ray(rays, i, ray);
        const BakedPixel px = nerfhip::baked_march(v, ray);
        if (rgb) {
            rgb[3 * i] = px.rgb[0];
            rgb[3 * i + 1] = px.rgb[1];
            rgb[3 * i + 2] = px.rgb[2];
        }
        if (depth) depth[i] = px.depth;
        if (opacity) opacity[i] = px.opacity;
    }
};

__global__ void __launch_bounds__(kBlock) baked_render(const float4* __restrict__ rays, int64_t n, BakedVol v, float* __restrict__ rgb,
                                                       float* __restrict__ depth, float* __restrict__ opacity) {
    const int64_t i = nerfhip::item_index();
    if (i < n) RenderItem{rays, v, rgb, depth, opacity}(i);
}

// The checks of the two render entry points: everything that can be refused is refused before a pointer is touched.
inline int render_args(const float* rays, int64_t n, const uint8_t* data, const int32_t* words, int N, const float* ranges, float cell,
                       float step, float t_stop, int white_back, const float* rgb, const float* depth, const float* opacity, BakedVol& v) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays && lattice_ok(N) && ranges);
    NERFHIP_CHECK_ARG(cell > 0.0f && finite_f32(cell));
    NERFHIP_CHECK_ARG(step >= 0.0625f && step <= 8.0f);
    NERFHIP_CHECK_ARG(t_stop >= 0.0f && t_stop < 1.0f);
    double diag2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const float lo = ranges[2 * a], hi = ranges[2 * a + 1];
        NERFHIP_CHECK_ARG(finite_f32(lo) && finite_f32(hi) && lo < hi);
        v.lo[a] = lo;
        v.hi[a] = hi;
        v.scale[a] = (float)(N - 1) / (hi - lo);
        NERFHIP_CHECK_ARG(v.scale[a] > 0.0f && finite_f32(v.scale[a]));
        diag2 += ((double)hi - (double)lo) * ((double)hi - (double)lo);
    }
    // the longest chord must not need more segments than a march may take
    NERFHIP_CHECK_ARG(sqrt(diag2) / ((double)step * (double)cell) <= (double)nerfhip::kBakedMaxSegments);
    v.points = (const uint32_t*)data;
    v.bits = (const uint32_t*)words;
    v.N = N;
    v.NB = (int)point_bricks(N);
    v.MB = (int)cell_bricks(N);
    v.cell = cell;
    v.step = step;
    v.t_stop = t_stop;
    v.white_back = white_back ? 1 : 0;
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rays && data);
    if (misaligned(rays, 16) || misaligned(data, 16) || misaligned(words, 4) || misaligned(rgb, 4) || misaligned(depth, 4) ||
        misaligned(opacity, 4))
        return NERFHIP_E_ALIGN;
    return 0;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" size_t nerfhip_baked_bytes(int N) {
    if (!lattice_ok(N)) return 0;
    return (size_t)bricked_points(N) * 4;
}

extern "C" int nerfhip_baked_scatter(const int32_t* records, int64_t K, int N, uint8_t* data, int32_t* n_bad, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(lattice_ok(N) && K >= 0 && K <= ((int64_t)1 << 32) && data && n_bad && (records || K == 0));
    if (misaligned(data, 16) || misaligned(records, 8) || misaligned(n_bad, 4)) return NERFHIP_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n16 = bricked_points(N) / 4;
    hipLaunchKernelGGL(baked_clear, dim3(blocks_of(n16)), dim3(kBlock), 0, s, (uint4*)data, n16, n_bad);
    if (K > 0)
        hipLaunchKernelGGL(baked_scatter, dim3(blocks_of(K)), dim3(kBlock), 0, s, (const uint2*)records, K, (uint32_t)N,
                           (uint32_t)point_bricks(N), (uint32_t*)data, n_bad);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_baked_from_dense(const uint8_t* rgba, int N, uint8_t* data, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(lattice_ok(N) && rgba && data);
    if (misaligned(data, 16) || misaligned(rgba, 4)) return NERFHIP_E_ALIGN;
    const int64_t n_points = bricked_points(N);
    hipLaunchKernelGGL(baked_permute, dim3(blocks_of(n_points)), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t*)rgba, (uint32_t)N,
                       (uint32_t)point_bricks(N), n_points, (uint32_t*)data);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_baked_bricks(const uint8_t* data, int N, int32_t* words, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(lattice_ok(N) && data && words);
    if (misaligned(data, 16) || misaligned(words, 4)) return NERFHIP_E_ALIGN;
    const int64_t MB = cell_bricks(N);
    const uint32_t n_bricks = (uint32_t)(MB * MB * MB), n_words = (n_bricks + 31) / 32;
    hipLaunchKernelGGL(baked_bricks, dim3(n_words), dim3(kWave), 0, (hipStream_t)stream, (const uint32_t*)data, N, (int)point_bricks(N),
                       (int)MB, n_bricks, (uint32_t*)words);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_baked_render(const float* rays, int64_t n, const uint8_t* data, const int32_t* words_or_null, int N,
                                    const float* ranges_host, float cell, float step, float t_stop, int white_back, float* rgb, float* depth,
                                    float* opacity, nerfhip_stream_t stream) {
    BakedVol v;
    const int e = render_args(rays, n, data, words_or_null, N, ranges_host, cell, step, t_stop, white_back, rgb, depth, opacity, v);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(baked_render, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, (const float4*)rays, n, v, rgb, depth,
                       opacity);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_baked_render_host(const float* rays, int64_t n, const uint8_t* data, const int32_t* words_or_null, int N,
                                         const float* ranges_host, float cell, float step, float t_stop, int white_back, float* rgb,
                                         float* depth, float* opacity) {
    BakedVol v;
    const int e = render_args(rays, n, data, words_or_null, N, ranges_host, cell, step, t_stop, white_back, rgb, depth, opacity, v);
    if (e || n == 0) return e;
    nerfhip::host_items(n, RenderItem{(const float4*)rays, v, rgb, depth, opacity});
    return 0;
}

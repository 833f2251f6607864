// Mesh decimation on the device: grid vertex clustering with mean or quadric placement.  Every routine that
// computes is decimate_core.h's, shared with the _host twins below; torch.sort runs between the calls (ops._mesh_decimate).
//
//   dc_bounds            a grid-stride loop over the vertices: counts the non-finite ones, folds the others' bounds (wave reduction,
//                        then at most 7 integer atomics per wave)
//   dc_keys              one thread per vertex: cell << 32 | vertex                                                          [sort]
//   dc_heads, dc_number  one thread per sorted vertex: segment heads, their block totals; the cluster numbers and segment starts
//   dc_entries           one thread per triangle: cluster << 32 | 3 t + k for its three corners                             [sort]
//   dc_mean, dc_quadric  one thread per cluster: loops bounded by the segment's length
//   dc_tri_keys          one thread per triangle: remap, flag, the two halves of the duplicate key                  [two sorts]
//   dc_duplicates        one thread per sorted triangle: equal to its predecessor -> flagged
//   dc_mark, dc_count_*  referenced clusters, block totals of the survivors and of the referenced; dc_scan_tri_totals: the counts
//   dc_compact_*         clusters, triangles, cluster_of
//
// The cross-block scans are block_scan.h's, with one single-workgroup launch over the block totals between the counting and the
// writing launch (dc_scan_totals: mesh.hip's scan_totals for one array).  Nothing is handed between workgroups within a launch, no
// atomics but the bounds' integer minima and maxima, no retry loops; nothing allocates, nothing synchronises.
#include "block_scan.h"
#include "common.h"
#include "decimate_core.h"
#include "mesh_core.h"
#include "twin_launch.h"

namespace {

using nerfhip::block_excl_scan;
using nerfhip::blocks_of;
using nerfhip::DecimateGrid;
using nerfhip::kDecimateMaxItems;
using nerfhip::kDecimateNoCell;
using nerfhip::misaligned;

constexpr int kBlock = nerfhip::kItemBlock;
constexpr int kScanBlock = 1024;    // the single workgroup that scans the block totals
constexpr unsigned kBoundsBlocks = 2048;    // dc_bounds: 8 blocks for each of the 256 compute units

// ---- bounds and keys ----------------------------------------------------------------------------------------------------------
// state: 8 words.  [0] the number of non-finite vertices, [1] zero, [2..4] / [5..7] the finite vertices' lo / hi in mesh_ordered's
// encoding.
__global__ void dc_state_init(uint32_t* __restrict__ state) {
    const int i = threadIdx.x;
    if (i < 8) state[i] = i < 2 ? 0u : nerfhip::mesh_ordered(nerfhip::float_from_bits(i < 5 ? 0x7f800000u : 0xff800000u));
}

__global__ void __launch_bounds__(kBlock) dc_bounds(const float* __restrict__ vertices, int64_t V, uint32_t* __restrict__ state) {
    const float inf = nerfhip::float_from_bits(0x7f800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    int bad = 0;
    // a grid of at most kBoundsBlocks blocks strides over the vertices: the atomics below are per wave, not per 64 vertices
    for (int64_t v = nerfhip::item_index(); v < V; v += (int64_t)gridDim.x * kBlock) {
        if (nerfhip::decimate_finite(vertices + 3 * v)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = nerfhip::mesh_min(lo[a], vertices[3 * v + a]);
                hi[a] = nerfhip::mesh_max(hi[a], vertices[3 * v + a]);
            }
        } else {
            ++bad;
        }
    }
    // every lane of the wave is here: the loop's exits are per lane, the shuffles below are not inside it
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = nerfhip::mesh_min(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = nerfhip::mesh_max(hi[a], __shfl_xor(hi[a], o, 64));
        }
        bad += __shfl_xor(bad, o, 64);
    }
    // An atomic only where the wave would move the bound it reads: the bounds only ever move outwards, so a stale read can cost
    // a needless atomic and never loses one (a few hundred thousand atomics on six words otherwise take milliseconds).
    if (nerfhip::lane_id() == 0) {
        if (bad) atomicAdd(state, (uint32_t)bad);
        if (lo[0] <= hi[0]) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const uint32_t l = nerfhip::mesh_ordered(lo[a]), h = nerfhip::mesh_ordered(hi[a]);
                if (l < __hip_atomic_load(state + 2 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(state + 2 + a, l);
                if (h > __hip_atomic_load(state + 5 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(state + 5 + a, h);
            }
        }
    }
}

struct KeyItem {
    const float* vertices;
    DecimateGrid g;
    int64_t* keys;
    __host__ __device__ void operator()(int64_t v) const { keys[v] = nerfhip::decimate_vertex_key(vertices + 3 * v, g, v); }
};

__global__ void __launch_bounds__(kBlock) dc_keys(const float* __restrict__ vertices, int64_t V, DecimateGrid g, int64_t* __restrict__ keys) {
    const int64_t v = nerfhip::item_index();
    if (v < V) KeyItem{vertices, g, keys}(v);
}

// ---- clusters -----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool segment_head(const int64_t* __restrict__ sorted_keys, int64_t i) {
    const int64_t c = sorted_keys[i] >> 32;
    return c != kDecimateNoCell && (i == 0 || (sorted_keys[i - 1] >> 32) != c);
}

__global__ void __launch_bounds__(kBlock) dc_heads(const int64_t* __restrict__ sorted_keys, int64_t V, int32_t* __restrict__ blk) {
    const int64_t i = nerfhip::item_index();
    int tot;
    block_excl_scan<kBlock>(i < V && segment_head(sorted_keys, i) ? 1 : 0, tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// One workgroup: exclusive offsets of the n block totals and their sum.
__global__ void __launch_bounds__(kScanBlock) dc_scan_totals(const int32_t* __restrict__ blk, int64_t n, int64_t* __restrict__ off,
                                                             int64_t* __restrict__ total) {
    const int64_t sum = nerfhip::block_offsets_scan<kScanBlock>(n, off, [&](int64_t i) { return blk[i]; });
    if (threadIdx.x == 0) *total = sum;
}

// Sorted position i of a vertex in cluster `num`: cluster_of, and the segment's start / end where i is its first / the last vertex
// of all clusters.  The one text of the kernel and the host loop.
__host__ __device__ inline void number_store(const int64_t* __restrict__ sorted_keys, int64_t V, int64_t i, bool head, int64_t num,
                                             int32_t* __restrict__ cluster_of, int32_t* __restrict__ seg_start) {
    const int64_t key = sorted_keys[i], vid = key & 0xffffffffll;
    if (vid >= V) return;
    if ((key >> 32) == kDecimateNoCell) {
        cluster_of[vid] = -1;
        return;
    }
    cluster_of[vid] = (int32_t)num;
    if (head) seg_start[num] = (int32_t)i;
    if (i == V - 1 || (sorted_keys[i + 1] >> 32) == kDecimateNoCell) seg_start[num + 1] = (int32_t)(i + 1);
}

__global__ void __launch_bounds__(kBlock) dc_number(const int64_t* __restrict__ sorted_keys, int64_t V, const int64_t* __restrict__ off,
                                                    int32_t* __restrict__ cluster_of, int32_t* __restrict__ seg_start) {
    const int64_t i = nerfhip::item_index();
    const int f = i < V && segment_head(sorted_keys, i) ? 1 : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(f, tot);
    if (i < V) number_store(sorted_keys, V, i, f, off[blockIdx.x] + ex + f - 1, cluster_of, seg_start);
}

// ---- placement ----------------------------------------------------------------------------------------------------------------
struct EntryItem {
    const int32_t* triangles;
    int64_t V;
    const int32_t* cluster_of;
    int64_t* keys;
    __host__ __device__ void operator()(int64_t t) const {
        int32_t id[3];
        const bool ok = nerfhip::decimate_triangle(triangles, t, V, cluster_of, id);
#pragma unroll
        for (int k = 0; k < 3; ++k) keys[3 * t + k] = ((ok ? (int64_t)id[k] : kDecimateNoCell) << 32) | (3 * t + k);
    }
};

__global__ void __launch_bounds__(kBlock) dc_entries(const int32_t* __restrict__ triangles, int64_t T, int64_t V,
                                                     const int32_t* __restrict__ cluster_of, int64_t* __restrict__ keys) {
    const int64_t t = nerfhip::item_index();
    if (t < T) EntryItem{triangles, V, cluster_of, keys}(t);
}

struct MeanItem {
    const float* vertices;
    int64_t V;
    const uint8_t* colors;    // may be null, with colors_out
    const int64_t* sorted_keys;
    const int32_t* seg_start;
    double* mean;
    float* positions;
    uint8_t* colors_out;
    __host__ __device__ void operator()(int64_t c) const {
        int64_t s0 = seg_start[c], s1 = seg_start[c + 1];
        s0 = s0 < 0 ? 0 : s0;
        s1 = s1 > V ? V : s1;
        double m[3] = {0.0, 0.0, 0.0};
        uint8_t rgb[3] = {0, 0, 0};
        if (s0 < s1) nerfhip::decimate_mean(vertices, V, colors, sorted_keys, s0, s1, m, rgb);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mean[3 * c + a] = m[a];
            positions[3 * c + a] = (float)m[a];
            if (colors_out) colors_out[3 * c + a] = rgb[a];
        }
    }
};

__global__ void __launch_bounds__(kBlock) dc_mean(const float* __restrict__ vertices, int64_t V, const uint8_t* __restrict__ colors,
                                                  const int64_t* __restrict__ sorted_keys, const int32_t* __restrict__ seg_start, int64_t C,
                                                  double* __restrict__ mean, float* __restrict__ positions, uint8_t* __restrict__ colors_out) {
    const int64_t c = nerfhip::item_index();
    if (c < C) MeanItem{vertices, V, colors, sorted_keys, seg_start, mean, positions, colors_out}(c);
}

struct QuadricItem {
    const float* vertices;
    int64_t V;
    const int32_t* triangles;
    int64_t T;
    const int64_t* sorted_keys;
    const int32_t* seg_start;
    const int64_t* sorted_entries;
    const double* mean;
    float* positions;
    DecimateGrid g;
    double eps;
    __host__ __device__ void operator()(int64_t c) const {
        const int64_t s0 = seg_start[c];
        if (s0 < 0 || s0 >= V) return;
        const int64_t e0 = nerfhip::decimate_lower_bound(sorted_entries, 3 * T, c << 32);
        const int64_t e1 = nerfhip::decimate_lower_bound(sorted_entries, 3 * T, (c + 1) << 32);
        double pos[3];
        nerfhip::decimate_quadric(vertices, V, triangles, T, sorted_entries, e0, e1, mean + 3 * c, sorted_keys[s0] >> 32, g, eps, pos);
#pragma unroll
        for (int a = 0; a < 3; ++a) positions[3 * c + a] = (float)pos[a];
    }
};

__global__ void __launch_bounds__(kBlock) dc_quadric(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles,
                                                     int64_t T, const int64_t* __restrict__ sorted_keys, const int32_t* __restrict__ seg_start,
                                                     const int64_t* __restrict__ sorted_entries, int64_t C, const double* __restrict__ mean,
                                                     float* __restrict__ positions, DecimateGrid g, double eps) {
    const int64_t c = nerfhip::item_index();
    if (c < C) QuadricItem{vertices, V, triangles, T, sorted_keys, seg_start, sorted_entries, mean, positions, g, eps}(c);
}

// ---- triangles ----------------------------------------------------------------------------------------------------------------
struct TriKeyItem {
    const int32_t* triangles;
    int64_t V;
    const int32_t* cluster_of;
    uint8_t* flags;
    int64_t *key_hi, *key_lo;
    __host__ __device__ void operator()(int64_t t) const {
        int64_t hi, lo;
        flags[t] = (uint8_t)nerfhip::decimate_triangle_key(triangles, t, V, cluster_of, hi, lo);
        key_hi[t] = hi;
        key_lo[t] = lo;
    }
};

__global__ void __launch_bounds__(kBlock) dc_tri_keys(const int32_t* __restrict__ triangles, int64_t T, int64_t V,
                                                      const int32_t* __restrict__ cluster_of, uint8_t* __restrict__ flags,
                                                      int64_t* __restrict__ key_hi, int64_t* __restrict__ key_lo) {
    const int64_t t = nerfhip::item_index();
    if (t < T) TriKeyItem{triangles, V, cluster_of, flags, key_hi, key_lo}(t);
}

// Sorted position i >= 1: a candidate whose (a, b, c) equals its predecessor's is a duplicate (the predecessor has the lower t).
struct DuplicateItem {
    const int64_t *sorted_hi, *sorted_lo;
    int64_t T;
    uint8_t* flags;
    __host__ __device__ void operator()(int64_t j) const {
        const int64_t i = j + 1;
        if (sorted_hi[i] == nerfhip::kDecimateNoKey || sorted_hi[i] != sorted_hi[i - 1]) return;
        if ((sorted_lo[i] >> 28) != (sorted_lo[i - 1] >> 28)) return;
        const int64_t t = sorted_lo[i] & nerfhip::kDecimateIdMask;
        if (t < T) flags[t] = nerfhip::kDecimateDuplicate;
    }
};

__global__ void __launch_bounds__(kBlock) dc_duplicates(const int64_t* __restrict__ sorted_hi, const int64_t* __restrict__ sorted_lo, int64_t T,
                                                        uint8_t* __restrict__ flags) {
    const int64_t j = nerfhip::item_index();
    if (j + 1 < T) DuplicateItem{sorted_hi, sorted_lo, T, flags}(j);
}

// ---- mark, count, compact -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) dc_zero(uint8_t* __restrict__ ref, int64_t C, int64_t* __restrict__ totals) {
    const int64_t i = nerfhip::item_index();
    if (i < C) ref[i] = 0;
    if (i < 5) totals[i] = 0;
}

struct MarkItem {
    const int32_t* triangles;
    int64_t V;
    const int32_t* cluster_of;
    const uint8_t* flags;
    int64_t C;
    uint8_t* ref;
    __host__ __device__ void operator()(int64_t t) const {
        int32_t id[3];
        if (flags[t] != nerfhip::kDecimateKeep || !nerfhip::decimate_triangle(triangles, t, V, cluster_of, id)) return;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (id[k] < C) ref[id[k]] = 1;    // the same value from every writer
    }
};

__global__ void __launch_bounds__(kBlock) dc_mark(const int32_t* __restrict__ triangles, int64_t T, int64_t V,
                                                  const int32_t* __restrict__ cluster_of, const uint8_t* __restrict__ flags, int64_t C,
                                                  uint8_t* __restrict__ ref) {
    const int64_t t = nerfhip::item_index();
    if (t < T) MarkItem{triangles, V, cluster_of, flags, C, ref}(t);
}

// Per block the survivors (blk) and, in `packed`, the block's four counts — survivors, bad, collapsed, duplicate — 16 bits each
// (each holds up to 256): one scan for the four.
__global__ void __launch_bounds__(kBlock) dc_count_tris(const uint8_t* __restrict__ flags, int64_t T, int32_t* __restrict__ blk,
                                                        int64_t* __restrict__ packed) {
    const int64_t t = nerfhip::item_index();
    int64_t tot;
    block_excl_scan<kBlock>(t < T ? (int64_t)1 << (16 * (flags[t] & 3)) : (int64_t)0, tot);
    if (threadIdx.x != 0) return;
    blk[blockIdx.x] = (int32_t)(tot & 0xffff);
    packed[blockIdx.x] = tot;
}

// One workgroup: dc_scan_totals for the survivors, after the sums of the other three counts over the packed block totals, which
// `off` holds on entry (thread i reads and later writes the elements i mod 1024) -> totals[0], totals[2..4].  No atomics.
__global__ void __launch_bounds__(kScanBlock) dc_scan_tri_totals(const int32_t* __restrict__ blk, int64_t n, int64_t* __restrict__ off,
                                                                 int64_t* __restrict__ totals) {
    int64_t mine[3] = {0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += kScanBlock) {
        const int64_t p = off[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) mine[k] += (p >> (16 * (k + 1))) & 0xffff;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int64_t all;
        block_excl_scan<kScanBlock>(mine[k], all);
        if (threadIdx.x == 0) totals[2 + k] = all;
    }
    const int64_t sum = nerfhip::block_offsets_scan<kScanBlock>(n, off, [&](int64_t i) { return blk[i]; });
    if (threadIdx.x == 0) totals[0] = sum;
}

__global__ void __launch_bounds__(kBlock) dc_count_ref(const uint8_t* __restrict__ ref, int64_t C, int32_t* __restrict__ blk) {
    const int64_t i = nerfhip::item_index();
    int tot;
    block_excl_scan<kBlock>(i < C ? (int)ref[i] : 0, tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kBlock) dc_compact_clusters(int64_t C, const uint8_t* __restrict__ ref, const int64_t* __restrict__ off,
                                                              const float* __restrict__ positions, const uint8_t* __restrict__ colors,
                                                              int32_t* __restrict__ vnew, float* __restrict__ out_vertices,
                                                              uint8_t* __restrict__ out_colors) {
    const int64_t c = nerfhip::item_index();
    const int f = c < C ? ref[c] : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(f, tot);
    if (c >= C) return;
    const int64_t id = off[blockIdx.x] + ex;
    vnew[c] = f ? (int32_t)id : -1;
    if (!f) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out_vertices[3 * id + a] = positions[3 * c + a];
        if (colors) out_colors[3 * id + a] = colors[3 * c + a];
    }
}

// Survivor t as output triangle `id`: its corners' clusters through vnew, in its own corner order.
__host__ __device__ inline void triangle_store(const int32_t* __restrict__ triangles, int64_t t, int64_t V, const int32_t* __restrict__ cluster_of,
                                               int64_t C, const int32_t* __restrict__ vnew, int64_t id, int32_t* __restrict__ out) {
    int32_t ids[3];
    nerfhip::decimate_triangle(triangles, t, V, cluster_of, ids);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * id + k] = ids[k] >= 0 && ids[k] < C ? vnew[ids[k]] : -1;
}

__global__ void __launch_bounds__(kBlock) dc_compact_tris(const int32_t* __restrict__ triangles, int64_t T, int64_t V,
                                                          const int32_t* __restrict__ cluster_of, const uint8_t* __restrict__ flags, int64_t C,
                                                          const int64_t* __restrict__ off, const int32_t* __restrict__ vnew,
                                                          int32_t* __restrict__ out) {
    const int64_t t = nerfhip::item_index();
    const int f = t < T && flags[t] == nerfhip::kDecimateKeep ? 1 : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(f, tot);
    if (f) triangle_store(triangles, t, V, cluster_of, C, vnew, off[blockIdx.x] + ex, out);
}

struct RemapItem {
    const int32_t* cluster_of;
    int64_t C;
    const int32_t* vnew;
    int32_t* out;
    __host__ __device__ void operator()(int64_t v) const {
        const int32_t c = cluster_of[v];
        out[v] = c >= 0 && c < C ? vnew[c] : -1;
    }
};

__global__ void __launch_bounds__(kBlock) dc_remap(const int32_t* __restrict__ cluster_of, int64_t V, int64_t C, const int32_t* __restrict__ vnew,
                                                   int32_t* __restrict__ out) {
    const int64_t v = nerfhip::item_index();
    if (v < V) RemapItem{cluster_of, C, vnew, out}(v);
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------
inline bool counts_ok(int64_t V, int64_t T) { return V >= 0 && V <= kDecimateMaxItems && T >= 0 && T <= kDecimateMaxItems; }

inline int grid_of(const float* lo_host, float cell, const int32_t* res_host, DecimateGrid& g) {
    NERFHIP_CHECK_ARG(lo_host && res_host && cell > 0.0f && nerfhip::finite_f32(cell));
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        NERFHIP_CHECK_ARG(nerfhip::finite_f32(lo_host[a]) && res_host[a] >= 1);
        g.lo[a] = lo_host[a];
        g.R[a] = res_host[a];
        cells *= res_host[a];
        NERFHIP_CHECK_ARG(cells < ((int64_t)1 << 31));
    }
    g.cell = cell;
    return 0;
}

inline int keys_args(const float* vertices, int64_t V, const float* lo_host, float cell, const int32_t* res_host, const int64_t* keys,
                     DecimateGrid& g) {
    NERFHIP_CHECK_ARG(counts_ok(V, 0));
    const int e = grid_of(lo_host, cell, res_host, g);
    if (e || V == 0) return e;
    NERFHIP_CHECK_ARG(vertices && keys);
    return misaligned(vertices, 4) || misaligned(keys, 8) ? NERFHIP_E_ALIGN : 0;
}

inline int clusters_args(const int64_t* sorted_keys, int64_t V, const int32_t* blk, const int64_t* off, const int32_t* cluster_of,
                         const int32_t* seg_start, const int64_t* totals) {
    NERFHIP_CHECK_ARG(counts_ok(V, 0) && totals);
    if (misaligned(totals, 8)) return NERFHIP_E_ALIGN;
    if (V == 0) return 0;
    NERFHIP_CHECK_ARG(sorted_keys && blk && off && cluster_of && seg_start);
    return misaligned(sorted_keys, 8) || misaligned(blk, 4) || misaligned(off, 8) || misaligned(cluster_of, 4) || misaligned(seg_start, 4)
               ? NERFHIP_E_ALIGN
               : 0;
}

inline int entries_args(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const int64_t* keys) {
    NERFHIP_CHECK_ARG(counts_ok(V, T));
    if (T == 0) return 0;
    NERFHIP_CHECK_ARG(triangles && keys && (cluster_of || V == 0));
    return misaligned(triangles, 4) || misaligned(cluster_of, 4) || misaligned(keys, 8) ? NERFHIP_E_ALIGN : 0;
}

inline int place_args(const float* vertices, int64_t V, const uint8_t* colors, const int32_t* triangles, int64_t T, const int64_t* sorted_keys,
                      const int32_t* seg_start, int64_t C, const int64_t* sorted_entries, const float* lo_host, float cell,
                      const int32_t* res_host, double eps, int placement, const double* mean, const float* positions, const uint8_t* colors_out,
                      DecimateGrid& g) {
    NERFHIP_CHECK_ARG(counts_ok(V, T) && C >= 0 && C <= V && (placement == 0 || placement == 1) && eps > 0.0 && eps <= 1.0);
    NERFHIP_CHECK_ARG(!colors == !colors_out);
    const int e = grid_of(lo_host, cell, res_host, g);
    if (e || C == 0) return e;
    NERFHIP_CHECK_ARG(vertices && sorted_keys && seg_start && mean && positions);
    NERFHIP_CHECK_ARG(placement == 0 || T == 0 || (triangles && sorted_entries));
    return misaligned(vertices, 4) || misaligned(triangles, 4) || misaligned(sorted_keys, 8) || misaligned(seg_start, 4) ||
                   misaligned(sorted_entries, 8) || misaligned(mean, 8) || misaligned(positions, 4)
               ? NERFHIP_E_ALIGN
               : 0;
}

inline int tri_keys_args(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags, const int64_t* key_hi,
                         const int64_t* key_lo) {
    NERFHIP_CHECK_ARG(counts_ok(V, T));
    if (T == 0) return 0;
    NERFHIP_CHECK_ARG(triangles && flags && key_hi && key_lo && (cluster_of || V == 0));
    return misaligned(triangles, 4) || misaligned(cluster_of, 4) || misaligned(key_hi, 8) || misaligned(key_lo, 8) ? NERFHIP_E_ALIGN : 0;
}

inline int duplicates_args(const int64_t* sorted_hi, const int64_t* sorted_lo, int64_t T, const uint8_t* flags) {
    NERFHIP_CHECK_ARG(counts_ok(0, T));
    if (T == 0) return 0;
    NERFHIP_CHECK_ARG(sorted_hi && sorted_lo && flags);
    return misaligned(sorted_hi, 8) || misaligned(sorted_lo, 8) ? NERFHIP_E_ALIGN : 0;
}

inline int mark_args(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags, int64_t C, const uint8_t* ref,
                     const int32_t* blk_t, const int64_t* off_t, const int32_t* blk_c, const int64_t* off_c, const int64_t* totals) {
    NERFHIP_CHECK_ARG(counts_ok(V, T) && C >= 0 && C <= V && totals);
    NERFHIP_CHECK_ARG(T == 0 || (triangles && flags && blk_t && off_t && (cluster_of || V == 0)));
    NERFHIP_CHECK_ARG(C == 0 || (ref && blk_c && off_c));
    return misaligned(triangles, 4) || misaligned(cluster_of, 4) || misaligned(blk_t, 4) || misaligned(off_t, 8) || misaligned(blk_c, 4) ||
                   misaligned(off_c, 8) || misaligned(totals, 8)
               ? NERFHIP_E_ALIGN
               : 0;
}

inline int compact_args(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags, int64_t C,
                        const uint8_t* ref, const int64_t* off_t, const int64_t* off_c, const float* positions, const uint8_t* colors,
                        const int32_t* vnew, const float* out_vertices, const int32_t* out_triangles, const uint8_t* out_colors,
                        const int32_t* out_cluster_of) {
    NERFHIP_CHECK_ARG(counts_ok(V, T) && C >= 0 && C <= V && !colors == !out_colors);
    NERFHIP_CHECK_ARG(T == 0 || (triangles && flags && off_t && out_triangles && (cluster_of || V == 0)));
    NERFHIP_CHECK_ARG(C == 0 || (ref && off_c && positions && vnew && out_vertices));
    NERFHIP_CHECK_ARG(V == 0 || (cluster_of && out_cluster_of));
    return misaligned(triangles, 4) || misaligned(cluster_of, 4) || misaligned(off_t, 8) || misaligned(off_c, 8) || misaligned(positions, 4) ||
                   misaligned(vnew, 4) || misaligned(out_vertices, 4) || misaligned(out_triangles, 4) || misaligned(out_cluster_of, 4)
               ? NERFHIP_E_ALIGN
               : 0;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" int nerfhip_mesh_decimate_bounds(const float* vertices, int64_t V, int32_t* state, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(counts_ok(V, 0) && state && (V == 0 || vertices));
    if (misaligned(vertices, 4) || misaligned(state, 4)) return NERFHIP_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dc_state_init, dim3(1), dim3(64), 0, s, (uint32_t*)state);
    if (V > 0)
        hipLaunchKernelGGL(dc_bounds, dim3(blocks_of(V) < kBoundsBlocks ? blocks_of(V) : kBoundsBlocks), dim3(kBlock), 0, s, vertices, V,
                           (uint32_t*)state);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_bounds_host(const float* vertices, int64_t V, int32_t* state) {
    NERFHIP_CHECK_ARG(counts_ok(V, 0) && state && (V == 0 || vertices));
    if (misaligned(vertices, 4) || misaligned(state, 4)) return NERFHIP_E_ALIGN;
    const float inf = nerfhip::float_from_bits(0x7f800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    int32_t bad = 0;
    for (int64_t v = 0; v < V; ++v) {
        if (!nerfhip::decimate_finite(vertices + 3 * v)) {
            ++bad;
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = nerfhip::mesh_min(lo[a], vertices[3 * v + a]);
            hi[a] = nerfhip::mesh_max(hi[a], vertices[3 * v + a]);
        }
    }
    state[0] = bad;
    state[1] = 0;
    for (int a = 0; a < 3; ++a) {
        state[2 + a] = (int32_t)nerfhip::mesh_ordered(lo[a]);
        state[5 + a] = (int32_t)nerfhip::mesh_ordered(hi[a]);
    }
    return 0;
}

extern "C" int nerfhip_mesh_decimate_keys(const float* vertices, int64_t V, const float* lo_host, float cell, const int32_t* res_host,
                                          int64_t* keys, nerfhip_stream_t stream) {
    DecimateGrid g;
    const int e = keys_args(vertices, V, lo_host, cell, res_host, keys, g);
    if (e || V == 0) return e;
    hipLaunchKernelGGL(dc_keys, dim3(blocks_of(V)), dim3(kBlock), 0, (hipStream_t)stream, vertices, V, g, keys);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_keys_host(const float* vertices, int64_t V, const float* lo_host, float cell, const int32_t* res_host,
                                               int64_t* keys) {
    DecimateGrid g;
    const int e = keys_args(vertices, V, lo_host, cell, res_host, keys, g);
    if (e || V == 0) return e;
    nerfhip::host_items(V, KeyItem{vertices, g, keys});
    return 0;
}

extern "C" int nerfhip_mesh_decimate_clusters(const int64_t* sorted_keys, int64_t V, int32_t* blk, int64_t* off, int32_t* cluster_of,
                                              int32_t* seg_start, int64_t* totals, nerfhip_stream_t stream) {
    const int e = clusters_args(sorted_keys, V, blk, off, cluster_of, seg_start, totals);
    if (e) return e;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = blocks_of(V);
    if (V > 0) hipLaunchKernelGGL(dc_heads, dim3(nb), dim3(kBlock), 0, s, sorted_keys, V, blk);
    hipLaunchKernelGGL(dc_scan_totals, dim3(1), dim3(kScanBlock), 0, s, (const int32_t*)blk, (int64_t)nb, off, totals);
    if (V > 0) hipLaunchKernelGGL(dc_number, dim3(nb), dim3(kBlock), 0, s, sorted_keys, V, (const int64_t*)off, cluster_of, seg_start);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_clusters_host(const int64_t* sorted_keys, int64_t V, int32_t* blk, int64_t* off, int32_t* cluster_of,
                                                   int32_t* seg_start, int64_t* totals) {
    const int e = clusters_args(sorted_keys, V, blk, off, cluster_of, seg_start, totals);
    if (e) return e;
    int64_t num = -1;
    for (int64_t i = 0; i < V; ++i) {
        const bool head = segment_head(sorted_keys, i);
        num += head;
        number_store(sorted_keys, V, i, head, num, cluster_of, seg_start);
    }
    totals[0] = num + 1;
    return 0;
}

extern "C" int nerfhip_mesh_decimate_entries(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, int64_t* keys,
                                             nerfhip_stream_t stream) {
    const int e = entries_args(triangles, T, V, cluster_of, keys);
    if (e || T == 0) return e;
    hipLaunchKernelGGL(dc_entries, dim3(blocks_of(T)), dim3(kBlock), 0, (hipStream_t)stream, triangles, T, V, cluster_of, keys);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_entries_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, int64_t* keys) {
    const int e = entries_args(triangles, T, V, cluster_of, keys);
    if (e || T == 0) return e;
    nerfhip::host_items(T, EntryItem{triangles, V, cluster_of, keys});
    return 0;
}

extern "C" int nerfhip_mesh_decimate_place(const float* vertices, int64_t V, const uint8_t* colors_or_null, const int32_t* triangles, int64_t T,
                                           const int64_t* sorted_keys, const int32_t* seg_start, int64_t C, const int64_t* sorted_entries,
                                           const float* lo_host, float cell, const int32_t* res_host, double eps, int placement, double* mean,
                                           float* positions, uint8_t* colors_out_or_null, nerfhip_stream_t stream) {
    DecimateGrid g;
    const int e = place_args(vertices, V, colors_or_null, triangles, T, sorted_keys, seg_start, C, sorted_entries, lo_host, cell, res_host, eps,
                             placement, mean, positions, colors_out_or_null, g);
    if (e || C == 0) return e;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dc_mean, dim3(blocks_of(C)), dim3(kBlock), 0, s, vertices, V, colors_or_null, sorted_keys, seg_start, C, mean, positions,
                       colors_out_or_null);
    if (placement == 1)
        hipLaunchKernelGGL(dc_quadric, dim3(blocks_of(C)), dim3(kBlock), 0, s, vertices, V, triangles, T, sorted_keys, seg_start, sorted_entries, C,
                           (const double*)mean, positions, g, eps);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_place_host(const float* vertices, int64_t V, const uint8_t* colors_or_null, const int32_t* triangles,
                                                int64_t T, const int64_t* sorted_keys, const int32_t* seg_start, int64_t C,
                                                const int64_t* sorted_entries, const float* lo_host, float cell, const int32_t* res_host,
                                                double eps, int placement, double* mean, float* positions, uint8_t* colors_out_or_null) {
    DecimateGrid g;
    const int e = place_args(vertices, V, colors_or_null, triangles, T, sorted_keys, seg_start, C, sorted_entries, lo_host, cell, res_host, eps,
                             placement, mean, positions, colors_out_or_null, g);
    if (e || C == 0) return e;
    nerfhip::host_items(C, MeanItem{vertices, V, colors_or_null, sorted_keys, seg_start, mean, positions, colors_out_or_null});
    if (placement == 1)
        nerfhip::host_items(C, QuadricItem{vertices, V, triangles, T, sorted_keys, seg_start, sorted_entries, mean, positions, g, eps});
    return 0;
}

extern "C" int nerfhip_mesh_decimate_tri_keys(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, uint8_t* flags,
                                              int64_t* key_hi, int64_t* key_lo, nerfhip_stream_t stream) {
    const int e = tri_keys_args(triangles, T, V, cluster_of, flags, key_hi, key_lo);
    if (e || T == 0) return e;
    hipLaunchKernelGGL(dc_tri_keys, dim3(blocks_of(T)), dim3(kBlock), 0, (hipStream_t)stream, triangles, T, V, cluster_of, flags, key_hi, key_lo);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_tri_keys_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, uint8_t* flags,
                                                   int64_t* key_hi, int64_t* key_lo) {
    const int e = tri_keys_args(triangles, T, V, cluster_of, flags, key_hi, key_lo);
    if (e || T == 0) return e;
    nerfhip::host_items(T, TriKeyItem{triangles, V, cluster_of, flags, key_hi, key_lo});
    return 0;
}

extern "C" int nerfhip_mesh_decimate_duplicates(const int64_t* sorted_hi, const int64_t* sorted_lo, int64_t T, uint8_t* flags,
                                                nerfhip_stream_t stream) {
    const int e = duplicates_args(sorted_hi, sorted_lo, T, flags);
    if (e || T < 2) return e;
    hipLaunchKernelGGL(dc_duplicates, dim3(blocks_of(T - 1)), dim3(kBlock), 0, (hipStream_t)stream, sorted_hi, sorted_lo, T, flags);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_duplicates_host(const int64_t* sorted_hi, const int64_t* sorted_lo, int64_t T, uint8_t* flags) {
    const int e = duplicates_args(sorted_hi, sorted_lo, T, flags);
    if (e || T < 2) return e;
    nerfhip::host_items(T - 1, DuplicateItem{sorted_hi, sorted_lo, T, flags});
    return 0;
}

extern "C" int nerfhip_mesh_decimate_mark(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags,
                                          int64_t C, uint8_t* ref, int32_t* blk_t, int64_t* off_t, int32_t* blk_c, int64_t* off_c,
                                          int64_t* totals, nerfhip_stream_t stream) {
    const int e = mark_args(triangles, T, V, cluster_of, flags, C, ref, blk_t, off_t, blk_c, off_c, totals);
    if (e) return e;
    hipStream_t s = (hipStream_t)stream;
    const unsigned bt = blocks_of(T), bc = blocks_of(C);
    hipLaunchKernelGGL(dc_zero, dim3(bc ? bc : 1), dim3(kBlock), 0, s, ref, C, totals);
    if (T > 0 && C > 0) hipLaunchKernelGGL(dc_mark, dim3(bt), dim3(kBlock), 0, s, triangles, T, V, cluster_of, flags, C, ref);
    if (T > 0) hipLaunchKernelGGL(dc_count_tris, dim3(bt), dim3(kBlock), 0, s, flags, T, blk_t, off_t);
    if (C > 0) hipLaunchKernelGGL(dc_count_ref, dim3(bc), dim3(kBlock), 0, s, (const uint8_t*)ref, C, blk_c);
    hipLaunchKernelGGL(dc_scan_tri_totals, dim3(1), dim3(kScanBlock), 0, s, (const int32_t*)blk_t, (int64_t)bt, off_t, totals);
    hipLaunchKernelGGL(dc_scan_totals, dim3(1), dim3(kScanBlock), 0, s, (const int32_t*)blk_c, (int64_t)bc, off_c, totals + 1);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_mark_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags,
                                               int64_t C, uint8_t* ref, int32_t* blk_t, int64_t* off_t, int32_t* blk_c, int64_t* off_c,
                                               int64_t* totals) {
    const int e = mark_args(triangles, T, V, cluster_of, flags, C, ref, blk_t, off_t, blk_c, off_c, totals);
    if (e) return e;
    for (int k = 0; k < 5; ++k) totals[k] = 0;
    for (int64_t c = 0; c < C; ++c) ref[c] = 0;
    if (C > 0) nerfhip::host_items(T, MarkItem{triangles, V, cluster_of, flags, C, ref});
    // the block totals and offsets as the device leaves them: the compaction reads the offsets
    for (int64_t t = 0; t < T; ++t) {
        if (t % kBlock == 0) {
            blk_t[t / kBlock] = 0;
            off_t[t / kBlock] = totals[0];
        }
        const int f = flags[t] & 3;
        if (f == nerfhip::kDecimateKeep) {
            ++blk_t[t / kBlock];
            ++totals[0];
        } else {
            ++totals[1 + f];
        }
    }
    for (int64_t c = 0; c < C; ++c) {
        if (c % kBlock == 0) {
            blk_c[c / kBlock] = 0;
            off_c[c / kBlock] = totals[1];
        }
        blk_c[c / kBlock] += ref[c];
        totals[1] += ref[c];
    }
    return 0;
}

extern "C" int nerfhip_mesh_decimate_compact(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags,
                                             int64_t C, const uint8_t* ref, const int64_t* off_t, const int64_t* off_c, const float* positions,
                                             const uint8_t* colors_or_null, int32_t* vnew, float* out_vertices, int32_t* out_triangles,
                                             uint8_t* out_colors_or_null, int32_t* out_cluster_of, nerfhip_stream_t stream) {
    const int e = compact_args(triangles, T, V, cluster_of, flags, C, ref, off_t, off_c, positions, colors_or_null, vnew, out_vertices,
                               out_triangles, out_colors_or_null, out_cluster_of);
    if (e) return e;
    hipStream_t s = (hipStream_t)stream;
    if (C > 0)
        hipLaunchKernelGGL(dc_compact_clusters, dim3(blocks_of(C)), dim3(kBlock), 0, s, C, ref, off_c, positions, colors_or_null, vnew,
                           out_vertices, out_colors_or_null);
    if (T > 0)
        hipLaunchKernelGGL(dc_compact_tris, dim3(blocks_of(T)), dim3(kBlock), 0, s, triangles, T, V, cluster_of, flags, C, off_t,
                           (const int32_t*)vnew, out_triangles);
    if (V > 0) hipLaunchKernelGGL(dc_remap, dim3(blocks_of(V)), dim3(kBlock), 0, s, cluster_of, V, C, (const int32_t*)vnew, out_cluster_of);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_decimate_compact_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of,
                                                  const uint8_t* flags, int64_t C, const uint8_t* ref, const int64_t* off_t, const int64_t* off_c,
                                                  const float* positions, const uint8_t* colors_or_null, int32_t* vnew, float* out_vertices,
                                                  int32_t* out_triangles, uint8_t* out_colors_or_null, int32_t* out_cluster_of) {
    const int e = compact_args(triangles, T, V, cluster_of, flags, C, ref, off_t, off_c, positions, colors_or_null, vnew, out_vertices,
                               out_triangles, out_colors_or_null, out_cluster_of);
    if (e) return e;
    int64_t id = 0;
    for (int64_t c = 0; c < C; ++c) {
        if (c % kBlock == 0) id = off_c[c / kBlock];
        vnew[c] = ref[c] ? (int32_t)id : -1;
        if (!ref[c]) continue;
        for (int a = 0; a < 3; ++a) {
            out_vertices[3 * id + a] = positions[3 * c + a];
            if (colors_or_null) out_colors_or_null[3 * id + a] = colors_or_null[3 * c + a];
        }
        ++id;
    }
    for (int64_t t = 0; t < T; ++t) {
        if (t % kBlock == 0) id = off_t[t / kBlock];
        if (flags[t] == nerfhip::kDecimateKeep) triangle_store(triangles, t, V, cluster_of, C, vnew, id++, out_triangles);
    }
    nerfhip::host_items(V, RemapItem{cluster_of, C, vnew, out_cluster_of});
    return 0;
}

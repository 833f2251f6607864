// Ray casting against a triangle mesh on the device: the hierarchy's build, the cast, and the two per-ray kernels
// that turn hits into pixels.  Every routine that computes is mesh_core.h's, shared with the _host twins below.
//
//   mesh_bounds        one thread per triangle: counts the bad ones, folds the good ones' bounds (wave reduction, then 6 atomics)
//   mesh_keys          one thread per triangle: its Morton key in those bounds            [torch.sort runs between the two calls]
//   mesh_leaves        one thread per leaf: packs its 4 sorted triangles, writes its box
//   mesh_level         one thread per node of one level: the union of its 8 children — one launch per level, so no box is read
//                      in the launch that wrote it (the L2s of the XCDs are not coherent within a launch)
//   mesh_cast          one thread per ray: mesh_cast_ray
//   mesh_shade, mixed_compose   one thread per ray
//
// Nothing allocates, nothing synchronises; no LDS, no scratch.
#include "common.h"
#include "mesh_core.h"
#include "twin_launch.h"

namespace {

using nerfhip::blocks_of;
using nerfhip::kMaxRays;
using nerfhip::MeshBvh;
using nerfhip::MeshHit;
using nerfhip::MeshVec4;
using nerfhip::misaligned;
using nerfhip::MixedPixel;

constexpr int kBlock = nerfhip::kItemBlock;
constexpr int64_t kMaxVertices = 0x7fffffff;    // a triangle names its vertices by int32

// ---- build --------------------------------------------------------------------------------------------------------------------
// state: 8 words.  [0] the number of bad triangles, [1] zero, [2..4] / [5..7] the bounds' lo / hi in mesh_ordered's encoding.
__global__ void mesh_state_init(uint32_t* __restrict__ state) {
    const int i = threadIdx.x;
    if (i < 8) state[i] = i < 2 ? 0u : nerfhip::mesh_ordered(nerfhip::float_from_bits(i < 5 ? 0x7f800000u : 0xff800000u));
}

__global__ void __launch_bounds__(kBlock) mesh_bounds(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles,
                                                      int64_t T, uint32_t* __restrict__ state) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const float inf = nerfhip::float_from_bits(0x7f800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    int bad = 0;
    if (t < T) {
        float p[9];
        if (nerfhip::mesh_triangle(vertices, V, triangles, t, p)) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    lo[a] = nerfhip::mesh_min(lo[a], p[3 * c + a]);
                    hi[a] = nerfhip::mesh_max(hi[a], p[3 * c + a]);
                }
        } else {
            bad = 1;
        }
    }
    // every lane of the wave is here: the early exits above are selects, not returns
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = nerfhip::mesh_min(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = nerfhip::mesh_max(hi[a], __shfl_xor(hi[a], o, 64));
        }
        bad += __shfl_xor(bad, o, 64);
    }
    if (nerfhip::lane_id() == 0) {
        if (bad) atomicAdd(state, (uint32_t)bad);
        if (lo[0] <= hi[0]) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(state + 2 + a, nerfhip::mesh_ordered(lo[a]));
                atomicMax(state + 5 + a, nerfhip::mesh_ordered(hi[a]));
            }
        }
    }
}

__global__ void __launch_bounds__(kBlock) mesh_keys(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles,
                                                    int64_t T, const uint32_t* __restrict__ state, int64_t* __restrict__ keys) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    float lo[3], hi[3], p[9];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = nerfhip::mesh_unordered(state[2 + a]);
        hi[a] = nerfhip::mesh_unordered(state[5 + a]);
    }
    const bool ok = nerfhip::mesh_triangle(vertices, V, triangles, t, p);
    keys[t] = nerfhip::mesh_key(p, ok, lo, hi, t);
}

__global__ void __launch_bounds__(kBlock) mesh_leaves(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles,
                                                      int64_t T, const int64_t* __restrict__ sorted_keys, int n0,
                                                      MeshVec4* __restrict__ tris, float* __restrict__ boxes) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n0) nerfhip::mesh_leaf(vertices, V, triangles, T, sorted_keys, j, tris, boxes);
}

__global__ void __launch_bounds__(kBlock) mesh_level(const float* __restrict__ child, int n_child, int n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) nerfhip::mesh_node(child, n_child, (int)i, out);
}

inline int build_args(const float* vertices, int64_t V, const int32_t* triangles, int64_t T) {
    NERFHIP_CHECK_ARG(T >= 0 && T <= nerfhip::kMeshMaxTriangles && V >= 0 && V <= kMaxVertices);
    NERFHIP_CHECK_ARG(T == 0 || triangles);
    NERFHIP_CHECK_ARG(V == 0 || vertices);
    if (misaligned(vertices, 4) || misaligned(triangles, 4)) return NERFHIP_E_ALIGN;
    return 0;
}

inline MeshBvh bvh_of(const float* tris, const float* boxes, int64_t T) {
    MeshBvh b;
    b.tris = (const MeshVec4*)tris;
    b.boxes = boxes;
    b.T = T;
    b.n0 = (int)((T + nerfhip::kMeshLeaf - 1) / nerfhip::kMeshLeaf);
    b.levels = nerfhip::mesh_levels(T);
    b.n_nodes = (int)nerfhip::mesh_nodes(T);
    return b;
}

// ---- cast, shade, compose -----------------------------------------------------------------------------------------------------
struct CastItem {
    const float4* rays;
    const MeshBvh& b;    // by reference: held by value, hipcc orders the traversal's instructions differently
    int32_t* tri;
    float *t, *b1, *b2;    // each may be null
    __host__ __device__ void operator()(int64_t i) const {
        float ray[8];
        nerfhip::load_ray(rays, i, ray);
        const MeshHit h = nerfhip::mesh_cast_ray(b, ray);
        tri[i] = h.tri;
        if (t) t[i] = h.t;
        if (b1) b1[i] = h.b1;
        if (b2) b2[i] = h.b2;
    }
};

__global__ void __launch_bounds__(kBlock) mesh_cast(const float4* __restrict__ rays, int64_t n, MeshBvh b, int32_t* __restrict__ tri,
                                                    float* __restrict__ t, float* __restrict__ b1, float* __restrict__ b2) {
    const int64_t i = nerfhip::item_index();
    if (i < n) CastItem{rays, b, tri, t, b1, b2}(i);
}

struct ShadeItem {
    const float* rays;
    const int32_t* tri;
    const float *b1, *b2, *vertices;
    int64_t V;
    const int32_t* triangles;
    int64_t T;
    const uint8_t* colors;    // may be null
    float* rgb;               // the pointers in front of the scalars: with rgb behind them hipcc keeps that tail of the struct in LDS
    float ambient, background;
    __host__ __device__ void operator()(int64_t i) const {
        float out[3];
        nerfhip::mesh_shade_ray(rays + 8 * i, tri[i], b1[i], b2[i], vertices, V, triangles, T, colors, ambient, background, out);
        rgb[3 * i] = out[0];
        rgb[3 * i + 1] = out[1];
        rgb[3 * i + 2] = out[2];
    }
};

__global__ void __launch_bounds__(kBlock) mesh_shade(const float* __restrict__ rays, int64_t n, const int32_t* __restrict__ tri,
                                                     const float* __restrict__ b1, const float* __restrict__ b2,
                                                     const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles,
                                                     int64_t T, const uint8_t* __restrict__ colors, float ambient, float background,
                                                     float* __restrict__ rgb) {
    const int64_t i = nerfhip::item_index();
    if (i < n) ShadeItem{rays, tri, b1, b2, vertices, V, triangles, T, colors, rgb, ambient, background}(i);
}

struct ComposeItem {
    int mode;
    const float *rgb_n, *depth_n, *opacity_n;
    const int32_t* tri;
    const float *t, *rgb_m;
    float tau, background;
    float *rgb, *depth, *opacity;
    uint8_t* mask;    // may be null
    __host__ __device__ void operator()(int64_t i) const {
        const MixedPixel px = nerfhip::mixed_compose_ray(mode, rgb_n + 3 * i, depth_n[i], opacity_n[i], tri[i], t[i], rgb_m + 3 * i, tau, background);
        rgb[3 * i] = px.rgb[0];
        rgb[3 * i + 1] = px.rgb[1];
        rgb[3 * i + 2] = px.rgb[2];
        depth[i] = px.depth;
        opacity[i] = px.opacity;
        if (mask) mask[i] = px.mask;
    }
};

__global__ void __launch_bounds__(kBlock) mixed_compose(int mode, int64_t n, const float* __restrict__ rgb_n, const float* __restrict__ depth_n,
                                                        const float* __restrict__ opacity_n, const int32_t* __restrict__ tri,
                                                        const float* __restrict__ t, const float* __restrict__ rgb_m, float tau,
                                                        float background, float* __restrict__ rgb, float* __restrict__ depth,
                                                        float* __restrict__ opacity, uint8_t* __restrict__ mask) {
    const int64_t i = nerfhip::item_index();
    if (i < n) ComposeItem{mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background, rgb, depth, opacity, mask}(i);
}

inline int cast_args(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int brute, const int32_t* tri,
                     const float* t, const float* b1, const float* b2) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays && T >= 0 && T <= nerfhip::kMeshMaxTriangles);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rays && tri);
    NERFHIP_CHECK_ARG(T == 0 || (tris && (boxes || brute)));
    if (misaligned(rays, 16) || misaligned(tris, 16) || misaligned(boxes, 4) || misaligned(tri, 4) || misaligned(t, 4) || misaligned(b1, 4) ||
        misaligned(b2, 4))
        return NERFHIP_E_ALIGN;
    return 0;
}

inline int shade_args(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2, const float* vertices, int64_t V,
                      const int32_t* triangles, int64_t T, float ambient, float background, const float* rgb) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays && T >= 0 && T <= nerfhip::kMeshMaxTriangles && V >= 0 && V <= kMaxVertices);
    NERFHIP_CHECK_ARG(ambient >= 0.0f && ambient <= 1.0f && nerfhip::finite_f32(background));
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rays && tri && b1 && b2 && rgb);
    NERFHIP_CHECK_ARG((T == 0 || triangles) && (V == 0 || vertices));
    if (misaligned(rays, 4) || misaligned(tri, 4) || misaligned(b1, 4) || misaligned(b2, 4) || misaligned(vertices, 4) ||
        misaligned(triangles, 4) || misaligned(rgb, 4))
        return NERFHIP_E_ALIGN;
    return 0;
}

inline int compose_args(int mode, int64_t n, const float* rgb_n, const float* depth_n, const float* opacity_n, const int32_t* tri,
                        const float* t, const float* rgb_m, float tau, float background, const float* rgb, const float* depth,
                        const float* opacity) {
    NERFHIP_CHECK_ARG((mode == nerfhip::kMixedZtest || mode == nerfhip::kMixedClip) && n >= 0 && n <= kMaxRays);
    NERFHIP_CHECK_ARG(tau > 0.0f && nerfhip::finite_f32(tau) && nerfhip::finite_f32(background));
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rgb_n && depth_n && opacity_n && tri && t && rgb_m && rgb && depth && opacity);
    if (misaligned(rgb_n, 4) || misaligned(depth_n, 4) || misaligned(opacity_n, 4) || misaligned(tri, 4) || misaligned(t, 4) ||
        misaligned(rgb_m, 4) || misaligned(rgb, 4) || misaligned(depth, 4) || misaligned(opacity, 4))
        return NERFHIP_E_ALIGN;
    return 0;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" size_t nerfhip_mesh_bvh_nodes(int64_t T) {
    if (T < 0 || T > nerfhip::kMeshMaxTriangles) return 0;
    return (size_t)nerfhip::mesh_nodes(T);
}

extern "C" int nerfhip_mesh_bvh_keys(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int64_t* keys, int32_t* state,
                                     nerfhip_stream_t stream) {
    const int e = build_args(vertices, V, triangles, T);
    if (e) return e;
    NERFHIP_CHECK_ARG(state && (keys || T == 0));
    if (misaligned(keys, 8) || misaligned(state, 4)) return NERFHIP_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_state_init, dim3(1), dim3(64), 0, s, (uint32_t*)state);
    if (T > 0) {
        hipLaunchKernelGGL(mesh_bounds, dim3(blocks_of(T)), dim3(kBlock), 0, s, vertices, V, triangles, T, (uint32_t*)state);
        hipLaunchKernelGGL(mesh_keys, dim3(blocks_of(T)), dim3(kBlock), 0, s, vertices, V, triangles, T, (const uint32_t*)state, keys);
    }
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_bvh_keys_host(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int64_t* keys,
                                          int32_t* state) {
    const int e = build_args(vertices, V, triangles, T);
    if (e) return e;
    NERFHIP_CHECK_ARG(state && (keys || T == 0));
    if (misaligned(keys, 8) || misaligned(state, 4)) return NERFHIP_E_ALIGN;
    const float inf = nerfhip::float_from_bits(0x7f800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, p[9];
    int32_t bad = 0;
    for (int64_t t = 0; t < T; ++t) {
        if (!nerfhip::mesh_triangle(vertices, V, triangles, t, p)) {
            ++bad;
            continue;
        }
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) {
                lo[a] = nerfhip::mesh_min(lo[a], p[3 * c + a]);
                hi[a] = nerfhip::mesh_max(hi[a], p[3 * c + a]);
            }
    }
    state[0] = bad;
    state[1] = 0;
    for (int a = 0; a < 3; ++a) {
        state[2 + a] = (int32_t)nerfhip::mesh_ordered(lo[a]);
        state[5 + a] = (int32_t)nerfhip::mesh_ordered(hi[a]);
    }
    for (int64_t t = 0; t < T; ++t) {
        const bool ok = nerfhip::mesh_triangle(vertices, V, triangles, t, p);
        keys[t] = nerfhip::mesh_key(p, ok, lo, hi, t);
    }
    return 0;
}

extern "C" int nerfhip_mesh_bvh_boxes(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const int64_t* sorted_keys,
                                      float* tris, float* boxes, nerfhip_stream_t stream) {
    const int e = build_args(vertices, V, triangles, T);
    if (e || T == 0) return e;
    NERFHIP_CHECK_ARG(sorted_keys && tris && boxes);
    if (misaligned(sorted_keys, 8) || misaligned(tris, 16) || misaligned(boxes, 4)) return NERFHIP_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    int n = (int)((T + nerfhip::kMeshLeaf - 1) / nerfhip::kMeshLeaf);
    hipLaunchKernelGGL(mesh_leaves, dim3(blocks_of(n)), dim3(kBlock), 0, s, vertices, V, triangles, T, sorted_keys, n, (MeshVec4*)tris, boxes);
    float* level = boxes;
    while (n > 1) {    // one launch per level: at most 9
        const int up = (n + nerfhip::kMeshFan - 1) / nerfhip::kMeshFan;
        float* out = level + 6 * (int64_t)n;
        hipLaunchKernelGGL(mesh_level, dim3(blocks_of(up)), dim3(kBlock), 0, s, (const float*)level, n, up, out);
        level = out;
        n = up;
    }
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_bvh_boxes_host(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const int64_t* sorted_keys,
                                           float* tris, float* boxes) {
    const int e = build_args(vertices, V, triangles, T);
    if (e || T == 0) return e;
    NERFHIP_CHECK_ARG(sorted_keys && tris && boxes);
    if (misaligned(sorted_keys, 8) || misaligned(tris, 16) || misaligned(boxes, 4)) return NERFHIP_E_ALIGN;
    int n = (int)((T + nerfhip::kMeshLeaf - 1) / nerfhip::kMeshLeaf);
    for (int64_t j = 0; j < n; ++j) nerfhip::mesh_leaf(vertices, V, triangles, T, sorted_keys, j, (MeshVec4*)tris, boxes);
    float* level = boxes;
    while (n > 1) {
        const int up = (n + nerfhip::kMeshFan - 1) / nerfhip::kMeshFan;
        float* out = level + 6 * (int64_t)n;
        for (int i = 0; i < up; ++i) nerfhip::mesh_node(level, n, i, out);
        level = out;
        n = up;
    }
    return 0;
}

extern "C" int nerfhip_mesh_cast(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int32_t* tri, float* t,
                                 float* b1, float* b2, nerfhip_stream_t stream) {
    const int e = cast_args(rays, n, tris, boxes, T, 0, tri, t, b1, b2);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(mesh_cast, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, (const float4*)rays, n, bvh_of(tris, boxes, T), tri,
                       t, b1, b2);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_cast_host(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int brute, int32_t* tri,
                                      float* t, float* b1, float* b2) {
    const int e = cast_args(rays, n, tris, boxes, T, brute, tri, t, b1, b2);
    if (e || n == 0) return e;
    const MeshBvh b = bvh_of(tris, brute ? nullptr : boxes, T);
    nerfhip::host_items(n, CastItem{(const float4*)rays, b, tri, t, b1, b2});
    return 0;
}

extern "C" int nerfhip_mesh_shade(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2, const float* vertices,
                                  int64_t V, const int32_t* triangles, int64_t T, const uint8_t* colors_or_null, float ambient,
                                  float background, float* rgb, nerfhip_stream_t stream) {
    const int e = shade_args(rays, n, tri, b1, b2, vertices, V, triangles, T, ambient, background, rgb);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(mesh_shade, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, rays, n, tri, b1, b2, vertices, V, triangles, T,
                       colors_or_null, ambient, background, rgb);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_shade_host(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2,
                                       const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* colors_or_null,
                                       float ambient, float background, float* rgb) {
    const int e = shade_args(rays, n, tri, b1, b2, vertices, V, triangles, T, ambient, background, rgb);
    if (e || n == 0) return e;
    nerfhip::host_items(n, ShadeItem{rays, tri, b1, b2, vertices, V, triangles, T, colors_or_null, rgb, ambient, background});
    return 0;
}

extern "C" int nerfhip_mixed_compose(int mode, int64_t n, const float* rgb_n, const float* depth_n, const float* opacity_n, const int32_t* tri,
                                     const float* t, const float* rgb_m, float tau, float background, float* rgb, float* depth,
                                     float* opacity, uint8_t* mask_or_null, nerfhip_stream_t stream) {
    const int e = compose_args(mode, n, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background, rgb, depth, opacity);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(mixed_compose, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, mode, n, rgb_n, depth_n, opacity_n, tri, t, rgb_m,
                       tau, background, rgb, depth, opacity, mask_or_null);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mixed_compose_host(int mode, int64_t n, const float* rgb_n, const float* depth_n, const float* opacity_n,
                                          const int32_t* tri, const float* t, const float* rgb_m, float tau, float background, float* rgb,
                                          float* depth, float* opacity, uint8_t* mask_or_null) {
    const int e = compose_args(mode, n, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background, rgb, depth, opacity);
    if (e || n == 0) return e;
    nerfhip::host_items(n, ComposeItem{mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background, rgb, depth, opacity, mask_or_null});
    return 0;
}

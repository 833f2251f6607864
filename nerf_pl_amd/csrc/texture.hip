// Texturing a triangle mesh on the device: the sample points of the per-triangle atlas, the atlas from the samples'
// colours, and the per-ray lookup.  Every routine that computes is texture_core.h's, shared with the _host twins below.
//
//   mesh_tex_points   one thread per sample: its point on the triangle's plane and (optionally) the triangle's fp64 unit normal
//   mesh_tex_atlas    one thread per 4 consecutive texels of a row, gathered: 12 byte loads, three 32-bit stores — every byte of
//                     the atlas is written exactly once, so nothing clears it first
//   mesh_shade_tex    one thread per ray: tex_shade_ray
//
// Nothing allocates, nothing synchronises; no LDS, no scratch, no atomics.
#include "common.h"
#include "texture_core.h"
#include "twin_launch.h"

namespace {

using nerfhip::blocks_of;
using nerfhip::kMaxRays;
using nerfhip::misaligned;
using nerfhip::TexGrid;

constexpr int kBlock = nerfhip::kItemBlock;
constexpr int64_t kMaxTriangles = (int64_t)1 << 28;    // mesh_core.h's kMeshMaxTriangles
constexpr int64_t kMaxVertices = 0x7fffffff;           // a triangle names its vertices by int32

struct PointsItem {
    const float* vertices;
    int64_t V;
    const int32_t* triangles;
    float* points;
    double* normals;    // may be null
    int R;
    __host__ __device__ void operator()(int64_t q) const {
        float p[3];
        double n[3];    // both plain locals, the flag instead of a pointer that may be null: an address that is chosen at run time
                        // would put them into scratch
        nerfhip::tex_point(vertices, V, triangles, R, q, normals != nullptr, p, n);
        points[3 * q] = p[0];
        points[3 * q + 1] = p[1];
        points[3 * q + 2] = p[2];
        if (normals) {
            normals[3 * q] = n[0];
            normals[3 * q + 1] = n[1];
            normals[3 * q + 2] = n[2];
        }
    }
};

__global__ void __launch_bounds__(kBlock) mesh_tex_points(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles,
                                                          int64_t K, int R, float* __restrict__ points, double* __restrict__ normals) {
    const int64_t q = nerfhip::item_index();
    if (q < K) PointsItem{vertices, V, triangles, points, normals, R}(q);
}

struct AtlasItem {
    const uint8_t* colors;
    uint32_t* atlas;    // (Ha, Wa, 3) bytes as 3 Ha Wa / 4 words
    TexGrid g;
    __host__ __device__ void operator()(int64_t item) const {
        uint32_t w[3];
        nerfhip::tex_atlas_words(g, colors, item, w);
        atlas[3 * item] = w[0];
        atlas[3 * item + 1] = w[1];
        atlas[3 * item + 2] = w[2];
    }
};

__global__ void __launch_bounds__(kBlock) mesh_tex_atlas(const uint8_t* __restrict__ colors, TexGrid g, int64_t items,
                                                         uint32_t* __restrict__ atlas) {
    const int64_t item = nerfhip::item_index();
    if (item < items) AtlasItem{colors, atlas, g}(item);
}

struct ShadeTexItem {
    const float* rays;
    const int32_t* tri;
    const float *b1, *b2, *vertices;
    int64_t V;
    const int32_t* triangles;
    const uint8_t* atlas;
    float* rgb;
    TexGrid g;
    int filter;
    float ambient, background;
    __host__ __device__ void operator()(int64_t i) const {
        float out[3];
        nerfhip::tex_shade_ray(rays + 8 * i, tri[i], b1[i], b2[i], vertices, V, triangles, g, atlas, filter, ambient, background, out);
        rgb[3 * i] = out[0];
        rgb[3 * i + 1] = out[1];
        rgb[3 * i + 2] = out[2];
    }
};

__global__ void __launch_bounds__(kBlock) mesh_shade_tex(const float* __restrict__ rays, int64_t n, const int32_t* __restrict__ tri,
                                                         const float* __restrict__ b1, const float* __restrict__ b2,
                                                         const float* __restrict__ vertices, int64_t V,
                                                         const int32_t* __restrict__ triangles, const uint8_t* __restrict__ atlas,
                                                         TexGrid g, int filter, float ambient, float background,
                                                         float* __restrict__ rgb) {
    const int64_t i = nerfhip::item_index();
    if (i < n) ShadeTexItem{rays, tri, b1, b2, vertices, V, triangles, atlas, rgb, g, filter, ambient, background}(i);
}

inline bool res_ok(int R) { return R >= 1 && R <= nerfhip::kTexMaxRes; }

// T, R and the atlas' sizes as include/nerfhip.h states them
inline bool atlas_ok(int64_t T, int R, int Wa, int Ha) {
    if (!res_ok(R) || T < 0 || T > kMaxTriangles) return false;
    if (Wa < R + 3 || Wa > nerfhip::kTexMaxSide || (Wa & 3)) return false;
    return Ha >= 0 && Ha == nerfhip::tex_height(T, R, Wa);
}

inline int points_args(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int R, const float* points,
                       const double* normals) {
    NERFHIP_CHECK_ARG(res_ok(R) && T >= 0 && T <= kMaxTriangles && V >= 0 && V <= kMaxVertices);
    NERFHIP_CHECK_ARG(T * nerfhip::tex_samples(R) <= nerfhip::kTexMaxSamples);
    if (T == 0) return 0;
    NERFHIP_CHECK_ARG(triangles && points && (V == 0 || vertices));
    if (misaligned(vertices, 4) || misaligned(triangles, 4) || misaligned(points, 4) || misaligned(normals, 8)) return NERFHIP_E_ALIGN;
    return 0;
}

inline int atlas_args(const uint8_t* colors, int64_t T, int R, int Wa, int Ha, const uint8_t* atlas) {
    NERFHIP_CHECK_ARG(atlas_ok(T, R, Wa, Ha));
    if (T == 0) return 0;    // Ha == 0: no byte to write
    NERFHIP_CHECK_ARG(colors && atlas);
    if (misaligned(atlas, 4)) return NERFHIP_E_ALIGN;
    return 0;
}

inline int shade_tex_args(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2, const float* vertices,
                          int64_t V, const int32_t* triangles, int64_t T, const uint8_t* atlas, int R, int Wa, int Ha, int filter,
                          float ambient, float background, const float* rgb) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays && V >= 0 && V <= kMaxVertices && atlas_ok(T, R, Wa, Ha));
    NERFHIP_CHECK_ARG(filter == nerfhip::kTexNearest || filter == nerfhip::kTexBilinear);
    NERFHIP_CHECK_ARG(ambient >= 0.0f && ambient <= 1.0f && nerfhip::finite_f32(background));
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rays && tri && b1 && b2 && rgb);
    NERFHIP_CHECK_ARG((T == 0 || (triangles && atlas)) && (V == 0 || vertices));
    if (misaligned(rays, 4) || misaligned(tri, 4) || misaligned(b1, 4) || misaligned(b2, 4) || misaligned(vertices, 4) ||
        misaligned(triangles, 4) || misaligned(atlas, 4) || misaligned(rgb, 4))
        return NERFHIP_E_ALIGN;
    return 0;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" int nerfhip_mesh_tex_samples(int R) { return res_ok(R) ? nerfhip::tex_samples(R) : 0; }

extern "C" int nerfhip_mesh_tex_height(int64_t T, int R, int Wa) {
    if (!res_ok(R) || T < 0 || T > kMaxTriangles || Wa < R + 3 || Wa > nerfhip::kTexMaxSide || (Wa & 3)) return 0;
    const int Ha = nerfhip::tex_height(T, R, Wa);
    return Ha < 0 ? 0 : Ha;
}

extern "C" int nerfhip_mesh_tex_points(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int R, float* points,
                                       double* normals_or_null, nerfhip_stream_t stream) {
    const int e = points_args(vertices, V, triangles, T, R, points, normals_or_null);
    if (e || T == 0) return e;
    const int64_t K = T * nerfhip::tex_samples(R);
    hipLaunchKernelGGL(mesh_tex_points, dim3(blocks_of(K)), dim3(kBlock), 0, (hipStream_t)stream, vertices, V, triangles, K, R, points,
                       normals_or_null);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_tex_points_host(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int R, float* points,
                                            double* normals_or_null) {
    const int e = points_args(vertices, V, triangles, T, R, points, normals_or_null);
    if (e || T == 0) return e;
    nerfhip::host_items(T * nerfhip::tex_samples(R), PointsItem{vertices, V, triangles, points, normals_or_null, R});
    return 0;
}

extern "C" int nerfhip_mesh_tex_atlas(const uint8_t* colors, int64_t T, int R, int Wa, int Ha, uint8_t* atlas, nerfhip_stream_t stream) {
    const int e = atlas_args(colors, T, R, Wa, Ha, atlas);
    if (e || T == 0) return e;
    const int64_t items = (int64_t)Ha * (Wa >> 2);
    hipLaunchKernelGGL(mesh_tex_atlas, dim3(blocks_of(items)), dim3(kBlock), 0, (hipStream_t)stream, colors,
                       nerfhip::tex_grid(T, R, Wa, Ha), items, (uint32_t*)atlas);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_tex_atlas_host(const uint8_t* colors, int64_t T, int R, int Wa, int Ha, uint8_t* atlas) {
    const int e = atlas_args(colors, T, R, Wa, Ha, atlas);
    if (e || T == 0) return e;
    nerfhip::host_items((int64_t)Ha * (Wa >> 2), AtlasItem{colors, (uint32_t*)atlas, nerfhip::tex_grid(T, R, Wa, Ha)});
    return 0;
}

extern "C" int nerfhip_mesh_shade_tex(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2,
                                      const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* atlas, int R,
                                      int Wa, int Ha, int filter, float ambient, float background, float* rgb, nerfhip_stream_t stream) {
    const int e = shade_tex_args(rays, n, tri, b1, b2, vertices, V, triangles, T, atlas, R, Wa, Ha, filter, ambient, background, rgb);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(mesh_shade_tex, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, rays, n, tri, b1, b2, vertices, V, triangles,
                       atlas, nerfhip::tex_grid(T, R, Wa, Ha), filter, ambient, background, rgb);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_shade_tex_host(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2,
                                           const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* atlas,
                                           int R, int Wa, int Ha, int filter, float ambient, float background, float* rgb) {
    const int e = shade_tex_args(rays, n, tri, b1, b2, vertices, V, triangles, T, atlas, R, Wa, Ha, filter, ambient, background, rgb);
    if (e || n == 0) return e;
    nerfhip::host_items(n, ShadeTexItem{rays, tri, b1, b2, vertices, V, triangles, atlas, rgb, nerfhip::tex_grid(T, R, Wa, Ha), filter,
                                        ambient, background});
    return 0;
}

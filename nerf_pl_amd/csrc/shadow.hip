// Shadows for mixed renders on the device: the any-hit query against mesh_cast's hierarchy, the shadow rows of a
// render, and the compose that applies the light.  Every routine that computes is shadow_core.h's, shared with the _host twins.
//
//   mesh_occluded    one thread per ray: mesh_occluded_ray
//   shadow_rays      one thread per output row (pixel i, sample k at row i K + k): a wave writes 2 KiB in one piece
//   light_compose    one thread per pixel: the mean over its K rows, then the factor
//
// Nothing allocates, nothing synchronises; no LDS, no scratch.
#include "common.h"
#include "shadow_core.h"
#include "twin_launch.h"

namespace {

using nerfhip::blocks_of;
using nerfhip::kMaxRays;
using nerfhip::MeshBvh;
using nerfhip::MeshVec4;
using nerfhip::misaligned;
using nerfhip::ShadowLight;
using nerfhip::ShadowPixel;

constexpr int kBlock = nerfhip::kItemBlock;
constexpr int64_t kMaxVertices = 0x7fffffff;

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

struct OccludedItem {
    const float4* rays;
    const MeshBvh& b;    // by reference, as meshcast.hip's CastItem holds it
    uint8_t* hit;
    __host__ __device__ void operator()(int64_t i) const {
        float ray[8];
        nerfhip::load_ray(rays, i, ray);
        hit[i] = nerfhip::mesh_occluded_ray(b, ray) ? 1 : 0;
    }
};

__global__ void __launch_bounds__(kBlock) mesh_occluded(const float4* __restrict__ rays, int64_t n, MeshBvh b, uint8_t* __restrict__ hit) {
    const int64_t i = nerfhip::item_index();
    if (i < n) OccludedItem{rays, b, hit}(i);
}

struct ShadowRaysItem {
    const float4* rays;
    const float* s;
    const int32_t* tri;    // may be null: no mesh layer, cosine 1
    const float* vertices;
    int64_t V;
    const int32_t* triangles;
    int64_t T;
    float4* rows;
    float* cosine;         // may be null
    ShadowLight L;
    __host__ __device__ void operator()(int64_t j) const {
        const int64_t i = j / L.K;
        const int k = (int)(j - i * L.K);
        float ray[8], row[8];
        nerfhip::load_ray(rays, i, ray);
        const ShadowPixel px = nerfhip::shadow_pixel(L, ray, s[i]);
        nerfhip::shadow_row(L, px, (uint32_t)i, k, row);
        rows[2 * j] = make_float4(row[0], row[1], row[2], row[3]);
        rows[2 * j + 1] = make_float4(row[4], row[5], row[6], row[7]);
        if (cosine && k == 0) cosine[i] = tri ? nerfhip::shadow_cosine(px, ray, tri[i], vertices, V, triangles, T) : 1.0f;
    }
};

__global__ void __launch_bounds__(kBlock) shadow_rays(const float4* __restrict__ rays, const float* __restrict__ s, int64_t rows_total,
                                                      const int32_t* __restrict__ tri, const float* __restrict__ vertices, int64_t V,
                                                      const int32_t* __restrict__ triangles, int64_t T, ShadowLight L,
                                                      float4* __restrict__ rows, float* __restrict__ cosine) {
    const int64_t j = nerfhip::item_index();
    if (j < rows_total) ShadowRaysItem{rays, s, tri, vertices, V, triangles, T, rows, cosine, L}(j);
}

struct LightComposeItem {
    const float* rgb;
    const uint8_t* mask;
    const float* cosine;
    const uint8_t* hit;
    const float* trans;    // may be null: 1
    float *rgb_out, *visibility;    // visibility may be null
    int K;
    float ambient, strength;
    __host__ __device__ void operator()(int64_t i) const {
        const bool mesh = mask[i] != 0;
        const float v = nerfhip::light_visibility(hit + i * K, mesh && trans ? trans + i * K : nullptr, K);
        const float f = nerfhip::light_factor(mesh, cosine[i], v, ambient, strength);
        rgb_out[3 * i] = rgb[3 * i] * f;
        rgb_out[3 * i + 1] = rgb[3 * i + 1] * f;
        rgb_out[3 * i + 2] = rgb[3 * i + 2] * f;
        if (visibility) visibility[i] = v;
    }
};

__global__ void __launch_bounds__(kBlock) light_compose(int64_t n, const float* __restrict__ rgb, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ cosine, const uint8_t* __restrict__ hit,
                                                        const float* __restrict__ trans, int K, float ambient, float strength,
                                                        float* __restrict__ rgb_out, float* __restrict__ visibility) {
    const int64_t i = nerfhip::item_index();
    if (i < n) LightComposeItem{rgb, mask, cosine, hit, trans, rgb_out, visibility, K, ambient, strength}(i);
}

inline int occluded_args(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int brute, const uint8_t* hit) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= kMaxRays && T >= 0 && T <= nerfhip::kMeshMaxTriangles);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rays && hit);
    NERFHIP_CHECK_ARG(T == 0 || (tris && (boxes || brute)));
    if (misaligned(rays, 16) || misaligned(tris, 16) || misaligned(boxes, 4)) return NERFHIP_E_ALIGN;
    return 0;
}

inline int shadow_args(const float* rays, const float* s, int64_t n, const int32_t* tri, const float* vertices, int64_t V,
                       const int32_t* triangles, int64_t T, int kind, float lx, float ly, float lz, float bias, float reach, int K,
                       float radius, int rotate, const float* rows, const float* cosine, ShadowLight& L) {
    NERFHIP_CHECK_ARG(K >= 1 && K <= nerfhip::kShadowMaxSamples && n >= 0 && n <= kMaxRays / K);
    NERFHIP_CHECK_ARG(kind == nerfhip::kLightDirectional || kind == nerfhip::kLightPoint);
    NERFHIP_CHECK_ARG(rotate == 0 || rotate == 1);
    NERFHIP_CHECK_ARG(bias > 0.0f && nerfhip::finite_f32(bias) && reach > 0.0f && nerfhip::finite_f32(reach));
    NERFHIP_CHECK_ARG(radius >= 0.0f && nerfhip::finite_f32(radius));
    NERFHIP_CHECK_ARG(nerfhip::shadow_light(kind, lx, ly, lz, bias, reach, K, radius, rotate, L));
    NERFHIP_CHECK_ARG(T >= 0 && T <= nerfhip::kMeshMaxTriangles && V >= 0 && V <= kMaxVertices);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rays && s && rows);
    NERFHIP_CHECK_ARG(!tri || ((T == 0 || triangles) && (V == 0 || vertices)));
    if (misaligned(rays, 16) || misaligned(rows, 16) || misaligned(s, 4) || misaligned(tri, 4) || misaligned(vertices, 4) ||
        misaligned(triangles, 4) || misaligned(cosine, 4))
        return NERFHIP_E_ALIGN;
    return 0;
}

inline int light_args(int64_t n, const float* rgb, const uint8_t* mask, const float* cosine, const uint8_t* hit, const float* trans, int K,
                      float ambient, float strength, const float* rgb_out, const float* visibility) {
    NERFHIP_CHECK_ARG(K >= 1 && K <= nerfhip::kShadowMaxSamples && n >= 0 && n <= kMaxRays / K);
    NERFHIP_CHECK_ARG(ambient >= 0.0f && ambient <= 1.0f && strength >= 0.0f && strength <= 1.0f);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rgb && mask && cosine && hit && rgb_out);
    if (misaligned(rgb, 4) || misaligned(cosine, 4) || misaligned(trans, 4) || misaligned(rgb_out, 4) || misaligned(visibility, 4))
        return NERFHIP_E_ALIGN;
    return 0;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" int nerfhip_mesh_occluded(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, uint8_t* hit,
                                     nerfhip_stream_t stream) {
    const int e = occluded_args(rays, n, tris, boxes, T, 0, hit);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(mesh_occluded, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, (const float4*)rays, n, bvh_of(tris, boxes, T),
                       hit);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_occluded_host(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int brute,
                                          uint8_t* hit) {
    const int e = occluded_args(rays, n, tris, boxes, T, brute, hit);
    if (e || n == 0) return e;
    const MeshBvh b = bvh_of(tris, brute ? nullptr : boxes, T);
    nerfhip::host_items(n, OccludedItem{(const float4*)rays, b, hit});
    return 0;
}

extern "C" int nerfhip_shadow_rays(const float* rays, const float* s, int64_t n, const int32_t* tri_or_null, const float* vertices, int64_t V,
                                   const int32_t* triangles, int64_t T, int kind, float lx, float ly, float lz, float bias, float reach,
                                   int K, float radius, int rotate, float* rows, float* cosine_or_null, nerfhip_stream_t stream) {
    ShadowLight L;
    const int e = shadow_args(rays, s, n, tri_or_null, vertices, V, triangles, T, kind, lx, ly, lz, bias, reach, K, radius, rotate, rows,
                              cosine_or_null, L);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(shadow_rays, dim3(blocks_of(n * K)), dim3(kBlock), 0, (hipStream_t)stream, (const float4*)rays, s, n * K, tri_or_null,
                       vertices, V, triangles, T, L, (float4*)rows, cosine_or_null);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_shadow_rays_host(const float* rays, const float* s, int64_t n, const int32_t* tri_or_null, const float* vertices,
                                        int64_t V, const int32_t* triangles, int64_t T, int kind, float lx, float ly, float lz, float bias,
                                        float reach, int K, float radius, int rotate, float* rows, float* cosine_or_null) {
    ShadowLight L;
    const int e = shadow_args(rays, s, n, tri_or_null, vertices, V, triangles, T, kind, lx, ly, lz, bias, reach, K, radius, rotate, rows,
                              cosine_or_null, L);
    if (e || n == 0) return e;
    nerfhip::host_items(n * K, ShadowRaysItem{(const float4*)rays, s, tri_or_null, vertices, V, triangles, T, (float4*)rows, cosine_or_null, L});
    return 0;
}

extern "C" int nerfhip_light_compose(int64_t n, const float* rgb, const uint8_t* mask, const float* cosine, const uint8_t* hit,
                                     const float* trans_or_null, int K, float ambient, float strength, float* rgb_out,
                                     float* visibility_or_null, nerfhip_stream_t stream) {
    const int e = light_args(n, rgb, mask, cosine, hit, trans_or_null, K, ambient, strength, rgb_out, visibility_or_null);
    if (e || n == 0) return e;
    hipLaunchKernelGGL(light_compose, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, n, rgb, mask, cosine, hit, trans_or_null, K,
                       ambient, strength, rgb_out, visibility_or_null);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_light_compose_host(int64_t n, const float* rgb, const uint8_t* mask, const float* cosine, const uint8_t* hit,
                                          const float* trans_or_null, int K, float ambient, float strength, float* rgb_out,
                                          float* visibility_or_null) {
    const int e = light_args(n, rgb, mask, cosine, hit, trans_or_null, K, ambient, strength, rgb_out, visibility_or_null);
    if (e || n == 0) return e;
    nerfhip::host_items(n, LightComposeItem{rgb, mask, cosine, hit, trans_or_null, rgb_out, visibility_or_null, K, ambient, strength});
    return 0;
}

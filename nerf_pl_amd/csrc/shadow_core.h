// Shadows for mixed renders: the per-ray and per-pixel routines of the kernels (shadow.hip) and of their host twins,
// from this one source.  Plain fp32 with separately rounded operations (the including file turns contraction off), IEEE division
// and square root, no libm: the device and the host give the same bits.
//
//   mesh_occluded_ray   any hit: is some good triangle accepted by mesh_test on the row's [near, far]?  mesh_core.h's ray, test,
//                       box test and pre-order walk, with limit = far, left at the first accepted triangle.
//   shadow_pixel/_row   the secondary rows of one pixel of a render: from its surface point p = o + s d towards K samples of a light.
//   shadow_cosine       max(n . l, 0) of a mesh pixel, n the hit triangle's geometric normal turned to the camera.
//   light_visibility, light_factor   the mean of the rows' answers and the factor it puts on the pixel's colour.
//
// The light is a square of half-width `radius` around its centre, facing the pixel: no trigonometry.  Its frame comes from the unit
// centre direction c by comparisons, cross products and one normalisation: e1 = normalise(c x axis), axis the coordinate axis on
// which |c| is smallest (x before y before z on a tie), e2 = c x e1.
//
// The sample offsets (u_k, v_k) in [-1, 1)^2 are the R2 sequence (the additive recurrence of the plastic number g, g^3 = g + 1) in
// 32-bit integers:  x_k = 2^31 + k A1,  y_k = 2^31 + k A2  (mod 2^32),  A1 = round(2^32 / g) = 3242174889,  A2 = round(2^32 / g^2)
// = 2447445414,  and  u = (x >> 8) 2^-23 - 1  (24 bits: exact in fp32).  Sample 0 is the centre.  With `rotate` pixel i adds
// h = hash(i) to every x and hash(h ^ 0x9e3779b9) to every y (a Cranley-Patterson shift), hash the 32-bit mixer
// x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.  tests/shadow_ref.py restates all of it.
#pragma once
#include "mesh_core.h"

namespace nerfhip {

constexpr int kShadowMaxSamples = 64;
constexpr int kLightDirectional = 0, kLightPoint = 1;
constexpr uint32_t kShadowA1 = 3242174889u, kShadowA2 = 2447445414u;
constexpr uint32_t kShadowHalf = 0x80000000u, kShadowSalt = 0x9e3779b9u;

// ---- any hit ------------------------------------------------------------------------------------------------------------------
// mesh_test accepts a triangle into an empty `best` iff the ray meets it (two-sided, watertight) at a finite t in [near, far]:
// that decision reads the triangle and the row only.  mesh_cast_ray returns tri >= 0 iff some triangle is accepted into an empty
// `best` (a later one can only replace it), so "occluded" is a property of the mesh and the row, and every traversal that tests at
// least the triangles of the boxes mesh_box_may_hit keeps at limit = far — conservative for exactly those acceptances — gives the
// same bit.  The walk is mesh_cast_ray's: stackless, pre-order, at most n_nodes visits for any input.
NH_TWIN_HD bool mesh_occluded_ray(const MeshBvh& b, const float* __restrict__ ray) {
    MeshHit best;
    best.tri = -1;
    best.t = best.b1 = best.b2 = 0.0f;
    const MeshRay r = mesh_ray(ray);
    if (!r.valid || b.T <= 0) return false;

    if (!b.boxes) {    // brute force, in storage order
        for (int64_t s = 0; s < b.T && best.tri < 0; ++s) mesh_test(r, b.tris[3 * s], b.tris[3 * s + 1], b.tris[3 * s + 2], best);
        return best.tri >= 0;
    }

    int level = b.levels - 1, i = 0;
    int n_level = 1;
    int off = b.n_nodes - 1;
    for (int visit = 0; visit < b.n_nodes; ++visit) {
        const bool may = mesh_box_may_hit(r, b.boxes + 6 * (int64_t)(off + i), r.far);
        if (may && level > 0) {         // descend to the first child
            --level;
            n_level = mesh_level_nodes(b.n0, level);
            off -= n_level;
            i *= kMeshFan;
            continue;
        }
        if (may) {
            const int64_t first = (int64_t)kMeshLeaf * i;
            for (int k = 0; k < kMeshLeaf; ++k) {
                const int64_t s = first + k;
                if (s < b.T && best.tri < 0) mesh_test(r, b.tris[3 * s], b.tris[3 * s + 1], b.tris[3 * s + 2], best);
            }
            if (best.tri >= 0) break;   // the first accepted triangle ends the walk
        }
        // the next node in pre-order
        bool done = false;
        for (int climb = 0; climb < kMeshMaxLevels; ++climb) {
            if (level == b.levels - 1) {
                done = true;
                break;
            }
            if ((i & (kMeshFan - 1)) != kMeshFan - 1 && i + 1 < n_level) {
                ++i;
                break;
            }
            off += n_level;
            ++level;
            n_level = mesh_level_nodes(b.n0, level);
            i >>= 3;
        }
        if (done) break;
    }
    return best.tri >= 0;
}

// ---- shadow rows --------------------------------------------------------------------------------------------------------------
struct ShadowLight {
    int kind;
    float l[3];    // directional: the unit direction towards the light; point: the light's position
    float bias, reach, radius;
    int K, rotate;
};

struct ShadowPixel {
    float p[3];    // the surface point
    float c[3];    // the unit direction from p to the light's centre
    float dist;    // how far a row towards the centre reaches: `reach`, or the distance to a point light
    bool valid;    // false: the pixel gets zero rows
};

NH_TWIN_HD uint32_t shadow_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

NH_TWIN_HD float shadow_unit_of(uint32_t x) { return (float)(x >> 8) * 1.1920928955078125e-07f - 1.0f; }    // (x >> 8) 2^-23 - 1

NH_TWIN_HD void shadow_offset(uint32_t i, int k, int rotate, float& u, float& v) {
    uint32_t x = kShadowHalf + (uint32_t)k * kShadowA1, y = kShadowHalf + (uint32_t)k * kShadowA2;
    if (rotate) {
        const uint32_t h = shadow_hash(i);
        x += h;
        y += shadow_hash(h ^ kShadowSalt);
    }
    u = shadow_unit_of(x);
    v = shadow_unit_of(y);
}

// v / |v| in place; returns |v|, and leaves v alone when that is zero or not finite (the caller tests the length)
NH_TWIN_HD float shadow_normalise(float* __restrict__ v) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (len > 0.0f && finite_f32(len)) {
        v[0] = v[0] / len;
        v[1] = v[1] / len;
        v[2] = v[2] / len;
    }
    return len;
}

// A light from its scalars: the direction of a directional light normalised once, here, on the host side of both entries.
// false: a non-finite value, or a directional light of zero (or overflowing) length.
NH_TWIN_HD bool shadow_light(int kind, float lx, float ly, float lz, float bias, float reach, int K, float radius, int rotate,
                             ShadowLight& L) {
    L.kind = kind;
    L.l[0] = lx, L.l[1] = ly, L.l[2] = lz;
    L.bias = bias, L.reach = reach, L.radius = radius;
    L.K = K, L.rotate = rotate;
    if (!(finite_f32(lx) && finite_f32(ly) && finite_f32(lz))) return false;
    if (kind == kLightDirectional) {
        const float len = shadow_normalise(L.l);
        return len > 0.0f && finite_f32(len);
    }
    return true;
}

// The surface point of one primary row and the direction to the light's centre.  No surface (s not finite or <= 0), a non-finite
// row or point, or a point on (or at an overflowing distance from) a point light: valid = false, every field 0.
NH_TWIN_HD ShadowPixel shadow_pixel(const ShadowLight& L, const float* __restrict__ ray, float s) {
    ShadowPixel px;
    px.p[0] = px.p[1] = px.p[2] = px.c[0] = px.c[1] = px.c[2] = px.dist = 0.0f;
    px.valid = false;
    const RayRow r = ray_row(ray);
    if (!(r.finite && finite_f32(s) && s > 0.0f)) return px;
    float p[3], c[3], dist = L.reach;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = r.o[a] + s * r.d[a];
        c[a] = L.l[a];
    }
    if (!(finite_f32(p[0]) && finite_f32(p[1]) && finite_f32(p[2]))) return px;
    if (L.kind == kLightPoint) {
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = L.l[a] - p[a];
        dist = shadow_normalise(c);
        if (!(dist > 0.0f && finite_f32(dist))) return px;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        px.p[a] = p[a];
        px.c[a] = c[a];
    }
    px.dist = dist;
    px.valid = true;
    return px;
}

// Row k of pixel i: [p, d_k, bias, far].  radius == 0 skips the offset (no multiplication by zero), so the K rows of a pixel are
// its K = 1 row in every bit.  A sample that coincides with p (or overflows) gives a zero row of its own.
NH_TWIN_HD void shadow_row(const ShadowLight& L, const ShadowPixel& px, uint32_t i, int k, float* __restrict__ row) {
#pragma unroll
    for (int q = 0; q < 8; ++q) row[q] = 0.0f;
    if (!px.valid) return;
    float d[3] = {px.c[0], px.c[1], px.c[2]};
    float far = px.dist;
    if (L.radius != 0.0f) {
        const float* c = px.c;
        const float ax = mesh_abs(c[0]), ay = mesh_abs(c[1]), az = mesh_abs(c[2]);
        const int axis = ax <= ay ? (ax <= az ? 0 : 2) : (ay <= az ? 1 : 2);
        float e1[3];    // c x axis
        e1[0] = axis == 0 ? 0.0f : (axis == 1 ? -c[2] : c[1]);
        e1[1] = axis == 0 ? c[2] : (axis == 1 ? 0.0f : -c[0]);
        e1[2] = axis == 0 ? -c[1] : (axis == 1 ? c[0] : 0.0f);
        shadow_normalise(e1);    // |c x axis| >= sqrt(2/3) for a unit c
        const float e2[3] = {c[1] * e1[2] - c[2] * e1[1], c[2] * e1[0] - c[0] * e1[2], c[0] * e1[1] - c[1] * e1[0]};
        float u, v;
        shadow_offset(i, k, L.rotate, u, v);
        const float su = L.radius * u, sv = L.radius * v;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float w = su * e1[a] + sv * e2[a];
            d[a] = L.kind == kLightPoint ? (L.l[a] + w) - px.p[a] : c[a] + w;
        }
        const float len = shadow_normalise(d);
        if (!(len > 0.0f && finite_f32(len))) return;
        far = L.kind == kLightPoint ? len : L.reach;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        row[a] = px.p[a];
        row[3 + a] = d[a];
    }
    row[6] = L.bias;
    row[7] = far;
}

// 1 off the mesh (tri < 0: the scene's shading is in its radiance).  On it max(n . c, 0) clamped to 1, n the geometric normal as
// mesh_shade_ray forms it, turned to the camera (n . d <= 0), c the pixel's direction to the light's centre; 0 for a pixel without
// rows, a triangle index outside [0, T), a vertex outside [0, V), and a normal of zero or non-finite length.
NH_TWIN_HD float shadow_cosine(const ShadowPixel& px, const float* __restrict__ ray, int32_t tri, const float* __restrict__ vertices,
                               int64_t V, const int32_t* __restrict__ triangles, int64_t T) {
    if (tri < 0) return 1.0f;
    if (!px.valid || (int64_t)tri >= T) return 0.0f;
    int32_t v[3];
    for (int c = 0; c < 3; ++c) {
        v[c] = triangles[3 * (int64_t)tri + c];
        if (v[c] < 0 || (int64_t)v[c] >= V) return 0.0f;
    }
    float p[9];
    for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a) p[3 * c + a] = vertices[3 * (int64_t)v[c] + a];
    const float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const float nd = (n[0] * ray[3] + n[1] * ray[4]) + n[2] * ray[5];
    float nl = (n[0] * px.c[0] + n[1] * px.c[1]) + n[2] * px.c[2];
    const float len = sqrtf(nn);
    if (!(len > 0.0f && finite_f32(len) && finite_f32(nd) && finite_f32(nl))) return 0.0f;
    if (nd > 0.0f) nl = -nl;
    const float cosine = nl / len;
    return cosine > 0.0f ? (cosine > 1.0f ? 1.0f : cosine) : 0.0f;
}

// ---- compose ------------------------------------------------------------------------------------------------------------------
// V of one pixel: the sum in k order of (hit_k ? 0 : 1) (times trans_k, where given) divided by K.
NH_TWIN_HD float light_visibility(const uint8_t* __restrict__ hit, const float* __restrict__ trans, int K) {
    float sum = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float open = hit[k] ? 0.0f : 1.0f;
        sum += trans ? open * trans[k] : open;
    }
    return sum / (float)K;
}

// What multiplies the pixel's rgb.  ambient = 1 and strength = 0 give an exact 1 on either layer.
NH_TWIN_HD float light_factor(bool mesh, float cosine, float V, float ambient, float strength) {
    return mesh ? ambient + ((1.0f - ambient) * cosine) * V : 1.0f - strength * (1.0f - V);
}

}  // namespace nerfhip

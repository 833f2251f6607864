// What a host/device core (a *_core.h: one per-item routine that serves a kernel and its _host twin) needs, once: the function
// qualifier, the finite test, the float/uint bit casts, and for the ray units the ray row and its clip to an axis-aligned box.
// Plain fp32 with separately rounded operations (the including file turns contraction off) and IEEE division: the device and the
// host produce the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NH_TWIN_HD __host__ __device__ inline
#else
#define NH_TWIN_HD inline
#endif

namespace nerfhip {

NH_TWIN_HD bool finite_f32(float v) {
    const float a = v < 0.0f ? -v : v;
    return a <= 3.402823466e+38f;    // false for NaN and +-inf
}
NH_TWIN_HD uint32_t float_bits(float v) {
    union {
        float f;
        uint32_t u;
    } c;
    c.f = v;
    return c.u;
}
NH_TWIN_HD float float_from_bits(uint32_t u) {
    union {
        float f;
        uint32_t u;
    } c;
    c.u = u;
    return c.f;
}

// One (n, 8) ray row = [o d near far].  finite = false: a NaN or an infinity in some column.
struct RayRow {
    float o[3], d[3];
    float near, far;
    bool finite;
};

NH_TWIN_HD RayRow ray_row(const float* __restrict__ ray) {
    RayRow r;
    r.near = ray[6];
    r.far = ray[7];
    r.finite = finite_f32(r.near) && finite_f32(r.far);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.o[a] = ray[a];
        r.d[a] = ray[3 + a];
        r.finite = r.finite && finite_f32(r.o[a]) && finite_f32(r.d[a]);
    }
    return r;
}

// Clip [near, far] of a finite row to the box [lo, hi] -> [tmin, tmax]; false when that is empty.  A zero component (either
// sign) leaves the interval alone or misses, and never divides.
NH_TWIN_HD bool ray_clip_box(const RayRow& r, const float* __restrict__ lo, const float* __restrict__ hi, float& tmin, float& tmax) {
    tmin = r.near;
    tmax = r.far;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (r.d[a] == 0.0f) {
            if (r.o[a] < lo[a] || r.o[a] > hi[a]) return false;
            continue;
        }
        const float ta = (lo[a] - r.o[a]) / r.d[a], tb = (hi[a] - r.o[a]) / r.d[a];
        tmin = fmaxf(tmin, fminf(ta, tb));
        tmax = fminf(tmax, fmaxf(ta, tb));
    }
    return tmin < tmax;
}

}  // namespace nerfhip

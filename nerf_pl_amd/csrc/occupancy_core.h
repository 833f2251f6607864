// One ray against the occupancy bitfield: the routine of the cull kernel (occupancy.hip) and of its host twin
// nerfhip_cull_rays_host, from this one source.  Plain fp32 with separately rounded operations (the including file turns
// contraction off), IEEE division, no transcendental: the device and the host produce the same bits.
//
// The ray is clipped to the grid's box and then walks the cells it pierces (Amanatides & Woo), from the front until the first
// occupied cell and from the back until the last.  A cell's planes are formed from its index at every step (lo + i h, the last
// one `hi` itself), never accumulated, so the error of a crossing parameter is that of one (p - o) / d whatever the grid size.
#pragma once
#include "twin.h"

namespace nerfhip {

struct OccGrid {
    const uint32_t* words;   // bit c = (iy M + ix) M + iz of word c >> 5
    int M;                   // cells per axis
    float lo[3], hi[3];      // axis ranges in ray order: x (-> ix), y (-> iy), z (-> iz)
    float h[3];              // (hi - lo) / M
};

struct OccVerdict {
    float t0, t1;
    uint8_t hit;
};

NH_TWIN_HD bool occ_bit(const OccGrid& g, int ix, int iy, int iz) {
    const uint32_t c = ((uint32_t)iy * (uint32_t)g.M + (uint32_t)ix) * (uint32_t)g.M + (uint32_t)iz;
    return (g.words[c >> 5] >> (c & 31)) & 1u;
}

// The plane with index i (0 .. M) of axis a.
NH_TWIN_HD float occ_plane(const OccGrid& g, int a, int i) { return i == g.M ? g.hi[a] : g.lo[a] + (float)i * g.h[a]; }

// The cell of axis a that holds coordinate p, clamped into the grid (a point on the upper face belongs to the last cell; a NaN
// or an overflowed p cannot leave the range).
NH_TWIN_HD int occ_cell(const OccGrid& g, int a, float p) {
    const float f = floorf((p - g.lo[a]) / g.h[a]);
    return (int)fminf(fmaxf(f, 0.0f), (float)(g.M - 1));
}

// Move the index of axis `ax` one cell along (dir = 1) or against (dir = -1) the ray; false when that leaves the grid.  Written
// as selects over the three axes so that the indices stay in registers.
NH_TWIN_HD bool occ_step(int* i, const float* d, int ax, int dir, int M) {
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (a != ax) continue;
        i[a] += d[a] > 0.0f ? dir : -dir;
        inside = i[a] >= 0 && i[a] < M;
    }
    return inside;
}

NH_TWIN_HD OccVerdict occ_cull_ray(const OccGrid& g, const float* __restrict__ ray) {
    const RayRow r = ray_row(ray);
    const float* o = r.o;
    const float* d = r.d;
    OccVerdict v;
    v.t0 = r.near;
    v.t1 = r.far;
    v.hit = 1;
    if (!r.finite) return v;         // culling never decides what it cannot reason about
    v.hit = 0;
    float tmin, tmax;
    if (!ray_clip_box(r, g.lo, g.hi, tmin, tmax)) return v;

    const int M = g.M;
    const int budget = 3 * M + 3;    // a walk changes one index by one per step and never turns back

    // ---- from the front: the first occupied cell ----
    int i[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) i[a] = occ_cell(g, a, o[a] + tmin * d[a]);
    float t = tmin, t0 = 0.0f, front_exit = 0.0f;
    bool found = false;
    for (int step = 0; step < budget; ++step) {
        // where the ray leaves this cell: the nearest of the three planes ahead
        float tn = INFINITY;
        int ax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (d[a] == 0.0f) continue;
            const float ta = (occ_plane(g, a, i[a] + (d[a] > 0.0f ? 1 : 0)) - o[a]) / d[a];
            if (ta < tn) {
                tn = ta;
                ax = a;
            }
        }
        if (occ_bit(g, i[0], i[1], i[2])) {
            found = true;
            t0 = t;
            front_exit = fminf(tmax, fmaxf(tn, t));
            break;
        }
        t = fmaxf(t, tn);
        if (!(t < tmax)) break;
        if (!occ_step(i, d, ax, 1, M)) break;
    }
    if (!found) return v;

    // ---- from the back: the last occupied cell ----
#pragma unroll
    for (int a = 0; a < 3; ++a) i[a] = occ_cell(g, a, o[a] + tmax * d[a]);
    float t1 = front_exit;
    t = tmax;
    for (int step = 0; step < budget; ++step) {
        if (occ_bit(g, i[0], i[1], i[2])) {
            t1 = t;
            break;
        }
        // where the ray entered this cell: the latest of the three planes behind
        float tp = -INFINITY;
        int ax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (d[a] == 0.0f) continue;
            const float ta = (occ_plane(g, a, i[a] + (d[a] > 0.0f ? 0 : 1)) - o[a]) / d[a];
            if (ta > tp) {
                tp = ta;
                ax = a;
            }
        }
        t = fminf(t, tp);
        if (!(t > t0)) break;        // back at the first occupied cell: its own exit stands
        if (!occ_step(i, d, ax, -1, M)) break;
    }
    t1 = fmaxf(t1, front_exit);      // the last occupied cell is never in front of the first one
    if (t0 < t1) {
        v.t0 = t0;
        v.t1 = t1;
        v.hit = 1;
    }
    return v;
}

}  // namespace nerfhip

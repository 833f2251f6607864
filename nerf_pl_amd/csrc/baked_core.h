// One ray through the baked RGBA volume: the routine of the render kernel (baked.hip) and of its host twin
// nerfhip_baked_render_host, from this one source.  Plain fp32 with separately rounded operations (the including file turns
// contraction off) and IEEE division and square root; the device and the host differ only in their exp2f / log2f.
//
// The volume is the N^3 RGBA8 lattice of a .vol file, indexed [iy, ix, iz], stored in 8^3-point bricks of 2 KiB (include/nerfhip.h
// holds the layout).  The ray is clipped to the lattice's box and marched in segments of step * cell world units; every segment
// takes one alpha-weighted trilinear sample at its midpoint, corrects the stored opacity (which belongs to a thickness of `cell`)
// to the segment's own length and composites front to back.  Segment k starts at t_in + k dt — formed from k, never accumulated —
// and the last one is cut at t_out, so the result is continuous in both ends.
//
// Skipping: a sample whose own cell lies in a cell brick with a clear bit gathers nothing (all 8 corners have A = 0: alpha is an
// exact 0 and T * 1 an exact T, so the result keeps its bits).  The march then leaps towards the brick's exit — the nearest of
// its three planes ahead, each formed from its index as occupancy_core.h forms a cell's — and lands at least one whole segment
// short of it, so every sample it passes over has its midpoint 1.5 segments inside a brick whose bit is clear; `step` >= 1/16
// keeps that margin far above the fp32 error of a lattice coordinate.  The landing sample tests its own bit like any other, and a
// landing outside the brick the leap started in takes the leap back: no sample is skipped on the strength of the walk alone.
#pragma once
#include "twin.h"

namespace nerfhip {

constexpr int kBakedMaxSegments = 1 << 20;    // the launch refuses a box whose diagonal needs more segments than this

struct BakedVol {
    const uint32_t* points;   // bricked lattice, one little-endian word per point: R | G << 8 | B << 16 | A << 24
    const uint32_t* bits;     // cell-brick bitfield, or null: every brick occupied
    int N, NB, MB;            // points, point bricks and cell bricks per axis
    float lo[3], hi[3];       // axis ranges in ray order: x (-> ix), y (-> iy), z (-> iz)
    float scale[3];           // (N - 1) / (hi - lo)
    float cell, step, t_stop;
    int white_back;
};

struct BakedPixel {
    float rgb[3], depth, opacity;
};

// The position, in points, of lattice point (iy, ix, iz) in the bricked volume.
NH_TWIN_HD uint64_t baked_point_index(int NB, uint32_t iy, uint32_t ix, uint32_t iz) {
    const uint64_t brick = ((uint64_t)(iy >> 3) * (uint32_t)NB + (ix >> 3)) * (uint32_t)NB + (iz >> 3);
    const uint32_t local = ((((iy & 7u) << 3) | (ix & 7u)) << 3) | (iz & 7u);
    return (brick << 9) | local;
}

NH_TWIN_HD BakedPixel baked_march(const BakedVol& v, const float* __restrict__ ray) {
    const float bg = v.white_back ? 1.0f : 0.0f;
    BakedPixel px;
    px.rgb[0] = px.rgb[1] = px.rgb[2] = bg;
    px.depth = 0.0f;
    px.opacity = 0.0f;

    const RayRow row = ray_row(ray);
    if (!row.finite) return px;
    const float* o = row.o;
    const float* d = row.d;
    const float dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(dn > 0.0f) || !finite_f32(dn)) return px;      // a zero direction (also one whose squares underflow or overflow)
    float t_in, t_out;
    if (!ray_clip_box(row, v.lo, v.hi, t_in, t_out)) return px;
    float rd[3], h[3];                                   // what a leap needs: 1 / d (0 for a zero component) and the point spacing
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        h[a] = (v.hi[a] - v.lo[a]) / (float)(v.N - 1);
        rd[a] = d[a] == 0.0f ? 0.0f : 1.0f / d[a];
    }

    const float dt = (v.step * v.cell) / dn;
    if (!(dt > 0.0f)) return px;
    const float inv_dt = 1.0f / dt;                      // only places a leap, which is conservative by a whole segment
    const int K = (int)fminf(ceilf((t_out - t_in) / dt), (float)(2 * kBakedMaxSegments));
    const float top = (float)(v.N - 2);

    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, depth = 0.0f, opacity = 0.0f;
    int k = 0, leap_from = -1;
    uint32_t leap_brick = 0;
    while (k < K) {
        const float ta = t_in + (float)k * dt;
        const float tb = fminf(ta + dt, t_out);
        const float delta = fmaxf(tb - ta, 0.0f);        // a K one too large in this arithmetic adds a segment of length 0
        const float tm = ta + delta * 0.5f;
        int c[3];
        float f[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float ga = (o[a] + tm * d[a] - v.lo[a]) * v.scale[a];
            const float cf = fminf(fmaxf(floorf(ga), 0.0f), top);
            c[a] = (int)cf;
            f[a] = fminf(fmaxf(ga - cf, 0.0f), 1.0f);
        }

        if (v.bits) {
            const uint32_t brick = ((uint32_t)(c[1] >> 3) * (uint32_t)v.MB + (uint32_t)(c[0] >> 3)) * (uint32_t)v.MB + (uint32_t)(c[2] >> 3);
            if (leap_from >= 0 && brick != leap_brick) {  // landed outside the brick that was left: walk it sample by sample
                k = leap_from + 1;
                leap_from = -1;
                continue;
            }
            leap_from = -1;
            if (!((v.bits[brick >> 5] >> (brick & 31u)) & 1u)) {
                // where the ray leaves this brick: the nearest of the three planes ahead
                float te = INFINITY;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (d[a] == 0.0f) continue;
                    const int first = (c[a] >> 3) << 3;
                    const int pi = d[a] > 0.0f ? (first + 8 < v.N - 1 ? first + 8 : v.N - 1) : first;
                    const float plane = pi == v.N - 1 ? v.hi[a] : v.lo[a] + (float)pi * h[a];
                    te = fminf(te, (plane - o[a]) * rd[a]);
                }
                const float kf = floorf((te - t_in) * inv_dt) - 1.0f;    // segment kf + 1 still ends at or before te
                int kn = k + 1;
                if (kf > (float)kn) {
                    kn = (int)fminf(kf, (float)K);
                    leap_from = k;
                    leap_brick = brick;
                }
                k = kn;
                continue;
            }
        }

        // alpha-weighted trilinear sample of the 8 corners, on the stored bytes: a = sa / 255, colour = sc / (255 sa)
        float sa = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int qy = q >> 2, qx = (q >> 1) & 1, qz = q & 1;
            const uint32_t p = v.points[baked_point_index(v.NB, (uint32_t)(c[1] + qy), (uint32_t)(c[0] + qx), (uint32_t)(c[2] + qz))];
            const float w = ((qy ? f[1] : 1.0f - f[1]) * (qx ? f[0] : 1.0f - f[0])) * (qz ? f[2] : 1.0f - f[2]);
            const float wa = w * (float)(p >> 24);
            sa += wa;
            sr += wa * (float)(p & 255u);
            sg += wa * (float)((p >> 8) & 255u);
            sb += wa * (float)((p >> 16) & 255u);
        }
        if (sa > 0.0f) {
            const float alpha_cell = fminf(sa / 255.0f, 1.0f);
            const float e = (delta * dn) / v.cell;       // the segment's world length in units of `cell`
            const float alpha = e > 0.0f ? 1.0f - exp2f(e * log2f(1.0f - alpha_cell)) : 0.0f;
            const float w = T * alpha;
            const float den = sa * 255.0f;
            r += w * (sr / den);
            g += w * (sg / den);
            b += w * (sb / den);
            depth += w * tm;
            opacity += w;
            T *= 1.0f - alpha;
            if (T < v.t_stop) break;
        }
        ++k;
    }
    const float rest = v.white_back ? 1.0f - opacity : 0.0f;
    px.rgb[0] = r + rest;
    px.rgb[1] = g + rest;
    px.rgb[2] = b + rest;
    px.depth = depth;
    px.opacity = opacity;
    return px;
}

}  // namespace nerfhip

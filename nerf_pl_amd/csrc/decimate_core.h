// Mesh decimation by grid vertex clustering (Rossignac-Borrel) with mean or quadric placement (Lindstrom 2000); DESIGN.md §22 and
// include/nerfhip.h state the contract.  The per-vertex, per-cluster and per-triangle routines of the kernels (decimate.hip) and of
// their host twins, from this one source.  fp32 quantisation with separately rounded operations and IEEE division, fp64 sums in a
// fixed order, fp64 IEEE division (the including file turns contraction off), floorf and no other libm call: the device and the
// host give the same bits.
#pragma once
#include "twin.h"

namespace nerfhip {

constexpr int64_t kDecimateMaxItems = (int64_t)1 << 28;       // vertices, triangles
constexpr int64_t kDecimateNoCell = 0x7fffffff;               // the cell (and cluster) of a key that belongs to none: sorts last
constexpr int64_t kDecimateIdMask = ((int64_t)1 << 28) - 1;
constexpr int64_t kDecimateNoKey = 0x7fffffffffffffffll;      // the rotation key of a triangle that is no candidate

enum { kDecimateKeep = 0, kDecimateBad = 1, kDecimateCollapsed = 2, kDecimateDuplicate = 3 };    // a triangle's flag

// The cell grid: lo (the per-axis minimum, or the origin), the cell size, R cells per axis.
struct DecimateGrid {
    float lo[3];
    float cell;
    int32_t R[3];
};

NH_TWIN_HD bool decimate_finite(const float* __restrict__ v) { return finite_f32(v[0]) && finite_f32(v[1]) && finite_f32(v[2]); }

// Cell number c = (q0 R1 + q1) R2 + q2 with q_a = floorf((v_a - lo_a) / cell); kDecimateNoCell for a non-finite vertex (or one
// outside the grid, which the wrappers' bounds rule out).
NH_TWIN_HD int64_t decimate_cell_of(const float* __restrict__ v, const DecimateGrid& g) {
    if (!decimate_finite(v)) return kDecimateNoCell;
    int64_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = v[a] - g.lo[a];
        const float f = floorf(d / g.cell);
        if (!(f >= 0.0f && (double)f < (double)g.R[a])) return kDecimateNoCell;
        q[a] = (int64_t)f;
    }
    return (q[0] * g.R[1] + q[1]) * g.R[2] + q[2];
}

NH_TWIN_HD int64_t decimate_vertex_key(const float* __restrict__ v, const DecimateGrid& g, int64_t id) {
    return (decimate_cell_of(v, g) << 32) | id;
}

// Mean of the members [s0, s1) of one cluster (sorted keys: ascending vertex id): fp64 sums in that order over the count;
// colours per channel (2 s + n) / (2 n) in integers.
NH_TWIN_HD void decimate_mean(const float* __restrict__ vertices, int64_t V, const uint8_t* __restrict__ colors,
                              const int64_t* __restrict__ sorted_keys, int64_t s0, int64_t s1, double* __restrict__ m, uint8_t* __restrict__ rgb) {
    double sum[3] = {0.0, 0.0, 0.0};
    int64_t csum[3] = {0, 0, 0};
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t v = sorted_keys[s] & 0xffffffffll;
        if (v >= V) continue;    // no key of decimate_vertex_key
#pragma unroll
        for (int a = 0; a < 3; ++a) sum[a] += (double)vertices[3 * v + a];
        if (colors) {
#pragma unroll
            for (int a = 0; a < 3; ++a) csum[a] += colors[3 * v + a];
        }
    }
    const int64_t n = s1 - s0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        m[a] = sum[a] / (double)n;
        if (colors) rgb[a] = (uint8_t)((2 * csum[a] + n) / (2 * n));
    }
}

// First position of `sorted` (n ascending keys) whose key is >= key: at most 31 steps.
NH_TWIN_HD int64_t decimate_lower_bound(const int64_t* __restrict__ sorted, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// x of (A + lambda I) x = -b by cofactors, A symmetric = [a00 a01 a02 a11 a12 a22]; 0 for a zero or non-finite trace and for a
// non-finite solution.
NH_TWIN_HD void decimate_solve(const double* __restrict__ A, const double* __restrict__ b, double eps, double* __restrict__ x) {
    x[0] = x[1] = x[2] = 0.0;
    const double trace = A[0] + A[3] + A[5];
    if (!(trace > 0.0 && trace <= 1.7976931348623157e308)) return;
    const double lambda = eps * trace;
    const double a00 = A[0] + lambda, a01 = A[1], a02 = A[2], a11 = A[3] + lambda, a12 = A[4], a22 = A[5] + lambda;
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double r[3] = {-b[0], -b[1], -b[2]};
    const double y[3] = {(c00 * r[0] + c01 * r[1] + c02 * r[2]) / det, (c01 * r[0] + c11 * r[1] + c12 * r[2]) / det,
                         (c02 * r[0] + c12 * r[1] + c22 * r[2]) / det};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ay = y[a] < 0.0 ? -y[a] : y[a];
        ok = ok && ay <= 1.7976931348623157e308;
    }
    if (ok) x[0] = y[0], x[1] = y[1], x[2] = y[2];
}

// Quadric placement of cluster `cl` in cell `c`: the entries [e0, e1) of sorted_entries (cluster << 32 | 3 t + k, ascending) name
// the triangles with a corner in the cluster, once per such corner; n = (p1 - p0) x (p2 - p0), d = -n . (p0 - m), A += n n^T,
// b += d n in that order; then the solve, and clamp(m + x) to the cell's box.
NH_TWIN_HD void decimate_quadric(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t T,
                                 const int64_t* __restrict__ sorted_entries, int64_t e0, int64_t e1, const double* __restrict__ m, int64_t c,
                                 const DecimateGrid& g, double eps, double* __restrict__ pos) {
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
    for (int64_t s = e0; s < e1; ++s) {
        const int64_t t = (sorted_entries[s] & 0xffffffffll) / 3;
        if (t >= T) continue;    // no entry of a triangle
        double p[3][3];
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t v = triangles[3 * t + k];
            in = in && v >= 0 && v < V;
#pragma unroll
            for (int a = 0; a < 3; ++a) p[k][a] = in ? (double)vertices[3 * v + a] : 0.0;
        }
        if (!in) continue;
        double u[3], w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            u[a] = p[1][a] - p[0][a];
            w[a] = p[2][a] - p[0][a];
        }
        const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double d = -((n[0] * (p[0][0] - m[0]) + n[1] * (p[0][1] - m[1])) + n[2] * (p[0][2] - m[2]));
        A[0] += n[0] * n[0];
        A[1] += n[0] * n[1];
        A[2] += n[0] * n[2];
        A[3] += n[1] * n[1];
        A[4] += n[1] * n[2];
        A[5] += n[2] * n[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) b[a] += d * n[a];
    }
    double x[3];
    decimate_solve(A, b, eps, x);
    const int64_t q[3] = {c / ((int64_t)g.R[1] * g.R[2]), (c / g.R[2]) % g.R[1], c % g.R[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double blo = (double)g.lo[a] + (double)q[a] * (double)g.cell, bhi = blo + (double)g.cell;
        const double y = m[a] + x[a];
        pos[a] = y < blo ? blo : (y > bhi ? bhi : y);
    }
}

// A good triangle: every index inside [0, V) and every corner in a cluster (cluster_of < 0: a non-finite vertex).  ids gets the
// corners' clusters.
NH_TWIN_HD bool decimate_triangle(const int32_t* __restrict__ triangles, int64_t t, int64_t V, const int32_t* __restrict__ cluster_of,
                                  int32_t* __restrict__ ids) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t v = triangles[3 * t + k];
        const bool in = v >= 0 && (int64_t)v < V;
        ids[k] = in ? cluster_of[v] : -1;
        ok = ok && ids[k] >= 0;
    }
    return ok;
}

// The flag of triangle t and the two halves of its duplicate key: hi = a << 28 | b, lo = c << 28 | t for (a, b, c) = the corner
// clusters rotated to put the smallest first.  A bad or collapsed triangle has hi = kDecimateNoKey.
NH_TWIN_HD int decimate_triangle_key(const int32_t* __restrict__ triangles, int64_t t, int64_t V, const int32_t* __restrict__ cluster_of,
                                     int64_t& hi, int64_t& lo) {
    int32_t id[3];
    hi = kDecimateNoKey;
    lo = t;
    if (!decimate_triangle(triangles, t, V, cluster_of, id)) return kDecimateBad;
    if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) return kDecimateCollapsed;
    const int r = (id[1] < id[0] && id[1] < id[2]) ? 1 : ((id[2] < id[0] && id[2] < id[1]) ? 2 : 0);
    const int64_t a = id[r], b = id[(r + 1) % 3], c = id[(r + 2) % 3];
    hi = (a << 28) | b;
    lo = (c << 28) | t;
    return kDecimateKeep;
}

}  // namespace nerfhip

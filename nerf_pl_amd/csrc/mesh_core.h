// Nearest-hit ray casting against a triangle mesh: the per-triangle, per-node and per-ray routines of the kernels
// (meshcast.hip) and of their host twins, from this one source.  Plain fp32 with separately rounded operations (the including file
// turns contraction off), IEEE division and square root, no libm: the device and the host give the same bits.
//
// The hierarchy has an implicit topology (include/nerfhip.h states the format): the triangles sorted by a Morton key, leaf j = sorted
// triangles [4j, 4j + 4), every node of a level above = 8 consecutive nodes of the level below, the levels concatenated from the
// leaves to the root.  No child pointers: a node is (level, i), and the traversal moves by index arithmetic.
//
// The triangle test is the watertight one of Woop, Benthin and Wald (JCGT 2013).  The ray's dominant axis becomes z, the triangle
// is translated to the ray's origin and sheared so that the ray runs along +z, and the 2D edge functions of the sheared vertices
// decide.  Each edge function is a difference of two separately rounded products: rounding is monotonic, so a non-zero difference
// has the exact sign, and an exact 0 is recomputed in double, where the products are exact.  The test is therefore an exact
// point-in-triangle test of the *sheared fp32 vertices*, and two triangles sharing an edge evaluate that edge's function from the
// same two sheared vertices with opposite sign: no ray passes between them.
#pragma once
#include "twin.h"

namespace nerfhip {

constexpr int64_t kMeshMaxTriangles = (int64_t)1 << 28;
constexpr int kMeshLeaf = 4;          // triangles per leaf
constexpr int kMeshFan = 8;           // children per inner node
constexpr int kMeshMaxLevels = 10;    // 2^28 triangles: 2^26 leaves, then 2^23, 2^20, ..., 2^2, 1
constexpr uint32_t kMeshBadMorton = 1u << 30;    // the key of a bad triangle: behind every good one

struct alignas(16) MeshVec4 {
    float x, y, z, w;
};

// The hierarchy as a cast reads it.
struct MeshBvh {
    const MeshVec4* tris;    // 3 units per sorted triangle: (v0, index bits), (v1, 0), (v2, 0); index -1: a bad triangle
    const float* boxes;      // (n_nodes, 6): lo xyz, hi xyz; null: test every triangle (the brute-force twin)
    int64_t T;
    int n0;                  // leaves
    int levels;              // 0 for T = 0
    int n_nodes;
};

struct MeshHit {
    int32_t tri;
    float t, b1, b2;
};

NH_TWIN_HD float mesh_abs(float v) { return v < 0.0f ? -v : v; }
// min and max in the total order that puts -0 below +0: exact and independent of the order of the operands (no NaN reaches them)
NH_TWIN_HD float mesh_min(float a, float b) { return (b < a || (b == a && (float_bits(b) >> 31))) ? b : a; }
NH_TWIN_HD float mesh_max(float a, float b) { return (b > a || (b == a && !(float_bits(b) >> 31))) ? b : a; }
// the same order on unsigned integers, for the atomics of the bounds
NH_TWIN_HD uint32_t mesh_ordered(float v) {
    const uint32_t u = float_bits(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
NH_TWIN_HD float mesh_unordered(uint32_t e) { return float_from_bits((e >> 31) ? (e & 0x7fffffffu) : ~e); }

NH_TWIN_HD int mesh_levels(int64_t T) {
    if (T <= 0) return 0;
    int64_t n = (T + kMeshLeaf - 1) / kMeshLeaf;
    int levels = 1;
    while (n > 1) {
        n = (n + kMeshFan - 1) / kMeshFan;
        ++levels;
    }
    return levels;
}
NH_TWIN_HD int64_t mesh_nodes(int64_t T) {
    if (T <= 0) return 0;
    int64_t n = (T + kMeshLeaf - 1) / kMeshLeaf, total = n;
    while (n > 1) {
        n = (n + kMeshFan - 1) / kMeshFan;
        total += n;
    }
    return total;
}
// nodes of level k: ceil(n0 / 8^k)  (a ceiling of ceilings is the ceiling of the whole)
NH_TWIN_HD int mesh_level_nodes(int n0, int k) { return (int)(((int64_t)n0 + (((int64_t)1 << (3 * k)) - 1)) >> (3 * k)); }

// ---- build --------------------------------------------------------------------------------------------------------------------
// The 9 coordinates of triangle t, or false for a bad triangle: an index outside [0, V) or a non-finite coordinate.
NH_TWIN_HD bool mesh_triangle(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t t,
                              float* __restrict__ p) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int32_t v = triangles[3 * t + c];
        const bool in = v >= 0 && (int64_t)v < V;
        ok = ok && in;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = in ? vertices[3 * (int64_t)v + a] : 0.0f;
            p[3 * c + a] = x;
            ok = ok && finite_f32(x);
        }
    }
    return ok;
}

NH_TWIN_HD uint32_t mesh_spread10(uint32_t v) {    // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// morton30 of the centroid quantised to 10 bits per axis in [lo, hi] (x in the highest bit of every triple) << 32 | t.
NH_TWIN_HD int64_t mesh_key(const float* __restrict__ p, bool ok, const float* __restrict__ lo, const float* __restrict__ hi, int64_t t) {
    uint32_t m = kMeshBadMorton;
    if (ok) {
        uint32_t q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float c = ((p[a] + p[3 + a]) + p[6 + a]) / 3.0f;
            const float ext = hi[a] - lo[a];
            const float x = ext > 0.0f ? ((c - lo[a]) / ext) * 1024.0f : 0.0f;
            q[a] = x >= 1023.0f ? 1023u : (x > 0.0f ? (uint32_t)x : 0u);    // NaN (an overflowed sum or extent) -> 0
        }
        m = (mesh_spread10(q[0]) << 2) | (mesh_spread10(q[1]) << 1) | mesh_spread10(q[2]);
    }
    return (int64_t)(((uint64_t)m << 32) | (uint64_t)(uint32_t)t);
}

// Leaf j: packs its (up to) 4 sorted triangles and writes their box.  A bad triangle, or a key whose index is outside [0, T),
// is stored with index -1 and zero coordinates and adds nothing to the box; a leaf of bad triangles only has the empty box
// (lo = +inf, hi = -inf), the neutral element of the levels above.
NH_TWIN_HD void mesh_leaf(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t T,
                          const int64_t* __restrict__ sorted_keys, int64_t j, MeshVec4* __restrict__ tris, float* __restrict__ boxes) {
    const float inf = float_from_bits(0x7f800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int64_t s = kMeshLeaf * j; s < kMeshLeaf * j + kMeshLeaf && s < T; ++s) {
        const int64_t t = (int64_t)(uint32_t)((uint64_t)sorted_keys[s] & 0xffffffffu);
        float p[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const bool ok = t < T && mesh_triangle(vertices, V, triangles, t, p);
        MeshVec4 u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u[c].x = ok ? p[3 * c] : 0.0f;
            u[c].y = ok ? p[3 * c + 1] : 0.0f;
            u[c].z = ok ? p[3 * c + 2] : 0.0f;
            u[c].w = 0.0f;
        }
        u[0].w = float_from_bits(ok ? (uint32_t)t : 0xffffffffu);
#pragma unroll
        for (int c = 0; c < 3; ++c) tris[3 * s + c] = u[c];
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    lo[a] = mesh_min(lo[a], p[3 * c + a]);
                    hi[a] = mesh_max(hi[a], p[3 * c + a]);
                }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        boxes[6 * j + a] = lo[a];
        boxes[6 * j + 3 + a] = hi[a];
    }
}

// Node i of a level above the leaves: the union of children [8 i, 8 i + 8) ∩ [0, n_child) of the level below.
NH_TWIN_HD void mesh_node(const float* __restrict__ child, int n_child, int i, float* __restrict__ out) {
    const float inf = float_from_bits(0x7f800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int c = kMeshFan * i; c < kMeshFan * i + kMeshFan && c < n_child; ++c) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = mesh_min(lo[a], child[6 * (int64_t)c + a]);
            hi[a] = mesh_max(hi[a], child[6 * (int64_t)c + 3 + a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[6 * (int64_t)i + a] = lo[a];
        out[6 * (int64_t)i + 3 + a] = hi[a];
    }
}

// ---- cast ---------------------------------------------------------------------------------------------------------------------
NH_TWIN_HD float mesh_pick(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// What the ray contributes to every triangle test: its row, and the shear of the watertight test.
struct MeshRay : RayRow {
    int kx, ky, kz;
    float Sx, Sy, Sz;
    bool valid;
};

// valid = false: the ray hits nothing (a non-finite value in any column, or a zero direction).  Every field is set on every path.
NH_TWIN_HD MeshRay mesh_ray(const float* __restrict__ ray) {
    MeshRay r;
    static_cast<RayRow&>(r) = ray_row(ray);
    const float ax = mesh_abs(r.d[0]), ay = mesh_abs(r.d[1]), az = mesh_abs(r.d[2]);
    const int kz = ax >= ay ? (ax >= az ? 0 : 2) : (ay >= az ? 1 : 2);
    const int k1 = kz == 2 ? 0 : kz + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    const float dk = mesh_pick(r.d[0], r.d[1], r.d[2], kz);
    r.valid = r.finite && dk != 0.0f;
    const float dz = r.valid ? dk : 1.0f;
    r.kz = kz;
    r.kx = dz < 0.0f ? k2 : k1;    // swapped for a negative dominant component: keeps the winding
    r.ky = dz < 0.0f ? k1 : k2;
    r.Sx = mesh_pick(r.d[0], r.d[1], r.d[2], r.kx) / dz;
    r.Sy = mesh_pick(r.d[0], r.d[1], r.d[2], r.ky) / dz;
    r.Sz = 1.0f / dz;
    return r;
}

// One triangle against the ray: updates `best` when it is hit within [near, far] and nearer than `best`, or as near with a lower
// index.  Two-sided.  `best.tri` < 0 means nothing was hit so far.
NH_TWIN_HD void mesh_test(const MeshRay& r, const MeshVec4& v0, const MeshVec4& v1, const MeshVec4& v2, MeshHit& best) {
    const int32_t index = (int32_t)float_bits(v0.w);
    if (index < 0) return;    // a bad triangle
    const float a0 = v0.x - r.o[0], a1 = v0.y - r.o[1], a2 = v0.z - r.o[2];
    const float b0 = v1.x - r.o[0], b1 = v1.y - r.o[1], b2 = v1.z - r.o[2];
    const float c0 = v2.x - r.o[0], c1 = v2.y - r.o[1], c2 = v2.z - r.o[2];
    const float Akz = mesh_pick(a0, a1, a2, r.kz), Bkz = mesh_pick(b0, b1, b2, r.kz), Ckz = mesh_pick(c0, c1, c2, r.kz);
    const float Ax = mesh_pick(a0, a1, a2, r.kx) - r.Sx * Akz, Ay = mesh_pick(a0, a1, a2, r.ky) - r.Sy * Akz;
    const float Bx = mesh_pick(b0, b1, b2, r.kx) - r.Sx * Bkz, By = mesh_pick(b0, b1, b2, r.ky) - r.Sy * Bkz;
    const float Cx = mesh_pick(c0, c1, c2, r.kx) - r.Sx * Ckz, Cy = mesh_pick(c0, c1, c2, r.ky) - r.Sy * Ckz;
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {    // on an edge or a vertex in fp32: the products are exact in double
        U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
        V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
        W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
    }
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return;
    const float det = U + V + W;
    if (det == 0.0f) return;
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const float t = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(t >= r.near && t <= r.far)) return;    // also a NaN or an infinite t
    if (best.tri >= 0 && !(t < best.t || (t == best.t && index < best.tri))) return;
    best.tri = index;
    best.t = t;
    best.b1 = V / det;
    best.b2 = W / det;
}

// May the node's box hold a triangle that mesh_test would still accept?  Conservative, by this argument.  mesh_test is an exact
// test of the sheared fp32 vertices (above), each of which differs from the exactly sheared vertex by the roundings of v - o, of S,
// of S * (v - o)_kz and of the final subtraction: less than 6 * 2^-24 M along kx and ky, where M bounds every |v - o| component
// of the box's contents — here the largest |lo - o|, |hi - o| over the axes.  An accepted ray therefore passes through a triangle
// whose vertices are moved by less than that within the kx-ky plane, so it passes through the box widened by it, and the accepted
// t — a convex combination of the S_z (v - o)_kz, a few 2^-24 M / |d_kz| from the parameter of that crossing — lies in the
// widened box's interval on every axis, because |d_a| <= |d_kz| turns a margin in space into at least that margin in t.  The box
// is widened by delta = 2^-18 M = 64 * 2^-24 M on every side, ten times the bound, which also covers the three roundings of each
// slab end below, plus 2^-126, which covers the roundings of the denormal range, where they are absolute (2^-150) and not
// relative.  A box of zero thickness is widened like any other.  A direction component that is zero (either sign) never
// divides: the axis only asks whether the origin lies within the widened slab.  The interval is cut to [near, limit] with
// limit = min(far, best t so far), keeping t == limit because an equal t with a lower index still wins.  A non-finite M (a box
// 1e38 wide) prunes nothing.  The empty box (lo > hi) holds nothing.
NH_TWIN_HD bool mesh_box_may_hit(const MeshRay& r, const float* __restrict__ box, float limit) {
    if (box[0] > box[3]) return false;
    float el[3], eh[3], M = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        el[a] = box[a] - r.o[a];
        eh[a] = box[3 + a] - r.o[a];
        const float m0 = mesh_abs(el[a]), m1 = mesh_abs(eh[a]);
        M = m0 > M ? m0 : M;
        M = m1 > M ? m1 : M;
    }
    if (!finite_f32(M)) return true;
    const float delta = M * 3.814697265625e-06f + 1.17549435e-38f;    // 2^-18 M + the smallest normal number
    float tn = r.near, tf = limit;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = el[a] - delta, h = eh[a] + delta;
        if (r.d[a] == 0.0f) {
            if (l > 0.0f || h < 0.0f) return false;
            continue;
        }
        const float t0 = l / r.d[a], t1 = h / r.d[a];
        const float lo_t = t0 < t1 ? t0 : t1, hi_t = t0 < t1 ? t1 : t0;
        tn = lo_t > tn ? lo_t : tn;    // an overflowed +-inf end orders as it should; no NaN: l, h and d are finite, d != 0
        tf = hi_t < tf ? hi_t : tf;
    }
    return tn <= tf;
}

// The nearest hit of one ray (n, 8) row = [o d near far].  A miss is tri = -1, t = b1 = b2 = 0.
//
// Traversal without a stack and without recursion: the state is (level, i, offset of the level in `boxes`).  A node that may be
// hit and is not a leaf is left for its first child 8 i; every other node is left for i + 1, after climbing while i is the last
// child of its parent (i % 8 == 7 or i + 1 == n_level).  That is a fixed pre-order in which every node is visited at most once,
// so the loop body runs at most n_nodes times — the hard bound of the loop counter below, for any input, boxes of garbage
// included — and the inner climb at most `levels` <= 10 times.  The level's size and offset come from n0 by arithmetic
// (mesh_level_nodes), so no private array is indexed and nothing lands in scratch.
NH_TWIN_HD MeshHit mesh_cast_ray(const MeshBvh& b, const float* __restrict__ ray) {
    MeshHit best;
    best.tri = -1;
    best.t = best.b1 = best.b2 = 0.0f;
    const MeshRay r = mesh_ray(ray);
    if (!r.valid || b.T <= 0) return best;

    if (!b.boxes) {    // brute force: every triangle, in storage order (the tie rule makes the order immaterial)
        for (int64_t s = 0; s < b.T; ++s) mesh_test(r, b.tris[3 * s], b.tris[3 * s + 1], b.tris[3 * s + 2], best);
        return best;
    }

    int level = b.levels - 1, i = 0;
    int n_level = 1;                    // the root's level has one node
    int off = b.n_nodes - 1;
    for (int visit = 0; visit < b.n_nodes; ++visit) {
        const float limit = best.tri >= 0 && best.t < r.far ? best.t : r.far;
        const bool may = mesh_box_may_hit(r, b.boxes + 6 * (int64_t)(off + i), limit);
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
                if (s < b.T) mesh_test(r, b.tris[3 * s], b.tris[3 * s + 1], b.tris[3 * s + 2], best);
            }
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
    return best;
}

// ---- shade and compose --------------------------------------------------------------------------------------------------------
// rgb of one ray: the barycentric blend of the hit triangle's vertex colours (bytes / 255; null: white) times
// ambient + (1 - ambient) |n . d| / (|n| |d|), n the geometric normal; the background for a miss, for a triangle index outside
// [0, T) and for a triangle that names a vertex outside [0, V).  A normal or direction of zero or non-finite length shades with
// `ambient` alone.
NH_TWIN_HD void mesh_shade_ray(const float* __restrict__ ray, int32_t tri, float b1, float b2, const float* __restrict__ vertices,
                               int64_t V, const int32_t* __restrict__ triangles, int64_t T, const uint8_t* __restrict__ colors,
                               float ambient, float background, float* __restrict__ rgb) {
    rgb[0] = rgb[1] = rgb[2] = background;
    if (tri < 0 || (int64_t)tri >= T) return;
    int32_t v[3];
    for (int c = 0; c < 3; ++c) {
        v[c] = triangles[3 * (int64_t)tri + c];
        if (v[c] < 0 || (int64_t)v[c] >= V) return;
    }
    float p[9];
    for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a) p[3 * c + a] = vertices[3 * (int64_t)v[c] + a];
    const float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float d[3] = {ray[3], ray[4], ray[5]};
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float nd = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    const float len = sqrtf(nn) * sqrtf(dd);
    float cosine = 0.0f;
    if (len > 0.0f && finite_f32(len) && finite_f32(nd)) {
        cosine = mesh_abs(nd) / len;
        cosine = cosine > 1.0f ? 1.0f : cosine;
    }
    const float shade = ambient + (1.0f - ambient) * cosine;
    const float b0 = (1.0f - b1) - b2;
    for (int a = 0; a < 3; ++a) {
        float c0 = 1.0f, c1 = 1.0f, c2 = 1.0f;
        if (colors) {
            c0 = (float)colors[3 * (int64_t)v[0] + a] / 255.0f;
            c1 = (float)colors[3 * (int64_t)v[1] + a] / 255.0f;
            c2 = (float)colors[3 * (int64_t)v[2] + a] / 255.0f;
        }
        rgb[a] = ((b0 * c0 + b1 * c1) + b2 * c2) * shade;
    }
}

constexpr int kMixedZtest = 0, kMixedClip = 1;

struct MixedPixel {
    float rgb[3], depth, opacity;
    uint8_t mask;
};

// ztest: the depth test of the Unity demo.  s = opacity >= tau ? depth / opacity : +inf; the mesh wins iff it is hit and t < s;
// the winner's rgb and depth pass through, opacity is 1 where the mesh wins, mask says where it won.
// clip: the inner render was made with far = min(far, t) on hit rays and without a background; the mesh (or the background on a
// miss) fills what it left: rgb = rgb_n + (1 - opacity_n) (hit ? rgb_m : background), depth = depth_n + (1 - opacity_n) t and
// opacity = 1 on a hit, depth_n and opacity_n on a miss; mask = hit.
NH_TWIN_HD MixedPixel mixed_compose_ray(int mode, const float* __restrict__ rgb_n, float depth_n, float opacity_n, int32_t tri, float t,
                                        const float* __restrict__ rgb_m, float tau, float background) {
    MixedPixel px;
    const bool hit = tri >= 0;
    if (mode == kMixedZtest) {
        const float s = opacity_n >= tau ? depth_n / opacity_n : float_from_bits(0x7f800000u);
        const bool mesh = hit && t < s;
        for (int a = 0; a < 3; ++a) px.rgb[a] = mesh ? rgb_m[a] : rgb_n[a];
        px.depth = mesh ? t : depth_n;
        px.opacity = mesh ? 1.0f : opacity_n;
        px.mask = mesh ? 1 : 0;
    } else {
        const float rest = 1.0f - opacity_n;
        for (int a = 0; a < 3; ++a) px.rgb[a] = rgb_n[a] + rest * (hit ? rgb_m[a] : background);
        px.depth = hit ? depth_n + rest * t : depth_n;
        px.opacity = hit ? 1.0f : opacity_n;
        px.mask = hit ? 1 : 0;
    }
    return px;
}

}  // namespace nerfhip

// The per-triangle texture atlas (include/nerfhip.h states the format): the per-sample, per-texel and per-ray
// routines of the kernels (texture.hip) and of their host twins, from this one source.  Index arithmetic in integers, points and
// the lookup in plain fp32 with separately rounded operations (the including file turns contraction off) and IEEE division and
// square root, normals in fp64 the same way: the device and the host give the same bits.
//
// One right-triangle patch per triangle, two patches per square block of edge B = R + 3, closed-form addresses.  Triangle t has
// the samples (i, j), i, j >= 0, i + j <= R + 1, at the barycentric weights (i / R, j / R) of vertices 1 and 2; the even triangle
// of a block puts sample (i, j) at the block's texel (i, j), the odd one at (B - 1 - i, B - 1 - j), and the texels in between
// (lx + ly = R + 2) repeat the even triangle's diagonal.  A lookup reads texels (i .. i + 1, j .. j + 1) with i, j <= R: all four
// are the triangle's own samples for a point inside it, and all four lie in the triangle's own block for any b1, b2 whatever.
#pragma once
#include "twin.h"

namespace nerfhip {

constexpr int kTexMaxRes = 64;
constexpr int kTexMaxSide = 16384;
constexpr int64_t kTexMaxSamples = (int64_t)1 << 30;    // T * n_tex per call
constexpr int kTexNearest = 0, kTexBilinear = 1;

NH_TWIN_HD int tex_samples(int R) { return (R + 2) * (R + 3) / 2; }
// sample number of the lattice point (i, j): the rows j = 0, 1, ... one after the other, row j holding i = 0 .. R + 1 - j
NH_TWIN_HD int tex_sample_number(int R, int i, int j) { return j * (R + 2) - j * (j - 1) / 2 + i; }

// (i, j) of sample number m.  Counted from the tip, row k = R + 1 - j holds k + 1 samples and starts at k (k + 1) / 2: the square
// root only guesses k, the two integer loops (at most one step each) decide.
NH_TWIN_HD void tex_sample_point(int R, int m, int& i, int& j) {
    const int back = tex_samples(R) - 1 - m;
    int k = (int)((sqrtf((float)(8 * back + 1)) - 1.0f) * 0.5f);
    while (k > 0 && k * (k + 1) / 2 > back) --k;
    while ((k + 1) * (k + 2) / 2 <= back) ++k;
    j = R + 1 - k;
    i = k - (back - k * (k + 1) / 2);
}

struct TexGrid {
    int R, B, Wa, Ha, nb;    // nb = Wa / B blocks per row
    int64_t T;
};

NH_TWIN_HD TexGrid tex_grid(int64_t T, int R, int Wa, int Ha) {
    TexGrid g;
    g.R = R, g.B = R + 3, g.Wa = Wa, g.Ha = Ha, g.nb = Wa / (R + 3), g.T = T;
    return g;
}

// rows of the atlas: B ceil(ceil(T / 2) / nb), or -1 when that exceeds kTexMaxSide
NH_TWIN_HD int tex_height(int64_t T, int R, int Wa) {
    const int64_t B = R + 3, nb = Wa / B, blocks = (T + 1) >> 1;
    const int64_t Ha = B * ((blocks + nb - 1) / nb);
    return Ha <= kTexMaxSide ? (int)Ha : -1;
}

// ---- points -------------------------------------------------------------------------------------------------------------------
// The 9 coordinates of triangle t, or false for a bad triangle (mesh_core.h's rule: an index outside [0, V) or a non-finite
// coordinate).
NH_TWIN_HD bool tex_triangle(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t t,
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

// Sample q = t n_tex + m: point = (v0 + b1 e1) + b2 e2 with b1 = (float)i / (float)R, b2 = (float)j / (float)R, e = v - v0; normal
// (when asked for) = the fp64 cross product of the fp32 edges over its length, (0, 0, 1) where that is zero or not finite.  A bad
// triangle gives (0, 0, 0) and (0, 0, 1).
NH_TWIN_HD void tex_point(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int R, int64_t q,
                          bool want_normal, float* __restrict__ point, double* __restrict__ normal) {
    const int n_tex = tex_samples(R);
    const int64_t t = q / n_tex;
    int i, j;
    tex_sample_point(R, (int)(q - t * n_tex), i, j);
    float p[9];
    const bool ok = tex_triangle(vertices, V, triangles, t, p);
    const float b1 = (float)i / (float)R, b2 = (float)j / (float)R;
    float e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = p[3 + a] - p[a];
        e2[a] = p[6 + a] - p[a];
        point[a] = ok ? (p[a] + b1 * e1[a]) + b2 * e2[a] : 0.0f;
    }
    if (!want_normal) return;
    const double x1 = e1[0], y1 = e1[1], z1 = e1[2], x2 = e2[0], y2 = e2[1], z2 = e2[2];
    const double n[3] = {y1 * z2 - z1 * y2, z1 * x2 - x1 * z2, x1 * y2 - y1 * x2};
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool unit = ok && len > 0.0 && len <= 1.7976931348623157e308;    // false for zero, NaN and +inf
#pragma unroll
    for (int a = 0; a < 3; ++a) normal[a] = unit ? n[a] / len : (a == 2 ? 1.0 : 0.0);
}

// ---- atlas --------------------------------------------------------------------------------------------------------------------
// The global sample that texel (x, y) shows, or -1 for a texel that is zero: a column behind the last whole block, a block
// without a triangle, the odd half of a block without an odd triangle.
NH_TWIN_HD int64_t tex_texel_sample(const TexGrid& g, int x, int y) {
    const int bx = x / g.B, by = y / g.B;
    if (bx >= g.nb) return -1;
    const int lx = x - bx * g.B, ly = y - by * g.B;
    int64_t t = 2 * ((int64_t)by * g.nb + bx);
    if (t >= g.T) return -1;
    const int s = lx + ly;
    int i = lx, j = ly;
    if (s == g.R + 2) {    // nobody's: the even triangle's diagonal once more
        i = lx >= 1 ? lx - 1 : 0;
        j = lx >= 1 ? ly : ly - 1;
    } else if (s > g.R + 2) {
        if (++t >= g.T) return -1;
        i = g.B - 1 - lx;
        j = g.B - 1 - ly;
    }
    return t * tex_samples(g.R) + tex_sample_number(g.R, i, j);
}

// 4 consecutive texels of a row, item = y (Wa / 4) + x / 4, as three 32-bit words (the atlas is little-endian bytes r g b).
NH_TWIN_HD void tex_atlas_words(const TexGrid& g, const uint8_t* __restrict__ colors, int64_t item, uint32_t* __restrict__ w) {
    const int per_row = g.Wa >> 2;
    const int y = (int)(item / per_row), x = 4 * (int)(item - (int64_t)y * per_row);
    uint8_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t q = tex_texel_sample(g, x + k, y);
#pragma unroll
        for (int a = 0; a < 3; ++a) b[3 * k + a] = q >= 0 ? colors[3 * q + a] : (uint8_t)0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        w[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
}

// ---- lookup -------------------------------------------------------------------------------------------------------------------
// clamp(b R, 0, R); a NaN gives 0
NH_TWIN_HD float tex_coord(float b, int R) {
    const float f = b * (float)R;
    return f > 0.0f ? (f < (float)R ? f : (float)R) : 0.0f;
}

// byte offset of the triangle's sample (i, j), 0 <= i, j <= R + 1, in the atlas
NH_TWIN_HD int64_t tex_address(const TexGrid& g, int32_t tri, int i, int j) {
    const int k = tri >> 1;
    const int by = k / g.nb, bx = k - by * g.nb;
    const int lx = (tri & 1) ? g.B - 1 - i : i, ly = (tri & 1) ? g.B - 1 - j : j;
    return 3 * ((int64_t)(by * g.B + ly) * g.Wa + (bx * g.B + lx));
}

// rgb of one ray: the triangle's texture at (b1, b2) — the nearest texel, or ((1-fu)(1-fv) c00 + fu (1-fv) c10) + ((1-fu) fv c01 +
// fu fv c11) of the four around it, c = byte / 255 — times mesh_shade_ray's ambient + (1 - ambient) |n . d| / (|n| |d|), written
// as it is there; the background by mesh_shade_ray's rules (a miss, tri >= T, a vertex index outside [0, V)).
NH_TWIN_HD void tex_shade_ray(const float* __restrict__ ray, int32_t tri, float b1, float b2, const float* __restrict__ vertices,
                              int64_t V, const int32_t* __restrict__ triangles, const TexGrid& g, const uint8_t* __restrict__ atlas,
                              int filter, float ambient, float background, float* __restrict__ rgb) {
    rgb[0] = rgb[1] = rgb[2] = background;
    if (tri < 0 || (int64_t)tri >= g.T) return;
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
        cosine = (nd < 0.0f ? -nd : nd) / len;
        cosine = cosine > 1.0f ? 1.0f : cosine;
    }
    const float shade = ambient + (1.0f - ambient) * cosine;
    const float fx = tex_coord(b1, g.R), fy = tex_coord(b2, g.R);
    if (filter == kTexNearest) {
        const uint8_t* c = atlas + tex_address(g, tri, (int)(fx + 0.5f), (int)(fy + 0.5f));
        for (int a = 0; a < 3; ++a) rgb[a] = ((float)c[a] / 255.0f) * shade;
        return;
    }
    const int i = (int)fx < g.R ? (int)fx : g.R, j = (int)fy < g.R ? (int)fy : g.R;
    const float fu = fx - (float)i, fv = fy - (float)j;
    const float w00 = (1.0f - fu) * (1.0f - fv), w10 = fu * (1.0f - fv), w01 = (1.0f - fu) * fv, w11 = fu * fv;
    const uint8_t *c00 = atlas + tex_address(g, tri, i, j), *c10 = atlas + tex_address(g, tri, i + 1, j);
    const uint8_t *c01 = atlas + tex_address(g, tri, i, j + 1), *c11 = atlas + tex_address(g, tri, i + 1, j + 1);
    for (int a = 0; a < 3; ++a) {
        const float t00 = (float)c00[a] / 255.0f, t10 = (float)c10[a] / 255.0f, t01 = (float)c01[a] / 255.0f, t11 = (float)c11[a] / 255.0f;
        rgb[a] = ((w00 * t00 + w10 * t10) + (w01 * t01 + w11 * t11)) * shade;
    }
}

}  // namespace nerfhip

// Stand-alone check of the mesh decimation's host twins (nerfhip_mesh_decimate_*_host; csrc/decimate_core.h) under a sanitizer, on a
// machine without a GPU.  No Python in the instrumented process, nothing preloaded:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/decimate_sanitize.cpp nerf_pl_amd/csrc/decimate.hip -fsanitize=address,undefined -o decimate_sanitize && ./decimate_sanitize
//
// For T = 0, 1, 5, 33, 257, 1000 it makes a seeded triangle soup (every 11th triangle bad: an index out of range or a NaN or
// infinite coordinate) with colours, and runs the passes in the order of ops._mesh_decimate with std::sort between them, for both
// placements, into heap blocks of exactly the stated sizes: a read or write outside a block is the sanitizer's to report.  The
// output is checked against the contract's invariants: the counts add up, every index is in range, no triangle is collapsed,
// every vertex is referenced, and two runs give the same bytes.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../include/nerfhip.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(next_u32() & 0xffffff) / 16777216.0f; }

template <class X>
static X* block(size_t count) {    // exactly count elements, 16-byte aligned, so the first byte past them is poisoned; null when empty
    void* p = nullptr;
    if (count && posix_memalign(&p, 16, count * sizeof(X))) abort();
    return (X*)p;
}

static float unordered(int32_t word) {    // csrc/mesh_core.h mesh_unordered
    const uint32_t e = (uint32_t)word, u = (e >> 31) ? (e & 0x7fffffffu) : ~e;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct Result {
    std::vector<float> vertices;
    std::vector<int32_t> triangles, cluster_of;
    std::vector<uint8_t> colors;
    int64_t counts[5] = {0, 0, 0, 0, 0};    // clusters, bad, collapsed, duplicate, unreferenced
};

#define CALL(expr)                                                                \
    do {                                                                          \
        const int e_ = (expr);                                                    \
        if (e_) {                                                                 \
            printf("T %lld: %s -> %d\n", (long long)T, #expr, e_);                \
            return false;                                                         \
        }                                                                         \
    } while (0)

static bool run(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* colors, float cell, int placement,
                Result& out) {
    out = Result();
    out.cluster_of.assign((size_t)V, -1);
    if (V == 0 || T == 0) return true;
    int32_t* st = block<int32_t>(8);
    CALL(nerfhip_mesh_decimate_bounds_host(vertices, V, st));
    if (st[0] == V) {
        out.counts[1] = T;
        free(st);
        return true;
    }
    float lo[3];
    int32_t res[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = unordered(st[2 + a]);
        res[a] = (int32_t)floorf((unordered(st[5 + a]) - lo[a]) / cell) + 1;
    }
    free(st);
    const size_t bv = (size_t)(V + 255) / 256, bt = (size_t)(T + 255) / 256;
    int64_t* keys = block<int64_t>((size_t)V);
    CALL(nerfhip_mesh_decimate_keys_host(vertices, V, lo, cell, res, keys));
    std::sort(keys, keys + V);
    int32_t* blk = block<int32_t>(bv);
    int64_t* off = block<int64_t>(bv);
    int32_t* cluster_of = block<int32_t>((size_t)V);
    int32_t* seg_start = block<int32_t>((size_t)V + 1);
    int64_t* totals = block<int64_t>(5);
    CALL(nerfhip_mesh_decimate_clusters_host(keys, V, blk, off, cluster_of, seg_start, totals));
    const int64_t C = totals[0];
    int64_t* entries = nullptr;
    if (placement == 1) {
        entries = block<int64_t>((size_t)T * 3);
        CALL(nerfhip_mesh_decimate_entries_host(triangles, T, V, cluster_of, entries));
        std::sort(entries, entries + 3 * T);
    }
    double* mean = block<double>((size_t)C * 3);
    float* positions = block<float>((size_t)C * 3);
    uint8_t* ccol = colors ? block<uint8_t>((size_t)C * 3) : nullptr;
    CALL(nerfhip_mesh_decimate_place_host(vertices, V, colors, triangles, T, keys, seg_start, C, entries, lo, cell, res, 1e-3, placement, mean,
                                          positions, ccol));
    uint8_t* flags = block<uint8_t>((size_t)T);
    int64_t* key_hi = block<int64_t>((size_t)T);
    int64_t* key_lo = block<int64_t>((size_t)T);
    CALL(nerfhip_mesh_decimate_tri_keys_host(triangles, T, V, cluster_of, flags, key_hi, key_lo));
    std::vector<int64_t> order((size_t)T);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(),
              [&](int64_t a, int64_t b) { return key_hi[a] != key_hi[b] ? key_hi[a] < key_hi[b] : key_lo[a] < key_lo[b]; });
    int64_t* sorted_hi = block<int64_t>((size_t)T);
    int64_t* sorted_lo = block<int64_t>((size_t)T);
    for (int64_t i = 0; i < T; ++i) {
        sorted_hi[i] = key_hi[order[(size_t)i]];
        sorted_lo[i] = key_lo[order[(size_t)i]];
    }
    CALL(nerfhip_mesh_decimate_duplicates_host(sorted_hi, sorted_lo, T, flags));
    const size_t bc = (size_t)(C + 255) / 256;
    uint8_t* ref = block<uint8_t>((size_t)C);
    int32_t* blk_t = block<int32_t>(bt);
    int64_t* off_t = block<int64_t>(bt);
    int32_t* blk_c = block<int32_t>(bc);
    int64_t* off_c = block<int64_t>(bc);
    CALL(nerfhip_mesh_decimate_mark_host(triangles, T, V, cluster_of, flags, C, ref, blk_t, off_t, blk_c, off_c, totals));
    const int64_t n_t = totals[0], n_v = totals[1];
    int32_t* vnew = block<int32_t>((size_t)C);
    // one element more than needed where the count may be zero: the entry points want a pointer, and write nothing there
    float* out_v = block<float>((size_t)(n_v ? n_v : 1) * 3);
    int32_t* out_t = block<int32_t>((size_t)(n_t ? n_t : 1) * 3);
    uint8_t* out_c = colors ? block<uint8_t>((size_t)(n_v ? n_v : 1) * 3) : nullptr;
    CALL(nerfhip_mesh_decimate_compact_host(triangles, T, V, cluster_of, flags, C, ref, off_t, off_c, positions, ccol, vnew, out_v, out_t, out_c,
                                            out.cluster_of.data()));
    out.vertices.assign(out_v, out_v + 3 * n_v);
    out.triangles.assign(out_t, out_t + 3 * n_t);
    if (colors) out.colors.assign(out_c, out_c + 3 * n_v);
    out.counts[0] = C;
    out.counts[1] = totals[2];
    out.counts[2] = totals[3];
    out.counts[3] = totals[4];
    out.counts[4] = C - n_v;
    for (void* p : {(void*)keys, (void*)blk, (void*)off, (void*)cluster_of, (void*)seg_start, (void*)totals, (void*)entries, (void*)mean,
                    (void*)positions, (void*)ccol, (void*)flags, (void*)key_hi, (void*)key_lo, (void*)sorted_hi, (void*)sorted_lo, (void*)ref,
                    (void*)blk_t, (void*)off_t, (void*)blk_c, (void*)off_c, (void*)vnew, (void*)out_v, (void*)out_t, (void*)out_c})
        free(p);
    return true;
}

int main() {
    int failures = 0;
    for (int64_t T : {0, 1, 5, 33, 257, 1000}) {
        const int64_t V = 3 * T;
        float* vertices = block<float>((size_t)V * 3);
        int32_t* triangles = block<int32_t>((size_t)T * 3);
        uint8_t* colors = block<uint8_t>((size_t)V * 3);
        int64_t n_bad = 0;
        for (int64_t t = 0; t < T; ++t) {
            float c[3] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)};
            for (int k = 0; k < 3; ++k) {
                for (int a = 0; a < 3; ++a) vertices[(3 * t + k) * 3 + a] = c[a] + uniform(-0.3f, 0.3f);
                triangles[3 * t + k] = (int32_t)(3 * t + k);
            }
            if (t % 11 == 7) {
                ++n_bad;
                if (t & 1)
                    triangles[3 * t + 1] = t & 2 ? (int32_t)V : -1;
                else
                    vertices[(3 * t + 2) * 3 + 1] = t & 2 ? NAN : INFINITY;
            }
        }
        for (int64_t i = 0; i < V * 3; ++i) colors[i] = (uint8_t)next_u32();
        for (int placement = 0; placement < 2; ++placement) {
            for (float cell : {0.5f, 0.1f}) {
                Result r, again;
                if (!run(vertices, V, triangles, T, placement ? colors : nullptr, cell, placement, r) ||
                    !run(vertices, V, triangles, T, placement ? colors : nullptr, cell, placement, again)) {
                    ++failures;
                    continue;
                }
                const int64_t n_v = (int64_t)r.vertices.size() / 3, n_t = (int64_t)r.triangles.size() / 3;
                bool ok = r.counts[1] == n_bad && r.counts[1] + r.counts[2] + r.counts[3] + n_t == T && r.counts[0] - r.counts[4] == n_v;
                std::vector<bool> used((size_t)n_v, false);
                for (int64_t t = 0; t < n_t; ++t) {
                    const int32_t* p = r.triangles.data() + 3 * t;
                    for (int k = 0; k < 3; ++k) {
                        ok = ok && p[k] >= 0 && p[k] < n_v;
                        if (p[k] >= 0 && p[k] < n_v) used[(size_t)p[k]] = true;
                    }
                    ok = ok && p[0] != p[1] && p[1] != p[2] && p[0] != p[2];
                }
                for (int64_t v = 0; v < n_v; ++v) ok = ok && used[(size_t)v];
                for (int64_t v = 0; v < V; ++v) ok = ok && r.cluster_of[(size_t)v] >= -1 && r.cluster_of[(size_t)v] < n_v;
                for (float x : r.vertices) ok = ok && isfinite(x);
                ok = ok && r.vertices.size() * sizeof(float) == again.vertices.size() * sizeof(float) &&
                     (r.vertices.empty() || !memcmp(r.vertices.data(), again.vertices.data(), r.vertices.size() * sizeof(float))) &&
                     r.triangles == again.triangles && r.colors == again.colors && r.cluster_of == again.cluster_of &&
                     (placement ? (int64_t)r.colors.size() == 3 * n_v : r.colors.empty());
                if (!ok) {
                    printf("T %lld placement %d cell %g: an invariant of the contract does not hold\n", (long long)T, placement, cell);
                    ++failures;
                }
                printf("T %4lld %s cell %.1f: %lld clusters, %lld bad, %lld collapsed, %lld duplicate, %lld unreferenced -> %lld vertices, %lld triangles\n",
                       (long long)T, placement ? "quadric" : "mean   ", cell, (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2],
                       (long long)r.counts[3], (long long)r.counts[4], (long long)n_v, (long long)n_t);
            }
        }
        free(colors);
        free(triangles);
        free(vertices);
    }
    printf(failures ? "FAILED\n" : "decimate_sanitize ok\n");
    return failures ? 1 : 0;
}

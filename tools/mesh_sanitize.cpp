// Stand-alone check of the mesh ray caster's host twins (nerfhip_mesh_bvh_*_host, nerfhip_mesh_cast_host, nerfhip_mesh_shade_host,
// nerfhip_mixed_compose_host; csrc/mesh_core.h) under a sanitizer, on a machine without a GPU.  No Python in the instrumented
// process, nothing preloaded:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/mesh_sanitize.cpp nerf_pl_amd/csrc/meshcast.hip -fsanitize=address,undefined -o mesh_sanitize && ./mesh_sanitize
//
// For T = 0, 1, 5, 33, 257 it makes a seeded triangle soup (every 11th triangle bad: an index out of range or a NaN coordinate),
// builds the hierarchy into heap blocks of exactly the stated sizes — T keys, 8 state words, T * 12 floats, nerfhip_mesh_bvh_nodes(T)
// * 6 floats — and casts rays of every kind (through the soup, beside it, from inside, axis-parallel with zeros of both signs,
// non-finite, zero direction, short windows) with the hierarchy and without it: the two must agree bit for bit, no bad triangle
// may be returned, and a read or write outside a block is the sanitizer's to report.  The hits are then shaded and composed.
// The cast runs again with t, b1 and b2 null (each alone and all three) and the compose with a null mask: the outputs that are
// supplied must keep the bits of the full call.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
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

int main() {
    int failures = 0;
    for (int64_t T : {0, 1, 5, 33, 257}) {
        const int64_t V = 3 * T;
        float* vertices = block<float>((size_t)V * 3);
        int32_t* triangles = block<int32_t>((size_t)T * 3);
        std::vector<bool> bad((size_t)T, false);
        for (int64_t t = 0; t < T; ++t) {
            float c[3] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)};
            for (int k = 0; k < 3; ++k) {
                for (int a = 0; a < 3; ++a) vertices[(3 * t + k) * 3 + a] = c[a] + uniform(-0.3f, 0.3f);
                triangles[3 * t + k] = (int32_t)(3 * t + k);
            }
            if (t % 11 == 7) {
                bad[(size_t)t] = true;
                if (t & 1)
                    triangles[3 * t + 1] = t & 2 ? (int32_t)V : -1;
                else
                    vertices[(3 * t + 2) * 3 + 1] = t & 2 ? NAN : INFINITY;
            }
        }
        int64_t* keys = block<int64_t>((size_t)T);
        int32_t* st = block<int32_t>(8);
        int e = nerfhip_mesh_bvh_keys_host(vertices, V, triangles, T, keys, st);
        if (e) {
            printf("T %lld: keys error %d\n", (long long)T, e);
            ++failures;
        }
        int64_t n_bad = 0;
        for (int64_t t = 0; t < T; ++t) n_bad += bad[(size_t)t];
        if (st[0] != n_bad) {
            printf("T %lld: %d bad triangles counted, %lld made\n", (long long)T, st[0], (long long)n_bad);
            ++failures;
        }
        std::sort(keys, keys + T);
        const size_t nodes = nerfhip_mesh_bvh_nodes(T);
        float* tris = block<float>((size_t)T * 12);
        float* boxes = block<float>(nodes * 6);
        e = nerfhip_mesh_bvh_boxes_host(vertices, V, triangles, T, keys, tris, boxes);
        if (e) {
            printf("T %lld: boxes error %d\n", (long long)T, e);
            ++failures;
        }

        const int n = 900;
        float* rays = block<float>((size_t)n * 8);
        for (int i = 0; i < n; ++i) {
            float* r = rays + 8 * i;
            for (int a = 0; a < 3; ++a) r[a] = uniform(-4.0f, 4.0f);
            for (int a = 0; a < 3; ++a) r[3 + a] = (uniform(-1.0f, 1.0f) - r[a]) * uniform(0.01f, 30.0f);
            r[6] = 0.0f;
            r[7] = 1e6f;
            if (i % 7 == 1)                                       // from inside
                for (int a = 0; a < 3; ++a) r[a] = uniform(-0.5f, 0.5f);
            if (i % 7 == 2) {                                     // axis-parallel, zeros of both signs
                r[3 + (i % 3)] = i & 8 ? 0.0f : -0.0f;
                r[3 + ((i + 1) % 3)] = i & 16 ? 0.0f : -0.0f;
            }
            if (i % 7 == 3) {                                     // a short window
                r[6] = uniform(0.0f, 0.2f);
                r[7] = r[6] + uniform(0.0f, 0.2f);
            }
            if (i % 7 == 4)                                       // beside the soup
                for (int a = 0; a < 3; ++a) r[3 + a] = r[a];
            if (i % 97 == 5) r[i % 8] = i & 1 ? NAN : INFINITY;
            if (i % 97 == 6) r[3] = r[4] = r[5] = i & 1 ? 0.0f : -0.0f;
        }
        int32_t* tri[2];
        float* out[2][3];
        for (int s = 0; s < 2; ++s) {
            tri[s] = block<int32_t>(n);
            for (int k = 0; k < 3; ++k) out[s][k] = block<float>(n);
            e = nerfhip_mesh_cast_host(rays, n, tris, s ? nullptr : boxes, T, s, tri[s], out[s][0], out[s][1], out[s][2]);
            if (e) {
                printf("T %lld brute %d: cast error %d\n", (long long)T, s, e);
                ++failures;
            }
        }
        bool same = !memcmp(tri[0], tri[1], sizeof(int32_t) * n);
        for (int k = 0; k < 3; ++k) same = same && !memcmp(out[0][k], out[1][k], sizeof(float) * n);
        if (!same) {
            printf("T %lld: the hierarchy changed the result\n", (long long)T);
            ++failures;
        }
        // t, b1 and b2 null, each alone and all three: what is supplied keeps the bits of the full call
        for (int skip = 0; skip < 4; ++skip) {
            float* o[3];
            for (int k = 0; k < 3; ++k) {
                o[k] = (k == skip || skip == 3) ? nullptr : out[1][k];
                if (o[k]) memset(o[k], 0xa5, sizeof(float) * n);
            }
            if (n) memset(tri[1], 0xa5, sizeof(int32_t) * n);
            e = nerfhip_mesh_cast_host(rays, n, tris, boxes, T, 0, tri[1], o[0], o[1], o[2]);
            bool kept = !e && !memcmp(tri[1], tri[0], sizeof(int32_t) * n);
            for (int k = 0; k < 3; ++k) kept = kept && (!o[k] || !memcmp(o[k], out[0][k], sizeof(float) * n));
            if (!kept) {
                printf("T %lld: cast with null outputs (%d): error %d or a supplied output differs\n", (long long)T, skip, e);
                ++failures;
            }
        }
        int hits = 0;
        for (int i = 0; i < n; ++i) {
            const int32_t h = tri[0][i];
            if (h < -1 || h >= T || (h >= 0 && bad[(size_t)h])) {
                printf("T %lld ray %d: triangle %d\n", (long long)T, i, h);
                ++failures;
            }
            hits += h >= 0;
        }

        // shade and compose what was hit
        uint8_t* colors = block<uint8_t>((size_t)V * 3);
        for (int64_t i = 0; i < V * 3; ++i) colors[i] = (uint8_t)next_u32();
        float* rgb_m = block<float>((size_t)n * 3);
        float* rgb_n = block<float>((size_t)n * 3);
        float* depth_n = block<float>(n);
        float* opacity_n = block<float>(n);
        float* rgb = block<float>((size_t)n * 3);
        float* depth = block<float>(n);
        float* opacity = block<float>(n);
        uint8_t* mask = block<uint8_t>(n);
        for (int i = 0; i < n; ++i) {
            for (int a = 0; a < 3; ++a) rgb_n[3 * i + a] = uniform(0, 1);
            opacity_n[i] = i % 5 ? uniform(0, 1) : 0.0f;
            depth_n[i] = opacity_n[i] * uniform(0, 8);
        }
        for (int pass = 0; pass < 2; ++pass) {
            e = nerfhip_mesh_shade_host(rays, n, tri[0], out[0][1], out[0][2], vertices, V, triangles, T, pass ? colors : nullptr,
                                        pass ? 0.25f : 1.0f, pass ? 1.0f : 0.0f, rgb_m);
            if (!e) e = nerfhip_mixed_compose_host(pass, n, rgb_n, depth_n, opacity_n, tri[0], out[0][0], rgb_m, 0.5f, (float)pass, rgb,
                                                   depth, opacity, mask);
            if (e) {
                printf("T %lld pass %d: shade / compose error %d\n", (long long)T, pass, e);
                ++failures;
            }
            // the mask null: rgb, depth and opacity keep the bits of the full call
            float* again[3] = {block<float>((size_t)n * 3), block<float>(n), block<float>(n)};
            e = nerfhip_mixed_compose_host(pass, n, rgb_n, depth_n, opacity_n, tri[0], out[0][0], rgb_m, 0.5f, (float)pass, again[0], again[1],
                                           again[2], nullptr);
            if (e || memcmp(again[0], rgb, sizeof(float) * 3 * n) || memcmp(again[1], depth, sizeof(float) * n) ||
                memcmp(again[2], opacity, sizeof(float) * n)) {
                printf("T %lld pass %d: compose without a mask: error %d or an output differs\n", (long long)T, pass, e);
                ++failures;
            }
            for (float* p : again) free(p);
        }
        printf("T %3lld: %zu boxes, %lld bad, %d of %d rays hit\n", (long long)T, nodes, (long long)n_bad, hits, n);
        for (int s = 0; s < 2; ++s) {
            free(tri[s]);
            for (int k = 0; k < 3; ++k) free(out[s][k]);
        }
        for (void* p : {(void*)colors, (void*)rgb_m, (void*)rgb_n, (void*)depth_n, (void*)opacity_n, (void*)rgb, (void*)depth, (void*)opacity,
                        (void*)mask, (void*)rays, (void*)boxes, (void*)tris, (void*)st, (void*)keys, (void*)triangles, (void*)vertices})
            free(p);
    }
    printf(failures ? "FAILED\n" : "mesh_sanitize ok\n");
    return failures ? 1 : 0;
}

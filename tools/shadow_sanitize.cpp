// Stand-alone check of the shadow units' host twins (nerfhip_mesh_occluded_host, nerfhip_shadow_rays_host,
// nerfhip_light_compose_host; csrc/shadow_core.h) under a sanitizer, on a machine without a GPU.  No Python in the instrumented
// process, nothing preloaded:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/shadow_sanitize.cpp nerf_pl_amd/csrc/shadow.hip nerf_pl_amd/csrc/meshcast.hip -fsanitize=address,undefined \
//       -o shadow_sanitize && ./shadow_sanitize
//
// For T = 0, 1, 5, 33, 257 it makes a seeded triangle soup (every 11th triangle bad) and its hierarchy, and for n = 0, 1, 5, 33,
// 257 and K = 1, 4 seeded primary rows with a surface distance each (no surface, NaN, zero and negative among them, and non-finite
// rows), and runs the three twins into heap blocks of exactly the stated sizes — n K rows of 8 floats, n cosines, n K hits, n
// colours — with both kinds of light, with and without a radius, a mesh layer, a cosine, a transmittance and a visibility: a read
// or write outside a block is the sanitizer's to report.  Checked on the way: the hierarchy and brute force agree on every row
// and agree with nerfhip_mesh_cast_host's tri >= 0; a zero row is never occluded; with radius 0 the K rows of a pixel are one
// row; the null-argument calls keep the bits of what they still write; ambient 1 and strength 0 return rgb.
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

static int failures = 0;
static void expect(bool ok, const char* what, long long T, long long n, int K) {
    if (ok) return;
    printf("T %lld n %lld K %d: %s\n", T, n, K, what);
    ++failures;
}

int main() {
    for (int64_t T : {0, 1, 5, 33, 257}) {
        const int64_t V = 3 * T;
        float* vertices = block<float>((size_t)V * 3);
        int32_t* triangles = block<int32_t>((size_t)T * 3);
        for (int64_t t = 0; t < T; ++t) {
            float c[3] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)};
            for (int k = 0; k < 3; ++k) {
                for (int a = 0; a < 3; ++a) vertices[(3 * t + k) * 3 + a] = c[a] + uniform(-0.3f, 0.3f);
                triangles[3 * t + k] = (int32_t)(3 * t + k);
            }
            if (t % 11 == 7) {
                if (t & 1)
                    triangles[3 * t + 1] = t & 2 ? (int32_t)V : -1;
                else
                    vertices[(3 * t + 2) * 3 + 1] = t & 2 ? NAN : INFINITY;
            }
        }
        int64_t* keys = block<int64_t>((size_t)T);
        int32_t* st = block<int32_t>(8);
        expect(!nerfhip_mesh_bvh_keys_host(vertices, V, triangles, T, keys, st), "keys", T, 0, 0);
        std::sort(keys, keys + T);
        const size_t nodes = nerfhip_mesh_bvh_nodes(T);
        float* tris = block<float>((size_t)T * 12);
        float* boxes = block<float>(nodes * 6);
        expect(!nerfhip_mesh_bvh_boxes_host(vertices, V, triangles, T, keys, tris, boxes), "boxes", T, 0, 0);

        long long rows_total = 0, rows_hit = 0;
        for (int64_t n : {0, 1, 5, 33, 257}) {
            float* rays = block<float>((size_t)n * 8);
            float* s = block<float>((size_t)n);
            int32_t* tri = block<int32_t>((size_t)n);
            for (int64_t i = 0; i < n; ++i) {
                float* r = rays + 8 * i;
                for (int a = 0; a < 3; ++a) r[a] = uniform(-4.0f, 4.0f);
                for (int a = 0; a < 3; ++a) r[3 + a] = (uniform(-1.0f, 1.0f) - r[a]) * uniform(0.2f, 3.0f);
                r[6] = 0.0f;
                r[7] = 1e6f;
                s[i] = uniform(0.1f, 1.2f);
                const float special[5] = {INFINITY, NAN, 0.0f, -1.0f, -INFINITY};
                if (i % 9 == 4) s[i] = special[(i / 9) % 5];
                if (i % 23 == 11) r[i % 8] = i & 1 ? NAN : INFINITY;
                if (i % 23 == 12) r[3] = r[4] = r[5] = i & 1 ? 0.0f : -0.0f;
                tri[i] = i % 3 == 0 ? -1 : (int32_t)(next_u32() % (uint32_t)(T + 2)) - (i % 7 == 0);    // up to T + 1: out of range too
            }
            for (int K : {1, 4}) {
                const size_t R = (size_t)n * K;
                float* rows = block<float>(R * 8);
                float* rows2 = block<float>(R * 8);
                float* cosine = block<float>((size_t)n);
                float* cosine2 = block<float>((size_t)n);
                uint8_t* hit = block<uint8_t>(R);
                uint8_t* hit2 = block<uint8_t>(R);
                int32_t* cast = block<int32_t>(R);
                uint8_t* mask = block<uint8_t>((size_t)n);
                float* rgb = block<float>((size_t)n * 3);
                float* trans = block<float>(R);
                float* out = block<float>((size_t)n * 3);
                float* out2 = block<float>((size_t)n * 3);
                float* vis = block<float>((size_t)n);
                for (int64_t i = 0; i < n; ++i) {
                    mask[i] = (uint8_t)(tri[i] >= 0 ? (i & 1 ? 1 : 255) : 0);
                    for (int a = 0; a < 3; ++a) rgb[3 * i + a] = uniform(0, 1);
                }
                for (size_t j = 0; j < R; ++j) trans[j] = uniform(0, 1);
                for (int kind = 0; kind < 2; ++kind)
                    for (float radius : {0.0f, 0.25f})
                        for (int rotate = 0; rotate < 2; ++rotate) {
                            const float l[3] = {kind ? 0.4f : 1.0f, kind ? -0.3f : 0.0f, kind ? 1.7f : 1.0f};
                            int e = nerfhip_shadow_rays_host(rays, s, n, tri, vertices, V, triangles, T, kind, l[0], l[1], l[2], 1e-3f, 50.0f, K,
                                                             radius, rotate, rows, cosine);
                            expect(!e, "shadow_rays", T, n, K);
                            // no mesh layer; no cosine: the rows keep their bits, the cosine is 1 / keeps its bits
                            e = nerfhip_shadow_rays_host(rays, s, n, nullptr, nullptr, 0, nullptr, 0, kind, l[0], l[1], l[2], 1e-3f, 50.0f, K, radius,
                                                         rotate, rows2, cosine2);
                            bool same = !e && (!R || !memcmp(rows, rows2, R * 32));
                            for (int64_t i = 0; i < n; ++i) same = same && cosine2[i] == 1.0f;
                            expect(same, "shadow_rays without a mesh layer", T, n, K);
                            if (R) memset(rows2, 0xa5, R * 32);
                            e = nerfhip_shadow_rays_host(rays, s, n, tri, vertices, V, triangles, T, kind, l[0], l[1], l[2], 1e-3f, 50.0f, K, radius,
                                                         rotate, rows2, nullptr);
                            expect(!e && (!R || !memcmp(rows, rows2, R * 32)), "shadow_rays without a cosine", T, n, K);
                            if (radius == 0.0f)
                                for (int64_t i = 0; i < n; ++i)
                                    for (int k = 1; k < K; ++k)
                                        expect(!memcmp(rows + 8 * (i * K), rows + 8 * (i * K + k), 32), "radius 0: the rows of a pixel differ", T, n, K);
                            for (int64_t i = 0; i < n; ++i) expect(cosine[i] >= 0.0f && cosine[i] <= 1.0f, "cosine outside [0, 1]", T, n, K);

                            e = nerfhip_mesh_occluded_host(rows, (int64_t)R, tris, boxes, T, 0, hit);
                            expect(!e, "mesh_occluded", T, n, K);
                            e = nerfhip_mesh_occluded_host(rows, (int64_t)R, tris, nullptr, T, 1, hit2);
                            expect(!e && (!R || !memcmp(hit, hit2, R)), "the hierarchy changed the answer", T, n, K);
                            e = nerfhip_mesh_cast_host(rows, (int64_t)R, tris, boxes, T, 0, cast, nullptr, nullptr, nullptr);
                            expect(!e, "mesh_cast", T, n, K);
                            for (size_t j = 0; j < R; ++j) {
                                expect(hit[j] == (cast[j] >= 0 ? 1 : 0), "occluded differs from the cast", T, n, K);
                                bool zero = true;
                                for (int q = 0; q < 8; ++q) zero = zero && rows[8 * j + q] == 0.0f;
                                expect(!(zero && hit[j]), "a zero row is occluded", T, n, K);
                                rows_hit += hit[j];
                            }
                            rows_total += (long long)R;

                            e = nerfhip_light_compose_host(n, rgb, mask, cosine, hit, trans, K, 0.3f, 0.7f, out, vis);
                            expect(!e, "light_compose", T, n, K);
                            e = nerfhip_light_compose_host(n, rgb, mask, cosine, hit, trans, K, 0.3f, 0.7f, out2, nullptr);
                            expect(!e && (!n || !memcmp(out, out2, (size_t)n * 12)), "light_compose without a visibility", T, n, K);
                            e = nerfhip_light_compose_host(n, rgb, mask, cosine, hit, nullptr, K, 0.3f, 0.7f, out2, vis);
                            expect(!e, "light_compose without a transmittance", T, n, K);
                            for (int64_t i = 0; i < n; ++i) expect(vis[i] >= 0.0f && vis[i] <= 1.0f, "visibility outside [0, 1]", T, n, K);
                            e = nerfhip_light_compose_host(n, rgb, mask, cosine, hit, trans, K, 1.0f, 0.0f, out2, nullptr);
                            expect(!e && (!n || !memcmp(rgb, out2, (size_t)n * 12)), "ambient 1, strength 0 changed rgb", T, n, K);
                        }
                for (void* p : {(void*)rows, (void*)rows2, (void*)cosine, (void*)cosine2, (void*)hit, (void*)hit2, (void*)cast, (void*)mask,
                                (void*)rgb, (void*)trans, (void*)out, (void*)out2, (void*)vis})
                    free(p);
            }
            free(rays);
            free(s);
            free(tri);
        }
        printf("T %3lld: %zu boxes, %lld of %lld shadow rows occluded\n", (long long)T, nodes, rows_hit, rows_total);
        for (void* p : {(void*)boxes, (void*)tris, (void*)st, (void*)keys, (void*)triangles, (void*)vertices}) free(p);
    }
    printf(failures ? "FAILED\n" : "shadow_sanitize ok\n");
    return failures ? 1 : 0;
}

// Stand-alone check of the texture atlas' host twins (nerfhip_mesh_tex_points_host, nerfhip_mesh_tex_atlas_host,
// nerfhip_mesh_shade_tex_host; csrc/texture_core.h) under a sanitizer, on a machine without a GPU.  No Python in the instrumented
// process, nothing preloaded:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/texture_sanitize.cpp nerf_pl_amd/csrc/texture.hip -fsanitize=address,undefined -o texture_sanitize && ./texture_sanitize
//
// For R = 1, 3, 8 and T = 0 .. 200 it makes a seeded triangle soup (every 11th triangle bad: an index out of range or a non-finite
// coordinate), computes the sample points with and without normals into heap blocks of exactly the stated sizes — K * 3 floats,
// K * 3 doubles, K * 3 colour bytes, Ha * Wa * 3 atlas bytes — fills the atlas at a narrow, a ragged and the square width, and
// shades rows of every kind with both filters: seeded hits of every triangle, and the crafted rows no cast produces (tri = -1,
// tri >= T, a bad triangle, b1 and b2 in {0, 1}, both 1, negative, huge, NaN, infinite).  A read or write outside a block is the
// sanitizer's to report; the program itself checks that a bad triangle's samples are (0, 0, 0) / (0, 0, 1), that the points do
// not depend on the normals being asked for, that no sentinel byte is left in the atlas, and that every shaded value is finite
// and within [0, 1].
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    long long calls = 0;
    for (int R : {1, 3, 8}) {
        const int n_tex = nerfhip_mesh_tex_samples(R), B = R + 3;
        if (n_tex != (R + 2) * (R + 3) / 2) {
            printf("R %d: %d samples\n", R, n_tex);
            ++failures;
        }
        for (int64_t T = 0; T <= 200; ++T) {
            const int64_t V = 3 * T, K = T * n_tex;
            float* vertices = block<float>((size_t)V * 3);
            int32_t* triangles = block<int32_t>((size_t)T * 3);
            std::vector<bool> bad((size_t)T, false);
            for (int64_t t = 0; t < T; ++t) {
                const float c[3] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)};
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
            float* points = block<float>((size_t)K * 3);
            float* points_only = block<float>((size_t)K * 3);
            double* normals = block<double>((size_t)K * 3);
            int e = nerfhip_mesh_tex_points_host(vertices, V, triangles, T, R, points, normals);
            if (!e) e = nerfhip_mesh_tex_points_host(vertices, V, triangles, T, R, points_only, nullptr);
            calls += 2;
            if (e || (K && memcmp(points, points_only, sizeof(float) * 3 * (size_t)K))) {
                printf("R %d T %lld: points error %d, or the points depend on the normals\n", R, (long long)T, e);
                ++failures;
            }
            for (int64_t q = 0; q < K; ++q) {
                const double* n = normals + 3 * q;
                const float* p = points + 3 * q;
                const double len = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
                const bool unit = fabs(len - 1.0) < 1e-12, finite = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
                const bool blank = p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f && n[0] == 0.0 && n[1] == 0.0 && n[2] == 1.0;
                if (!unit || !finite || (bad[(size_t)(q / n_tex)] && !blank)) {
                    printf("R %d T %lld sample %lld: point %g %g %g normal %g %g %g\n", R, (long long)T, (long long)q, p[0], p[1], p[2],
                           n[0], n[1], n[2]);
                    ++failures;
                    break;
                }
            }
            uint8_t* colors = block<uint8_t>((size_t)K * 3);
            for (int64_t i = 0; i < K * 3; ++i) colors[i] = (uint8_t)(1 + next_u32() % 200);    // never the sentinel, never 0

            const int64_t blocks = (T + 1) / 2;
            int nb = 1;
            while ((int64_t)nb * nb < blocks) ++nb;
            while ((nb * B) % 4) ++nb;
            const int widths[3] = {(B + 3) / 4 * 4, (3 * B + 4) / 4 * 4, nb * B};    // one block per row; ragged; about square
            for (int Wa : widths) {
                const int Ha = nerfhip_mesh_tex_height(T, R, Wa);
                if ((Ha == 0) != (T == 0) || Ha % B) {
                    printf("R %d T %lld Wa %d: height %d\n", R, (long long)T, Wa, Ha);
                    ++failures;
                    continue;
                }
                const size_t bytes = (size_t)Ha * Wa * 3;
                uint8_t* atlas = block<uint8_t>(bytes);
                if (bytes) memset(atlas, 0xEE, bytes);
                e = nerfhip_mesh_tex_atlas_host(colors, T, R, Wa, Ha, atlas);
                ++calls;
                size_t left = 0;
                for (size_t i = 0; i < bytes; ++i) left += atlas[i] == 0xEE;
                if (e || left) {
                    printf("R %d T %lld Wa %d: atlas error %d, %zu sentinel bytes left\n", R, (long long)T, Wa, e, left);
                    ++failures;
                }
                // rows: 4 seeded hits of every triangle, then the crafted ones for a handful of triangle numbers
                const float crafted[14][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {-0.25f, 0.5f}, {0.5f, -0.25f}, {-3, -3}, {7, 9}, {0.5f, 0.5f},
                                              {1e30f, -1e30f}, {NAN, 0.5f}, {0.25f, NAN}, {INFINITY, -INFINITY}, {0.999999f, 0.000001f}};
                const int64_t numbers[10] = {-1, -7, T, T + 5, 0x7fffffff, 0, 1, 7, T - 2, T - 1};
                const int64_t n = 4 * T + 14 * 10;
                float* rays = block<float>((size_t)n * 8);
                int32_t* tri = block<int32_t>((size_t)n);
                float* b1 = block<float>((size_t)n);
                float* b2 = block<float>((size_t)n);
                float* rgb = block<float>((size_t)n * 3);
                for (int64_t i = 0; i < n; ++i) {
                    for (int a = 0; a < 8; ++a) rays[8 * i + a] = uniform(-1, 1);
                    if (i < 4 * T) {
                        tri[i] = (int32_t)(i / 4);
                        b1[i] = uniform(0, 1);
                        b2[i] = uniform(0, 1 - b1[i]);
                    } else {
                        const int64_t r = i - 4 * T;
                        tri[i] = (int32_t)numbers[r / 14];
                        b1[i] = crafted[r % 14][0];
                        b2[i] = crafted[r % 14][1];
                    }
                }
                for (int filter = 0; filter < 2; ++filter) {
                    const float ambient = filter ? 0.25f : 1.0f, background = 0.5f;
                    e = nerfhip_mesh_shade_tex_host(rays, n, tri, b1, b2, vertices, V, triangles, T, atlas, R, Wa, Ha, filter, ambient,
                                                    background, rgb);
                    ++calls;
                    if (e) {
                        printf("R %d T %lld Wa %d filter %d: shade error %d\n", R, (long long)T, Wa, filter, e);
                        ++failures;
                        continue;
                    }
                    for (int64_t i = 0; i < n; ++i) {
                        const int64_t h = tri[i];
                        const bool back = h < 0 || h >= T || (bad[(size_t)h] && (h & 1));    // the odd bad ones name a vertex outside
                        bool ok = true;
                        for (int a = 0; a < 3; ++a) {
                            const float c = rgb[3 * i + a];
                            ok = ok && (back ? c == background : (c >= 0.0f && c <= 1.0f));
                        }
                        if (!ok) {
                            printf("R %d T %lld Wa %d filter %d row %lld (tri %lld): %g %g %g\n", R, (long long)T, Wa, filter, (long long)i,
                                   (long long)h, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
                            ++failures;
                            break;
                        }
                    }
                }
                for (void* p : {(void*)rgb, (void*)b2, (void*)b1, (void*)tri, (void*)rays, (void*)atlas}) free(p);
            }
            for (void* p : {(void*)colors, (void*)normals, (void*)points_only, (void*)points, (void*)triangles, (void*)vertices}) free(p);
        }
        printf("R %d: T = 0 .. 200 done\n", R);
    }
    printf("%lld calls\n", calls);
    printf(failures ? "FAILED\n" : "texture_sanitize ok\n");
    return failures ? 1 : 0;
}

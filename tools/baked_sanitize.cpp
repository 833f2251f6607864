// Stand-alone check of the baked-volume march's host twin (nerfhip_baked_render_host, csrc/baked_core.h) under a sanitizer, on a
// machine without a GPU.  No Python in the instrumented process, nothing preloaded:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/baked_sanitize.cpp nerf_pl_amd/csrc/baked.hip -fsanitize=address,undefined -o baked_sanitize && ./baked_sanitize
//
// For N = 2, 9, 17, 33 it makes a seeded lattice (60 % empty), bricks it by the layout of include/nerfhip.h into a heap block of
// exactly nerfhip_baked_bytes(N) bytes, forms the cell-brick bitfield by its rule into exactly ceil(MB^3 / 32) words, and marches
// rays of every kind (through the box, beside it, inside it, axis-parallel with zeros of both signs, non-finite) at step 1/16, 0.5
// and 8 with the bitfield and without it: the two must agree bit for bit, and a read outside a block is the sanitizer's to report.
// A last pass hands null to rgb, depth and opacity in turn: the outputs that are supplied must keep the bits of the full call.
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

int main() {
    const float ranges[6] = {-1.0f, 1.5f, -0.75f, 1.0f, 0.25f, 2.5f};
    int failures = 0;
    for (int N : {2, 9, 17, 33}) {
        const int NB = (N + 7) / 8, MB = (N - 1 + 7) / 8;
        const size_t bytes = nerfhip_baked_bytes(N);
        if (bytes != (size_t)NB * NB * NB * 2048) return 2;
        uint8_t* data = (uint8_t*)aligned_alloc(16, bytes);
        memset(data, 0, bytes);
        std::vector<uint8_t> alpha((size_t)N * N * N, 0);
        for (int iy = 0; iy < N; ++iy)
            for (int ix = 0; ix < N; ++ix)
                for (int iz = 0; iz < N; ++iz) {
                    if (next_u32() % 10 < 6) continue;
                    const size_t brick = ((size_t)(iy >> 3) * NB + (ix >> 3)) * NB + (iz >> 3);
                    uint8_t* p = data + brick * 2048 + (size_t)((((iy & 7) * 8) + (ix & 7)) * 8 + (iz & 7)) * 4;
                    for (int c = 0; c < 4; ++c) p[c] = (uint8_t)(1 + next_u32() % 255);
                    alpha[((size_t)iy * N + ix) * N + iz] = p[3];
                }
        const size_t n_words = ((size_t)MB * MB * MB + 31) / 32;
        int32_t* words = (int32_t*)calloc(n_words, sizeof(int32_t));
        for (int by = 0; by < MB; ++by)
            for (int bx = 0; bx < MB; ++bx)
                for (int bz = 0; bz < MB; ++bz) {
                    bool occupied = false;
                    for (int iy = 8 * by; iy <= 8 * by + 8 && iy < N; ++iy)
                        for (int ix = 8 * bx; ix <= 8 * bx + 8 && ix < N; ++ix)
                            for (int iz = 8 * bz; iz <= 8 * bz + 8 && iz < N; ++iz) occupied = occupied || alpha[((size_t)iy * N + ix) * N + iz];
                    const uint32_t c = (uint32_t)((by * MB + bx) * MB + bz);
                    if (occupied) words[c >> 5] = (int32_t)((uint32_t)words[c >> 5] | (1u << (c & 31)));
                }
        const int n = 600;
        float* rays = (float*)aligned_alloc(16, sizeof(float) * 8 * n);
        for (int i = 0; i < n; ++i) {
            float* r = rays + 8 * i;
            const float mid[3] = {0.25f, 0.125f, 1.375f};
            for (int a = 0; a < 3; ++a) r[a] = mid[a] + uniform(-4.0f, 4.0f);
            for (int a = 0; a < 3; ++a) r[3 + a] = (mid[a] + uniform(-1.0f, 1.0f) - r[a]) * uniform(0.2f, 1.5f);
            r[6] = 0.0f;
            r[7] = 20.0f;
            if (i % 7 == 1)                                       // inside the box
                for (int a = 0; a < 3; ++a) r[a] = mid[a] + uniform(-0.5f, 0.5f);
            if (i % 7 == 2) {                                     // axis-parallel, zeros of both signs
                r[3 + (i % 3)] = i & 8 ? 0.0f : -0.0f;
                r[3 + ((i + 1) % 3)] = i & 16 ? 0.0f : -0.0f;
            }
            if (i % 7 == 3) r[7] = uniform(0.5f, 4.0f);           // far inside
            if (i % 97 == 5) r[i % 8] = i & 1 ? NAN : INFINITY;
            if (i % 97 == 6) r[3] = r[4] = r[5] = 0.0f;
        }
        float* out[2][3];
        for (int s = 0; s < 2; ++s) {
            out[s][0] = (float*)malloc(sizeof(float) * 3 * n);
            out[s][1] = (float*)malloc(sizeof(float) * n);
            out[s][2] = (float*)malloc(sizeof(float) * n);
        }
        const float cell = 2.5f / (float)N;
        for (float step : {0.0625f, 0.5f, 8.0f})
            for (int white = 0; white < 2; ++white)
                for (float t_stop : {0.0f, 0.01f}) {
                    for (int s = 0; s < 2; ++s) {
                        const int e = nerfhip_baked_render_host(rays, n, data, s ? words : nullptr, N, ranges, cell, step, t_stop, white,
                                                                out[s][0], out[s][1], out[s][2]);
                        if (e) {
                            printf("N %d step %g: error %d\n", N, step, e);
                            ++failures;
                        }
                    }
                    if (memcmp(out[0][0], out[1][0], sizeof(float) * 3 * n) || memcmp(out[0][1], out[1][1], sizeof(float) * n) ||
                        memcmp(out[0][2], out[1][2], sizeof(float) * n)) {
                        printf("N %d step %g white %d t_stop %g: the bitfield changed the result\n", N, step, white, t_stop);
                        ++failures;
                    }
                }
        // every optional output null in turn: the outputs that are supplied keep the bits of the full call (out[1], the last one)
        const size_t size[3] = {sizeof(float) * 3 * n, sizeof(float) * n, sizeof(float) * n};
        for (int skip = 0; skip < 3; ++skip) {
            float* o[3];
            for (int k = 0; k < 3; ++k) {
                o[k] = k == skip ? nullptr : out[0][k];
                if (o[k]) memset(o[k], 0xa5, size[k]);
            }
            const int e = nerfhip_baked_render_host(rays, n, data, words, N, ranges, cell, 8.0f, 0.01f, 1, o[0], o[1], o[2]);
            for (int k = 0; k < 3; ++k)
                if (e || (o[k] && memcmp(o[k], out[1][k], size[k]))) {
                    printf("N %d: output %d null: error %d or output %d differs from the full call\n", N, skip, e, k);
                    ++failures;
                }
        }
        double sum = 0;
        for (int i = 0; i < n; ++i) sum += out[1][2][i];
        printf("N %2d: %d rays, mean opacity %.4f\n", N, n, sum / n);
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) free(out[s][k]);
        free(rays);
        free(words);
        free(data);
    }
    printf(failures ? "FAILED\n" : "baked_sanitize ok\n");
    return failures ? 1 : 0;
}

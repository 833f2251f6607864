// How exactly does v_mfma_scale_f32_32x32x64_f8f6f4 (A = e5m2, B = e4m3, as mlp_bwd_dw_f8_kernel issues it) add its 64 products?
//   hipcc --offload-arch=gfx950 -O2 tools/probes/probe_fp8_accum.hip -o tools/probes/bin/probe_fp8_accum && tools/probes/bin/probe_fp8_accum
// Random in-range operands and block scales, one MFMA per trial, against the fp64 sum of the exact products (host).  Prints, per
// operand distribution, the worst |D - ref| in units of 2^-24 * (sum |products| + |C|) and of 2^-24 * (max |product|): the first
// is what tests/test_gpu_f8_exact.py puts in the place of the 64 fp32 roundings of a block.
// Operand layout (tools/probes/probe_fp8.hip): lane (row m = l & 31, H = l >> 5) holds 32 bytes, bytes 16 blk + b = K index
// 32 blk + 16 H + b; the scale operand's byte 0 of lanes 0..31 scales block 0 of row m, of lanes 32..63 block 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__global__ void k_mfma(const uint32_t* a_img, const uint32_t* b_img, const int* sa, const int* sb, const float* c_in, float* d, int trials) {
    const int lane = threadIdx.x;
    for (int t = blockIdx.x; t < trials; t += gridDim.x) {
        i32x8 a, b;
        f32x16 c;
        for (int i = 0; i < 8; ++i) {
            a[i] = (int)a_img[((size_t)t * 64 + lane) * 8 + i];
            b[i] = (int)b_img[((size_t)t * 64 + lane) * 8 + i];
        }
        for (int r = 0; r < 16; ++r) c[r] = c_in[((size_t)t * 64 + lane) * 16 + r];
        c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 1, 0, 0, sa[t * 64 + lane], 0, sb[t * 64 + lane]);
        for (int r = 0; r < 16; ++r) d[((size_t)t * 64 + lane) * 16 + r] = c[r];
    }
}

static double dec(int q, int ebits, int mbits, int bias) {
    const int mag = q & ((1 << (ebits + mbits)) - 1), ef = mag >> mbits, mf = mag & ((1 << mbits) - 1);
    const double v = ef == 0 ? std::ldexp((double)mf, 1 - bias - mbits) : std::ldexp((double)(mf | (1 << mbits)), ef - bias - mbits);
    return (q >> (ebits + mbits)) & 1 ? -v : v;
}
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

int main() {
    const int T = 512;
    // distributions: (a) every finite code, (b) magnitudes within 4 binades of the top (a layer's large values), (c) one sign
    // (no cancellation), (d) as (a) with a nonzero accumulator input
    const char* names[4] = {"all finite codes", "top 4 binades", "top 4 binades, one sign", "all finite codes, C != 0"};
    std::vector<uint32_t> ha((size_t)T * 64 * 8), hb((size_t)T * 64 * 8);
    std::vector<int> hsa(T * 64), hsb(T * 64);
    std::vector<float> hc((size_t)T * 64 * 16), hd((size_t)T * 64 * 16);
    uint32_t *da, *db; int *dsa, *dsb; float *dc, *dd;
    CK(hipMalloc(&da, ha.size() * 4)); CK(hipMalloc(&db, hb.size() * 4)); CK(hipMalloc(&dsa, hsa.size() * 4));
    CK(hipMalloc(&dsb, hsb.size() * 4)); CK(hipMalloc(&dc, hc.size() * 4)); CK(hipMalloc(&dd, hd.size() * 4));
    for (int dist = 0; dist < 4; ++dist) {
        auto code = [&](bool e5m2) -> uint32_t {
            for (;;) {
                uint32_t q = rnd() & 0xff;
                const int mag = q & 0x7f;
                if (e5m2 ? mag >= 0x7c : mag >= 0x7f) continue;
                if (dist == 1 || dist == 2) {
                    const int ef = e5m2 ? mag >> 2 : mag >> 3, top = e5m2 ? 30 : 15;
                    if (ef < top - 3) continue;
                    if (dist == 2) q &= 0x7f;
                }
                return q;
            }
        };
        for (size_t i = 0; i < ha.size(); ++i) {
            ha[i] = code(true) | code(true) << 8 | code(true) << 16 | code(true) << 24;
            hb[i] = code(false) | code(false) << 8 | code(false) << 16 | code(false) << 24;
        }
        for (int i = 0; i < T * 64; ++i) { hsa[i] = 110 + (int)(rnd() % 24); hsb[i] = 118 + (int)(rnd() % 12); }
        for (size_t i = 0; i < hc.size(); ++i) hc[i] = dist == 3 ? (float)((int)(rnd() % 2001) - 1000) * 1e3f : 0.0f;
        CK(hipMemcpy(da, ha.data(), ha.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dsa, hsa.data(), hsa.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, hsb.data(), hsb.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dc, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_mfma, dim3(64), dim3(64), 0, 0, da, db, dsa, dsb, dc, dd, T);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(hd.data(), dd, hd.size() * 4, hipMemcpyDeviceToHost));
        double worst_sum = 0, worst_max = 0, worst_blk = 0;
        long inexact = 0, total = 0;
        for (int t = 0; t < T; ++t)
            for (int m = 0; m < 32; ++m)
                for (int n = 0; n < 32; ++n) {
                    double ref = 0, tabs = 0, tmax = 0, blk_abs[2] = {0, 0};
                    for (int k = 0; k < 64; ++k) {
                        const int blk = k >> 5, H = (k >> 4) & 1, b = k & 15;
                        const uint8_t* ab = (const uint8_t*)&ha[((size_t)t * 64 + 32 * H + m) * 8];
                        const uint8_t* bb = (const uint8_t*)&hb[((size_t)t * 64 + 32 * H + n) * 8];
                        const double sA = std::ldexp(1.0, (hsa[t * 64 + 32 * blk + m] & 0xff) - 127);
                        const double sB = std::ldexp(1.0, (hsb[t * 64 + 32 * blk + n] & 0xff) - 127);
                        const double p = dec(ab[16 * blk + b], 5, 2, 15) * sA * dec(bb[16 * blk + b], 4, 3, 7) * sB;
                        ref += p; tabs += std::fabs(p); blk_abs[blk] += std::fabs(p);
                        if (std::fabs(p) > tmax) tmax = std::fabs(p);
                    }
                    const int lane = 32 * ((m >> 2) & 1) + n, r = (m & 3) + 4 * (m >> 3);
                    const double c0 = hc[((size_t)t * 64 + lane) * 16 + r];
                    const double got = hd[((size_t)t * 64 + lane) * 16 + r], err = std::fabs(got - (ref + c0));
                    const double u = std::ldexp(1.0, -24);
                    total++;
                    if (err != 0) inexact++;
                    if (tabs + std::fabs(c0) > 0 && err / (u * (tabs + std::fabs(c0))) > worst_sum) worst_sum = err / (u * (tabs + std::fabs(c0)));
                    if (tmax > 0 && err / (u * tmax) > worst_max) worst_max = err / (u * tmax);
                    const double big = blk_abs[0] > blk_abs[1] ? blk_abs[0] : blk_abs[1];
                    if (big > 0 && err / (u * big) > worst_blk) worst_blk = err / (u * big);
                }
        std::printf("%-28s: %ld of %ld results differ from fp64; worst error = %.1f x 2^-24 sum|products| = %.1f x 2^-24 max|product| "
                    "= %.1f x 2^-24 of the larger 32-block's sum\n", names[dist], inexact, total, worst_sum, worst_max, worst_blk);
    }
    return 0;
}

// Scoring and logging of rendered images on the device.
//
//   nerfhip_ssim            kornia 0.2.0 `kornia.losses.ssim` behind the reference's metrics.py:15-20 (1 - 2 * dssim), as a map
//                           and / or as its mean
//   nerfhip_depth_colormap  utils/visualization.py:6-17 `visualize_depth`: nan_to_num, min / max, 8-bit index, colour table
//
// SSIM.  One workgroup of 256 threads owns a 32 x 32 tile of output pixels of one image and channel.  It stages the tile and its
// halo of ws/2 pixels (zeros outside the image: the padded zeros take part in every mean) of both images in LDS once, applies
// the window's row pass to the five products (x1, x2, x1^2, x2^2, x1 x2) into LDS and the column pass from there.
//
// The windowed second moments do not cancel: before the products are formed each image is centred on the mean c of the pixels
// the workgroup staged (padded zeros become -c, so every window still sees the reference's samples, all shifted by c).  Variance
// and covariance are shift-invariant, so  filt(x'^2) - filt(x')^2  is the reference's  filt(x^2) - mu^2  with operands of the
// size of the local contrast instead of the size of the pixel values: on a flat or near-white image the fp32 rounding of the
// reference's form (up to 1.5e-3 of the map against the floor C2 = 9e-4) is gone.  mu = filt(x') + c.
// Centring helps a window that lies inside the image and hurts one that is mostly padding (there the SHIFTED samples are large
// and nearly constant); with w_in the window weight that falls inside the image, the cancellation of the plain form grows as
// 1 / (1 - w_in) and that of the centred form as 1 / w_in.  An image so small that no window has w_in >= 1/2 is therefore not
// centred (c = 0, the reference's own form: a host decision per call).
//
// The mean is deterministic: every workgroup writes the fp64 sum of its tile (fixed in-block order) to the workspace, and a
// second one-workgroup launch folds the partial sums in index order.  No float atomics, no state between calls.
#include "common.h"

#include <float.h>
#include <math.h>

namespace nerfhip {
namespace {

constexpr int kTile = 32, kThreads = 256, kMaxR = 5;
constexpr int kFoldThreads = 256;

struct SsimWindow {
    float g[2 * kMaxR + 1];
};

// fixed-order block sums (4 waves of 64): lanes by xor-shuffle, waves in index order
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }   // NaN stays NaN

// element (plane = b * C + c, y, x) of a planar (B,C,H,W) or interleaved (B,H,W,C) image
template <bool kInterleaved>
__device__ __forceinline__ int64_t pixel_index(int b, int c, int C, int H, int W, int y, int x) {
    if (kInterleaved) return (((int64_t)b * H + y) * W + x) * C + c;
    return (((int64_t)b * C + c) * H + y) * W + x;
}

template <int WS, bool kInterleaved>
__global__ void __launch_bounds__(kThreads) ssim_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int C, int H,
                                                        int W, int tiles_x, int tiles_y, SsimWindow win, int centre,
                                                        float* __restrict__ map, double* __restrict__ partial) {
    constexpr int R = WS / 2, SIDE = kTile + 2 * R;
    __shared__ float s1[SIDE * SIDE], s2[SIDE * SIDE];
    __shared__ float hb[5][SIDE * kTile];
    __shared__ float red_f[4];
    __shared__ double red_d[4];

    const int tile = (int)blockIdx.x;
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, plane = tile / (tiles_x * tiles_y);
    const int b = plane / C, c = plane % C;
    const int x0 = tx * kTile, y0 = ty * kTile;
    const int tid = (int)threadIdx.x;

    // ---- stage tile + halo, zero outside the image; sum the staged pixels for the centre
    float sum1 = 0.0f, sum2 = 0.0f;
    for (int i = tid; i < SIDE * SIDE; i += kThreads) {
        const int ly = i / SIDE, lx = i - ly * SIDE;
        const int y = y0 + ly - R, x = x0 + lx - R;
        float a = 0.0f, d = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int64_t p = pixel_index<kInterleaved>(b, c, C, H, W, y, x);
            a = img1[p];
            d = img2[p];
        }
        s1[i] = a;
        s2[i] = d;
        sum1 += a;
        sum2 += d;
    }
    // pixels of the image inside the staged square (at least the tile's own first pixel)
    const int ny = min(y0 + kTile + R, H) - max(y0 - R, 0), nx = min(x0 + kTile + R, W) - max(x0 - R, 0);
    const float inv_count = centre ? 1.0f / (float)(ny * nx) : 0.0f;
    const float c1 = block_sum(sum1, red_f) * inv_count;
    const float c2 = block_sum(sum2, red_f) * inv_count;      // (block_sum's leading barrier orders the two uses of red_f)

    // ---- row pass: SIDE rows x kTile columns of the five centred products
    for (int i = tid; i < SIDE * kTile; i += kThreads) {
        const int ly = i / kTile, lx = i - ly * kTile;
        float h1 = 0.0f, h2 = 0.0f, h11 = 0.0f, h22 = 0.0f, h12 = 0.0f;
#pragma unroll
        for (int k = 0; k < WS; ++k) {
            const float w = win.g[k];
            const float a = s1[ly * SIDE + lx + k] - c1, d = s2[ly * SIDE + lx + k] - c2;
            h1 += w * a;
            h2 += w * d;
            h11 += w * (a * a);
            h22 += w * (d * d);
            h12 += w * (a * d);
        }
        hb[0][i] = h1;
        hb[1][i] = h2;
        hb[2][i] = h11;
        hb[3][i] = h22;
        hb[4][i] = h12;
    }
    __syncthreads();

    // ---- column pass + the map
    const float C1 = 1e-4f, C2 = 9e-4f;      // (0.01 * 1)^2, (0.03 * 1)^2
    double acc = 0.0;
    for (int i = tid; i < kTile * kTile; i += kThreads) {
        const int ly = i / kTile, lx = i - ly * kTile;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        float m1 = 0.0f, m2 = 0.0f, v11 = 0.0f, v22 = 0.0f, v12 = 0.0f;
#pragma unroll
        for (int k = 0; k < WS; ++k) {
            const float w = win.g[k];
            const int j = (ly + k) * kTile + lx;
            m1 += w * hb[0][j];
            m2 += w * hb[1][j];
            v11 += w * hb[2][j];
            v22 += w * hb[3][j];
            v12 += w * hb[4][j];
        }
        const float s11 = v11 - m1 * m1, s22 = v22 - m2 * m2, s12 = v12 - m1 * m2;
        const float mu1 = m1 + c1, mu2 = m2 + c2;
        const float num = ((2.0f * mu1) * mu2 + C1) * (2.0f * s12 + C2);
        const float den = (mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2);
        const float dssim = clamp01(1.0f - num / den) * 0.5f;
        const float value = 1.0f - 2.0f * dssim;
        if (map) map[pixel_index<kInterleaved>(b, c, C, H, W, y, x)] = value;
        acc += (double)value;
    }
    if (partial) {      // (uniform over the workgroup)
        const double total = block_sum(acc, red_d);
        if (tid == 0) partial[tile] = total;
    }
}

__global__ void __launch_bounds__(kFoldThreads) ssim_fold_kernel(const double* __restrict__ partial, int n_partial, double count,
                                                                 float* __restrict__ mean) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < n_partial; i += kFoldThreads) acc += partial[i];
    const double total = block_sum(acc, red);
    if (threadIdx.x == 0) *mean = (float)(total / count);
}

inline bool ssim_tiles(int B, int C, int H, int W, int64_t* tiles, int* tiles_x, int* tiles_y) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return false;
    *tiles_x = (W + kTile - 1) / kTile;
    *tiles_y = (H + kTile - 1) / kTile;
    *tiles = (int64_t)B * C * *tiles_x * *tiles_y;
    return *tiles <= INT32_MAX;
}

// the largest window weight that falls inside an image of `len` pixels along one axis (1 when the window fits)
inline double ssim_inside_weight(const double* g, int ws, int len) {
    if (len >= ws) return 1.0;
    double best = 0.0;
    for (int k = 0; k + len <= ws; ++k) {
        double sum = 0.0;
        for (int i = 0; i < len; ++i) sum += g[k + i];
        best = sum > best ? sum : best;
    }
    return best;
}

template <bool kInterleaved>
void ssim_launch(int ws, unsigned tiles, hipStream_t s, const float* img1, const float* img2, int C, int H, int W, int tiles_x,
                 int tiles_y, const SsimWindow& win, int centre, float* map, double* partial) {
#define NH_SSIM_CASE(N)                                                                                                       \
    case N:                                                                                                                   \
        hipLaunchKernelGGL((ssim_kernel<N, kInterleaved>), dim3(tiles), dim3(kThreads), 0, s, img1, img2, C, H, W, tiles_x, \
                           tiles_y, win, centre, map, partial);                                                              \
        break;
    switch (ws) {
        NH_SSIM_CASE(3)
        NH_SSIM_CASE(5)
        NH_SSIM_CASE(7)
        NH_SSIM_CASE(9)
        NH_SSIM_CASE(11)
    }
#undef NH_SSIM_CASE
}

// ------------------------------------------------------------------------------------------------------------ depth colour map
constexpr int kDepthThreads = 256, kDepthMaxBlocks = 1024;

__device__ __forceinline__ float nan_to_num(float v) {      // numpy's, float32
    if (!(v == v)) return 0.0f;
    if (v == INFINITY) return FLT_MAX;
    if (v == -INFINITY) return -FLT_MAX;
    return v;
}

// min and max of a block's values (order-independent, so any fold is deterministic)
__device__ __forceinline__ void block_min_max(float& mi, float& ma, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mi = fminf(mi, __shfl_xor(mi, o, 64));
        ma = fmaxf(ma, __shfl_xor(ma, o, 64));
    }
    __syncthreads();
    if (lane_id() == 0) {
        red[threadIdx.x >> 6] = mi;
        red[4 + (threadIdx.x >> 6)] = ma;
    }
    __syncthreads();
    mi = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    ma = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

__global__ void __launch_bounds__(kDepthThreads) depth_min_max_kernel(const float* __restrict__ depth, int64_t n,
                                                                      float* __restrict__ partial) {
    __shared__ float red[8];
    float mi = FLT_MAX, ma = -FLT_MAX;      // nan_to_num leaves nothing outside [-FLT_MAX, FLT_MAX]
    for (int64_t i = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDepthThreads) {
        const float v = nan_to_num(depth[i]);
        mi = fminf(mi, v);
        ma = fmaxf(ma, v);
    }
    block_min_max(mi, ma, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = mi;
        partial[2 * blockIdx.x + 1] = ma;
    }
}

__global__ void __launch_bounds__(kDepthThreads) depth_color_kernel(const float* __restrict__ depth, int64_t n,
                                                                    const float* __restrict__ partial, int n_partial,
                                                                    const unsigned char* __restrict__ table,
                                                                    float* __restrict__ out_chw, unsigned char* __restrict__ out_hwc) {
    __shared__ float red[8];
    __shared__ unsigned char lut[768];
    float mi = FLT_MAX, ma = -FLT_MAX;
    for (int i = (int)threadIdx.x; i < n_partial; i += kDepthThreads) {
        mi = fminf(mi, partial[2 * i]);
        ma = fmaxf(ma, partial[2 * i + 1]);
    }
    for (int i = (int)threadIdx.x; i < 768; i += kDepthThreads) lut[i] = table[i];
    block_min_max(mi, ma, red);             // (its barriers also publish lut)
    const float scale = (ma - mi) + 1e-8f;
    const int64_t i = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    if (i >= n) return;
    const float x = (nan_to_num(depth[i]) - mi) / scale;
    const float v = 255.0f * x;
    // astype(uint8) of a value in [0, 255]; NaN (inf / inf when the image holds both infinities) -> 0, as numpy on x86-64
    const int idx = (v == v) ? ((int)v & 255) : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned char byte = lut[3 * idx + k];
        if (out_chw) out_chw[(int64_t)k * n + i] = (float)byte / 255.0f;
        if (out_hwc) out_hwc[3 * i + k] = byte;
    }
}

inline int depth_blocks(int64_t n) {
    const int64_t blocks = (n + kDepthThreads - 1) / kDepthThreads;
    return (int)(blocks < kDepthMaxBlocks ? blocks : kDepthMaxBlocks);
}

}  // namespace
}  // namespace nerfhip

using namespace nerfhip;

extern "C" size_t nerfhip_ssim_workspace_bytes(int B, int C, int H, int W) {
    int64_t tiles;
    int tiles_x, tiles_y;
    if (!ssim_tiles(B, C, H, W, &tiles, &tiles_x, &tiles_y)) return 0;
    return (size_t)tiles * sizeof(double);
}

extern "C" int nerfhip_ssim(const float* img1, const float* img2, int B, int C, int H, int W, int window_size, int layout, float* map,
                            float* mean, void* workspace, nerfhip_stream_t stream) {
    int64_t tiles;
    int tiles_x, tiles_y;
    NERFHIP_CHECK_ARG(window_size >= 3 && window_size <= 2 * kMaxR + 1 && (window_size & 1));
    NERFHIP_CHECK_ARG(layout == NERFHIP_IMAGE_PLANAR || layout == NERFHIP_IMAGE_INTERLEAVED);
    NERFHIP_CHECK_ARG(ssim_tiles(B, C, H, W, &tiles, &tiles_x, &tiles_y));
    if (tiles == 0) return 0;
    NERFHIP_CHECK_ARG(img1 && img2 && (!mean || workspace));
    NERFHIP_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    if (!map && !mean) return 0;

    SsimWindow win;
    double g[2 * kMaxR + 1], total = 0.0;
    for (int i = 0; i < window_size; ++i) {
        const double d = (double)(i - window_size / 2);
        g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        total += g[i];
    }
    for (int i = 0; i < window_size; ++i) g[i] /= total;
    for (int i = 0; i < 2 * kMaxR + 1; ++i) win.g[i] = i < window_size ? (float)g[i] : 0.0f;
    const int centre = ssim_inside_weight(g, window_size, H) * ssim_inside_weight(g, window_size, W) >= 0.5;

    hipStream_t s = (hipStream_t)stream;
    double* partial = mean ? (double*)workspace : nullptr;
    if (layout == NERFHIP_IMAGE_INTERLEAVED)
        ssim_launch<true>(window_size, (unsigned)tiles, s, img1, img2, C, H, W, tiles_x, tiles_y, win, centre, map, partial);
    else
        ssim_launch<false>(window_size, (unsigned)tiles, s, img1, img2, C, H, W, tiles_x, tiles_y, win, centre, map, partial);
    if (mean)
        hipLaunchKernelGGL(ssim_fold_kernel, dim3(1), dim3(kFoldThreads), 0, s, partial, (int)tiles,
                           (double)B * (double)C * (double)H * (double)W, mean);
    return nerfhip_launch_status();
}

extern "C" size_t nerfhip_depth_colormap_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return (size_t)depth_blocks(n) * 2 * sizeof(float);
}

extern "C" int nerfhip_depth_colormap(const float* depth, int64_t n, const uint8_t* table, float* out_chw, uint8_t* out_hwc,
                                      void* workspace, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= (int64_t)INT32_MAX * kDepthThreads);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(depth && table && workspace && ((uintptr_t)workspace & 3) == 0);
    if (!out_chw && !out_hwc) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = depth_blocks(n);
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(depth_min_max_kernel, dim3(blocks), dim3(kDepthThreads), 0, s, depth, n, partial);
    hipLaunchKernelGGL(depth_color_kernel, dim3((unsigned)((n + kDepthThreads - 1) / kDepthThreads)), dim3(kDepthThreads), 0, s, depth,
                       n, partial, blocks, table, out_chw, out_hwc);
    return nerfhip_launch_status();
}

// Scene loading (datasets/blender.py:47-58, 90-95): what the reference does per image with PIL + torchvision on the host —
// PNG scanline reconstruction, Image.resize(LANCZOS) of an 8-bit RGBA image, ToTensor and the blend onto white — as integer /
// separately rounded fp32 kernels whose results equal the reference's bytes and floats.  The host only reads and inflates the
// files and builds the resampling taps (double precision).  Layouts, byte counts and timings: DESIGN.md, scene loading.
#include "common.h"

namespace {

constexpr int kBlock = 256;          // threads of the per-pixel kernels (4 waves)
constexpr int kRowsMax = 1024;       // rows one workgroup of the unfilter kernel reconstructs side by side

inline int blocks(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

// ---- PNG unfilter --------------------------------------------------------------------------------------------------------------
// Filters 3 (Average) and 4 (Paeth) predict a byte from its reconstructed left, up and up-left neighbours, so a pixel depends on
// everything above and left of it.  One workgroup per image walks the anti-diagonals: thread r owns row y0 + r of the current
// strip of blockDim.x rows and reconstructs pixel x = t - r at step t.  `left` and `up-left` never leave its registers; `up` is
// the pixel row r - 1 made one step earlier, handed over as one dword through a double-buffered LDS array (consecutive threads,
// consecutive banks) with one barrier per step.  The first row of a later strip reads `up` from the finished output of the
// strip before.  W + rows - 1 steps per strip, each a barrier and an LDS round trip: the kernel is bound by that latency, not by
// bytes or arithmetic, and the parallelism is across images (one CU each).
template <int CH>
__global__ void __launch_bounds__(kRowsMax) png_unfilter(const uint8_t* __restrict__ streams, uint8_t* __restrict__ out,
                                                         int32_t* __restrict__ error_flags, int H, int W) {
    __shared__ uint32_t hand[2][kRowsMax];
    const int64_t stride = 1 + (int64_t)W * CH;
    const uint8_t* src = streams + (int64_t)blockIdx.x * H * stride;
    uint8_t* dst = out + (int64_t)blockIdx.x * H * W * CH;
    const int r = (int)threadIdx.x, rows = (int)blockDim.x;
    int bad = 0;
    for (int y0 = 0; y0 < H; y0 += rows) {
        const int y = y0 + r;
        const bool live = y < H;
        const uint8_t* row = src + (int64_t)(live ? y : 0) * stride;
        int filter = live ? row[0] : 0;
        if (filter > 4) {            // unknown filter type: flag the image, treat the row as unfiltered
            bad = 1;
            filter = 0;
        }
        uint32_t left = 0, upleft = 0, next = 0;
        if (live) {
#pragma unroll
            for (int c = 0; c < CH; ++c) next |= (uint32_t)row[1 + c] << (8 * c);
        }
        const int n_strip = min(rows, H - y0);
        const int steps = W + n_strip - 1;
        for (int t = 0; t < steps; ++t) {
            const int x = t - r;
            if (live && x >= 0 && x < W) {
                const uint32_t cur = next;
                if (x + 1 < W) {     // the next pixel's filtered bytes, in flight across the barrier
                    next = 0;
#pragma unroll
                    for (int c = 0; c < CH; ++c) next |= (uint32_t)row[1 + (int64_t)(x + 1) * CH + c] << (8 * c);
                }
                uint32_t up = 0;
                if (r > 0) {
                    up = hand[(t + 1) & 1][r - 1];
                } else if (y > 0) {
                    const uint8_t* above = dst + ((int64_t)(y - 1) * W + x) * CH;
#pragma unroll
                    for (int c = 0; c < CH; ++c) up |= (uint32_t)above[c] << (8 * c);
                }
                uint32_t px = 0;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int a = (left >> (8 * c)) & 255, b = (up >> (8 * c)) & 255, cc = (upleft >> (8 * c)) & 255;
                    int pred = 0;
                    if (filter == 1) {
                        pred = a;
                    } else if (filter == 2) {
                        pred = b;
                    } else if (filter == 3) {
                        pred = (a + b) >> 1;
                    } else if (filter == 4) {
                        const int pa = abs(b - cc), pb = abs(a - cc), pc = abs(a + b - 2 * cc);
                        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : cc);
                    }
                    px |= (uint32_t)((((cur >> (8 * c)) & 255) + pred) & 255) << (8 * c);
                }
                hand[t & 1][r] = px;
                uint8_t* o = dst + ((int64_t)y * W + x) * CH;
                if (CH == 4) {
                    *(uint32_t*)o = px;
                } else {
#pragma unroll
                    for (int c = 0; c < CH; ++c) o[c] = (uint8_t)(px >> (8 * c));
                }
                left = px;
                upleft = up;
            }
            __syncthreads();
        }
        // the strip's last row is in HBM before the next strip's first row reads it (the loop's last barrier orders it within the
        // workgroup)
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) error_flags[blockIdx.x] = bad;
}

// ---- Image.resize(size, LANCZOS) on 8-bit RGBA ---------------------------------------------------------------------------------
// Pillow's arithmetic: RGBA -> RGBa (premultiplied), one pass per axis whose size changes with 22-bit fixed-point taps and an
// 8-bit intermediate, RGBa -> RGBA.  The taps come from the host; nothing here is floating point.
__device__ __forceinline__ uint32_t premultiply(uint32_t p) {
    const uint32_t a = p >> 24;
    uint32_t o = p & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t t = ((p >> (8 * c)) & 255) * a + 128;
        o |= (((t >> 8) + t) >> 8) << (8 * c);
    }
    return o;
}

__device__ __forceinline__ uint32_t unpremultiply(uint32_t p) {
    const uint32_t a = p >> 24;
    if (a == 0 || a == 255) return p;
    uint32_t o = p & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t v = (255u * ((p >> (8 * c)) & 255)) / a;
        o |= (v > 255u ? 255u : v) << (8 * c);
    }
    return o;
}

// clip(s >> 22, 0, 255), written as a clamp of the sum followed by a logical shift.  Shift-then-clamp is what hipcc (ROCm 7)
// turns into gfx950's v_ashr_pk_u8_i32 and then ORs further bytes onto the result's upper half as if it were zero; on an
// MI355X that half was not, and out-of-range sums came back with wrong blue and alpha bytes.
__device__ __forceinline__ uint32_t clip8(int s) {
    const int top = (256 << 22) - 1;
    s = s < 0 ? 0 : (s > top ? top : s);
    return (uint32_t)s >> 22;
}

// One axis: in (n, in_h, in_w) pixels -> out (n, out_h, out_w), where the axis `VERTICAL` names goes from in_len to out_len and
// the other one is kept.  One thread per output pixel, all four channels.  A tap window that the table would place outside the
// input is clamped to it, so a malformed table gives wrong colours, never a wrong address.
template <bool VERTICAL>
__global__ void __launch_bounds__(kBlock) resample_axis(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n_out,
                                                        int in_h, int in_w, int out_h, int out_w, const int32_t* __restrict__ xmin,
                                                        const int32_t* __restrict__ count, const int32_t* __restrict__ taps,
                                                        int ksize, int premul_in, int unpremul_out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_out) return;
    const int ox = (int)(i % out_w), oy = (int)((i / out_w) % out_h);
    const int64_t img = i / ((int64_t)out_w * out_h);
    const int o = VERTICAL ? oy : ox, in_len = VERTICAL ? in_h : in_w;
    int x0 = xmin[o], cnt = count[o];
    x0 = x0 < 0 ? 0 : (x0 > in_len ? in_len : x0);
    cnt = cnt < 0 ? 0 : (cnt > ksize ? ksize : cnt);
    cnt = cnt > in_len - x0 ? in_len - x0 : cnt;
    const int32_t* k = taps + (int64_t)o * ksize;
    const uint32_t* p = in + img * in_h * in_w + (VERTICAL ? (int64_t)x0 * in_w + ox : (int64_t)oy * in_w + x0);
    const int64_t step = VERTICAL ? in_w : 1;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21, s3 = 1 << 21;
    for (int j = 0; j < cnt; ++j) {
        uint32_t v = p[j * step];
        if (premul_in) v = premultiply(v);
        const int w = k[j];
        s0 += (int)(v & 255) * w;
        s1 += (int)((v >> 8) & 255) * w;
        s2 += (int)((v >> 16) & 255) * w;
        s3 += (int)(v >> 24) * w;
    }
    uint32_t r = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16) | (clip8(s3) << 24);
    if (unpremul_out) r = unpremultiply(r);
    out[i] = r;
}

__global__ void __launch_bounds__(kBlock) copy_pixels(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = in[i];
}

// ---- ToTensor + blend onto white (blender.py:56-58, 93) ------------------------------------------------------------------------
// f = byte / 255 in fp32; rgb = f_c * f_a + (1 - f_a) as a multiply, a subtraction and an addition, each rounded (common.h keeps
// contraction off); valid_mask = alpha > 0.
__global__ void __launch_bounds__(kBlock) rgba_to_rgb_white(const uint32_t* __restrict__ rgba, float* __restrict__ rgb,
                                                            uint8_t* __restrict__ valid_mask, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = rgba[i];
    const float fa = nh_div((float)(p >> 24), 255.0f);
    const float rest = nh_sub(1.0f, fa);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = nh_div((float)((p >> (8 * c)) & 255), 255.0f);
        rgb[3 * i + c] = nh_add(nh_mul(f, fa), rest);
    }
    if (valid_mask) valid_mask[i] = (p >> 24) > 0;
}

}  // namespace

extern "C" int nerfhip_png_unfilter(const uint8_t* streams, uint8_t* out, int32_t* error_flags, int n_images, int H, int W, int ch,
                                    nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n_images >= 0 && H >= 0 && W >= 0 && (ch == 1 || ch == 3 || ch == 4));
    if (n_images == 0) return 0;
    NERFHIP_CHECK_ARG(error_flags);
    if (H == 0 || W == 0) return (int)hipMemsetAsync(error_flags, 0, sizeof(int32_t) * n_images, (hipStream_t)stream);
    NERFHIP_CHECK_ARG(streams && out);
    NERFHIP_CHECK_ARG(ch != 4 || ((uintptr_t)out & 3) == 0);
    const int rows = H >= kRowsMax ? kRowsMax : ((H + NERFHIP_WAVE - 1) / NERFHIP_WAVE) * NERFHIP_WAVE;
    const dim3 grid(n_images), block(rows);
    if (ch == 1)
        hipLaunchKernelGGL(png_unfilter<1>, grid, block, 0, (hipStream_t)stream, streams, out, error_flags, H, W);
    else if (ch == 3)
        hipLaunchKernelGGL(png_unfilter<3>, grid, block, 0, (hipStream_t)stream, streams, out, error_flags, H, W);
    else
        hipLaunchKernelGGL(png_unfilter<4>, grid, block, 0, (hipStream_t)stream, streams, out, error_flags, H, W);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_resize_rgba_lanczos(const uint8_t* in, uint8_t* out, uint8_t* workspace, int n_images, int in_h, int in_w,
                                           int out_h, int out_w, const int32_t* xmin_h, const int32_t* count_h, const int32_t* taps_h,
                                           int ksize_h, const int32_t* xmin_v, const int32_t* count_v, const int32_t* taps_v,
                                           int ksize_v, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n_images >= 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0);
    if (n_images == 0) return 0;
    NERFHIP_CHECK_ARG(in && out && in != out);
    NERFHIP_CHECK_ARG((((uintptr_t)in | (uintptr_t)out | (uintptr_t)workspace) & 3) == 0);
    const bool horiz = in_w != out_w, vert = in_h != out_h;
    NERFHIP_CHECK_ARG(!horiz || (xmin_h && count_h && taps_h && ksize_h > 0));
    NERFHIP_CHECK_ARG(!vert || (xmin_v && count_v && taps_v && ksize_v > 0));
    NERFHIP_CHECK_ARG(!(horiz && vert) || (workspace && workspace != in && workspace != out));
    NERFHIP_CHECK_ARG((int64_t)n_images * in_h * in_w < ((int64_t)1 << 38) && (int64_t)n_images * out_h * out_w < ((int64_t)1 << 38));
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t* src = (const uint32_t*)in;
    uint32_t* dst = (uint32_t*)out;
    if (!horiz && !vert) {           // Pillow returns a copy: no premultiply round trip
        const int64_t n = (int64_t)n_images * in_h * in_w;
        hipLaunchKernelGGL(copy_pixels, dim3(blocks(n)), dim3(kBlock), 0, s, src, dst, n);
        return nerfhip_launch_status();
    }
    if (horiz) {
        uint32_t* mid = vert ? (uint32_t*)workspace : dst;
        const int64_t n = (int64_t)n_images * in_h * out_w;
        hipLaunchKernelGGL(resample_axis<false>, dim3(blocks(n)), dim3(kBlock), 0, s, src, mid, n, in_h, in_w, in_h, out_w, xmin_h,
                           count_h, taps_h, ksize_h, 1, vert ? 0 : 1);
        src = mid;
    }
    if (vert) {
        const int64_t n = (int64_t)n_images * out_h * out_w;
        hipLaunchKernelGGL(resample_axis<true>, dim3(blocks(n)), dim3(kBlock), 0, s, src, dst, n, in_h, out_w, out_h, out_w, xmin_v,
                           count_v, taps_v, ksize_v, horiz ? 0 : 1, 1);
    }
    return nerfhip_launch_status();
}

extern "C" int nerfhip_rgba_to_rgb_white(const uint8_t* rgba, float* rgb, uint8_t* valid_mask, int64_t n, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n >= 0);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(rgba && rgb && ((uintptr_t)rgba & 3) == 0);
    hipLaunchKernelGGL(rgba_to_rgb_white, dim3(blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t*)rgba, rgb,
                       valid_mask, n);
    return nerfhip_launch_status();
}

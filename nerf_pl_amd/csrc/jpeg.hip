// Baseline JPEG decoding for LLFF scenes (datasets/llff.py:226,312: `Image.open(p).convert('RGB')`), bit-equal to Pillow's
// libjpeg-turbo defaults (JDCT_ISLOW, fancy upsampling).  The host parses the markers (imageio_min.jpeg_parse) and
// Huffman-decodes the scan (nerfhip_jpeg_entropy_decode below: plain C++, no GPU); the device does everything per sample:
//   jpeg_idct      coefficients -> 8-bit component planes (dequantise, islow IDCT, +128, range limit)
//   jpeg_to_rgbx   planes -> (n, H, W, 4) RGBX (triangle chroma upsampling, fixed-point YCbCr -> RGB, crop, X = 255)
// Bytes per 4032 x 3024 4:2:0 image (12.19 M luma + 2 x 3.05 M chroma samples, already whole MCUs):
//   jpeg_idct      reads 36.6 MB of int16 coefficients, writes 18.3 MB of planes
//   jpeg_to_rgbx   reads 18.3 MB of planes (chroma neighbours come from cache), writes 48.8 MB
// Both are memory-bound.  Timings: DESIGN.md, scene loading.
#include "common.h"
#include "jpeg_huff.h"

namespace {

constexpr int kBlock = 256;              // threads of both kernels (4 waves)
constexpr int kDctPerGroup = kBlock / 8; // 8 lanes own one 8 x 8 block, so a wave owns 8 whole blocks
constexpr int kPad = 9;                  // LDS row stride in dwords: a column read of 8 lanes lands on 8 different banks

// ---- entropy decoding (host) ---------------------------------------------------------------------------------------------------
// (the tables and the zigzag order: jpeg_huff.h, shared with the split decoder of jpeg_entropy.hip)
using nerfhip::jpeg::HuffTable;
using nerfhip::jpeg::build_table;
using nerfhip::jpeg::kLook;

// MSB-first bit reader over the entropy-coded bytes of one restart interval.  Reads past the end deliver zeros and are
// counted: the caller checks `overrun()` after each block, so no input byte outside [p, end) is ever touched.
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int bits = 0;
    int64_t missing = 0;                 // zero bits invented past the end of the data
    BitReader(const uint8_t* b, const uint8_t* e) : p(b), end(e) {}
    void fill() {
        while (bits <= 56) {
            uint32_t byte = 0;
            if (p < end) {
                byte = *p;
                if (byte == 0xff) {
                    if (p + 1 < end && p[1] == 0x00) {
                        p += 2;          // stuffed zero
                    } else {             // a marker (or a lone 0xff at the end): the interval's data stops here
                        end = p;
                        byte = 0;
                        missing += 8;
                    }
                } else {
                    ++p;
                }
            } else {
                missing += 8;
            }
            acc |= (uint64_t)byte << (56 - bits);
            bits += 8;
        }
    }
    uint32_t peek(int n) { return (uint32_t)(acc >> (64 - n)); }
    void skip(int n) {
        acc <<= n;
        bits -= n;
    }
    bool overrun() const { return missing > bits; }   // consumed more bits than the data holds
};

// One Huffman symbol, or -1 for a code the table does not hold.
inline int decode_symbol(BitReader& br, const HuffTable& t) {
    if (br.bits < 16) br.fill();
    const uint32_t e = t.look[br.peek(kLook)];
    if (e) {
        br.skip(e >> 8);
        return e & 255;
    }
    const int32_t code16 = (int32_t)br.peek(16);
    for (int l = kLook + 1; l <= 16; ++l) {
        const int32_t code = code16 >> (16 - l);
        if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l]) {
            br.skip(l);
            return t.symbols[t.valptr[l] + code - t.mincode[l]];
        }
    }
    return -1;
}

inline int receive_extend(BitReader& br, int s) {
    if (s == 0) return 0;
    if (br.bits < s) br.fill();
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One 8 x 8 block into `out` (64 int16, natural order, zeroed here).  0 or a negative error code.
inline int decode_block(BitReader& br, const HuffTable& dc, const HuffTable& ac, int& pred, int16_t* out) {
    for (int i = 0; i < 64; ++i) out[i] = 0;
    int s = decode_symbol(br, dc);
    if (s < 0 || s > 11) return NERFHIP_E_DATA;
    pred += receive_extend(br, s);
    out[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return NERFHIP_E_DATA;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;          // end of block
            k += 16;
            continue;
        }
        k += r;
        if (k > 63 || s > 10) return NERFHIP_E_DATA;
        out[nerfhip::jpeg::zigzag(k)] = (int16_t)receive_extend(br, s);
        ++k;
    }
    return br.overrun() ? NERFHIP_E_DATA : 0;
}

// ---- dequantise + inverse DCT (jidctint.c's arithmetic: 13-bit constants, 2 extra bits after pass 1) ---------------------------
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;

// The 8-point inverse transform both passes share: v[0..7] in, v[0..7] out, each output rounded and shifted right by `shift`.
// The even part carries the DC term scaled by 2^13; 32-bit wraparound on absurd inputs is defined (unsigned arithmetic).
__device__ __forceinline__ void idct8(int (&v)[8], int shift) {
    int z2 = v[2], z3 = v[6];
    int z1 = (z2 + z3) * F_0_541196100;
    int tmp2 = z1 + z3 * (-F_1_847759065);
    int tmp3 = z1 + z2 * F_0_765366865;
    int tmp0 = (int)((unsigned)(v[0] + v[4]) << kConstBits);
    int tmp1 = (int)((unsigned)(v[0] - v[4]) << kConstBits);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7];
    tmp1 = v[5];
    tmp2 = v[3];
    tmp3 = v[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336;
    tmp1 *= F_2_053119869;
    tmp2 *= F_3_072711026;
    tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 *= -F_1_961570560;
    z4 *= -F_0_390180644;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int half = 1 << (shift - 1);
    v[0] = (tmp10 + tmp3 + half) >> shift;
    v[7] = (tmp10 - tmp3 + half) >> shift;
    v[1] = (tmp11 + tmp2 + half) >> shift;
    v[6] = (tmp11 - tmp2 + half) >> shift;
    v[2] = (tmp12 + tmp1 + half) >> shift;
    v[5] = (tmp12 - tmp1 + half) >> shift;
    v[3] = (tmp13 + tmp0 + half) >> shift;
    v[4] = (tmp13 - tmp0 + half) >> shift;
}

// libjpeg's range-limit table behind the inverse DCT: index (x & 1023) into [128..255, 255 x 384, 0 x 384, 0..127].
__device__ __forceinline__ uint32_t idct_limit(int x) {
    x &= 1023;
    if (x >= 512) x -= 1024;
    x += 128;
    return (uint32_t)(x < 0 ? 0 : (x > 255 ? 255 : x));
}

struct JpegPlanes {
    int n_comp;                  // 1 or 3
    int bw[3], bh[3];            // blocks per row / rows of blocks of each component (whole MCUs)
    int64_t offset[3];           // byte offset of each component's plane inside one image's planes
    int64_t image_bytes;         // planes of one image
    int64_t blocks;              // blocks of one image, all components
};

// grid (ceil(blocks / 32), n_images).  Lane j of a block's 8 lanes: loads coefficient row j (16 bytes) and the matching row of the
// quantisation table, multiplies, and leaves the products in LDS; pass 1 on column j; pass 2 on row j; stores 8 samples (8 bytes).
__global__ void __launch_bounds__(kBlock) jpeg_idct(const int16_t* __restrict__ c0, const int16_t* __restrict__ c1,
                                                    const int16_t* __restrict__ c2, const uint16_t* __restrict__ quant,
                                                    uint8_t* __restrict__ planes, JpegPlanes g) {
    __shared__ int ws[kDctPerGroup][8][kPad];
    const int slot = (int)threadIdx.x >> 3, j = (int)threadIdx.x & 7;
    const int64_t img = blockIdx.y;
    int64_t b = (int64_t)blockIdx.x * kDctPerGroup + slot;
    const bool live = b < g.blocks;
    int comp = 0;
    if (live && g.n_comp == 3) {
        const int64_t n0 = (int64_t)g.bw[0] * g.bh[0], n1 = (int64_t)g.bw[1] * g.bh[1];
        if (b >= n0 + n1) {
            comp = 2;
            b -= n0 + n1;
        } else if (b >= n0) {
            comp = 1;
            b -= n0;
        }
    }
    int v[8];
    if (live) {
        const int16_t* base = comp == 0 ? c0 : (comp == 1 ? c1 : c2);
        const int64_t per_image = (int64_t)g.bw[comp] * g.bh[comp];
        const uint4 raw = *(const uint4*)(base + ((img * per_image + b) * 64 + j * 8));
        const uint4 q = *(const uint4*)(quant + ((img * g.n_comp + comp) * 64 + j * 8));
        const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ws[slot][j][2 * i] = (int)(int16_t)(rw[i] & 0xffff) * (int)(qw[i] & 0xffff);
            ws[slot][j][2 * i + 1] = (int)(int16_t)(rw[i] >> 16) * (int)(qw[i] >> 16);
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = ws[slot][r][j];
        idct8(v, kConstBits - kPass1Bits);
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[slot][r][j] = v[r];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ws[slot][j][i];
        idct8(v, kConstBits + kPass1Bits + 3);
        uint2 o;
        o.x = idct_limit(v[0]) | (idct_limit(v[1]) << 8) | (idct_limit(v[2]) << 16) | (idct_limit(v[3]) << 24);
        o.y = idct_limit(v[4]) | (idct_limit(v[5]) << 8) | (idct_limit(v[6]) << 16) | (idct_limit(v[7]) << 24);
        const int bw = g.bw[comp];
        const int64_t by = b / bw, bx = b % bw;
        *(uint2*)(planes + img * g.image_bytes + g.offset[comp] + ((by * 8 + j) * bw + bx) * 8) = o;
    }
}

// ---- upsample + colour ---------------------------------------------------------------------------------------------------------
// jdsample.c's triangle filters, restated per output sample.  cw, chh: the chroma plane's real (downsampled) size, whose last
// column and row are the filter's edges; stride: its padded row length.
__device__ __forceinline__ int chroma_h2v1(const uint8_t* p, int64_t stride, int cw, int x, int y) {
    const uint8_t* row = p + (int64_t)y * stride;
    const int i = x >> 1, here = row[i];
    if (x & 1) return i == cw - 1 ? here : (3 * here + row[i + 1] + 2) >> 2;
    return i == 0 ? here : (3 * here + row[i - 1] + 1) >> 2;
}

__device__ __forceinline__ int chroma_h2v2(const uint8_t* p, int64_t stride, int cw, int chh, int x, int y) {
    const int r = y >> 1;
    const int other = (y & 1) ? (r + 1 < chh ? r + 1 : chh - 1) : (r > 0 ? r - 1 : 0);   // the nearer neighbour row, replicated at the edges
    const uint8_t* near_row = p + (int64_t)r * stride;
    const uint8_t* far_row = p + (int64_t)other * stride;
    const int i = x >> 1;
    const int here = 3 * near_row[i] + far_row[i];
    if (x & 1) return i == cw - 1 ? (4 * here + 7) >> 4 : (3 * here + 3 * near_row[i + 1] + far_row[i + 1] + 7) >> 4;
    return i == 0 ? (4 * here + 8) >> 4 : (3 * here + 3 * near_row[i - 1] + far_row[i - 1] + 8) >> 4;
}

__device__ __forceinline__ uint32_t clamp8(int x) { return (uint32_t)(x < 0 ? 0 : (x > 255 ? 255 : x)); }

// One thread per output pixel.  hs, vs: luma sampling factors (chroma is 1 x 1); fancy: the chroma planes are wider than 2
// samples, so libjpeg-turbo filters them instead of replicating.
__global__ void __launch_bounds__(kBlock) jpeg_to_rgbx(const uint8_t* __restrict__ planes, uint32_t* __restrict__ out, int64_t n_out,
                                                       int H, int W, int hs, int vs, int fancy, JpegPlanes g) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_out) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int64_t img = i / ((int64_t)W * H);
    const uint8_t* base = planes + img * g.image_bytes;
    const int lum = base[g.offset[0] + (int64_t)y * g.bw[0] * 8 + x];
    if (g.n_comp == 1) {
        out[i] = 0xff000000u | (uint32_t)(lum * 0x010101);
        return;
    }
    const uint8_t* pb = base + g.offset[1];
    const uint8_t* pr = base + g.offset[2];
    const int64_t stride = (int64_t)g.bw[1] * 8;
    const int cw = (W + hs - 1) / hs, chh = (H + vs - 1) / vs;
    int cb, cr;
    if (hs == 1) {
        cb = pb[(int64_t)y * stride + x];
        cr = pr[(int64_t)y * stride + x];
    } else if (!fancy) {
        const int64_t at = (int64_t)(y / vs) * stride + (x >> 1);
        cb = pb[at];
        cr = pr[at];
    } else if (vs == 1) {
        cb = chroma_h2v1(pb, stride, cw, x, y);
        cr = chroma_h2v1(pr, stride, cw, x, y);
    } else {
        cb = chroma_h2v2(pb, stride, cw, chh, x, y);
        cr = chroma_h2v2(pr, stride, cw, chh, x, y);
    }
    // jdcolor.c: 16-bit scaled constants, the two chroma terms of green summed before the shift
    cb -= 128;
    cr -= 128;
    const int r = lum + ((91881 * cr + 32768) >> 16);
    const int gg = lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int bl = lum + ((116130 * cb + 32768) >> 16);
    out[i] = clamp8(r) | (clamp8(gg) << 8) | (clamp8(bl) << 16) | 0xff000000u;
}

bool plan(int H, int W, int n_comp, int hs, int vs, JpegPlanes& g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return false;
    if (n_comp == 1) {
        if (hs != 1 || vs != 1) return false;
    } else if (n_comp == 3) {
        if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    } else {
        return false;
    }
    const int mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * vs - 1) / (8 * vs);
    g.n_comp = n_comp;
    int64_t at = 0;
    g.blocks = 0;
    for (int c = 0; c < 3; ++c) {
        const bool used = c < n_comp;
        g.bw[c] = used ? mx * (c == 0 ? hs : 1) : 0;
        g.bh[c] = used ? my * (c == 0 ? vs : 1) : 0;
        g.offset[c] = at;
        at += (int64_t)g.bw[c] * g.bh[c] * 64;
        g.blocks += (int64_t)g.bw[c] * g.bh[c];
    }
    g.image_bytes = at;
    return true;
}

}  // namespace

extern "C" int nerfhip_jpeg_entropy_decode(const uint8_t* scan, int64_t scan_bytes, int n_comp, const int32_t* comp,
                                           const uint8_t* huffman, int huffman_mask, int mcus_x, int mcus_y, int restart_interval,
                                           int16_t* const* coef, const int64_t* coef_blocks) {
    NERFHIP_CHECK_ARG(scan && scan_bytes > 0 && comp && huffman && coef && coef_blocks);
    NERFHIP_CHECK_ARG((n_comp == 1 || n_comp == 3) && mcus_x > 0 && mcus_y > 0 && restart_interval >= 0);
    NERFHIP_CHECK_ARG(mcus_x <= 8192 && mcus_y <= 8192);
    HuffTable tables[8];
    for (int t = 0; t < 8; ++t) {
        if (!((huffman_mask >> t) & 1)) continue;
        if (!build_table(huffman + t * 272, tables[t])) return NERFHIP_E_DATA;
    }
    int h[3], v[3], bw[3];
    const HuffTable* dc[3];
    const HuffTable* ac[3];
    for (int c = 0; c < n_comp; ++c) {
        h[c] = comp[4 * c];
        v[c] = comp[4 * c + 1];
        const int td = comp[4 * c + 2], ta = comp[4 * c + 3];
        NERFHIP_CHECK_ARG(h[c] >= 1 && h[c] <= 2 && v[c] >= 1 && v[c] <= 2 && td >= 0 && td < 4 && ta >= 0 && ta < 4);
        NERFHIP_CHECK_ARG(coef[c]);
        dc[c] = &tables[td];
        ac[c] = &tables[4 + ta];
        if (!dc[c]->present || !ac[c]->present) return NERFHIP_E_DATA;   // the scan names a table the file never defines
        bw[c] = mcus_x * h[c];
        NERFHIP_CHECK_ARG(coef_blocks[c] >= (int64_t)bw[c] * mcus_y * v[c]);
    }
    const uint8_t* p = scan;
    const uint8_t* const end = scan + scan_bytes;
    const int64_t n_mcu = (int64_t)mcus_x * mcus_y;
    const int64_t per_interval = restart_interval > 0 ? restart_interval : n_mcu;
    int expect_rst = 0;
    for (int64_t first = 0; first < n_mcu; first += per_interval) {
        // Inside entropy-coded data 0xff is followed by a stuffed zero or by a marker, so the intervals can be cut apart at the
        // RSTm markers (m counting modulo 8) before any bit is decoded.
        const uint8_t* stop = p;
        while (stop < end && !(stop[0] == 0xff && stop + 1 < end && stop[1] >= 0xd0 && stop[1] <= 0xd7)) ++stop;
        BitReader br(p, stop);
        int pred[3] = {0, 0, 0};
        const int64_t last = first + per_interval < n_mcu ? first + per_interval : n_mcu;
        for (int64_t m = first; m < last; ++m) {
            const int my = (int)(m / mcus_x), mx = (int)(m % mcus_x);
            for (int c = 0; c < n_comp; ++c)
                for (int yy = 0; yy < v[c]; ++yy)
                    for (int xx = 0; xx < h[c]; ++xx) {
                        const int64_t blk = (int64_t)(my * v[c] + yy) * bw[c] + (mx * h[c] + xx);
                        const int e = decode_block(br, *dc[c], *ac[c], pred[c], coef[c] + blk * 64);
                        if (e) return e;
                    }
        }
        if (last < n_mcu) {
            if (stop + 1 >= end || stop[1] != 0xd0 + expect_rst) return NERFHIP_E_DATA;
            p = stop + 2;
            expect_rst = (expect_rst + 1) & 7;
        }
    }
    return 0;
}

extern "C" size_t nerfhip_jpeg_planes_bytes(int H, int W, int n_comp, int hs, int vs) {
    JpegPlanes g;
    return plan(H, W, n_comp, hs, vs, g) ? (size_t)g.image_bytes : 0;
}

extern "C" int nerfhip_jpeg_decode(const int16_t* coef_y, const int16_t* coef_cb, const int16_t* coef_cr, const uint16_t* quant,
                                   uint8_t* planes, uint8_t* out, int n_images, int H, int W, int n_comp, int hs, int vs,
                                   nerfhip_stream_t stream) {
    JpegPlanes g;
    NERFHIP_CHECK_ARG(n_images >= 0 && n_images <= 65535 && plan(H, W, n_comp, hs, vs, g));
    if (n_images == 0) return 0;
    NERFHIP_CHECK_ARG(coef_y && quant && planes && out && (n_comp == 1 || (coef_cb && coef_cr)));
    if ((((uintptr_t)coef_y | (uintptr_t)coef_cb | (uintptr_t)coef_cr | (uintptr_t)quant) & 15) || ((uintptr_t)planes & 7) ||
        ((uintptr_t)out & 3))
        return NERFHIP_E_ALIGN;
    NERFHIP_CHECK_ARG((g.blocks + kDctPerGroup - 1) / kDctPerGroup < ((int64_t)1 << 31));
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct, dim3((unsigned)((g.blocks + kDctPerGroup - 1) / kDctPerGroup), (unsigned)n_images), dim3(kBlock), 0,
                       s, coef_y, coef_cb, coef_cr, quant, planes, g);
    const int64_t n_out = (int64_t)n_images * H * W;
    NERFHIP_CHECK_ARG((n_out + kBlock - 1) / kBlock < ((int64_t)1 << 31));
    const int cw = (W + hs - 1) / hs;
    hipLaunchKernelGGL(jpeg_to_rgbx, dim3((unsigned)((n_out + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, planes, (uint32_t*)out, n_out, H,
                       W, hs, vs, (hs == 2 && cw > 2) ? 1 : 0, g);
    return nerfhip_launch_status();
}

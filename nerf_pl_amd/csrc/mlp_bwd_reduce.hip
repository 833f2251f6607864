// K2b, phases B (end) and C: the partial slabs of the weight-gradient launch become the gradient tensors.
//   mlp_bwd_reduce_kernel sums a job's split slabs, un-permutes features and writes the (out,in) gradient tensors + biases [+ Adam].
//   mlp_bwd_fold_kernel — xyz_encoding_final is a linear layer without activation: its saved input / output gradient are not needed
//   (mlp_layout.h kDwJobs).  The dir job forms G = dY_dir^T h8 instead of dY_dir^T f; this small fp32 kernel finishes
//   dW_dir[:, :256] = G W_f^T + s b_f^T,  dW_final = W_dx^T G,  db_final = W_dx^T s  from G, s = db_dir and the fp32 fold block
//   of the packed W^T image.
#include "mlp_device.h"
#include "adam_math.h"
#include "mlp_bwd_dw.h"

namespace nerfhip {

// one gradient element: written (or accumulated) and, with Adam fused, applied
struct GradEmit {
    const AdamFused& A;
    AdamCoef ac;
    int accumulate, model;
    __device__ __forceinline__ void operator()(float* dst, float val) const {
        const float g = accumulate ? *dst + val : val;
        *dst = g;
        if (A.state) {
            const size_t e = (size_t)(dst - A.grad0[model]);
            adam_elem(A.param[model][e], g, A.m[model][e], A.v[model][e], ac, A.beta2, A.eps, A.wd);
        }
    }
};

// sum split slabs, undo the fragment/feature permutation, write (out,in) row-major gradients [and apply Adam].
// Columns of enc kDwEncFold (the dir job's h8 section) are the G matrix of the folded final layer, the dir job's bias sums its s:
// both also go — plainly — to the model's fold scratch for mlp_bwd_fold_kernel; the final layer's own job has nothing here.
// One 256-thread block per (job, 32x32 tile): thread = one float4 (rows o..o+3 of one column) of the 1024-float
// tile, summed over the job's splits with independent 16-B loads.
// F8: operand rows/columns arrive in the order ds_read_b64_tr_b8 delivers them (m -> slab m >> 4, half (m >> 3) & 1, slot m & 7)
// instead of natural feature order, and the bias partials hold one value per row.
template <bool F8>
__global__ __launch_bounds__(256) void mlp_bwd_reduce_kernel(DwJobTable jobs, const float* __restrict__ slabs, GradTable G,
                                                              float* __restrict__ fold_scratch, int accumulate, AdamFused A) {
    const int jid = blockIdx.y;
    const DwJob jb = jobs.job[jid];
    const int model = jid / kNumDwJobs;
    const int fold = jobs.fold_of[jid];                 // >= 0: this job's partials live in job `fold`'s slabs (blocks dw_fold_block(X tile))
    const int nsplit = jobs.nsplit[fold >= 0 ? fold : jid], s0 = jobs.soff[fold >= 0 ? fold : jid];
    const bool derived = jid % kNumDwJobs == kDwJobFinal;              // finished by mlp_bwd_fold_kernel
    const int n_ot = derived ? 0 : jb.dy_slabs / 2, n_xt = (jb.x1_slabs + jb.x2_slabs) / 2;
    float* const scratch = fold_scratch + (size_t)model * kFoldScratchFloats;
    const int n_out = kParamOut[jb.param], ldw = kParamIn[jb.param];
    const int tile = blockIdx.x;                       // (ot, xt) pairs + one extra block per ot for the bias
    const int ot = tile / (kDwMaxXTiles + 1), xt = tile % (kDwMaxXTiles + 1);
    AdamCoef ac;
    if (A.state) ac = adam_coef(A.state[0] + 1.0f, A.lr, A.beta1, A.beta2);
    const GradEmit emit{A, ac, accumulate, model};
    if (ot < n_ot && xt == kDwMaxXTiles) {             // bias: lanes (m,0) + (m,1)
        const int m = threadIdx.x;
        if (m < 32) {
            float sacc = 0.f;
            for (int sp = 0; sp < nsplit; ++sp) {
                const float* sl = slabs + (size_t)(s0 + sp) * kDwSlabFloats + (size_t)8 * kDwMaxXTiles * 64 * 16 +
                                  (fold >= 0 ? kDwFoldRow0 : ot) * 64;
                sacc += F8 ? sl[m] : sl[m] + sl[m + 32];
            }
            const int o = F8 ? 32 * ot + chain_feature(m >> 4, f8_row_h(m & 15), f8_row_j(m & 15)) : 32 * ot + m;
            if (o < n_out) {
                emit(G.b[jid] + o, sacc);
                if (jid % kNumDwJobs == kDwJobDir) scratch[kFoldS + o] = sacc;
            }
        }
    } else if (ot < n_ot && xt < n_xt) {
        const int e4 = threadIdx.x;                    // float4 e4 of the block (dw_store_block: register-major): lane = e4 & 63, r = 4*(e4>>6)+k
        const float4* src = reinterpret_cast<const float4*>(slabs + (size_t)s0 * kDwSlabFloats +
                                                            ((size_t)(fold >= 0 ? dw_fold_block(xt) : ot * kDwMaxXTiles + xt) * 64) * 16) + e4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
        for (int sp = 0; sp < nsplit; ++sp) {
            const float4 v = src[(size_t)sp * (kDwSlabFloats / 4)];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        const int lane = e4 & 63, rq = e4 >> 6;
        const int h = lane >> 5, ncol = lane & 31;
        const int m0 = 8 * rq + 4 * h;                     // operand rows m0 .. m0+3  (reg r = 4*rq + k -> (r&3) = k, r>>2 = rq)
        // natural order: row m = feature 32 ot + m.  F8: m -> feature chain_feature(m >> 4, (m >> 3) & 1, m & 7) of the tile
        const int o0 = F8 ? 32 * ot + chain_feature(m0 >> 4, f8_row_h(m0 & 15), f8_row_j(m0 & 15)) : 32 * ot + m0;   // k adds to (m & 3)
        const int xi = 32 * xt + ncol;
        int xs = xi >> 4;
        const int i = xi & 15;
        const int sh = F8 ? f8_row_h(i) : slab_nat_h(i), sj = F8 ? f8_row_j(i) : slab_nat_j(i);     // slot (h, j) inside slab xs
        int enc, col0;
        if (xs < jb.x1_slabs) { enc = jb.x1_enc; col0 = jb.x1_col0; }
        else { xs -= jb.x1_slabs; enc = jb.x2_enc; col0 = jb.x2_col0; }
        int col;
        if (enc == 0 || enc == kDwEncFold) col = col0 + chain_feature(xs, sh, sj);
        else {
            const int ch = (enc == 1) ? xyz_slot_channel(xs, sh, sj) : dir_slot_channel(xs, sh, sj);
            col = ch < 0 ? -1 : col0 + ch;
        }
        if (enc == kDwEncFold) {                           // G[o][h8 feature]: this call's sum, never accumulated, never an Adam input
            const float vals[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (o0 + k < n_out) scratch[kFoldG + (size_t)(o0 + k) * kW + col] = vals[k];
        } else if (col >= 0 && col < ldw) {
            const float vals[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int o = o0 + k;
                if (o < n_out) emit(G.w[jid] + (size_t)o * ldw + col, vals[k]);
            }
        }
    }
    if (A.state) {
        // arrival ticket (as adam_kernel): the last workgroup of the launch advances the step counter, after every workgroup
        // that uses it has read the old value
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned* ticket = reinterpret_cast<unsigned*>(A.state + 1);
            const unsigned prev = atomicAdd(ticket, 1u);
            if (prev == gridDim.x * gridDim.y - 1) {
                *ticket = 0u;
                A.state[0] = A.state[0] + 1.0f;
            }
        }
    }
}

constexpr int kFoldBlocks = 32 + 64 + 1;
// Latency, not arithmetic, is what this launch costs (it sits between the reduce and the optimizer): a workgroup fetches BOTH
// operands of its tile whole — one round trip to L2 / HBM — and only then multiplies out of LDS, on the fp32 MFMA
// (v_mfma_f32_32x32x2_f32: an fmaf chain per output, as in the fp32 kernels), each of its 4 waves over a quarter of the inner
// dimension; the four partial tiles are summed in a fixed order.  (First version: 32-deep slices, eight dependent round trips, 15 us
// in the step; second: one round trip and a VALU loop bound by its LDS reads, ~6 us.)
__global__ __launch_bounds__(256) void mlp_bwd_fold_kernel(FoldArgs F, const float* __restrict__ fold_scratch, int accumulate, AdamFused A) {
    constexpr int PA = 257, PB = 33;                      // LDS row pitches (floats): conflict-free reads
    __shared__ float lds[2 * 32 * PA];
    __shared__ float part[4][16][64];
    const int model = blockIdx.y, bx = blockIdx.x, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const float* __restrict__ Gm = fold_scratch + (size_t)model * kFoldScratchFloats + kFoldG;
    const float* __restrict__ sv = fold_scratch + (size_t)model * kFoldScratchFloats + kFoldS;
    const float* __restrict__ Wf = F.image[model] + (size_t)kFoldWf * 256;
    const float* __restrict__ Wdx = F.image[model] + (size_t)kFoldWdx * 256;
    const float* __restrict__ bf = F.image[model] + (size_t)kFoldBf * 256;
    AdamCoef ac;
    if (A.state) ac = adam_coef(A.state[0], A.lr, A.beta1, A.beta2);          // (the reduce launch before this one advanced the counter)
    const GradEmit emit{A, ac, accumulate, model};
    if (bx == kFoldBlocks - 1) {
        // db_final[t] = sum_j W_dx[j][t] s[j]: four partial chains, the loads independent
        float a4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int j = 0; j < 128; j += 4)
#pragma unroll
            for (int q = 0; q < 4; ++q) a4[q] = __builtin_fmaf(Wdx[(size_t)(j + q) * 256 + t], sv[j + q], a4[q]);
        emit(F.gb_final[model] + t, (a4[0] + a4[1]) + (a4[2] + a4[3]));
        return;
    }
    const bool dir = bx < 32;
    // tile origin: dW_dir rows j0.. x columns m0.. | dW_final rows m0.. x columns k0..
    const int row0 = dir ? 32 * (bx >> 3) : 32 * ((bx - 32) >> 3), col0 = dir ? 32 * (bx & 7) : 32 * ((bx - 32) & 7);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int m = lane & 31, kh = lane >> 5;              // MFMA operand lane: row / column m, inner index parity kh
    if (dir) {
        // out[j][c] = sum_k G[j0 + j][k] W_f[m0 + c][k]:  A[j][k] = G rows, B[k][c] = W_f rows; both staged row-major, pitch PA
        float* sa = lds;
        float* sb = lds + 32 * PA;
        float4 va[8], vb[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {                     // row (t >> 6) + 4 i, floats 4 (t & 63) ..
            const int row = (t >> 6) + 4 * i;
            va[i] = reinterpret_cast<const float4*>(Gm + (size_t)(row0 + row) * 256)[t & 63];
            vb[i] = reinterpret_cast<const float4*>(Wf + (size_t)(col0 + row) * 256)[t & 63];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = ((t >> 6) + 4 * i) * PA + 4 * (t & 63);
            sa[o] = va[i].x; sa[o + 1] = va[i].y; sa[o + 2] = va[i].z; sa[o + 3] = va[i].w;
            sb[o] = vb[i].x; sb[o + 1] = vb[i].y; sb[o + 2] = vb[i].z; sb[o + 3] = vb[i].w;
        }
        __syncthreads();
        const float* pa = sa + m * PA + 64 * wave + kh;   // this wave's quarter of k
        const float* pb = sb + m * PA + 64 * wave + kh;
#pragma unroll 8
        for (int k = 0; k < 64; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k], pb[k], acc, 0, 0, 0);
    } else {
        // out[r][c] = sum_j W_dx[j][m0 + r] G[j][k0 + c]:  A[r][j] = W_dx columns, B[j][c] = G rows; staged [j][32], pitch PB
        float* sa = lds;
        float* sb = lds + 128 * PB;
        const int c = t & 31, r0 = t >> 5;
        float va[16], vb[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {                    // row r0 + 8 i (of 128), column c
            va[i] = Wdx[(size_t)(r0 + 8 * i) * 256 + row0 + c];
            vb[i] = Gm[(size_t)(r0 + 8 * i) * 256 + col0 + c];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sa[(r0 + 8 * i) * PB + c] = va[i];
            sb[(r0 + 8 * i) * PB + c] = vb[i];
        }
        __syncthreads();
        const float* pa = sa + (32 * wave + kh) * PB + m; // this wave's quarter of j
        const float* pb = sb + (32 * wave + kh) * PB + m;
#pragma unroll 8
        for (int j = 0; j < 32; j += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[j * PB], pb[j * PB], acc, 0, 0, 0);
    }
    // the four waves' partial tiles, summed in wave order; C/D layout: lane -> column lane & 31, register r -> row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wave][r][lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = wave + 4 * i;
        const float v = ((part[0][r][lane] + part[1][r][lane]) + part[2][r][lane]) + part[3][r][lane];
        const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = col0 + (lane & 31);
        if (dir) emit(F.gw_dir[model] + (size_t)row * kParamIn[9] + col, __builtin_fmaf(sv[row], bf[col], v));
        else emit(F.gw_final[model] + (size_t)row * 256 + col, v);
    }
}

void launch_reduce(bool f8, const DwJobTable& jt, const float* slabs, const GradTable& G, float* fold_scratch, int accumulate,
                   const AdamFused& A, hipStream_t s) {
    const dim3 rgrid(8 * (kDwMaxXTiles + 1), (unsigned)jt.njobs);
    if (f8) hipLaunchKernelGGL(mlp_bwd_reduce_kernel<true>, rgrid, dim3(256), 0, s, jt, slabs, G, fold_scratch, accumulate, A);
    else hipLaunchKernelGGL(mlp_bwd_reduce_kernel<false>, rgrid, dim3(256), 0, s, jt, slabs, G, fold_scratch, accumulate, A);
}
void launch_fold(const FoldArgs& F, const float* fold_scratch, int n_models, int accumulate, const AdamFused& A, hipStream_t s) {
    hipLaunchKernelGGL(mlp_bwd_fold_kernel, dim3(kFoldBlocks, (unsigned)n_models), dim3(256), 0, s, F, fold_scratch, accumulate, A);
}

}  // namespace nerfhip

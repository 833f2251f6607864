// K2b, phase B with fp8 storage (mlp_bwd_dw.hip holds the bf16 / fp32 form of the same launch)
#include "mlp_device.h"
#include "f8_store.h"
#include "mlp_bwd_dw.h"

namespace nerfhip {

#if NERFHIP_DW_PROBE
__device__ unsigned g_dw_f8_probe[1024 * 8 * 8];    // [workgroup][wave][iters, wait, barrier, issue, compute, total, job, depth]
#endif

// ================================================================================================
// Phase B, fp8 storage (NERFHIP_BF16_F8): dW = dY^T X on v_mfma_scale_f32_32x32x64_f8f6f4
// ================================================================================================
// Same decomposition as mlp_bwd_dw_kernel (workgroup = (layer job, point split), wave w = 32 dY features x all X tiles,
// fp32 accumulators in registers), but the operands are the e4m3 slab-pair pieces of mlp_layout.h ("fp8 storage"): one
// 1 KiB piece = 32 points x 32 features, i.e. HALF the bytes per point of the bf16 kernel, and one MFMA consumes K = 64
// points = two wave tiles per iteration.
//   operand fragment of v_mfma_scale_f32_32x32x64_f8f6f4 (measured, tools/probes/probe_fp8.hip): lane (row m = l & 31,
//   H = l >> 5) holds 32 bytes; bytes 0..15 belong to K block 0, bytes 16..31 to K block 1 (for both lane halves); the
//   scale operand of lanes 0..31 scales block 0 of row m, that of lanes 32..63 block 1.
//   => block 0 = tile T0, block 1 = tile T1 of the iteration; lane half H supplies points 16H .. 16H+15 of each.
//   ds_read_b64_tr_b8 (measured): within a 16-lane group, result lane c (column c & 7, row parity c >> 3) byte b = byte
//   (c & 7) of the 8-byte chunk addressed by source lane 2b + (c >> 3).  Source lane r therefore points at the chunk of
//   (point 8g + (r >> 1), half r & 1) and the group's 16 result lanes become the 16 features (h = c >> 3, j = c & 7) of one
//   slab with 8 consecutive points in their bytes.
// LDS image of a piece: 16-byte unit u = 16 g + 8 h + (n & 7) <- global unit (lane) 32 h + n, n = 8 g + (n & 7): the 32
// lanes of one ds_read pass (2 slabs x 8 points x 2 halves) cover one aligned 256-byte block => conflict free.
struct DwF8Job {
    int dy_pair0, dy_pairs, dy_pos0;               // pieces / scale-table index of the dY section
    int x1_pair0, x1_pairs, x1_pos0;
    int x2_pair0, x2_pairs, x2_pos0;
};

__global__ __launch_bounds__(512, 2)
void mlp_bwd_dw_f8_kernel(DwJobTable jobs, float* __restrict__ slabs) {
    constexpr int DEPTH = 4;                                   // ring stages
    constexpr int MAXP = 36;                                   // pieces per stage: 2 tiles x (8 dY + 10 X) pairs
    constexpr int LPW = 5;                                     // piece DMAs per wave per stage (8 x 5 >= 36)
    constexpr int STAGE_BYTES = MAXP * kPieceBytes;
    constexpr int SCALE_BYTES = 256;                           // per wave per stage: [tile][16 dwords]
    __shared__ __attribute__((aligned(1024))) char ring[DEPTH * STAGE_BYTES + DEPTH * 8 * SCALE_BYTES];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int jid = 0;
#pragma unroll
    for (int j = 1; j < kDwMaxJobs; ++j) jid += ((int)blockIdx.x >= jobs.soff[j]) ? 1 : 0;
    const int nsplit = jobs.nsplit[jid], split = (int)blockIdx.x - jobs.soff[jid];
    const DwJob jb = jobs.job[jid];
    const int64_t ntiles = jobs.ntiles[jid];
    const uint8_t* __restrict__ acts_base = jobs.acts[jid];
    const uint8_t* __restrict__ dys_base = jobs.dys[jid];
    const int dyp = jb.dy_slabs / 2, x1p = jb.x1_slabs / 2, x2p = jb.x2_slabs / 2;
    const int n_ot = dyp, n_xt = x1p + x2p;
    // the dir layer's workgroups also form the sigma head's gradient (same X section h8, read once; see mlp_bwd_dw_kernel): their tile
    // carries the dY_sigma pair as its LAST piece and the section's scale in slot 3 of the wave's scale dwords; the waves 4..7 (the
    // dir layer has 4 dY tiles) multiply it by the h8 tiles 2 (w - 4), 2 (w - 4) + 1
    const bool fold = jobs.fold_of[(jid / kNumDwJobs) * kNumDwJobs + kDwJobSigma] == jid;
    const int np = dyp + n_xt + (fold ? 1 : 0);                // pieces per tile
    const int dy_pair0 = jb.dy_off / 2, x1_pair0 = jb.x1_off / 2, x2_pair0 = jb.x2_off / 2;
    // tile PAIRS per split (K = 64 points per MFMA); ntiles is a multiple of 8
    const int64_t npairs = ntiles / 2;
    const int64_t per = (npairs + nsplit - 1) / nsplit;
    const int64_t p_first = (int64_t)split * per;
    const int64_t my_pairs = (p_first >= npairs) ? 0 : ((npairs - p_first < per) ? npairs - p_first : per);
    const unsigned lds_base = (unsigned)(uintptr_t)ring;
    const unsigned lds_scales = lds_base + (unsigned)(DEPTH * STAGE_BYTES);

    // DMA source unit of LDS unit `lane` (see the header comment): global lane 32 h + 8 g + (n & 7)
    const int dma_unit = ((lane >> 3) & 1) * 32 + 8 * (lane >> 4) + (lane & 7);
    // scale DMA: lane i < 32 -> (tile i >> 4, slot i & 15) lands at dword i of the wave's scale area: slot 0 = the dY
    // section's scale, slot 1 = the x1 section's, slots >= 2 = the x2 section's (x1's when there is no x2)
    const int s_tile = (lane >> 4) & 1, s_slot = lane & 15;
    const bool s_sigma = fold && s_slot == 3;
    const int s_from_dy = s_slot == 0 || s_sigma;
    const int s_pos = s_sigma ? f8_dy_section(kDySigma)
                              : (s_slot == 0 ? f8_dy_section(jb.dy_off)
                                             : ((s_slot == 1 || x2p == 0) ? f8_x_section(jb.x1_off) : f8_x_section(jb.x2_off)));
    // which piece of a tile pair each of this wave's LPW DMAs fetches does not depend on the stage: (dY or X block, byte offset from
    // the pair's first tile block, LDS offset in the stage) once, ahead of the loop (wave-uniform; the stage loop only adds the pair's
    // two block pointers — the selection used to be a branch ladder per DMA)
    bool p_dy[LPW];
    unsigned p_off[LPW], p_dst[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        int pi = wave + 8 * i;
        if (pi >= 2 * np) pi = 2 * np - 1;                                           // duplicate DMA of the last piece
        const int tl = pi >= np ? 1 : 0, pp = pi - tl * np;
        int pair;
        if (pp < dyp) { p_dy[i] = true; pair = dy_pair0 + pp; }
        else if (fold && pp == np - 1) { p_dy[i] = true; pair = kDySigma / 2; }
        else if (pp < dyp + x1p) { p_dy[i] = false; pair = x1_pair0 + pp - dyp; }
        else { p_dy[i] = false; pair = x2_pair0 + pp - dyp - x1p; }
        p_off[i] = (unsigned)(pair * kPieceBytes + tl * (p_dy[i] ? f8_dy_tile_bytes() : f8_act_tile_bytes()));
        p_dst[i] = (unsigned)(pi * kPieceBytes);
    }
    auto issue_stage = [&](int64_t it) {
        int64_t P = p_first + (it < my_pairs ? it : my_pairs - 1);                   // past the end: re-fetch the last pair
        if (P >= npairs) P = npairs - 1;
        const unsigned slot = lds_base + (unsigned)((it % DEPTH) * STAGE_BYTES);
        const uint8_t* dyb = dys_base + (size_t)(2 * P) * f8_dy_tile_bytes();
        const uint8_t* acb = acts_base + (size_t)(2 * P) * f8_act_tile_bytes();
#pragma unroll
        for (int i = 0; i < LPW; ++i)
            glds16_nt((p_dy[i] ? dyb : acb) + p_off[i] + dma_unit * 16, slot + p_dst[i]);
        {
            const uint8_t* src = s_from_dy ? dyb + (size_t)s_tile * f8_dy_tile_bytes() + f8_dy_scale_off()
                                           : acb + (size_t)s_tile * f8_act_tile_bytes() + f8_act_scale_off();
            glds4(src + 4 * s_pos, lds_scales + (unsigned)(((it % DEPTH) * 8 + wave) * SCALE_BYTES));
        }
    };

    f32x16 acc[kDwMaxXTiles];
    f32x16 accb;
#pragma unroll
    for (int r = 0; r < 16; ++r) accb[r] = 0.0f;
#pragma unroll
    for (int x = 0; x < kDwMaxXTiles; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[x][r] = 0.0f;

#pragma unroll
    for (int s = 0; s < DEPTH - 1; ++s) issue_stage(s);
#if NERFHIP_DW_PROBE
    unsigned pr_wait = 0, pr_bar = 0, pr_issue = 0, pr_comp = 0;
    const uint64_t pr_t00 = __builtin_amdgcn_s_memrealtime();
#endif

    // per-lane read geometry: H = lane >> 5 (points 16H..16H+15 of each tile), s = slab of the pair, r = source row
    const int H = lane >> 5, sl = (lane >> 4) & 1, r = lane & 15;
    const int rd_off = ((2 * H) * 16 + (r & 1) * 8 + (r >> 1)) * 16 + sl * 8;        // read q: + (q & 1) * 256, tile (q >> 1): + np KiB
    const int tile1 = np * kPieceBytes;
    i32x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = 0x38383838;                                 // e4m3 1.0

    // The iteration loop exists once per X-tile count of the jobs (2 first layer, 4 rgb head, 8 the 256 x 256 layers and the sigma
    // head, 9 dir layer, 10 skip layer), chosen by ONE wave-uniform switch outside it: with n_xt a compile-time constant the X
    // loop is straight-line code, the next tile's four transposing LDS reads are in flight while the current tile's MFMA issues,
    // and the compiler schedules across tiles.  (With the runtime guard `if (x < n_xt)` every tile was a branch target of its own:
    // 4 ds_read -> s_waitcnt lgkmcnt(0) -> MFMA, ten times per iteration in the same registers — the kernel was bound by ten
    // exposed LDS round trips per ring stage, not by HBM: "a workgroup's time follows its iteration count, not its bytes".)
    auto run = [&](auto nxt_c, auto fold_c) {
        constexpr int NXT = decltype(nxt_c)::value;
        constexpr bool FOLD = decltype(fold_c)::value;
        for (int64_t it = 0; it < my_pairs; ++it) {
            // stage `it` landed (DEPTH-2 younger stages of LPW + 1 DMAs may still fly), everyone done with stage it-1
#if NERFHIP_DW_PROBE
            const unsigned t0 = shader_cycles();
            wait_vm<(DEPTH - 2) * (LPW + 1)>();
            const unsigned t1 = shader_cycles();
            asm volatile("s_barrier" ::: "memory");
            const unsigned t2 = shader_cycles();
            pr_wait += t1 - t0;
            pr_bar += t2 - t1;
#else
            wait_vm_barrier<(DEPTH - 2) * (LPW + 1)>();
#endif
            issue_stage(it + DEPTH - 1);
#if NERFHIP_DW_PROBE
            const unsigned t3 = shader_cycles();
            pr_issue += t3 - t2;
#endif
            if (wave < n_ot) {
                const char* st_base = ring + (it % DEPTH) * STAGE_BYTES + rd_off;
                const char* sc_base = ring + DEPTH * STAGE_BYTES + ((it % DEPTH) * 8 + wave) * SCALE_BYTES + H * 64;
                auto load_frag = [&](const char* pb) {
                    i32x8 f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                            (__attribute__((address_space(3))) i32x2*)(pb + (q >> 1) * tile1 + (q & 1) * 256));
                        f[2 * q] = v[0];
                        f[2 * q + 1] = v[1];
                    }
                    return f;
                };
                const char* x_base = st_base + dyp * kPieceBytes;
                // software pipeline, pinned with sched_barriers (left alone, hipcc sinks every tile's reads back to just before
                // its MFMA: one exposed LDS round trip per tile): the reads of tiles x + 1 and x + 2 are in flight when MFMA x issues
                constexpr int RD = 3;
                const i32x8 a = load_frag(st_base + wave * kPieceBytes);
                const int sa = *reinterpret_cast<const int*>(sc_base);
                const int sx1 = *reinterpret_cast<const int*>(sc_base + 4), sx2 = *reinterpret_cast<const int*>(sc_base + 8);
                i32x8 b[RD];
                b[0] = load_frag(x_base);
                if (NXT > 1) b[1] = load_frag(x_base + kPieceBytes);
                __builtin_amdgcn_sched_barrier(0);
                accb = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, ones, accb, kDyMfmaFormat, 0, 0, sa, 0, 127);   // bias: dY x 1.0
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int x = 0; x < NXT; ++x) {
                    if (x + 2 < NXT) b[(x + 2) % RD] = load_frag(x_base + (x + 2) * kPieceBytes);
                    __builtin_amdgcn_sched_barrier(0);
                    // A = dY: e5m2 (cbsz 1), B = X: e4m3 (blgp 0); lanes 0..31 carry tile T0's section scales, lanes 32..63 T1's
                    acc[x] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b[x % RD], acc[x], kDyMfmaFormat, 0, 0, sa, 0, x < x1p ? sx1 : sx2);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else if constexpr (FOLD) {
                // the folded sigma head: dY_sigma pair (the tile's last piece) x X pieces 1 + 2 (w - 4), 2 + 2 (w - 4) of the stage (piece
                // 0 is enc_dir) into acc[0], acc[1]; wave 4 also forms the bias partial (dY_sigma x 1.0)
                const char* st_base = ring + (it % DEPTH) * STAGE_BYTES + rd_off;
                const char* sc_base = ring + DEPTH * STAGE_BYTES + ((it % DEPTH) * 8 + wave) * SCALE_BYTES + H * 64;
                auto load_frag = [&](const char* pb) {
                    i32x8 f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                            (__attribute__((address_space(3))) i32x2*)(pb + (q >> 1) * tile1 + (q & 1) * 256));
                        f[2 * q] = v[0];
                        f[2 * q + 1] = v[1];
                    }
                    return f;
                };
                const char* xs = st_base + (dyp + 1 + 2 * (wave - kDwFoldRow0)) * kPieceBytes;
                const i32x8 a_sg = load_frag(st_base + (np - 1) * kPieceBytes);
                const i32x8 b0 = load_frag(xs), b1 = load_frag(xs + kPieceBytes);
                const int sa_sg = *reinterpret_cast<const int*>(sc_base + 12), sx2 = *reinterpret_cast<const int*>(sc_base + 8);
                acc[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a_sg, b0, acc[0], kDyMfmaFormat, 0, 0, sa_sg, 0, sx2);
                acc[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a_sg, b1, acc[1], kDyMfmaFormat, 0, 0, sa_sg, 0, sx2);
                if (wave == kDwFoldRow0)
                    accb = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a_sg, ones, accb, kDyMfmaFormat, 0, 0, sa_sg, 0, 127);
            }
#if NERFHIP_DW_PROBE
            pr_comp += shader_cycles() - t3;
#endif
        }
    };
    switch (n_xt) {
        case 2: run(std::integral_constant<int, 2>{}, std::false_type{}); break;
        case 4: run(std::integral_constant<int, 4>{}, std::false_type{}); break;
        case 8: run(std::integral_constant<int, 8>{}, std::false_type{}); break;
        case 9:
            if (fold) run(std::integral_constant<int, 9>{}, std::true_type{});       // dir layer + folded sigma head
            else run(std::integral_constant<int, 9>{}, std::false_type{});
            break;
        default: run(std::integral_constant<int, 10>{}, std::false_type{}); break;          // 10 = kDwMaxXTiles (the skip layer)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // drain the look-ahead DMAs before exit

    if (wave < n_ot) {
        float* slb = slabs + (size_t)blockIdx.x * kDwSlabFloats;
#pragma unroll
        for (int x = 0; x < kDwMaxXTiles; ++x) {
            if (x < n_xt) dw_store_block(slb + (size_t)(wave * kDwMaxXTiles + x) * 1024, acc[x], lane);
        }
        // bias partials: every column of accb equals sum_p dY[p][row]; lanes 0 and 32 hold column 0 (rows 4H + (r&3) + 8(r>>2))
        if ((lane & 31) == 0) {
            float* bdst = slb + 8 * kDwMaxXTiles * 64 * 16 + wave * 64;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) bdst[(rr & 3) + 8 * (rr >> 2) + 4 * H] = accb[rr];
        }
    } else if (fold) {                           // the sigma head's partials: blocks dw_fold_block(2 (w - 4)), (.. + 1); bias row kDwFoldRow0
        float* slb = slabs + (size_t)blockIdx.x * kDwSlabFloats;
        dw_store_block(slb + (size_t)dw_fold_block(2 * (wave - kDwFoldRow0)) * 1024, acc[0], lane);
        dw_store_block(slb + (size_t)dw_fold_block(2 * (wave - kDwFoldRow0) + 1) * 1024, acc[1], lane);
        if (wave == kDwFoldRow0 && (lane & 31) == 0) {
            float* bdst = slb + 8 * kDwMaxXTiles * 64 * 16 + kDwFoldRow0 * 64;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) bdst[(rr & 3) + 8 * (rr >> 2) + 4 * H] = accb[rr];
        }
    }
#if NERFHIP_DW_PROBE
    if (lane == 0 && blockIdx.x < 1024) {
        unsigned* pr = g_dw_f8_probe + ((size_t)blockIdx.x * 8 + wave) * 8;
        pr[0] = (unsigned)my_pairs; pr[1] = pr_wait; pr[2] = pr_bar; pr[3] = pr_issue; pr[4] = pr_comp;
        pr[5] = (unsigned)(__builtin_amdgcn_s_memrealtime() - pr_t00);        // 100 MHz ticks
        pr[6] = (unsigned)jid; pr[7] = DEPTH;
    }
#endif
}

void launch_dw_f8(const DwJobTable& jt, float* slabs, int nwg, hipStream_t s) {
    hipLaunchKernelGGL(mlp_bwd_dw_f8_kernel, dim3(nwg), dim3(512), 0, s, jt, slabs);
}
#if NERFHIP_DW_PROBE
int read_dw_f8_probe(unsigned* host_dst, int n_words) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_dw_f8_probe), (size_t)n_words * 4, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
}
#endif

}  // namespace nerfhip

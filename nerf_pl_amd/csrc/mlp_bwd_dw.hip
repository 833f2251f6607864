// K2b, phase B: the weight gradients of the fused NeRF MLP, bf16 / fp32 operands (e4m3 / e5m2 storage: mlp_bwd_dw_f8.hip).
//     dW_l = dY_l^T X_l with the POINTS as the MFMA K dimension.  dY/X tiles are DMA'd global->LDS in fragment order (lane-linear, no
//     address math) and transposed on the fly by ds_read_b64_tr_b16 (bf16) so that lane = feature, regs = points; fp32 gathers with
//     ds_read_b32.  A workgroup owns one (layer, point-range) job (the host's plan: mlp_dw_plan.h): wave w = output tile w against all
//     X tiles, fp32 accumulators in registers for the whole range, one partial slab per workgroup; mlp_bwd_reduce_kernel
//     (mlp_bwd_reduce.hip) sums the slabs.  HBM-bound by construction: 2*256*256 FLOP per 2*256*2 B = 128 FLOP/B.
#include "mlp_device.h"
#include "mlp_bwd_dw.h"

namespace nerfhip {

#if NERFHIP_DW_PROBE
__device__ unsigned g_dw_probe[1024 * 8 * 8];       // [workgroup][wave][iters, wait, barrier, issue, compute, total, job, depth]
#endif

// bf16 dW ring: the whole LDS of a CU, cut into as many stages as the JOB's stage size allows, at most kDwMaxDepth (round 4; the depth
// itself measured neutral — 4 stages of 36 KiB run the same 480 us — the waves never wait for data)
constexpr int kDwRingKiB = 160, kDwMaxDepth = 12;
// bf16: B fragments in flight (ring of RD, RD - 1 steps ahead of the MFMA): one dY tile per wave | the 2-D wave split (SPLIT2D below)
constexpr int kDwFragRing = 5, kDwFragRing2D = 4;

template <int PREC> struct DwTraits;
template <> struct DwTraits<NERFHIP_BF16> {
    static constexpr int SPP = 1;            // 1 KiB pieces per slab
    static constexpr int RING_BYTES = kDwRingKiB * 1024;      // cut into stages of the job class's own size (dw_depth)
    static constexpr int DEPTH = 0, STAGE_BYTES = 0;                  // (fp32 only: a fixed 2 x 72 KiB ring)
};
template <> struct DwTraits<NERFHIP_F32> {
    static constexpr int SPP = 2;
    static constexpr int DEPTH = 2;
    static constexpr int MAXP = 72;
    static constexpr int STAGE_BYTES = MAXP * kPieceBytes;
    static constexpr int RING_BYTES = DEPTH * STAGE_BYTES;
};

// ring stages of a job class whose stage is `pieces` KiB
template <int PREC> NH_HD constexpr int dw_depth(int pieces) {
    if (PREC != NERFHIP_BF16) return DwTraits<PREC>::DEPTH;
    const int d = DwTraits<PREC>::RING_BYTES / (pieces * kPieceBytes);
    return d > kDwMaxDepth ? kDwMaxDepth : d;
}

// sum of a bf16 A fragment's 8 values into two running fp32 partials (the bias gradient: dY summed over the points): v_dot2_f32_bf16
// against (1, 1), two chains, instead of 8 dependent cvt + add per fragment
__device__ __forceinline__ void dw_bias_sum(const bf16x8& a, float& s0, float& s1) {
    const bf16x2 one = {(__bf16)1.0f, (__bf16)1.0f};
    s0 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2{a[0], a[1]}, one, s0, false);
    s1 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2{a[2], a[3]}, one, s1, false);
    s0 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2{a[4], a[5]}, one, s0, false);
    s1 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2{a[6], a[7]}, one, s1, false);
}

// Slab `ks` (wave-uniform) of the F-frequency encoding of v in the forward's slot order — the arithmetic of the bf16 forward's
// encode_slots (mlp_fwd_kernel.h, the hardware-sincos path: x / 2 pi as a hi + lo pair, exact power-of-two scaling, v_fract, hardware
// v_sin / v_cos in revolutions), operation for operation, so that the regenerated operand has the bits the forward multiplied by:
// pair p = 4 ks + q is channel p % 3 at frequency 2^(2 (p / 3) + h); the slots behind the last pair hold the identity channels.
template <int F, int SLABS>
__device__ __forceinline__ bf16x8 dw_encode_slab(const float (&v)[3], int h, int ks) {
    constexpr int NPAIR = 3 * (F / 2);
    constexpr float kInv2PiHi = 0.15915494f, kInv2PiLo = 6.4206297e-9f;
    float rh[3], rl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float vs = h ? 2.0f * v[c] : v[c];
        rh[c] = vs * kInv2PiHi;
        rl[c] = __builtin_fmaf(vs, kInv2PiHi, -rh[c]) + vs * kInv2PiLo;
    }
    bf16x8 out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = 4 * ks + q;
        float s, co;
        if (p < NPAIR) {
            const int i = p / 3, c = p - 3 * i;
            const float sc = (float)(1 << (2 * i));
            const float rhc = c == 0 ? rh[0] : (c == 1 ? rh[1] : rh[2]), rlc = c == 0 ? rl[0] : (c == 1 ? rl[1] : rl[2]);
            const float t = __builtin_amdgcn_fractf(rhc * sc) + rlc * sc;
            s = __builtin_amdgcn_sinf(t);
            co = __builtin_amdgcn_cosf(t);
        } else {
            const int tail = 2 * (p - NPAIR);
            s = (tail == 0) ? (h ? v[2] : v[0]) : 0.0f;
            co = (tail == 0) ? (h ? 0.0f : v[1]) : 0.0f;
        }
        out[2 * q] = (__bf16)s;
        out[2 * q + 1] = (__bf16)co;
    }
    return out;
}

template <int PREC>
__global__ __launch_bounds__(512, 2)
void mlp_bwd_dw_kernel(DwJobTable jobs, float* __restrict__ slabs) {
    constexpr int SPP = DwTraits<PREC>::SPP;
    constexpr int SLAB_BYTES = SPP * kPieceBytes;
    constexpr int IL = act_il(PREC);
    // The ring is sized in BYTES, not stages (round 4): a stage of a job is its own (dY + X slabs) KiB, and the ring holds as many
    // of them as fit — bf16: 4 for the skip layer (36 KiB), 5 for the 256 x 256 layers, 6 / 8 / 8 / 12 for the dir / first / sigma /
    // rgb jobs.  Job class = (X tiles, slabs per stage): the iteration loop exists once per class, so the stage count, the DMAs
    // per wave and the counted vmcnt of its wait are compile-time constants.
    constexpr int RING_BYTES = DwTraits<PREC>::RING_BYTES;
    __shared__ __attribute__((aligned(1024))) char ring[RING_BYTES];

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
    [[maybe_unused]] const float* __restrict__ enc_rays = jobs.enc_rays[jid / kNumDwJobs];      // non-null: regenerate the encodings
    [[maybe_unused]] const float* __restrict__ enc_z = jobs.enc_z[jid / kNumDwJobs];
    [[maybe_unused]] const int enc_tpr = jobs.enc_tpr[jid / kNumDwJobs];
    const int n_ot = jb.dy_slabs / 2;
    const int n_xs = jb.x1_slabs + jb.x2_slabs;
    const int n_xt = n_xs / 2;
    // contiguous tile range per split (consecutive iterations stay inside the same 2 MiB pages: a tile block is
    // 167 KiB; the strided assignment touched 2-3 new pages per iteration per workgroup)
    const int64_t per = (ntiles + nsplit - 1) / nsplit;
    const int64_t t_first = (int64_t)split * per;
    const int64_t my_tiles = (t_first >= ntiles) ? 0 : ((ntiles - t_first < per) ? ntiles - t_first : per);
    const unsigned lds_base = (unsigned)(uintptr_t)ring;

    // stage image: [dy slabs][x1 slabs][x2 slabs], each slab SPP 1 KiB pieces at 1 KiB pitch.  The DMA writes
    // LDS lane-linearly (16-B unit L of a piece <- lane L) but each lane chooses WHICH global 16-B unit it
    // fetches: bf16 pieces are stored in HBM as [half h][point n] and land in LDS as unit (2n+h) for even slabs
    // and (2n+h)^8 for odd slabs, so that the 32 lanes of a ds_read_b64_tr_b16 group (4 points x 2 halves x
    // 2 slabs x 2 j-halves) hit 32 distinct bank pairs.  (The linear [h][n] image was 4-way conflicted: the h,
    // slab and k-step strides are all multiples of 256 B.)
    const int dma_off_even = (PREC == NERFHIP_BF16) ? ((lane & 1) * 32 + (lane >> 1)) * 16 : lane * 16;
    const int dma_off_odd = (PREC == NERFHIP_BF16) ? ((lane & 1) * 32 + ((lane ^ 8) >> 1)) * 16 : lane * 16;

    f32x16 acc[kDwMaxXTiles];
#pragma unroll
    for (int x = 0; x < kDwMaxXTiles; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[x][r] = 0.0f;
    float dbacc = 0.0f;
    [[maybe_unused]] float dbacc2 = 0.0f;             // (second chain of the dot2 bias sums)

    // per-lane transposing-read geometry (bf16): 16-lane group g reads a [4 points][16 features] tile whose
    // 8-byte chunks are (point row = c>>2, feature block = c&3) of lane c; feature block b lives in half
    // h=b&1, j-half b>>1 of the slab image  [h][point n][8 x bf16].
    const int grp = lane >> 4, c = lane & 15;
    // image unit of (point n, half h) = (2n + h) ^ (8 * slab parity);  n = 8*(grp>>1) + (c>>2) + 4*s + 16*q
    // (s = second read of the k-step, q = k-step): bit 3 of the unit is s, so odd slabs swap the two reads.
    const int tr_off = (grp & 1) * SLAB_BYTES + (2 * (8 * (grp >> 1) + (c >> 2)) + ((c & 3) & 1)) * 16 + ((c & 3) >> 1) * 8;
    const int tr_s0 = (grp & 1) ? 128 : 0, tr_s1 = 128 - tr_s0;
    [[maybe_unused]] auto load_frag = [&](const char* pb, int q) { return load_frag_tr16(pb, tr_off, tr_s0, tr_s1, q); };
    // fp32 gather geometry: lane (m = l&31, k = l>>5): feature m -> slab m>>4, natural i = m&15 -> (h,j)
    const int m32 = lane & 31, kk = lane >> 5;
    const int f32_off = (m32 >> 4) * SLAB_BYTES + (slab_nat_h(m32 & 15) * 32) * 32 + slab_nat_j(m32 & 15) * 4;
#if NERFHIP_DW_PROBE
    unsigned pr_wait = 0, pr_bar = 0, pr_issue = 0, pr_comp = 0, pr_depth = 0;
    const uint64_t pr_t00 = __builtin_amdgcn_s_memrealtime();
#endif

    // One copy of the iteration loop per job class (X tiles NXT, slabs per stage NSL): straight-line X loop with the next tiles'
    // LDS reads in flight under the current tile's MFMA (see mlp_bwd_dw_f8_kernel), LPW = ceil(pieces / 8) DMAs per wave per stage
    // (the surplus of the last round re-fetches the stage's last piece: every wave issues the SAME count, so one immediate
    // vmcnt serves all), D ring stages.
    auto run = [&](auto nxt_c, auto nsl_c, auto regen_c) {
        constexpr int NXT = decltype(nxt_c)::value, NSL = decltype(nsl_c)::value;
        // REGEN (bf16; classes whose x1 section is an input encoding: first layer, skip layer, dir layer): the ENC encoding slabs of a
        // stage are not fetched — waves 0 .. ENC - 1 form one slab each from the tile's depths (128 B, DMA'd one stage AHEAD of the
        // stage's pieces into a small ring behind the stages) and the ray (scalar loads), and write it where the DMA would have put it
        constexpr bool REGEN = decltype(regen_c)::value;
        static_assert(!REGEN || (PREC == NERFHIP_BF16 && (NXT == 2 || NXT == 9 || NXT == 10)), "classes with an encoding section");
        constexpr int ENC = REGEN ? (NXT == 9 ? kDirSlabs : kXyzSlabs) : 0;
        constexpr int DYS = NXT == 9 ? 8 : 16;                     // (REGEN) dY slabs ahead of the encoding section in the stage image
        // class (9, 28) = the dir layer with the sigma head folded in: stage = [dY_dir 8][enc_dir 2][h8 16][dY_sigma 2] slabs; the
        // waves 4..7 (no dY tile of the dir layer is theirs) multiply dY_sigma by the h8 tiles 2 (w - 4), 2 (w - 4) + 1
        constexpr bool FOLD = NXT == 9 && NSL == kDwFoldStageSlabs;
        // round 6, bf16: the classes with 8 dY tiles and 8 | 10 X tiles — (8, 32), (10, 36): 85 % of the launch's
        // workgroups — give wave (wi = wave >> 1, wj = wave & 1) the dY tiles 2 wi, 2 wi + 1 against the X tiles XW wj .. XW wj + XW - 1
        // (XW = 4 | 5) instead of 1 x (8 | 10): 6 | 7 operand fragments from LDS per k-step instead of 9 | 11
        // (profiles/r06_dw_bisect.txt, variant M)
        constexpr bool SPLIT2D = (PREC == NERFHIP_BF16) && (NXT == 8 || NXT == 10) && (NSL - 2 * NXT >= 16);
        constexpr int NP = NSL * SPP;                              // 1 KiB pieces per stage
        constexpr int NPD = NP - ENC;                              // ... of which are fetched
        constexpr int LPWD = (NPD + 7) / 8;                        // piece DMAs per wave per stage
        constexpr int LPW = LPWD + (REGEN ? 1 : 0);                // + the next stage's depths (every wave: one vmcnt immediate for all)
        constexpr int STAGE = (PREC == NERFHIP_BF16) ? NP * kPieceBytes : DwTraits<PREC>::STAGE_BYTES;
        constexpr int ZSLOT = 256;                                 // bytes of one stage's depths in LDS: 64 lanes x 4 B (lanes 32.. repeat)
        constexpr int D0 = dw_depth<PREC>(NP);
        constexpr int D = (REGEN && D0 * (STAGE + ZSLOT) > RING_BYTES) ? D0 - 1 : D0;
        static_assert(D >= 2 && D * (STAGE + (REGEN ? ZSLOT : 0)) <= RING_BYTES, "ring stages of this job class");
        static_assert((D - 2) * LPW <= 63, "counted vmcnt");
#if NERFHIP_DW_PROBE
        pr_depth = D;
#endif
        int s_issue = 0, s_use = 0;               // ring slots of the next stage to fetch / to consume (wave-uniform, wrap at D)
        // the stage a fetch goes to: tile block pointers + ring slot (wave-uniform), then one DMA per piece
        const uint8_t* abase = nullptr;
        const uint8_t* dbase = nullptr;
        unsigned slot = 0;
        auto stage_tile = [&](int64_t it) {
            int64_t T = t_first + (it < my_tiles ? it : my_tiles - 1);   // past the end: re-fetch
            if (T >= ntiles) T = ntiles - 1;
            return T;
        };
        // (REGEN) depths of stage `st`: ring of D slots behind the stages, slot = st mod D
        const float* zsrc = nullptr;
        unsigned zslot = 0;
        int z_issue = 0, g_slot = 0;
        const unsigned lds_z = lds_base + (unsigned)(D * STAGE);
        auto next_z = [&](int64_t st) {
            zsrc = enc_z + stage_tile(st) * 32 + (lane & 31);
            zslot = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_z + (unsigned)(z_issue * ZSLOT)));
            z_issue = (z_issue + 1 == D) ? 0 : z_issue + 1;
        };
        auto next_stage = [&](int64_t it) {
            const int64_t T = stage_tile(it);
            abase = acts_base + tile_block_off(T, act_tile_bytes(PREC), IL);      // (bf16: the block's pieces are IL KiB apart, mlp_layout.h)
            dbase = dys_base + tile_block_off(T, kDySlabs * 64 * (16 * SPP), IL);
            slot = lds_base + (unsigned)(s_issue * STAGE);
            s_issue = (s_issue + 1 == D) ? 0 : s_issue + 1;
            if constexpr (REGEN) next_z(it + 1);
        };
        // (REGEN) the encoding slab `wave` of stage `st` (ring slot g_slot, depths in z slot g_slot) written into the stage image in the
        // unit order the DMA gives the fetched slabs: (point n, half h) -> unit (2 n + h) ^ (8 x slab parity)
        // The ray (origin, direction) of a stage's tile by SCALAR loads (constant address space, wave-uniform address), fetched one
        // iteration before it is used: a vector load in the loop makes hipcc drain vmcnt — the whole DMA ring — every iteration
        // (measured: the launch 400 -> 600 us), and a scalar load issued where it is needed puts a memory round trip into the
        // iteration of every generating wave, hence — one barrier per stage — of the workgroup (430 us).
        float ray_next[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        auto load_ray = [&](int64_t st) {
            if (wave < ENC) {
                const unsigned r = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)stage_tile(st) / (unsigned)enc_tpr));
                typedef const float __attribute__((address_space(4))) * ConstF;
                const ConstF rp = (ConstF)(uintptr_t)(enc_rays + (size_t)r * 8);
#pragma unroll
                for (int c = 0; c < 6; ++c) ray_next[c] = rp[c];
            }
        };
        auto gen_stage = [&](int64_t st) {
            if (wave < ENC) {
                const int n = lane & 31, h = lane >> 5;
                bf16x8 e;
                if constexpr (NXT == 9) {
                    const float dv[3] = {ray_next[3], ray_next[4], ray_next[5]};
                    e = dw_encode_slab<4, kDirSlabs>(dv, h, wave);
                } else {
                    const float zv = *reinterpret_cast<const float*>(ring + D * STAGE + g_slot * ZSLOT + n * 4);
                    float xv[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) xv[c] = nh_add(ray_next[c], nh_mul(ray_next[3 + c], zv));      // o + d z   rendering.py:206-207
                    e = dw_encode_slab<10, kXyzSlabs>(xv, h, wave);
                }
                const int unit = (2 * n + h) ^ ((wave & 1) ? 8 : 0);
                *reinterpret_cast<bf16x8*>(ring + g_slot * STAGE + (DYS + wave) * SLAB_BYTES + unit * 16) = e;
            }
            g_slot = (g_slot + 1 == D) ? 0 : g_slot + 1;
            load_ray(st + 1);
        };
        // The last of a wave's LPW DMAs per stage: when the stage has REM = NP mod 8 pieces left for it (4 or 2 in the bf16 classes), the
        // 8 waves SHARE them — 8 / REM waves per piece, each fetching its 64 REM / 8 lanes' units under an EXEC mask — instead of
        // 8 - REM waves re-fetching the stage's last piece: every wave still issues the same count (one immediate vmcnt), and no byte
        // is fetched twice (round 4: the re-fetches were up to a quarter of a small job's DMAs, and nt loads do not stay in L2).
        constexpr int REM = NPD % 8;
        constexpr bool SHARE_LAST = (PREC == NERFHIP_BF16) && (REM == 4 || REM == 2);
        const int share_piece = NPD - REM + (SHARE_LAST ? (wave * REM) / 8 : 0);
        const unsigned long long share_mask = REM == 4 ? (0xffffffffull << (32 * (wave & 1))) : (0xffffull << (16 * (wave & 3)));
        auto issue_piece = [&](int i) {
            if constexpr (REGEN) {
                if (i == LPW - 1) {                                             // the NEXT stage's depths
                    glds4(zsrc, zslot);
                    return;
                }
            }
            int pi = wave + 8 * i;
            const bool shared = SHARE_LAST && i == LPWD - 1;
            if (shared) pi = share_piece;
            if (pi >= NPD) pi = NPD - 1;                                        // (classes without sharing) duplicate DMA of the last piece
            if (REGEN && pi >= DYS) pi += ENC;                                  // fetched piece -> piece of the stage image
            const int sl = pi / SPP, sub = pi % SPP;
            const uint8_t* src;
            if (FOLD && sl >= kDwFoldSigmaSlab) src = dbase + (size_t)(kDySigma + sl - kDwFoldSigmaSlab) * 64 * (16 * SPP) * IL;
            else if (sl < jb.dy_slabs) src = dbase + (size_t)(jb.dy_off + sl) * 64 * (16 * SPP) * IL;
            else if (sl < jb.dy_slabs + jb.x1_slabs) src = abase + (size_t)(jb.x1_off + sl - jb.dy_slabs) * 64 * (16 * SPP) * IL;
            else src = abase + (size_t)(jb.x2_off + sl - jb.dy_slabs - jb.x1_slabs) * 64 * (16 * SPP) * IL;
            // fp32: a slab is 64 lanes x 32 B; piece `sub` = lanes' bytes [16*sub, 16*sub+16) is NOT contiguous,
            // so DMA whole 1 KiB lines instead: line q of the slab = lanes 32q..32q+31 (32 B each).
            const uint8_t* g = src + (size_t)sub * kPieceBytes + ((sl & 1) ? dma_off_odd : dma_off_even);
            // (the destination is wave-uniform; said so, because hipcc otherwise shares a VGPR copy of pi x 1 KiB with the source address)
            const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(slot + (unsigned)(pi * kPieceBytes)));
            if (shared) glds16_nt_masked(g, dst, share_mask);
            else glds16_nt(g, dst);
        };
        auto issue_stage = [&](int64_t it) {
            next_stage(it);
#pragma unroll
            for (int i = 0; i < LPW; ++i) issue_piece(i);
        };
        // bf16: the next stage's DMAs are issued one by one BETWEEN the MFMAs of the current stage (round 4).  Issued in one block at
        // the top of the iteration — all 8 waves at once — they are 32-36 KiB through the CU's 64 B/clk texture-address path:
        // tools/dw_probe.py measured 0.35 us of every 1.5 us iteration in that block, 0.27 us at the barrier behind it and no time
        // at all waiting for data.  One DMA every DMA_STEP MFMAs hides the path's back-pressure under the other wave's MFMAs.
        constexpr bool SPREAD = (PREC == NERFHIP_BF16);
        constexpr int DMA_STEP = (2 * NXT) / LPW > 0 ? (2 * NXT) / LPW : 1;
        if constexpr (REGEN) {                    // stage 0's depths lead the queue
            next_z(0);
            glds4(zsrc, zslot);
            load_ray(0);
        }
#pragma unroll
        for (int s = 0; s < D - 1; ++s) issue_stage(s);
        if constexpr (REGEN) {
            wait_vm<(D - 1) * LPW>();             // (this wave's copy of) stage 0's depths landed; every wave fetched the same 128 B
            gen_stage(0);
        }
        for (int64_t it = 0; it < my_tiles; ++it) {
            // stage `it` landed (D-2 younger stages may still fly), everyone done with stage it-1
#if NERFHIP_DW_PROBE
            const unsigned t0 = shader_cycles();
            wait_vm<(PREC == NERFHIP_BF16) ? (D - 2) * LPW : 0>();
            const unsigned t1 = shader_cycles();
            asm volatile("s_barrier" ::: "memory");
            const unsigned t2 = shader_cycles();
            pr_wait += (t1 - t0) & 0xffffffffu;
            pr_bar += (t2 - t1) & 0xffffffffu;
#else
            wait_vm_barrier<(PREC == NERFHIP_BF16) ? (D - 2) * LPW : 0>();
#endif
            if (SPREAD && (SPLIT2D || wave < n_ot)) next_stage(it + D - 1);
            else issue_stage(it + D - 1);
#if NERFHIP_DW_PROBE
            const unsigned t3 = shader_cycles();
            pr_issue += (t3 - t2) & 0xffffffffu;
#endif
            const char* st_base = ring + s_use * STAGE;
            s_use = (s_use + 1 == D) ? 0 : s_use + 1;
            if constexpr (SPLIT2D) {
                constexpr int XW = NXT / 2, NF = 2 * XW, RD = kDwFragRing2D;
                static_assert(RD >= 2 && RD <= NF, "B fragment ring");
                const int wi = wave >> 1, wj = wave & 1;
                const char* dyb = st_base + (4 * wi) * SLAB_BYTES;                       // dY tiles 2 wi, 2 wi + 1
                const char* x_all = st_base + 16 * SLAB_BYTES;
                const char* xb = x_all + (2 * XW * wj) * SLAB_BYTES;                    // X tiles XW wj ..
                // piece k of the next stage is issued behind B step dma_after(k): the LPW DMAs spread evenly over the NF steps
                auto dma_after = [](int k) constexpr { return ((k + 1) * NF) / LPW - 1; };
                bf16x8 a[2][2], b[RD];
                a[0][0] = load_frag(dyb, 0);
                a[0][1] = load_frag(dyb + 2 * SLAB_BYTES, 0);
#pragma unroll
                for (int f = 0; f < RD - 1; ++f) b[f] = load_frag(xb + 2 * (f % XW) * SLAB_BYTES, f / XW);
                a[1][0] = load_frag(dyb, 1);
                a[1][1] = load_frag(dyb + 2 * SLAB_BYTES, 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int f = 0; f < NF; ++f) {        // B step f = (k-step f / XW, X tile f % XW of this wave): two MFMAs
                    if (f + RD - 1 < NF) b[(f + RD - 1) % RD] = load_frag(xb + 2 * ((f + RD - 1) % XW) * SLAB_BYTES, (f + RD - 1) / XW);
                    __builtin_amdgcn_sched_barrier(0);
                    acc[2 * (f % XW)] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f / XW][0], b[f % RD], acc[2 * (f % XW)], 0, 0, 0);
                    acc[2 * (f % XW) + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f / XW][1], b[f % RD], acc[2 * (f % XW) + 1], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (f == 0 || f == XW) {          // bias partial of dY tile 2 wi + wj (its two waves share the pair's two tiles)
                        const bf16x8 ab = wj ? a[f / XW][1] : a[f / XW][0];
                        dw_bias_sum(ab, dbacc, dbacc2);
                    }
                    if constexpr (SPREAD) {
#pragma unroll
                        for (int k = 0; k < LPW; ++k)
                            if (dma_after(k) == f) {
                                issue_piece(k);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                    }
                }
            } else if (wave < n_ot) {
                const char* dy_base = st_base + (2 * wave) * SLAB_BYTES;
                const char* x_base = st_base + jb.dy_slabs * SLAB_BYTES;
                if constexpr (PREC == NERFHIP_BF16) {
                    // The tile's 2 x NXT MFMAs (two 16-point k-steps q, X tiles x) as ONE software pipeline pinned with sched_barriers
                    // (see mlp_bwd_dw_f8_kernel): the transposing reads of step m + RD - 1 are in flight when MFMA m issues, across
                    // the k-step boundary too (round 4: the pipeline used to drain and refill at every k-step — two exposed LDS
                    // round trips per ring stage with both waves of a SIMD in lock-step), and the bias sums (16 VALU per k-step)
                    // sit behind the first MFMAs instead of in front of them.
                    constexpr int RD = kDwFragRing, NM = 2 * NXT;
                    const bf16x8 a0 = load_frag(dy_base, 0);
                    bf16x8 b[RD];
#pragma unroll
                    for (int m = 0; m < RD - 1; ++m)
                        if (m < NM) b[m] = load_frag(x_base + 2 * (m % NXT) * SLAB_BYTES, m / NXT);
                    const bf16x8 a1 = load_frag(dy_base, 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const int x = m % NXT;
                        if (m + RD - 1 < NM) b[(m + RD - 1) % RD] = load_frag(x_base + 2 * ((m + RD - 1) % NXT) * SLAB_BYTES, (m + RD - 1) / NXT);
                        __builtin_amdgcn_sched_barrier(0);
                        acc[x] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(m < NXT ? a0 : a1, b[m % RD], acc[x], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        if (m == 1) dw_bias_sum(a0, dbacc, dbacc2);
                        if (m == NXT + 1 || (NXT == 1 && m == 1)) dw_bias_sum(a1, dbacc, dbacc2);
                        if constexpr (SPREAD) {
                            if (m % DMA_STEP == DMA_STEP - 1 && m / DMA_STEP < LPW) {
                                issue_piece(m / DMA_STEP);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                    if constexpr (SPREAD) {                            // (pieces the MFMA count did not reach)
#pragma unroll
                        for (int i = (2 * NXT) / DMA_STEP; i < LPW; ++i) issue_piece(i);
                    }
                } else {
#pragma unroll 4
                    for (int ks = 0; ks < 16; ++ks) {                  // 2 points per k-step
                        const int pt = 2 * ks + kk;
                        const float a = *reinterpret_cast<const float*>(dy_base + f32_off + pt * 32);
                        dbacc += a;
#pragma unroll
                        for (int x = 0; x < NXT; ++x) {
                            const float b = *reinterpret_cast<const float*>(x_base + 2 * x * SLAB_BYTES + f32_off + pt * 32);
                            acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[x], 0, 0, 0);
                        }
                    }
                }
            } else if constexpr (FOLD) {
                // the folded sigma head: wave w = 4..7, dY_sigma (one tile) x the h8 tiles 2 (w - 4), 2 (w - 4) + 1 = X tiles 1 + .. of
                // the stage (tile 0 is enc_dir) into acc[0], acc[1]; wave 4 also sums dY_sigma for the bias
                const char* sg = st_base + kDwFoldSigmaSlab * SLAB_BYTES;
                const char* xs = st_base + (jb.dy_slabs + 2 * (1 + 2 * (wave - kDwFoldRow0))) * SLAB_BYTES;
                if constexpr (PREC == NERFHIP_BF16) {
                    const bf16x8 a0 = load_frag(sg, 0), b00 = load_frag(xs, 0), b10 = load_frag(xs + 2 * SLAB_BYTES, 0);
                    const bf16x8 a1 = load_frag(sg, 1), b01 = load_frag(xs, 1), b11 = load_frag(xs + 2 * SLAB_BYTES, 1);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b00, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b10, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b01, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b11, acc[1], 0, 0, 0);
                    if (wave == kDwFoldRow0) {
                        dw_bias_sum(a0, dbacc, dbacc2);
                        dw_bias_sum(a1, dbacc, dbacc2);
                    }
                } else {
#pragma unroll 4
                    for (int ks = 0; ks < 16; ++ks) {
                        const int pt = 2 * ks + kk;
                        const float a = *reinterpret_cast<const float*>(sg + f32_off + pt * 32);
                        dbacc += a;
                        const float b0 = *reinterpret_cast<const float*>(xs + f32_off + pt * 32);
                        const float b1 = *reinterpret_cast<const float*>(xs + 2 * SLAB_BYTES + f32_off + pt * 32);
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
                    }
                }
            }
            // (REGEN) the NEXT stage's encoding slabs, behind this stage's MFMAs: its depths came with stage `it`'s pieces (landed at
            // this iteration's wait); the writes are visible to all behind the next barrier (whose wait includes lgkmcnt(0))
            if constexpr (REGEN) gen_stage(it + 1);
#if NERFHIP_DW_PROBE
            pr_comp += (shader_cycles() - t3) & 0xffffffffu;
#endif
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // drain the look-ahead DMAs before exit
        // this workgroup's partial sums: [dY tile][X tile] blocks of 1024 floats (dw_store_block) + one bias row per dY tile
        float* sl = slabs + (size_t)blockIdx.x * kDwSlabFloats;
        dbacc += dbacc2;
        if constexpr (SPLIT2D) {
            constexpr int XW = NXT / 2;
            const int wi = wave >> 1, wj = wave & 1;
#pragma unroll
            for (int xl = 0; xl < XW; ++xl)
#pragma unroll
                for (int d = 0; d < 2; ++d)
                    dw_store_block(sl + (size_t)((2 * wi + d) * kDwMaxXTiles + XW * wj + xl) * 1024, acc[2 * xl + d], lane);
            sl[8 * kDwMaxXTiles * 64 * 16 + (2 * wi + wj) * 64 + lane] = dbacc;
        } else if (wave < n_ot) {
#pragma unroll
            for (int x = 0; x < NXT; ++x) dw_store_block(sl + (size_t)(wave * kDwMaxXTiles + x) * 1024, acc[x], lane);
            sl[8 * kDwMaxXTiles * 64 * 16 + wave * 64 + lane] = dbacc;
        } else if constexpr (FOLD) {             // the sigma head's partials: blocks dw_fold_block(2 (w - 4)), (.. + 1); bias row kDwFoldRow0
            dw_store_block(sl + (size_t)dw_fold_block(2 * (wave - kDwFoldRow0)) * 1024, acc[0], lane);
            dw_store_block(sl + (size_t)dw_fold_block(2 * (wave - kDwFoldRow0) + 1) * 1024, acc[1], lane);
            if (wave == kDwFoldRow0) sl[8 * kDwMaxXTiles * 64 * 16 + kDwFoldRow0 * 64 + lane] = dbacc;
        }
    };
    // job classes of mlp_layout.h kDwJobs: (X tiles, dY + X slabs per stage)
    using std::integral_constant;
    using std::false_type;
    using std::true_type;
    bool regen = false;
    if constexpr (PREC == NERFHIP_BF16) regen = enc_rays != nullptr;         // (host: only with the sigma head folded into the dir job)
    switch (n_xt) {
        case 2:                                                                                        // first layer: 16 + 4
            if constexpr (PREC == NERFHIP_BF16) {
                if (regen) { run(integral_constant<int, 2>{}, integral_constant<int, 20>{}, true_type{}); break; }
            }
            run(integral_constant<int, 2>{}, integral_constant<int, 20>{}, false_type{});
            break;
        case 4: run(integral_constant<int, 4>{}, integral_constant<int, 10>{}, false_type{}); break;   // rgb head: 2 + 8
        case 8:
            if (jb.dy_slabs == 16) run(integral_constant<int, 8>{}, integral_constant<int, 32>{}, false_type{});     // 256 x 256 layers: 16 + 16
            else run(integral_constant<int, 8>{}, integral_constant<int, 18>{}, false_type{});         // sigma head on its own: 2 + 16
            break;
        case 9:
            if (jobs.fold_of[(jid / kNumDwJobs) * kNumDwJobs + kDwJobSigma] == jid) {                  // dir layer + folded sigma head: 8 + 18 + 2
                if constexpr (PREC == NERFHIP_BF16) {
                    if (regen) { run(integral_constant<int, 9>{}, integral_constant<int, kDwFoldStageSlabs>{}, true_type{}); break; }
                }
                run(integral_constant<int, 9>{}, integral_constant<int, kDwFoldStageSlabs>{}, false_type{});
            } else {
                run(integral_constant<int, 9>{}, integral_constant<int, 26>{}, false_type{});          // dir layer: 8 + 18
            }
            break;
        default:                                                                                       // skip layer: 16 + 20 (kDwMaxXTiles)
            if constexpr (PREC == NERFHIP_BF16) {
                if (regen) { run(integral_constant<int, 10>{}, integral_constant<int, 36>{}, true_type{}); break; }
            }
            run(integral_constant<int, 10>{}, integral_constant<int, 36>{}, false_type{});
            break;
    }
#if NERFHIP_DW_PROBE
    if (lane == 0 && blockIdx.x < 1024) {
        unsigned* pr = g_dw_probe + ((size_t)blockIdx.x * 8 + wave) * 8;
        pr[0] = (unsigned)my_tiles; pr[1] = pr_wait; pr[2] = pr_bar; pr[3] = pr_issue; pr[4] = pr_comp;
        pr[5] = (unsigned)(__builtin_amdgcn_s_memrealtime() - pr_t00);        // 100 MHz ticks
        pr[6] = (unsigned)jid; pr[7] = pr_depth;
    }
#endif
}

// every job of mlp_layout.h has one of the kernel's classes (the switch above)
NH_HD constexpr bool dw_job_has_class(const DwJob& j) {
    const int nxt = (j.x1_slabs + j.x2_slabs) / 2, nsl = j.dy_slabs + j.x1_slabs + j.x2_slabs;
    return (nxt == 2 && nsl == 20) || (nxt == 4 && nsl == 10) || (nxt == 8 && ((nsl == 32 && j.dy_slabs == 16) || (nsl == 18 && j.dy_slabs != 16))) ||
           (nxt == 9 && nsl == 26) || (nxt == 10 && nsl == 36);
}
NH_HD constexpr bool dw_jobs_have_classes() {
    for (int j = 0; j < kNumDwJobs; ++j)
        if (!dw_job_has_class(kDwJobs[j])) return false;
    return true;
}
static_assert(dw_jobs_have_classes(), "mlp_bwd_dw_kernel: a weight-gradient job without a compiled job class");

void launch_dw(int prec, const DwJobTable& jt, float* slabs, int nwg, hipStream_t s) {
    if (prec == NERFHIP_BF16) hipLaunchKernelGGL(mlp_bwd_dw_kernel<NERFHIP_BF16>, dim3(nwg), dim3(512), 0, s, jt, slabs);
    else hipLaunchKernelGGL(mlp_bwd_dw_kernel<NERFHIP_F32>, dim3(nwg), dim3(512), 0, s, jt, slabs);
}
#if NERFHIP_DW_PROBE
int read_dw_probe(unsigned* host_dst, int n_words) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_dw_probe), (size_t)n_words * 4, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
}
#endif

}  // namespace nerfhip

// Device code shared by every MLP translation unit (fused forward / render, backward chain, weight gradient, pack, dx, linear):
// vector types, per-precision launch traits, the global -> LDS DMA primitives, counted waits, the LDS weight ring and the slab
// stores.  ONE definition of each: a fix to the ring's vmcnt accounting, to the DMAs' m0 save / restore or to the store-data
// hazard rule is made here.
#pragma once
#include <type_traits>

#include "common.h"
#include "mlp_layout.h"

#ifndef NERFHIP_STREAM_PROBE
#define NERFHIP_STREAM_PROBE 0  // debug builds: the activation-saving forward / the backward chain record the time their waves spend at
#endif                          // the weight ring's s_waitcnt and s_barrier (results of the launch are invalid; tools/stream_probe.py)

namespace nerfhip {
using namespace mlp;

// cache-policy bits of the write-once stores (saved activations, dY): 2 = nt — written once, read by another kernel: -7 %, whole
// training step 1.65 -> 1.51 ms
constexpr int kStoreAux = 2;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((ext_vector_type(8))) int i32x8;

// Slab type and launch geometry of the register-resident kernels (forward, render, backward chain).  bf16: 8 waves (2 per SIMD, 256
// regs each) = 256 points / workgroup: the second wave of a SIMD fills the matrix pipe while the first waits (LDS, chunk barrier) or
// issues its epilogue VALU.  fp32: 4 waves (1 per SIMD, 512 regs; an fp32 slab set is 128 registers).  (Round 1 measured a
// 4-wave/512-register bf16 activation-saving build as bimodal across MI355X boxes — 376 us on some, ~900 us on others, same
// binary — hence 8 waves everywhere.)
template <int PREC> struct PrecTraits;
template <> struct PrecTraits<NERFHIP_BF16> {
    using Slab = bf16x8;                 // 8 input features of one point (4 VGPRs)
    static constexpr int NW = 8, WPS = 2;
};
template <> struct PrecTraits<NERFHIP_F32> {
    using Slab = f32x8;                  // 8 VGPRs
    static constexpr int NW = 4, WPS = 1;
};

__device__ __forceinline__ void make_slab(bf16x8& s, const float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = (__bf16)v[j];
}
__device__ __forceinline__ void make_slab(f32x8& s, const float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = v[j];
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E) — guarantees static register indexing
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// ---- global -> LDS DMA ------------------------------------------------------------------------------------------------------------
// one 16-byte-per-lane global->LDS DMA; LDS destination = wave-uniform `lds_dst` + lane*16; source = wave-uniform base (SGPR pair) +
// per-lane byte offset `voff`
__device__ __forceinline__ void glds16_s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}
// the same from a per-lane address, non-temporal: for streams every byte of which is read once (the dW kernels' dY / X slabs: 508 -> 466 us)
__device__ __forceinline__ void glds16_nt(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}
// the same for the lanes of `mask` only (wave-uniform): the LDS image is lane-linear, so the other lanes' 16-byte units are simply not
// fetched; the instruction still counts once in vmcnt
__device__ __forceinline__ void glds16_nt_masked(const void* gsrc, unsigned lds_dst, unsigned long long mask) {
    unsigned keep;
    unsigned long long keep_exec;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b64 %1, exec\n\ts_mov_b32 m0, %3\n\ts_mov_b64 exec, %4\n\tglobal_load_lds_dwordx4 %2, off nt\n\t"
        "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
        : "=&s"(keep), "=&s"(keep_exec)
        : "v"(gsrc), "s"(lds_dst), "s"(mask)
        : "memory");
}
// 4 bytes per lane, global -> LDS (lane L lands at lds_dst + 4 L)
__device__ __forceinline__ void glds4(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}

// ---- counted waits ----------------------------------------------------------------------------------------------------------------
// s_waitcnt vmcnt(N) [+ s_barrier], N a compile-time constant of the loop it sits in
template <int N>
__device__ __forceinline__ void wait_vm_barrier() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
// the same for an N that straight-line code folds to a constant (the ring's store counts): 0..8, then multiples of 4 up to 48
// (round DOWN = safe: under-counting only over-waits)
template <bool BARRIER>
__device__ __forceinline__ void wait_vm_counted(int n) {
#define NH_WB(N) case N: if constexpr (BARRIER) wait_vm_barrier<N>(); else wait_vm<N>(); break;
    switch (n < 0 ? 0 : (n > 48 ? 48 : (n <= 8 ? n : (n & ~3)))) {
        NH_WB(0) NH_WB(1) NH_WB(2) NH_WB(3) NH_WB(4) NH_WB(5) NH_WB(6) NH_WB(7) NH_WB(8)
        NH_WB(12) NH_WB(16) NH_WB(20) NH_WB(24) NH_WB(28) NH_WB(32) NH_WB(36) NH_WB(40) NH_WB(44) NH_WB(48)
        default: if constexpr (BARRIER) wait_vm_barrier<0>(); else wait_vm<0>(); break;
    }
#undef NH_WB
}

// ---- the LDS weight ring ----------------------------------------------------------------------------------------------------------
// The packed weight stream (A-fragment order, 1 KiB lane-linear pieces) travels global -> LDS through a ring of kSlots x 32 KiB
// chunks shared by the workgroup's NW waves: every wave issues LPW of a chunk's DMAs, one s_barrier per chunk, two chunks always in
// flight (counted vmcnt, never drained to 0).  NCH = chunks of the stream; COUNT_STORES: the kernel also issues vector-memory stores
// (activation-saving forward, backward chain), which vmcnt counts too.
template <int NW_, int NCH_, bool COUNT_STORES>
struct RingStream {
    static constexpr int NW = NW_, NCH = NCH_;
    static constexpr int LPW = kChunkPieces / NW;   // DMA instructions per wave per chunk
    const uint8_t* gsrc;     // the packed stream (wave-uniform: an SGPR base, no per-piece VALU address)
    unsigned voff;           // lane*16, the one constant per-lane VGPR offset of every DMA
    unsigned lds_base;       // LDS byte address of the ring
    int wave;                // wave index in the workgroup (SGPR)
    int pending;             // vector-memory STORE instructions issued since the last boundary (COUNT_STORES).
                             // Straight-line code: the optimiser folds this to a constant at every boundary.
    int pending_prev;        // ... and in the interval before that
#if NERFHIP_STREAM_PROBE
    unsigned pr_wait = 0, pr_bar = 0, pr_n = 0;     // 10 ns ticks at the boundaries' s_waitcnt / s_barrier, boundaries passed
#endif

    __device__ __forceinline__ void issue_piece(int c, int k) const {      // k-th of this wave's LPW pieces of chunk c
        const int piece = wave + k * NW;
        glds16_s(gsrc + ((size_t)c * kChunkPieces + piece) * kPieceBytes, voff,
                 lds_base + (unsigned)((c % kSlots) * kChunkBytes + piece * kPieceBytes));
    }
    __device__ __forceinline__ void issue_chunk(int c) const {
#pragma unroll
        for (int i = 0; i < LPW; ++i) issue_piece(c, i);
    }
    // Called once for EVERY piece index G of the stream, in increasing order, right before piece G is read: the
    // first piece of a chunk is the chunk boundary.  (Measured: spreading the LPW refill DMAs over the chunk and
    // staggering them between the two halves of the workgroup — instead of one burst behind the barrier — is
    // SLOWER: 203 vs 184 us forward, and 3x on the 4-wave SAVE variant; the burst stays.)
    template <int G>
    __device__ __forceinline__ void at_piece() {
        if constexpr (G % kChunkPieces == 0) boundary(G / kChunkPieces);
    }
    // Called by every wave right before the first piece of chunk c is read.
    __device__ __forceinline__ void boundary(int c) {
        // (1) my DMAs for chunk c have landed (chunk c+1's may stay in flight), my LDS reads of chunk c-1
        // have returned; (2) barrier: same holds for every wave => chunk c is readable and the slot of
        // chunk c-1 is free; (3) refill that slot with chunk c+2.
        // vmcnt retires in issue order and counts stores too: the ops younger than chunk c's DMAs are the
        // LPW DMAs of chunk c+1 plus the `pending` activation stores issued since the previous boundary
        // (older stores are waited for as well — harmless).  Under-counting only over-waits.
        if constexpr (COUNT_STORES) {
            // chunk c's DMAs were issued at boundary c-2; younger than them are the stores of the interval before the previous
            // boundary (pending_prev), chunk c+1's DMAs and the stores since the previous boundary (pending) => stores get two
            // chunk intervals to retire before a boundary waits for them
            const int n = (c + 1 < NCH ? LPW : 0) + pending + pending_prev;
            pending_prev = pending;
            pending = 0;
#if NERFHIP_STREAM_PROBE
            const unsigned t0 = (unsigned)__builtin_amdgcn_s_memrealtime();
            wait_vm_counted<false>(n);
            const unsigned t1 = (unsigned)__builtin_amdgcn_s_memrealtime();
            asm volatile("s_barrier" ::: "memory");
            const unsigned t2 = (unsigned)__builtin_amdgcn_s_memrealtime();
            pr_wait += t1 - t0; pr_bar += t2 - t1; pr_n += 1;
#else
            wait_vm_counted<true>(n);
#endif
        } else if (c + 1 < NCH) {
            wait_vm_barrier<LPW>();
        } else {
            wait_vm_barrier<0>();
        }
        if (c + 2 < NCH) issue_chunk(c + 2);
    }
};

// ---- slab stores ------------------------------------------------------------------------------------------------------------------
// One slab of one lane (16 B bf16 / 32 B fp32) through a buffer descriptor, 16 bytes per store, at byte offset `off` (per-lane, 32-bit:
// no 64-bit address VGPR pairs competing with the accumulators); counted in `pending` for the ring's boundaries.
// soffset stays the constant 0 — every wave-uniform offset goes into the descriptor's base or into `off`: with a wave-uniform soffset
// in an SGPR, LLVM's hazard recognizer assumes the ">64-bit store data followed by a VALU write of the data VGPR" hazard cannot occur
// and lets the next VALU instruction overwrite v[d:d+3] right behind the store — on gfx950 that corrupts lanes 12-15 of every 16
// (measured: dY slabs with 0x4000 patterns from the following v_and).  With soffset = 0 the compiler inserts the wait states.
template <typename Slab>
__device__ __forceinline__ void store_slab_b128(int& pending, __amdgpu_buffer_rsrc_t rsrc, const Slab& s, unsigned off) {
    const u32x4* src = reinterpret_cast<const u32x4*>(&s);
#pragma unroll
    for (int q = 0; q < (int)(sizeof(Slab) / 16); ++q) {
        __builtin_amdgcn_raw_buffer_store_b128(src[q], rsrc, off + 16 * q, 0, kStoreAux);
        pending += 1;
    }
}

// ---- weight-gradient kernels (mlp_bwd_dw.hip, mlp_bwd_dw_f8.hip) -----------------------------------------------------------------
// One (dY tile, X tile) block of a workgroup's partial slab: 1024 floats, REGISTER-major since round 6 — float4 q of lane l at
// float4 index 64 q + l, so that every store instruction of the epilogue writes 1 KiB contiguous (lane-major, a lane's 16 floats
// together, made each of them 64 separate 16-byte pieces: profiles/r06_dw_bisect.txt, variants 7 -> F).  mlp_bwd_reduce_kernel
// decodes the same order.
__device__ __forceinline__ void dw_store_block(float* __restrict__ block, const f32x16& a, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        reinterpret_cast<float4*>(block)[64 * q + lane] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
}
// wall clock in 10 ns ticks (s_memrealtime, 100 MHz) — the probe builds' time base
__device__ __forceinline__ unsigned shader_cycles() { return (unsigned)__builtin_amdgcn_s_memrealtime(); }

// Transposing fragment read (bf16): MFMA operand fragment of k-step q from a slab-pair image at `pb` — two ds_read_b64_tr_b16
// (per-lane geometry tr_off, tr_s0 / tr_s1: mlp_bwd_dw_kernel) turn [point][feature] into lane = feature, registers = points
__device__ __forceinline__ bf16x8 load_frag_tr16(const char* pb, int tr_off, int tr_s0, int tr_s1, int q) {
    union { s16x4 h2[2]; bf16x8 v; } f;
    f.h2[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(pb + tr_off + q * 512 + tr_s0));
    f.h2[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(pb + tr_off + q * 512 + tr_s1));
    return f.v;
}

}  // namespace nerfhip

// K2b: backward of the fused NeRF MLP (autograd mirror of reference models/nerf.py:100-124 as driven by
// train.py:103-117 `loss.backward()`) — the C ABI.  The kernels, one translation unit each, behind their launchers:
//
//  A  mlp_bwd_chain.hip  — per 32-point wave tile, the same register-resident chain as the forward, run in
//     reverse with W^T streamed through the LDS ring:  g_h(l-1) = W_l^T g_a(l),  g_a = g_h * relu'(h)
//     (masks read from the activations the forward saved).  Emits every dL/d(pre-activation) as slabs in
//     the forward's fragment order.  MFMA-bound, ~0.93x the forward's MFMA count.
//  B  mlp_bwd_dw.hip / mlp_bwd_dw_f8.hip — dW_l = dY_l^T X_l with the POINTS as the MFMA K dimension; a workgroup owns one
//     (layer, point-range) job of the split plan (mlp_dw_plan.h) and leaves one partial slab; mlp_bwd_reduce.hip sums the
//     slabs, un-permutes features and writes the (out,in) gradient tensors + biases.
//  C  mlp_bwd_reduce.hip mlp_bwd_fold_kernel — finishes the folded final layer's gradients from the dir job's G.
#include "common.h"
#include "mlp_layout.h"
#include "mlp_bwd_chain.h"
#include "mlp_bwd_dw.h"
#include "mlp_dw_plan.h"

static_assert(kPlanF32 == NERFHIP_F32 && kPlanBf16 == NERFHIP_BF16 && kPlanBf16F8 == NERFHIP_BF16_F8, "mlp_dw_plan.h dtype codes");
static inline bool valid_dtype(int dtype) { return dtype == NERFHIP_F32 || dtype == NERFHIP_BF16 || dtype == NERFHIP_BF16_F8; }
static inline int compute_prec(int dtype) { return dtype == NERFHIP_F32 ? NERFHIP_F32 : NERFHIP_BF16; }
#if NERFHIP_DW_PROBE
static bool g_probe_f8 = false;      // which dW kernel the last launch ran (nerfhip_debug_dw_probe reads that one's accounts)
#endif

extern "C" size_t nerfhip_mlp_dy_bytes(int64_t n_points, int dtype) {
    if (n_points < 0 || !valid_dtype(dtype)) return 0;
    if (dtype == NERFHIP_BF16_F8) return (size_t)act_tiles(n_points, dtype) * nerfhip::mlp::f8_dy_tile_bytes();
    return (size_t)act_tiles(n_points, dtype) * nerfhip::mlp::kDySlabs * 64 * (dtype == NERFHIP_BF16 ? 16 : 32);
}

extern "C" int nerfhip_mlp_dw_splits(int64_t n_points, int dtype) {      // total (job, split) workgroups / partial slabs
    if (n_points <= 0 || !valid_dtype(dtype)) return 0;
    return dw_plan(&n_points, 1, dtype, nullptr);
}
// workspace = the launch's partial slabs, then one fold scratch (G, s) per model
static size_t dw_workspace_bytes(int nwg, int n_models) {
    return ((size_t)nwg * nerfhip::mlp::kDwSlabFloats + (size_t)n_models * nerfhip::mlp::kFoldScratchFloats) * sizeof(float);
}
extern "C" size_t nerfhip_mlp_dw_workspace_bytes(int64_t n_points, int dtype) {
    const int nwg = nerfhip_mlp_dw_splits(n_points, dtype);
    return nwg > 0 ? dw_workspace_bytes(nwg, 1) : 0;
}
extern "C" size_t nerfhip_mlp_dw_workspace_bytes_multi(const int64_t* n_points_host, int n_models, int dtype) {
    if (!n_points_host || n_models < 1 || n_models > nerfhip::kDwMaxModels || !valid_dtype(dtype)) return 0;
    for (int m = 0; m < n_models; ++m)
        if (n_points_host[m] <= 0) return 0;
    return dw_workspace_bytes(dw_plan(n_points_host, n_models, dtype, nullptr), n_models);
}

// The split plan itself (host logic, no GPU): splits_out[12 m + j] = workgroups of weight-gradient job j of model m, stage_kib_out
// (NULL ok) = KiB one ring iteration of that job moves.  Returns the number of workgroups.
extern "C" int nerfhip_mlp_dw_plan(const int64_t* n_points_host, int n_models, int dtype, int* splits_out, int* stage_kib_out) {
    if (!n_points_host || !splits_out || n_models < 1 || n_models > nerfhip::kDwMaxModels || !valid_dtype(dtype)) return NERFHIP_E_BADARG;
    for (int m = 0; m < n_models; ++m)
        if (n_points_host[m] <= 0) return NERFHIP_E_BADARG;
    nerfhip::DwJobTable jt;
    const int total = dw_plan(n_points_host, n_models, dtype, &jt);
    for (int j = 0; j < n_models * nerfhip::mlp::kNumDwJobs; ++j) {
        splits_out[j] = jt.nsplit[j];
        if (stage_kib_out) {
            int slabs = jt.job[j].dy_slabs + jt.job[j].x1_slabs + jt.job[j].x2_slabs;
            if (jt.fold_of[j] >= 0 || jt.nsplit[j] == 0) slabs = 0;                   // folded into another job's stage / derived
            for (int k = 0; k < n_models * nerfhip::mlp::kNumDwJobs; ++k)
                if (jt.fold_of[k] == j) slabs += jt.job[k].dy_slabs;
            stage_kib_out[j] = dtype == NERFHIP_F32 ? 2 * slabs : slabs;            // (the e4m3 kernel moves TWO tiles of slabs / 2 KiB each)
        }
    }
    return total;
}

extern "C" int nerfhip_mlp_bwd_multi(int n_models, const float* const* g_out_host, const float* const* out_host,
                                     const int64_t* n_host, const void* const* packed_bwd_host, const void* const* acts_host,
                                     void* const* dys_host, void* dw_workspace, float* const* grad_w_host,
                                     float* const* grad_b_host, int accumulate, int dtype, int phases, const float* g_scale,
                                     const nerfhip_adam_fused* adam, nerfhip_stream_t stream) {
    return nerfhip_mlp_bwd_multi_rays(n_models, g_out_host, out_host, n_host, packed_bwd_host, acts_host, dys_host, dw_workspace, grad_w_host,
                                      grad_b_host, accumulate, dtype, phases, g_scale, adam, nullptr, stream);
}

extern "C" int nerfhip_mlp_bwd_multi_rays(int n_models, const float* const* g_out_host, const float* const* out_host,
                                          const int64_t* n_host, const void* const* packed_bwd_host, const void* const* acts_host,
                                          void* const* dys_host, void* dw_workspace, float* const* grad_w_host,
                                          float* const* grad_b_host, int accumulate, int dtype, int phases, const float* g_scale,
                                          const nerfhip_adam_fused* adam, const nerfhip_enc_source* enc, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n_models >= 1 && n_models <= nerfhip::kDwMaxModels);
    if (!valid_dtype(dtype)) return NERFHIP_E_UNSUPPORTED;
    bool regen[nerfhip::kDwMaxModels] = {false, false};      // (kernel arguments only: the plan below is the size query's)
    if (enc) {
        // the encodings are formed in the bf16 weight-gradient kernel only
        if (dtype != NERFHIP_BF16) return NERFHIP_E_UNSUPPORTED;
        for (int m = 0; m < n_models; ++m) {
            if (!enc->rays[m]) continue;                              // (this model's encodings were saved)
            NERFHIP_CHECK_ARG(enc->z[m] && enc->S[m] > 0 && enc->S[m] % 32 == 0 && n_host[m] % 256 == 0 && n_host[m] % enc->S[m] == 0);
            NERFHIP_CHECK_ARG(n_host[m] / 32 < (int64_t)1 << 31);
            if ((((uintptr_t)enc->rays[m]) | ((uintptr_t)enc->z[m])) & 15) return NERFHIP_E_ALIGN;
            regen[m] = true;
        }
    }
    NERFHIP_CHECK_ARG(g_out_host && out_host && n_host && packed_bwd_host && acts_host && dys_host && grad_w_host && grad_b_host);
    NERFHIP_CHECK_ARG(!(adam && accumulate));
    nerfhip::GradTable G;
    nerfhip::DwJobTable jt;
    for (int m = 0; m < n_models; ++m) {
        NERFHIP_CHECK_ARG(n_host[m] > 0);           // (an empty batch launches nothing: the single-model entry point handles it)
        NERFHIP_CHECK_ARG(g_out_host[m] && out_host[m] && packed_bwd_host[m] && acts_host[m] && dys_host[m] && dw_workspace);
        if ((((uintptr_t)g_out_host[m]) | ((uintptr_t)out_host[m]) | ((uintptr_t)packed_bwd_host[m]) | ((uintptr_t)acts_host[m]) |
             ((uintptr_t)dys_host[m])) & 15)
            return NERFHIP_E_ALIGN;
    }
    const int nwg = dw_plan(n_host, n_models, dtype, &jt);
    for (int m = 0; m < nerfhip::kDwMaxModels; ++m) {
        const bool on = m < n_models && regen[m];
        jt.enc_rays[m] = on ? enc->rays[m] : nullptr;
        jt.enc_z[m] = on ? enc->z[m] : nullptr;
        jt.enc_tpr[m] = on ? enc->S[m] / 32 : 1;
    }
    float* const fold_scratch = (float*)dw_workspace + (size_t)nwg * nerfhip::mlp::kDwSlabFloats;
    nerfhip::FoldArgs F;
    for (int m = 0; m < nerfhip::kDwMaxModels; ++m) {
        const int mm = m < n_models ? m : 0;
        F.image[m] = reinterpret_cast<const float*>((const uint8_t*)packed_bwd_host[mm] +
                                                    (size_t)nerfhip::mlp::bwd_padded_pieces(compute_prec(dtype)) * nerfhip::mlp::kPieceBytes);
        F.gw_final[m] = grad_w_host[12 * mm + 8];
        F.gb_final[m] = grad_b_host[12 * mm + 8];
        F.gw_dir[m] = grad_w_host[12 * mm + 9];
    }
    for (int j = 0; j < nerfhip::kDwMaxJobs; ++j) {
        const int jj = j < jt.njobs ? j : 0, m = jj / nerfhip::mlp::kNumDwJobs, prm = nerfhip::mlp::kDwJobs[jj % nerfhip::mlp::kNumDwJobs].param;
        NERFHIP_CHECK_ARG(grad_w_host[12 * m + prm] && grad_b_host[12 * m + prm]);
        G.w[j] = grad_w_host[12 * m + prm];
        G.b[j] = grad_b_host[12 * m + prm];
        jt.acts[j] = (const uint8_t*)acts_host[m];
        jt.dys[j] = (const uint8_t*)dys_host[m];
    }
    nerfhip::AdamFused A;
    A.state = nullptr;
    A.lr = A.beta1 = A.beta2 = A.eps = A.wd = 0.f;
    for (int m = 0; m < nerfhip::kDwMaxModels; ++m) { A.param[m] = A.m[m] = A.v[m] = nullptr; A.grad0[m] = nullptr; }
    if (adam) {
        NERFHIP_CHECK_ARG(adam->state && adam->n_models == n_models);
        for (int m = 0; m < n_models; ++m) {
            NERFHIP_CHECK_ARG(adam->param[m] && adam->exp_avg[m] && adam->exp_avg_sq[m] && adam->grad_flat[m]);
            A.param[m] = adam->param[m]; A.m[m] = adam->exp_avg[m]; A.v[m] = adam->exp_avg_sq[m]; A.grad0[m] = adam->grad_flat[m];
        }
        A.state = adam->state; A.lr = adam->lr; A.beta1 = adam->beta1; A.beta2 = adam->beta2; A.eps = adam->eps; A.wd = adam->weight_decay;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool do_chain = phases & 1, do_dw = phases & 2, do_reduce = phases & 4;
    if (do_chain) {                                 // ONE launch for the chains of all models (fine first: the long one leads)
        int64_t tiles[nerfhip::kDwMaxModels];
        for (int m = 0; m < n_models; ++m) tiles[m] = act_tiles(n_host[m], dtype);
        nerfhip::launch_bwd_chain(n_models, g_out_host, g_scale, out_host, n_host, packed_bwd_host, acts_host, dys_host, dtype, tiles, s);
    }
    if (do_dw) {
        if (dtype == NERFHIP_BF16_F8) nerfhip::launch_dw_f8(jt, (float*)dw_workspace, nwg, s);
        else nerfhip::launch_dw(dtype, jt, (float*)dw_workspace, nwg, s);
#if NERFHIP_DW_PROBE
        g_probe_f8 = dtype == NERFHIP_BF16_F8;
#endif
    }
    if (do_reduce) {
        nerfhip::launch_reduce(dtype == NERFHIP_BF16_F8, jt, (const float*)dw_workspace, G, fold_scratch, accumulate, A, s);
        nerfhip::launch_fold(F, (const float*)fold_scratch, n_models, accumulate, A, s);
    }
    return nerfhip_launch_status();
}

#if NERFHIP_DW_PROBE
// debug builds only (not part of include/nerfhip.h): the dW kernels' per-wave cycle accounts of the last launch
extern "C" int nerfhip_debug_dw_probe(unsigned* host_dst, int n_words) {
    if (!host_dst || n_words < 0 || n_words > 1024 * 8 * 8) return NERFHIP_E_BADARG;
    return g_probe_f8 ? nerfhip::read_dw_f8_probe(host_dst, n_words) : nerfhip::read_dw_probe(host_dst, n_words);
}
#endif

extern "C" int nerfhip_mlp_bwd_phases(const float* g_out, const float* out, int64_t n, const void* packed_bwd, const void* acts,
                                      void* dys, void* dw_workspace, float* const* grad_w_host, float* const* grad_b_host,
                                      int accumulate, int dtype, int phases, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(n >= 0);
    if (!valid_dtype(dtype)) return NERFHIP_E_UNSUPPORTED;
    NERFHIP_CHECK_ARG(grad_w_host && grad_b_host);
    for (int i = 0; i < 12; ++i) NERFHIP_CHECK_ARG(grad_w_host[i] && grad_b_host[i]);
    if (n == 0) return 0;
    return nerfhip_mlp_bwd_multi(1, &g_out, &out, &n, &packed_bwd, &acts, &dys, dw_workspace, grad_w_host, grad_b_host, accumulate,
                                 dtype, phases, nullptr, nullptr, stream);
}

extern "C" int nerfhip_mlp_bwd(const float* g_out, const float* out, int64_t n, const void* packed_bwd, const void* acts,
                               void* dys, void* dw_workspace, float* const* grad_w_host, float* const* grad_b_host,
                               int accumulate, int dtype, nerfhip_stream_t stream) {
    return nerfhip_mlp_bwd_phases(g_out, out, n, packed_bwd, acts, dys, dw_workspace, grad_w_host, grad_b_host, accumulate, dtype, 7,
                                  stream);
}

// The weight-gradient launches of the MLP backward (mlp_bwd_dw.hip, mlp_bwd_dw_f8.hip, mlp_bwd_reduce.hip): their argument tables and
// launchers, called by the C ABI in mlp_bwd.hip.  Host-only C++ (no HIP header): mlp_dw_plan.h fills the job table with a plain g++ too.
#pragma once
#include <stdint.h>

#include "mlp_layout.h"

typedef struct ihipStream_t* hipStream_t;      // (as <hip/hip_runtime_api.h> declares it)

#ifndef NERFHIP_DW_PROBE
#define NERFHIP_DW_PROBE 0       // debug builds: every wave of the dW kernels accumulates where its cycles go (tools/dw_probe.py)
#endif

namespace nerfhip {
using namespace mlp;

// Jobs + their point-range splits.  A workgroup = (job, split); how many splits a job gets is the host's plan (dw_plan, mlp_dw_plan.h).
// One launch serves up to kDwMaxModels models (a training step's fine and coarse network): job j belongs to model j / 12 and
// carries that model's tensors, so ONE dW launch and ONE reduce launch cover the whole step.
constexpr int kDwMaxModels = 2;
constexpr int kDwMaxJobs = kDwMaxModels * kNumDwJobs;
struct DwJobTable {
    DwJob job[kDwMaxJobs];
    int nsplit[kDwMaxJobs];
    int soff[kDwMaxJobs + 1];     // prefix sums: workgroup / partial-slab index of (job j, split 0); = total for j >= njobs
    const uint8_t* acts[kDwMaxJobs];   // saved activations of the job's model
    const uint8_t* dys[kDwMaxJobs];    // dY slabs of the job's model
    int64_t ntiles[kDwMaxJobs];        // 32-point wave tiles of the job's model
    int njobs;
    // The sigma head's job has no workgroups of its own — its X (h8: 16 slabs per tile) is also the second X section of the DIR job
    // since round 6 (mlp_layout.h kDwJobs; rounds 4-5: of the final layer's job) — so the dir job's workgroups also form dW_sigma:
    // their waves 4..7, idle otherwise (the job has 4 dY tiles), each multiply dY_sigma by two of the eight h8 tiles.
    // fold_of[sigma job] = the dir job's index (its partial slabs hold the sigma partials in rows 4..7, which it does not use),
    // -1 everywhere else.
    int fold_of[kDwMaxJobs];
    // Encodings regenerated instead of read (bf16, nerfhip_mlp_bwd_multi_rays): per MODEL the rays (B,8), the depths (B,S) its forward
    // ran on and S / 32 (tiles per ray); enc_rays[m] == nullptr: the job's x1 section is read from the saved activations as before.
    const float* enc_rays[kDwMaxModels];
    const float* enc_z[kDwMaxModels];
    int enc_tpr[kDwMaxModels];
};
static_assert(kDwJobs[kDwJobDir].x2_off == kDwJobs[kDwJobSigma].x1_off && kDwJobs[kDwJobDir].x2_slabs == 16 && kDwJobs[kDwJobDir].x1_slabs == 2 &&
              kDwJobs[kDwJobSigma].x1_slabs == 16 && kDwJobs[kDwJobSigma].dy_slabs == 2 && kDwJobs[kDwJobDir].dy_slabs == 8 &&
              kDwJobs[kDwJobSigma].x2_slabs == 0, "the sigma head and the dir layer read the same h8 section");
// the folded sigma head in a dir-job partial slab: wave w = 4..7 holds (dY_sigma tile 0) x (h8 tiles 2 (w - 4), 2 (w - 4) + 1) in
// blocks (row w, columns 0, 1); its bias partial is bias row kDwFoldRow0 (written by wave 4)
constexpr int kDwFoldRow0 = 4;
NH_HD constexpr int dw_fold_block(int xt) { return (kDwFoldRow0 + xt / 2) * kDwMaxXTiles + (xt & 1); }     // block index of h8 tile xt
constexpr int kDwFoldStageSlabs = 28;  // [dY_dir 8][enc_dir 2][h8 16][dY_sigma 2]
constexpr int kDwFoldSigmaSlab = 26;   // first dY_sigma slab of that stage

struct GradTable {
    float* w[kDwMaxJobs];     // per JOB: job j writes parameter tensor kDwJobs[j % 12].param of model j / 12
    float* b[kDwMaxJobs];
};

// Adam fused into the reduce (single-GPU training step: no all-reduce sits between the gradients and the update).  A model's
// parameters, exp_avg and exp_avg_sq live in flat fp32 buffers laid out exactly like its flat gradient buffer (optim.py
// FlatAdam, ops.mlp_bwd), so gradient element e updates element e of each.  `state` = {step count, arrival ticket} as in
// adam_kernel (optim.hip); nullptr = plain reduce.
struct AdamFused {
    float* param[kDwMaxModels];
    float* m[kDwMaxModels];
    float* v[kDwMaxModels];
    const float* grad0[kDwMaxModels];     // base of the model's flat gradient buffer
    float* state;
    float lr, beta1, beta2, eps, wd;
};

// ================================================================================================
// Phase C: the folded final layer (mlp_layout.h kDwJobs)
// ================================================================================================
//     dW_dir[j][m]   = sum_k G[j][k] W_f[m][k] + s[j] b_f[m]      (j < 128, m < 256: the first 256 columns of dir_encoding's weight)
//     dW_final[m][k] = sum_j W_dx[j][m] G[j][k]                    (m, k < 256)
//     db_final[m]    = sum_j W_dx[j][m] s[j]
// fp32 FMAs in a fixed order (2 x 8.4 M per model).  One 256-thread workgroup per 32 x 32 output tile, operands staged through LDS
// in 32-deep slices: blocks 0..31 the dW_dir tiles, 32..95 the dW_final tiles, 96 the bias.  W_f, W_dx, b_f come from the fold
// block of the packed W^T image — a snapshot taken before the step's update, so with Adam fused the update of one block cannot
// reach the operands of another.
struct FoldArgs {
    const float* image[kDwMaxModels];      // fold block of the model's packed W^T image
    float* gw_final[kDwMaxModels];
    float* gb_final[kDwMaxModels];
    float* gw_dir[kDwMaxModels];
};

// (job, split) workgroups `nwg` of the plan in jt, one partial slab each in `slabs`; prec = NERFHIP_F32 | NERFHIP_BF16
void launch_dw(int prec, const DwJobTable& jt, float* slabs, int nwg, hipStream_t s);
void launch_dw_f8(const DwJobTable& jt, float* slabs, int nwg, hipStream_t s);                      // NERFHIP_BF16_F8
// partial slabs -> gradient tensors (+ fused Adam), then the folded final layer from the G, s the reduce left in fold_scratch
void launch_reduce(bool f8, const DwJobTable& jt, const float* slabs, const GradTable& G, float* fold_scratch, int accumulate,
                   const AdamFused& A, hipStream_t s);
void launch_fold(const FoldArgs& F, const float* fold_scratch, int n_models, int accumulate, const AdamFused& A, hipStream_t s);
#if NERFHIP_DW_PROBE
// debug builds: the per-wave cycle accounts the last launch of the kernel left ([workgroup][wave][8] words), 0 or -100
int read_dw_probe(unsigned* host_dst, int n_words);
int read_dw_f8_probe(unsigned* host_dst, int n_words);
#endif
}  // namespace nerfhip

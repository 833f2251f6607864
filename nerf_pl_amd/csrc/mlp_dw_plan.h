// The split plan of the weight-gradient launch: which workgroup = which (job, point range).  Host-only C++ — plain integer
// arithmetic over mlp_layout.h's job list, compiled into the C ABI (mlp_bwd.hip) and, by a plain g++, into tests/host/dw_plan_check.cpp.
#pragma once
#include "mlp_bwd_dw.h"

constexpr int kPlanF32 = 0, kPlanBf16 = 1, kPlanBf16F8 = 2;      // dtype codes: NERFHIP_F32 / _BF16 / _BF16_F8 of include/nerfhip.h

// Target workgroup count of the dW launch.  fp32: 2 rounds of 256 CUs at 1 workgroup/CU.  bf16: ONE round — with the pipelined inner
// loop the kernel itself is as fast in one round as in two (585 vs 591 us merged), and every workgroup less is a 330 KB partial slab
// not written and not re-read by the reduce: the bf16 step 1.265 -> 1.196 ms on the same box.  e4m3: one round too, see below.
constexpr int kDwWgsF32 = 512, kDwWgsBf16 = 256, kDwWgsF8 = 256;

// 32-point wave tiles of n_points, padded to whole workgroups of the forward (8 waves; fp32: 4)
static int64_t act_tiles(int64_t n_points, int dtype) {
    const int64_t ppw = 32 * (dtype == kPlanF32 ? 4 : 8);
    return (n_points + ppw - 1) / ppw * (ppw / 32);
}

// The split plan: which workgroup = which (job, point range).
// Rounds 1-3 gave every workgroup the SAME number of ring iterations: until the inner loops were software-pipelined (round 3) an
// iteration cost ten exposed LDS round trips whatever its bytes, and splits in proportion to the jobs' bytes measured 268-306 us
// against 225-232 us (e4m3, 1024 x 192 points).  The e4m3 launch still plans that way; the bf16 launch — see below — no longer.
// e4m3 kernel: ONE round of the 256 CUs (measured at 1024 x 192: 207-215 us vs 233-247 us for 384-768 workgroups, and half the
// split-K partials for the reduce kernel: 23 -> 12.5 us); bf16 one round too (every workgroup less is a 330 KB partial slab neither
// written nor re-read), fp32 two rounds (2,882 vs 3,244 us).
// Several models in one launch (a training step's fine + coarse network): the workgroups are shared out ACROSS the models — a model
// with a third of the points gets a third of the splits per job — instead of a second, short launch that cannot hide its pipeline
// fill (coarse pass alone: 0.49 of the HBM peak vs 0.62 for the fine pass).
// Round 4: with the inner loops pipelined (round 3) an iteration's time DOES follow its bytes — per-workgroup wall clocks of the
// merged bf16 launch (tools/dw_probe.py, profiles/r04_dw_probe_call14_block_issue.txt): 0.69 / 0.91 / 0.82 / 1.05 / 1.40 / 1.63 us per iteration for
// stages of 10 / 18 / 20 / 26 / 32 / 36 KiB, i.e. ~0.3 us + 35 ns per KiB.  With equal iteration counts the skip-layer workgroups
// ran 626 us, the 256 x 256 layers 537 us and the rgb / first / sigma / dir jobs 280-430 us: the launch waited for 32 of its 256
// workgroups while a quarter of the CUs idled for a third of it.  The plan now equalises iterations x (a + b x stage KiB).
// The cost model is deliberately the coarse linear one.  A table of the per-class costs measured under a balanced plan (0.72 / 0.95 /
// 0.94 / 1.13 / 1.58 / 1.81 us per iteration for 10 / 18 / 20 / 26 / 32 / 36 KiB stages) makes every workgroup finish within 3 % of
// the others (profiles/r04_dw_probe_bf16_table_plan.txt) and the launch SLOWER: 473-480 us against 455-458 us in the same call —
// with the linear model the first-layer and dir-layer workgroups finish ~15 % early, and the bandwidth they release goes to the
// 256 x 256 and skip-layer workgroups that end the launch, whose partial slabs then do not all land in the same microseconds.
// Round 6: with the 2 x 4 wave split, the dot2 bias sums and the register-major epilogue an iteration's fixed part shrank; the sweep of
// profiles/r06_dw_plan_cost_ab.txt (one box, three alternating rounds) has 150 + 45 / KiB at 449-452 us in the step against 466-469 us for
// round 4's 300 + 35 / KiB, 100 + 50 the same, 50 + 55 and 0 + 60 (bytes-proportional) slower again.
constexpr int kDwCostA = 150, kDwCostB = 45;      // bf16: ns per ring iteration = kDwCostA + kDwCostB x (KiB of a stage)
// a workgroup should run at least this many ring iterations: the DEPTH-stage DMA pipeline takes ~4 to fill, and every split costs a
// 330 KB partial slab the reduce kernel re-reads
constexpr int kDwMinIters = 48;
static int dw_target_wgs(int dtype) { return dtype == kPlanBf16F8 ? kDwWgsF8 : dtype == kPlanBf16 ? kDwWgsBf16 : kDwWgsF32; }
// n_points[m] points of model m (m < n_models).  Fills jt (nsplit, soff, job, ntiles, njobs; the tensor pointers are the
// caller's) when non-null; returns the number of workgroups = partial slabs.  The plan depends on these arguments alone — not on
// whether the launch regenerates the encodings (nerfhip_mlp_bwd_multi_rays): both forms run the same workgroups, hence the same fp32
// summation order and bit-identical gradients, and the size query (nerfhip_mlp_dw_workspace_bytes_multi) sizes what the launch uses.
static int dw_plan(const int64_t* n_points, int n_models, int dtype, nerfhip::DwJobTable* jt) {
    using namespace nerfhip;
    using namespace nerfhip::mlp;
    const int njobs = n_models * kNumDwJobs;
    int64_t units[kDwMaxJobs];     // ring iterations of a job if it were one workgroup (f8: tile PAIRS)
    int64_t cap[kDwMaxJobs];
    int ns[kDwMaxJobs];
    int64_t cost[kDwMaxJobs];      // time of one ring iteration of the job (ns): kDwCostA + kDwCostB x (dY + X slabs of a stage)
    int total = 0;
    for (int j = 0; j < njobs; ++j) {
        const int64_t tiles = act_tiles(n_points[j / kNumDwJobs], dtype);
        const DwJob& jb = kDwJobs[j % kNumDwJobs];
        // (the e4m3 launch keeps equal iteration counts: with the byte-weighted plan it measured 336 us against 254 us; the fp32
        // launch has not been re-measured)
        const int ca = dtype == kPlanBf16 ? kDwCostA : 1;
        const int cb = dtype == kPlanBf16 ? kDwCostB : 0;
        // the sigma head's 2 dY slabs ride in the dir job's stage: the dir layer's workgroups also form the sigma head's gradient (same
        // X section: h8 read once; bf16 since round 4, e4m3 and fp32 since round 5, into the dir job since round 6).  (With the
        // encodings regenerated the first, skip and dir jobs fetch less than they are priced for and simply finish early.)
        cost[j] = ca + (int64_t)cb * (jb.dy_slabs + jb.x1_slabs + jb.x2_slabs + (j % kNumDwJobs == kDwJobDir ? 2 : 0));
        units[j] = tiles / (dtype == kPlanBf16F8 ? 2 : 1);
        cap[j] = units[j] / kDwMinIters;
        if (cap[j] < 1) cap[j] = 1;
        // no workgroups of their own: the final layer (derived from the dir job's G by mlp_bwd_fold_kernel, mlp_layout.h kDwJobs) and,
        // folded, the sigma head (the dir layer's workgroups form dW_sigma too)
        if (j % kNumDwJobs == kDwJobFinal || j % kNumDwJobs == kDwJobSigma) {
            cap[j] = 0;
            ns[j] = 0;
            continue;
        }
        ns[j] = 1;
        ++total;
    }
    // greedy: the next workgroup goes to the job whose workgroups currently run the LONGEST (iterations x time per iteration);
    // ties go to the jobs with the most bytes per iteration (the 256 x 256 layers, jobs 1..8 of a model), then to the lower index
    const int target = dw_target_wgs(dtype);
    while (total < target) {
        int best = -1;
        for (int j = 0; j < njobs; ++j) {
            if (ns[j] >= cap[j]) continue;
            if (best < 0) { best = j; continue; }
            const int64_t a = units[j] * cost[j] * ns[best], b = units[best] * cost[best] * ns[j];   // time per workgroup of j vs best
            const int jj = j % kNumDwJobs, bb = best % kNumDwJobs;
            const bool j_big = jj >= 1 && jj <= 7, b_big = bb >= 1 && bb <= 7;
            if (a > b || (a == b && j_big && !b_big)) best = j;
        }
        if (best < 0) break;
        ++ns[best];
        ++total;
    }
    if (jt) {
        int off = 0;
        for (int j = 0; j < kDwMaxJobs; ++j) {
            const int jj = j < njobs ? j : 0;
            jt->job[j] = kDwJobs[jj % kNumDwJobs];
            jt->nsplit[j] = j < njobs ? ns[j] : 0;
            jt->soff[j] = off;
            jt->ntiles[j] = act_tiles(n_points[jj / kNumDwJobs], dtype);
            jt->fold_of[j] = (j < njobs && ns[j] == 0 && j % kNumDwJobs == kDwJobSigma) ? j - kDwJobSigma + kDwJobDir : -1;
            if (j < njobs) off += ns[j];
        }
        jt->soff[kDwMaxJobs] = off;
        jt->njobs = njobs;
    }
    return total;
}

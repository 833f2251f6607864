// Host-side check of nerf_pl_amd/csrc/mlp_dw_plan.h: the split plan is plain C++ that a g++ without any HIP header compiles.  Prints
// the workgroup totals of the benchmark step (fine 1024 x 192 + coarse 1024 x 64 points in one launch) for dtypes 2, 1, 0
// (e4m3 storage, bf16, fp32); run by tests/test_layout_host.py.
#include <cstdio>

#include "mlp_dw_plan.h"

int main() {
    const int64_t n[2] = {1024 * 192, 1024 * 64};
    nerfhip::DwJobTable jt;
    for (int dtype = 2; dtype >= 0; --dtype) {
        const int total = dw_plan(n, 2, dtype, &jt);
        std::printf("%d%s", total == jt.soff[nerfhip::kDwMaxJobs] ? total : -1, dtype ? " " : "\n");
    }
    return 0;
}

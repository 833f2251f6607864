// Prints the "fp8 storage" index maps of nerf_pl_amd/csrc/mlp_layout.h that oracle/f8_exact.py restates in Python, one table per
// line ("name v0 v1 ..."): compiled with g++ and compared entry by entry by tests/test_f8_exact_host.py.
#include <cstdio>
#include <initializer_list>

#include "mlp_layout.h"

using namespace nerfhip::mlp;

static void name(const char* n) { std::printf("%s", n); }
static void val(long long v) { std::printf(" %lld", v); }
static void end() { std::printf("\n"); }

int main() {
    name("consts");
    for (long long v : {(long long)kF8ActPairs, (long long)kF8DyPairs, (long long)f8_act_gate_off(), (long long)f8_act_scale_off(),
                        (long long)f8_act_tile_bytes(), (long long)f8_dy_scale_off(), (long long)f8_dy_tile_bytes(),
                        (long long)act_il(1, true), (long long)kActFeat, (long long)kDyFeat})
        val(v);
    end();
    name("f8_x_section");
    for (int s = 0; s < kActSlabs; ++s) val(f8_x_section(s));
    end();
    name("f8_dy_section");
    for (int s = 0; s < kDySlabs; ++s) val(f8_dy_section(s));
    end();
    name("f8_row_h");
    for (int m = 0; m < 16; ++m) val(f8_row_h(m));
    end();
    name("f8_row_j");
    for (int m = 0; m < 16; ++m) val(f8_row_j(m));
    end();
    // feature (chain section) of operand row m of pair 0, as mlp_bwd_reduce_kernel<true> maps it
    name("row_feature");
    for (int m = 0; m < 32; ++m) val(chain_feature(m >> 4, f8_row_h(m & 15), f8_row_j(m & 15)));
    end();
    return 0;
}

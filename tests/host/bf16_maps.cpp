// Prints the index maps of nerf_pl_amd/csrc/mlp_layout.h that oracle/bf16_exact.py restates in Python, one table per line
// ("name v0 v1 ..."): compiled with g++ and compared entry by entry by tests/test_bf16_exact_host.py.
#include <cstdio>
#include <initializer_list>

#include "mlp_layout.h"

using namespace nerfhip::mlp;

static void name(const char* n) { std::printf("%s", n); }
static void val(long long v) { std::printf(" %lld", v); }
static void end() { std::printf("\n"); }

int main() {
    name("consts");
    for (long long v : {(long long)kXyzCh, (long long)kDirCh, (long long)kW, (long long)kXyzSlabs, (long long)kDirSlabs, (long long)kPieceBytes,
                        (long long)kActEncX, (long long)kActEncD, (long long)kActH0, (long long)kActFeat, (long long)kActT, (long long)kActSlabs,
                        (long long)kMaskPieces, (long long)kMaskPieceT, (long long)kDyRgb, (long long)kDyDir, (long long)kDyFeat,
                        (long long)kDySigma, (long long)kDyH0, (long long)kDySlabs, (long long)act_mask_off(1), (long long)act_tile_bytes(1),
                        (long long)kDySlabs * slab_bytes(1), (long long)act_il(1), (long long)kNumLayers, (long long)kSigmaLayer,
                        (long long)kDirLayer, (long long)bias_block_start(1), (long long)bias_block_pieces(1)})
        val(v);
    end();
    name("act_h");
    for (int l = 1; l <= 8; ++l) val(act_h(l));
    end();
    name("dy_h");
    for (int l = 1; l <= 8; ++l) val(dy_h(l));
    end();
    name("mask_piece_h");
    for (int l = 1; l <= 8; ++l) val(mask_piece_h(l));
    end();
    name("chain_feature");
    for (int ks = 0; ks < 16; ++ks)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 8; ++j) val(chain_feature(ks, h, j));
    end();
    name("xyz_slot_channel");
    for (int ks = 0; ks < kXyzSlabs; ++ks)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 8; ++j) val(xyz_slot_channel(ks, h, j));
    end();
    name("dir_slot_channel");
    for (int ks = 0; ks < kDirSlabs; ++ks)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 8; ++j) val(dir_slot_channel(ks, h, j));
    end();
    name("gate_word");
    for (int i = 0; i < 128; ++i) val(gate_word(i));
    end();
    name("gate_bit");
    for (int i = 0; i < 128; ++i) val(gate_bit(i));
    end();
    name("tile_block_off");
    for (int il : {1, 8})
        for (int t = 0; t < 20; ++t) val((long long)tile_block_off(t, act_tile_bytes(1), il));
    end();
    name("layers");
    for (int L = 0; L < kNumLayers; ++L)
        for (long long v : {(long long)kLayers[L].param, (long long)kLayers[L].nt, (long long)kLayers[L].n_out, (long long)kLayers[L].kind,
                            (long long)kLayers[L].enc_slabs, (long long)kLayers[L].chain_slabs, (long long)layer_start(L, 1)})
            val(v);
    end();
    name("layer_in_col");
    for (int L = 0; L < kNumLayers; ++L)
        for (int ks = 0; ks < layer_slabs(L); ++ks)
            for (int h = 0; h < 2; ++h)
                for (int j = 0; j < 8; ++j) val(layer_in_col(L, ks, h, j));
    end();
    name("dw_jobs");
    for (int j = 0; j < kNumDwJobs; ++j) {
        const DwJob& b = kDwJobs[j];
        for (int v : {b.param, b.dy_off, b.dy_slabs, b.x1_off, b.x1_slabs, b.x1_col0, b.x1_enc, b.x2_off, b.x2_slabs, b.x2_col0, b.x2_enc}) val(v);
    }
    end();
    return 0;
}

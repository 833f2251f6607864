// Stand-alone check of the split entropy decoder's host twin under a sanitizer: reads the streams that tools/jpeg_split_sanitize.py
// wrote (the synthetic edge and damaged streams of tests/tools/jpeg_synth.py and the baseline files of tests/golden/jpeg_mini),
// decodes each with nerfhip_jpeg_entropy_decode and, for several subsequence sizes, with nerfhip_jpeg_entropy_decode_split, and
// demands equal verdicts and equal coefficients.  Every buffer is a heap block of exactly the documented size, so a read or write
// outside one is the sanitizer's to report.  No GPU is touched: both entry points are host functions.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/nerfhip.h"

static bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0, runs = 0, refused = 0, failures = 0;
    for (;;) {
        int32_t head[20];   // name bytes, n_comp, comp[12], mcus_x, mcus_y, restart, mask, scan bytes, expected verdict
        if (!read_exact(f, head, sizeof head)) break;
        std::string name((size_t)head[0], ' ');
        if (!read_exact(f, &name[0], name.size())) return 2;
        const int n_comp = head[1], mcus_x = head[14], mcus_y = head[15], restart = head[16], mask = head[17], scan_bytes = head[18];
        uint8_t* huffman = (uint8_t*)malloc(8 * 272);
        uint8_t* scan = (uint8_t*)malloc((size_t)scan_bytes);
        if (!read_exact(f, huffman, 8 * 272) || !read_exact(f, scan, (size_t)scan_bytes)) return 2;
        ++cases;
        int64_t blocks[3] = {0, 0, 0};
        for (int c = 0; c < n_comp; ++c) blocks[c] = (int64_t)mcus_x * head[2 + 4 * c] * mcus_y * head[3 + 4 * c];
        int16_t* want[3] = {nullptr, nullptr, nullptr};
        int16_t* got[3] = {nullptr, nullptr, nullptr};
        for (int c = 0; c < n_comp; ++c) {
            want[c] = (int16_t*)calloc((size_t)blocks[c] * 64, 2);
            got[c] = (int16_t*)malloc((size_t)blocks[c] * 64 * 2);
        }
        const int reference = nerfhip_jpeg_entropy_decode(scan, scan_bytes, n_comp, head + 2, huffman, mask, mcus_x, mcus_y, restart, want, blocks);
        if (reference != head[19]) {
            printf("FAIL %s: the sequential decoder answers %d, the case expects %d\n", name.c_str(), reference, head[19]);
            ++failures;
        }
        const int64_t n_mcu = (int64_t)mcus_x * mcus_y;
        const int intervals = restart > 0 ? (int)((n_mcu + restart - 1) / restart) : 1;
        const int sizes[5] = {32, 64, 256, 1024, 4096};
        for (int bits : sizes) {
            const size_t ws_bytes = nerfhip_jpeg_entropy_workspace_bytes(1, scan_bytes, intervals, bits);
            if (!ws_bytes) return 2;
            void* ws = aligned_alloc(256, ws_bytes);
            int64_t* offsets = (int64_t*)malloc(16);
            int32_t* small = (int32_t*)malloc(16);           // mask, restart, status, progress
            offsets[0] = 0;
            offsets[1] = scan_bytes;
            small[0] = mask;
            small[1] = restart;
            nerfhip_jpeg_batch b;
            memset(&b, 0, sizeof b);
            b.scans = scan;
            b.offsets = offsets;
            b.huffman = huffman;
            b.huffman_masks = small;
            b.restart_intervals = small + 1;
            b.total_bytes = b.max_scan_bytes = scan_bytes;
            b.max_intervals = intervals;
            b.n_images = 1;
            b.n_comp = n_comp;
            memcpy(b.comp, head + 2, sizeof b.comp);
            b.mcus_x = mcus_x;
            b.mcus_y = mcus_y;
            b.subseq_bits = bits;
            b.workspace = ws;
            b.status = small + 2;
            b.progress = small + 3;
            for (int c = 0; c < n_comp; ++c) memset(got[c], 0, (size_t)blocks[c] * 64 * 2);
            const int e = nerfhip_jpeg_entropy_decode_split(&b, got[0], got[1], got[2]);
            ++runs;
            bool ok = e == 0 && small[2] == reference;
            if (ok && reference == 0)
                for (int c = 0; c < n_comp; ++c) ok = ok && memcmp(got[c], want[c], (size_t)blocks[c] * 64 * 2) == 0;
            if (reference != 0) ++refused;
            if (!ok) {
                printf("FAIL %s at %d bits: call %d, status %d, the sequential decoder %d\n", name.c_str(), bits, e, small[2], reference);
                ++failures;
            }
            free(ws);
            free(offsets);
            free(small);
        }
        for (int c = 0; c < n_comp; ++c) {
            free(want[c]);
            free(got[c]);
        }
        free(huffman);
        free(scan);
    }
    fclose(f);
    printf("%d streams, %d split decodes (%d of refused streams), %d failures\n", cases, runs, refused, failures);
    return failures ? 1 : 0;
}

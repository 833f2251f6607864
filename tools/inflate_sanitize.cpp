// Stand-alone check of the device inflate's host twin under a sanitizer: reads the streams that tools/inflate_sanitize.py wrote
// (the whole corpus of tests/inflate_streams.py with the verdicts and bytes the Python side recorded from zlib), inflates each
// with nerfhip_inflate_host — alone, and again in batches of up to 16 streams of one output size with a gap between the rows —
// and demands zlib's verdicts and bytes.  The stream, the offsets, the status words and the output are heap blocks of exactly
// the documented size (the output behind 0 .. 15 bytes of padding, so that every alignment of `out` occurs): a read or write
// outside one is the sanitizer's to report.  No GPU is touched: the entry point is a host function.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/nerfhip.h"

struct Case {
    std::string name;
    std::vector<uint8_t> stream, expect;
    int64_t out_bytes;
    int verdict;
};

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int failures = 0;

// cases[first .. first + n) in one call, rows `gap` bytes apart beyond out_bytes, `out` shifted by `shift` bytes
static void run(const std::vector<Case>& cases, size_t first, int n, int64_t gap, int shift) {
    const int64_t out_bytes = cases[first].out_bytes, stride = out_bytes + gap;
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += cases[first + i].stream.size();
    uint8_t* data = (uint8_t*)malloc(total ? total : 1);
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int32_t* status = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
    const size_t out_size = (size_t)shift + (size_t)((int64_t)(n - 1) * stride + out_bytes);     // the last row has no gap behind it
    uint8_t* block = (uint8_t*)malloc(out_size ? out_size : 1);
    memset(block, 0xa5, out_size);
    offsets[0] = 0;
    for (int i = 0; i < n; ++i) {
        const std::vector<uint8_t>& s = cases[first + i].stream;
        if (!s.empty()) memcpy(data + offsets[i], s.data(), s.size());
        offsets[i + 1] = offsets[i] + (int64_t)s.size();
        status[i] = 77;
    }
    uint8_t* out = block + shift;
    const int e = nerfhip_inflate_host(total ? data : nullptr, offsets, (int64_t)total, n, out_size > (size_t)shift ? out : nullptr, out_bytes,
                                       stride, status);
    if (e != 0) {
        printf("FAIL %s: the call answers %d\n", cases[first].name.c_str(), e);
        ++failures;
    }
    for (int i = 0; e == 0 && i < n; ++i) {
        const Case& c = cases[first + i];
        bool ok = status[i] == c.verdict;
        if (ok && c.verdict == 0 && out_bytes > 0) ok = memcmp(out + (int64_t)i * stride, c.expect.data(), (size_t)out_bytes) == 0;
        for (int64_t g = 0; ok && i + 1 < n && g < gap; ++g) ok = out[(int64_t)i * stride + out_bytes + g] == 0xa5;
        if (!ok) {
            printf("FAIL %s (batch of %d, shift %d): status %d, zlib %d\n", c.name.c_str(), n, shift, status[i], c.verdict);
            ++failures;
        }
    }
    for (int k = 0; k < shift; ++k)
        if (block[k] != 0xa5) {
            printf("FAIL %s: a byte in front of the output changed\n", cases[first].name.c_str());
            ++failures;
            break;
        }
    free(block);
    free(status);
    free(offsets);
    free(data);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<Case> cases;
    for (;;) {
        int64_t head[4];        // name bytes, stream bytes, out_bytes, zlib's verdict (0 or NERFHIP_E_DATA)
        if (fread(head, 1, sizeof head, f) != sizeof head) break;
        Case c;
        c.name.resize((size_t)head[0]);
        c.stream.resize((size_t)head[1]);
        c.out_bytes = head[2];
        c.verdict = (int)head[3];
        if (c.verdict == 0) c.expect.resize((size_t)head[2]);
        if (!read_exact(f, &c.name[0], c.name.size()) || !read_exact(f, c.stream.data(), c.stream.size()) ||
            !read_exact(f, c.expect.data(), c.expect.size()))
            return 2;
        cases.push_back(std::move(c));
    }
    fclose(f);
    int refused = 0, batches = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        run(cases, i, 1, 0, (int)(i % 16));
        if (cases[i].verdict != 0) ++refused;
    }
    for (size_t i = 0; i < cases.size();) {
        int n = 1;
        while (n < 16 && i + n < cases.size() && cases[i + n].out_bytes == cases[i].out_bytes) ++n;
        run(cases, i, n, 5, (int)(batches % 16));
        ++batches;
        i += (size_t)n;
    }
    printf("%zu streams (%d refused by zlib) alone and in %d batches, %d failures\n", cases.size(), refused, batches, failures);
    return failures ? 1 : 0;
}

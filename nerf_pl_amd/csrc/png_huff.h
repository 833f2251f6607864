// Length-limited Huffman code lengths of the PNG encoder (png.hip), written once for both sides: the
// strip kernel runs it on LDS arrays, nerfhip_png_code_lengths runs it on the host so that a CPU test can hold it to the numpy
// restatement (tests/png_ref.py) on histograms no image produces.  Every loop is bounded by the symbol count.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace nerfhip {

constexpr int kHuffMaxSymbols = 286;      // deflate's literal/length alphabet; the code-length alphabet has 19
constexpr int kHuffMaxLimit = 15;

struct HuffScratch {
    uint32_t weight[2 * kHuffMaxSymbols];      // the used symbols in ascending (count, symbol) order, then the merged nodes
    uint16_t parent[2 * kHuffMaxSymbols];
    uint16_t depth[2 * kHuffMaxSymbols];
    uint16_t order[kHuffMaxSymbols];           // rank -> symbol
    uint16_t bl_count[kHuffMaxLimit + 1];
};

// Rank of symbol i among the used symbols in ascending (count, symbol) order; counts[i] > 0.
__host__ __device__ inline int huff_rank(const uint32_t* counts, int n, int i) {
    const uint32_t ci = counts[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const uint32_t cj = counts[j];
        r += (cj != 0 && (cj < ci || (cj == ci && j < i))) ? 1 : 0;
    }
    return r;
}

// Lengths from the ranked symbols s.order[0..m): plain Huffman by the two-queue merge (of two equal weights the merged node goes
// before the leaf, the earlier before the later within a queue), depths above `limit` folded into it, the Kraft sum repaired one unit of
// 2^-limit at a time (one leaf of the longest shorter length goes one level down and takes a leaf of length `limit` as its
// sibling), lengths handed back longest first to the ascending order.  One used symbol gets length 1, none leaves all zero.
template <typename Len>
__host__ __device__ inline void huff_from_order(const uint32_t* counts, int n, int m, int limit, Len* lengths, HuffScratch& s) {
    for (int i = 0; i < n; ++i) lengths[i] = 0;
    if (m <= 0) return;
    if (m == 1) {
        lengths[s.order[0]] = 1;
        return;
    }
    for (int i = 0; i < m; ++i) s.weight[i] = counts[s.order[i]];
    int leaf = 0, node = m;
    for (int next = m; next < 2 * m - 1; ++next) {
        uint32_t w = 0;
        for (int k = 0; k < 2; ++k) {
            const bool take_leaf = leaf < m && (node >= next || s.weight[leaf] < s.weight[node]);
            const int x = take_leaf ? leaf++ : node++;
            w += s.weight[x];
            s.parent[x] = (uint16_t)next;
        }
        s.weight[next] = w;
    }
    s.depth[2 * m - 2] = 0;
    for (int k = 2 * m - 3; k >= 0; --k) s.depth[k] = (uint16_t)(s.depth[s.parent[k]] + 1);
    for (int b = 0; b <= limit; ++b) s.bl_count[b] = 0;
    for (int k = 0; k < m; ++k) {
        const int d = s.depth[k] < limit ? s.depth[k] : limit;
        ++s.bl_count[d];
    }
    int excess = -(1 << limit);               // Kraft sum minus one, in units of 2^-limit: at most 286 << 14
    for (int b = 1; b <= limit; ++b) excess += (int)s.bl_count[b] << (limit - b);
    // More leaves were folded than units are in excess (each folded leaf adds less than one), and a step takes one leaf from
    // `limit` per unit: bl_count[limit] stays positive.  m <= 286 < 2^limit leaves cannot all stand at `limit` with an excess,
    // so a shorter length exists; the bound on `bits` only keeps a broken invariant from spinning.
    for (; excess > 0; --excess) {
        int bits = limit - 1;
        while (bits > 0 && s.bl_count[bits] == 0) --bits;
        if (bits == 0) break;
        --s.bl_count[bits];
        s.bl_count[bits + 1] = (uint16_t)(s.bl_count[bits + 1] + 2);
        --s.bl_count[limit];
    }
    int k = 0;
    for (int bits = limit; bits >= 1; --bits)
        for (int c = s.bl_count[bits]; c > 0 && k < m; --c) lengths[s.order[k++]] = (Len)bits;
}

// The whole construction by one caller (the host entry point; the kernel's 19-symbol code-length alphabet).
template <typename Len>
__host__ __device__ inline void huff_lengths(const uint32_t* counts, int n, int limit, Len* lengths, HuffScratch& s) {
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (counts[i]) {
            s.order[huff_rank(counts, n, i)] = (uint16_t)i;
            ++m;
        }
    huff_from_order(counts, n, m, limit, lengths, s);
}

}  // namespace nerfhip

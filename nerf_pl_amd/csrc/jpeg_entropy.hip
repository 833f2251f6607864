// Huffman-decoding a batch of baseline JPEG scans on the device, by self-synchronising passes (Weissenberger & Schmidt, "Massively
// Parallel Huffman Decoding on GPUs", ICPP 2018): the bit stream of every restart interval is cut into subsequences of S bits, one
// thread each; a decoder started at a wrong position falls into step with the true one, so every thread carries its exit state on
// into the following subsequences until what it finds there is what it would have written.  The symbol step, the tables and the bit
// fetch are jpeg_huff.h's, shared with the sequential host decoder of jpeg.hip, whose coefficients these equal bit for bit.
//
//   jent_count     1 thread / 64-byte chunk of a scan: classifies the bytes (data, stuffing, RSTm, end), counts data bytes and markers
//   jent_prepare   1 workgroup / image: checks the image's sizes, builds its Huffman tables, turns the counts into offsets (scan)
//   jent_compact   1 thread / chunk: the data bytes to their place; where each restart interval's data starts and ends; the
//                  markers' numbers
//   jent_cut       1 workgroup / image: the markers' count; cuts the intervals into subsequences (offsets scan)
//   jent_map       1 thread / subsequence: its restart interval (binary search)
//   jent_sync      256 subsequences / workgroup: decode from (start, slot 0, k 0), then lockstep rounds inside the workgroup
//   jent_carry     1 thread / workgroup boundary and round: the last record of a workgroup carried on into the next one's
//   jent_offsets   1 workgroup / image: exclusive scan of the records' block counts
//   jent_emit      1 thread / subsequence: decode again from the true entry state, store the non-zero coefficients
//   jent_dc        1 workgroup / image: DC differences -> DC values (prefix sums in decode order, reset per restart interval)
//
// No kernel waits on another workgroup; every loop is bounded by its arguments (a symbol consumes at least one bit).  The data
// bytes are read from global memory through bounds-checked dword fetches, the tables from LDS in jent_sync and jent_emit.
// nerfhip_jpeg_entropy_decode_split runs the same steps on the host (no GPU): the per-thread bodies of map, carry and emit are the
// very functions the kernels call; prepare, sync, offsets and dc are restated without barriers.
#include <limits.h>

#include "block_scan.h"
#include "common.h"
#include "jpeg_huff.h"

namespace {

using namespace nerfhip;
using namespace nerfhip::jpeg;

constexpr int kNT = 256;                 // threads per workgroup = subsequences per workgroup
constexpr int kChunk = 64;               // scan bytes one thread classifies at a time
constexpr int64_t kMaxScan = (int64_t)1 << 28;   // bit positions stay below 2^31

// What the kernels need of the frame: per slot (block inside the MCU) 4-bit fields, per component 4-bit fields.
struct Geom {
    int n_comp, n_slots, mcus_x, mcus_y;
    uint32_t dc_ids, ac_ids;             // slot -> table index (DC 0..3, AC 4..7)
    uint32_t comp_of, xx_of, yy_of;      // slot -> component, block column / row inside the MCU
    uint32_t hs, vs;                     // component -> sampling factors
};
NH_HD inline int comp_h(const Geom& g, int c) { return (int)((g.hs >> (4 * c)) & 15); }
NH_HD inline int comp_v(const Geom& g, int c) { return (int)((g.vs >> (4 * c)) & 15); }
NH_HD inline int64_t comp_blocks(const Geom& g, int c) { return (int64_t)g.mcus_x * comp_h(g, c) * g.mcus_y * comp_v(g, c); }
// raster index of block (xx, yy) of MCU `mcu` inside component c's plane of blocks
NH_HD inline int64_t raster_block(const Geom& g, int c, int64_t mcu, int xx, int yy) {
    const int h = comp_h(g, c), v = comp_v(g, c);
    const int64_t my = mcu / g.mcus_x, mx = mcu % g.mcus_x;
    return (my * v + yy) * ((int64_t)g.mcus_x * h) + mx * h + xx;
}

bool make_geom(int n_comp, const int32_t* comp, int mcus_x, int mcus_y, Geom& g) {
    if (!(n_comp == 1 || n_comp == 3) || mcus_x < 1 || mcus_y < 1 || mcus_x > 8192 || mcus_y > 8192) return false;
    g = Geom{n_comp, 0, mcus_x, mcus_y, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < n_comp; ++c) {
        const int h = comp[4 * c], v = comp[4 * c + 1], td = comp[4 * c + 2], ta = comp[4 * c + 3];
        if (h < 1 || h > 2 || v < 1 || v > 2 || td < 0 || td > 3 || ta < 0 || ta > 3) return false;
        g.hs |= (uint32_t)h << (4 * c);
        g.vs |= (uint32_t)v << (4 * c);
        for (int yy = 0; yy < v; ++yy)
            for (int xx = 0; xx < h; ++xx) {
                if (g.n_slots == 6) return false;        // more blocks per MCU than 2x2 luma + two chroma
                const int s = 4 * g.n_slots++;
                g.dc_ids |= (uint32_t)td << s;
                g.ac_ids |= (uint32_t)(4 + ta) << s;
                g.comp_of |= (uint32_t)c << s;
                g.xx_of |= (uint32_t)xx << s;
                g.yy_of |= (uint32_t)yy << s;
            }
    }
    return true;
}

// The workspace of one batch.  Everything is sized from numbers the host knows: the longest scan, the most restart intervals.
struct Layout {
    int n, S, max_int, wgs;              // images, bits per subsequence, restart intervals per image (capacity), workgroups / image
    int64_t cap;                         // subsequences per image (capacity) = wgs * 256
    int64_t words;                       // dwords of one image's compacted data
    int64_t chunks;                      // 64-byte chunks of the longest scan
    HuffTable* tables;                   // (n, 8)
    uint32_t* data;                      // (n, words): the data bytes in stream order
    int32_t* int_start;                  // (n, max_int + 1): data bytes in front of each interval
    int32_t* int_term;                   // (n, max_int): data bytes in front of the interval's first "other marker" (INT_MAX: none)
    int64_t* first_sub;                  // (n, max_int + 1): first subsequence of each interval
    int64_t* chunk_off;                  // (n, chunks): data bytes (low 32 bits) and restart markers (high) in front of each chunk
    int32_t* sub_int;                    // (n, cap): the subsequence's interval, -1 behind the last
    uint64_t* rec;                       // (n, cap): records
    uint64_t* tail;                      // (2, n, wgs): the last record of each workgroup as the carry round of that parity reads it
    int64_t* blk_off;                    // (n, cap): blocks finished in front of each subsequence
    int32_t* n_sub;                      // (n): subsequences in use
    uint16_t* dc_base;                   // (n, max_int, 3): the running DC sum in front of each interval
    int64_t* totals;                     // (n): data bytes (low 32 bits) and restart markers (high) of the whole scan
};

bool make_layout(int n, int64_t max_scan_bytes, int max_int, int S, char* base, Layout& L, size_t& bytes) {
    if (n < 1 || n > 65535 || max_scan_bytes < 1 || max_scan_bytes > kMaxScan || max_int < 1 || max_int > (1 << 26)) return false;
    if (S < 32 || S > 4096 || (S & 31)) return false;
    L.n = n;
    L.S = S;
    L.max_int = max_int;
    // an interval of b data bits takes max(1, ceil(b / S)) subsequences: all of them at most bits / S + intervals
    const int64_t subs = (max_scan_bytes * 8 + S - 1) / S + max_int;
    L.wgs = (int)((subs + kNT - 1) / kNT);
    L.cap = (int64_t)L.wgs * kNT;
    L.words = (max_scan_bytes + 3) / 4 + 1;
    L.chunks = (max_scan_bytes + kChunk - 1) / kChunk;
    if (!base) base = (char*)(uintptr_t)256;             // the size query: any aligned address, nothing is dereferenced
    char* at = base;
    L.tables = carve<HuffTable>(at, (size_t)n * 8);
    L.data = carve<uint32_t>(at, (size_t)n * L.words);
    L.int_start = carve<int32_t>(at, (size_t)n * (max_int + 1));
    L.int_term = carve<int32_t>(at, (size_t)n * max_int);
    L.first_sub = carve<int64_t>(at, (size_t)n * (max_int + 1));
    L.chunk_off = carve<int64_t>(at, (size_t)n * L.chunks);
    L.sub_int = carve<int32_t>(at, (size_t)n * L.cap);
    L.rec = carve<uint64_t>(at, (size_t)n * L.cap);
    L.tail = carve<uint64_t>(at, (size_t)2 * n * L.wgs);
    L.blk_off = carve<int64_t>(at, (size_t)n * L.cap);
    L.n_sub = carve<int32_t>(at, (size_t)n);
    L.dc_base = carve<uint16_t>(at, (size_t)n * max_int * 3);
    L.totals = carve<int64_t>(at, (size_t)n);
    bytes = (size_t)(at - base);
    return true;
}

// ---- what one subsequence is -------------------------------------------------------------------------------------------------------
struct Sub {
    int j;                               // restart interval
    int64_t q;                           // index inside the interval
    int64_t n_in_interval;               // subsequences of the interval
    int64_t start, end, valid_end;       // bits of the image's segment: [start, end) is the subsequence, valid_end the interval's end
};

NH_HD inline Sub sub_at(const Layout& L, int img, int64_t s) {
    Sub u;
    u.j = L.sub_int[(int64_t)img * L.cap + s];
    const int64_t* fs = L.first_sub + (int64_t)img * (L.max_int + 1);
    const int32_t* is = L.int_start + (int64_t)img * (L.max_int + 1);
    const int32_t term = L.int_term[(int64_t)img * L.max_int + u.j];
    u.q = s - fs[u.j];
    u.n_in_interval = fs[u.j + 1] - fs[u.j];
    const int64_t first = (int64_t)is[u.j] * 8;
    u.valid_end = (int64_t)(term < is[u.j + 1] ? term : is[u.j + 1]) * 8;
    u.start = first + u.q * L.S;
    u.end = u.start + L.S < u.valid_end ? u.start + L.S : u.valid_end;
    if (u.start > u.valid_end) u.start = u.valid_end;     // an interval without data: its one subsequence is empty
    return u;
}

NH_HD inline Segment segment_of(const Layout& L, int img) { return Segment{L.data + (int64_t)img * L.words, L.words}; }

NH_HD inline SlotTables slot_tables(const Geom& g, const HuffTable* tables) { return SlotTables{tables, g.dc_ids, g.ac_ids, g.n_slots}; }

// ---- bodies without barriers: shared by the kernels and the host twin -------------------------------------------------------------
NH_HD inline void map_body(const Layout& L, int img, int64_t s) {
    int32_t j = -1;
    if (s < L.n_sub[img]) {
        const int64_t* fs = L.first_sub + (int64_t)img * (L.max_int + 1);
        int lo = 0, hi = L.max_int;      // fs[lo] <= s < fs[hi] (the entries behind the image's last interval repeat its total)
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (fs[mid] <= s) lo = mid; else hi = mid;
        }
        j = lo;
    }
    L.sub_int[(int64_t)img * L.cap + s] = j;
}

// Round `round` at the boundary behind workgroup g: carries that workgroup's last record on into the next one's subsequences until
// one of them holds what the carried state gives, and leaves the next workgroup's last record for the next round.  True when a
// record changed.
NH_HD inline bool carry_body(const Layout& L, const Geom& g, const HuffTable* tables, int img, int wg, int round) {
    const int64_t T = L.n_sub[img], s0 = (int64_t)(wg + 1) * kNT;
    if (s0 >= T) return false;
    uint64_t* rec = L.rec + (int64_t)img * L.cap;
    const uint64_t* tail_in = L.tail + ((int64_t)(round & 1) * L.n + img) * L.wgs;
    uint64_t* tail_out = L.tail + ((int64_t)((round + 1) & 1) * L.n + img) * L.wgs;
    const int j = L.sub_int[(int64_t)img * L.cap + s0 - 1];
    const int64_t interval_end = L.first_sub[(int64_t)img * (L.max_int + 1) + j + 1];
    int64_t stop = s0 + kNT < T ? s0 + kNT : T;
    if (interval_end < stop) stop = interval_end;
    const Segment seg = segment_of(L, img);
    const SlotTables tb = slot_tables(g, tables);
    State st = record_state(tail_in[wg]);
    bool changed = false;
    for (int64_t s = s0; s < stop; ++s) {
        const Sub u = sub_at(L, img, s);
        const uint64_t now = walk(seg, u.end, u.valid_end, tb, st);
        if (now == rec[s]) break;
        rec[s] = now;
        changed = true;
        st = record_state(now);
    }
    if (s0 + kNT - 1 < T) tail_out[wg + 1] = rec[s0 + kNT - 1];
    return changed;
}

// Subsequence s again, from its true entry state: the non-zero coefficients go to coef[c] (n, blocks_c, 64).  True when the
// subsequence shows the stream to be damaged.
NH_HD inline bool emit_body(const Layout& L, const Geom& g, const HuffTable* tables, const int32_t* restart, int img, int64_t s,
                            int16_t* c0, int16_t* c1, int16_t* c2) {
    const Sub u = sub_at(L, img, s);
    const int64_t* fs = L.first_sub + (int64_t)img * (L.max_int + 1);
    const int64_t* off = L.blk_off + (int64_t)img * L.cap;
    const int64_t n_mcu = (int64_t)g.mcus_x * g.mcus_y, ri = restart[img] > 0 ? restart[img] : n_mcu;
    int64_t blk = (int64_t)u.j * ri * g.n_slots + (off[s] - off[fs[u.j]]);
    const int64_t last_mcu = (u.j + 1) * ri < n_mcu ? (u.j + 1) * ri : n_mcu;
    const int64_t limit = last_mcu * g.n_slots;
    const Segment seg = segment_of(L, img);
    const SlotTables tb = slot_tables(g, tables);
    State st = {u.start, 0, 0};
    if (u.q > 0) st = record_state(L.rec[(int64_t)img * L.cap + s - 1]);
    bool bad = false;
    int16_t* block = nullptr;
    while (st.p < u.end && blk < limit) {
        if (!block) {                    // the addresses come from the block index alone, which is below `limit`
            const int slot = (int)(blk % g.n_slots);
            const int c = (int)((g.comp_of >> (4 * slot)) & 15);
            const int64_t r = raster_block(g, c, blk / g.n_slots, (int)((g.xx_of >> (4 * slot)) & 15), (int)((g.yy_of >> (4 * slot)) & 15));
            block = (c == 0 ? c0 : (c == 1 ? c1 : c2)) + ((int64_t)img * comp_blocks(g, c) + r) * 64;
        }
        const Symbol sym = step(seg, u.valid_end, tb, st);
        bad = bad || sym.bad || st.p > u.valid_end;      // the symbol reached behind the interval's data
        if (sym.has_value && sym.value != 0) block[zigzag(sym.at)] = (int16_t)sym.value;
        if (sym.finished) {
            ++blk;
            block = nullptr;
        }
    }
    if (u.q + 1 == u.n_in_interval && blk < limit) bad = true;   // the interval's data ends before its last MCU
    return bad;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------
struct Batch {
    const uint8_t* scans;
    const int64_t* offsets;
    const uint8_t* huffman;
    const int32_t* masks;
    const int32_t* restart;
    int64_t total_bytes, max_scan_bytes;
};

__device__ __forceinline__ void stage_tables(HuffTable* lds, const HuffTable* global) {
    const uint32_t* src = (const uint32_t*)global;
    uint32_t* dst = (uint32_t*)lds;
    for (int i = threadIdx.x; i < (int)(8 * sizeof(HuffTable) / 4); i += kNT) dst[i] = src[i];
    __syncthreads();
}

// data bytes and restart markers of chunk c of a scan, as low and high half of one value
NH_HD inline int64_t chunk_counts(const uint8_t* scan, int64_t n, int64_t c) {
    int64_t v = 0;
    const int64_t end = (c + 1) * kChunk < n ? (c + 1) * kChunk : n;
    for (int64_t i = c * kChunk; i < end; ++i) {
        const int cls = classify(scan, n, i);
        v += cls == kData ? 1 : (cls == kRestart ? ((int64_t)1 << 32) : 0);
    }
    return v;
}

NH_HD inline int64_t intervals_of(const Geom& g, int32_t ri) {
    const int64_t n_mcu = (int64_t)g.mcus_x * g.mcus_y;
    return ri > 0 ? (n_mcu + ri - 1) / ri : 1;
}

NH_HD inline int64_t subs_of_interval(const Layout& L, int img, int64_t j) {
    const int32_t* is = L.int_start + (int64_t)img * (L.max_int + 1);
    const int32_t term = L.int_term[(int64_t)img * L.max_int + j];
    const int64_t bits = (int64_t)((term < is[j + 1] ? term : is[j + 1]) - is[j]) * 8;
    const int64_t n = (bits + L.S - 1) / L.S;
    return n > 0 ? n : 1;
}

// 0, or NERFHIP_E_BADARG for an image whose offsets, restart interval or sizes the batch's arguments do not cover
NH_HD inline int check_image(const Batch& b, const Layout& L, const Geom& g, int img) {
    const int64_t o0 = b.offsets[img], o1 = b.offsets[img + 1];
    const int32_t ri = b.restart[img];
    return (o0 < 0 || o1 <= o0 || o1 > b.total_bytes || o1 - o0 > b.max_scan_bytes || ri < 0 || intervals_of(g, ri) > L.max_int)
               ? NERFHIP_E_BADARG : 0;
}

// grid (ceil(chunks / 256), n): data bytes and restart markers of every 64-byte chunk
__global__ void __launch_bounds__(kNT) jent_count(Batch b, Layout L, Geom g) {
    const int img = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (check_image(b, L, g, img) != 0) return;
    const int64_t n = b.offsets[img + 1] - b.offsets[img];
    if (c < (n + kChunk - 1) / kChunk) L.chunk_off[(int64_t)img * L.chunks + c] = chunk_counts(b.scans + b.offsets[img], n, c);
}

// grid n: the image's verdict so far, its tables, the chunks' counts -> their offsets
__global__ void __launch_bounds__(kNT) jent_prepare(Batch b, Layout L, Geom g, int32_t* __restrict__ status, int32_t* __restrict__ progress) {
    const int img = blockIdx.x, t = threadIdx.x;
    __shared__ int verdict;
    if (t == 0) {
        L.n_sub[img] = 0;
        if (img == 0) *progress = 0;
        verdict = check_image(b, L, g, img);
    }
    __syncthreads();
    if (verdict != 0) {
        if (t == 0) status[img] = verdict;
        return;
    }
    __syncthreads();
    const int64_t n = b.offsets[img + 1] - b.offsets[img];
    const int n_int = (int)intervals_of(g, b.restart[img]);
    int32_t* term = L.int_term + (int64_t)img * L.max_int;
    HuffTable* tables = L.tables + (int64_t)img * 8;
    if (t < 8) {
        tables[t].present = false;
        if ((b.masks[img] >> t) & 1)
            if (!build_table(b.huffman + ((int64_t)img * 8 + t) * 272, tables[t])) verdict = NERFHIP_E_DATA;   // (every writer stores this value)
    }
    for (int j = t; j < n_int; j += kNT) term[j] = INT_MAX;
    int64_t* coff = L.chunk_off + (int64_t)img * L.chunks;
    // in place: thread i % 256 reads count i before it writes offset i
    const int64_t totals = block_offsets_scan<kNT>((n + kChunk - 1) / kChunk, coff, [&](int64_t c) { return coff[c]; });
    if (t == 0) {
        L.totals[img] = totals;
        L.int_start[(int64_t)img * (L.max_int + 1)] = 0;
        for (int c = 0; c < g.n_slots; ++c)
            if (!tables[(g.dc_ids >> (4 * c)) & 15].present || !tables[(g.ac_ids >> (4 * c)) & 15].present) verdict = NERFHIP_E_DATA;
    }
    __syncthreads();
    if (t == 0) status[img] = verdict;
}

// grid (ceil(chunks / 256), n): every chunk's data bytes to their place, the restart markers' and end markers' positions
__global__ void __launch_bounds__(kNT) jent_compact(Batch b, Layout L, Geom g, int32_t* __restrict__ status) {
    const int img = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (status[img] != 0) return;        // (as jent_prepare left it: nobody writes 0 here)
    const uint8_t* scan = b.scans + b.offsets[img];
    const int64_t n = b.offsets[img + 1] - b.offsets[img];
    if (c >= (n + kChunk - 1) / kChunk) return;
    const int n_int = (int)intervals_of(g, b.restart[img]);
    int32_t* is = L.int_start + (int64_t)img * (L.max_int + 1);
    int32_t* term = L.int_term + (int64_t)img * L.max_int;
    uint8_t* out = (uint8_t*)(L.data + (int64_t)img * L.words);
    const int64_t at = L.chunk_off[(int64_t)img * L.chunks + c];
    int32_t d = (int32_t)(at & 0xffffffff);
    int64_t m = at >> 32;
    const int64_t end = (c + 1) * kChunk < n ? (c + 1) * kChunk : n;
    for (int64_t i = c * kChunk; i < end; ++i) {
        const int cls = classify(scan, n, i);
        if (cls == kData) {
            out[d++] = scan[i];
        } else if (cls == kRestart) {
            if (m < n_int) is[m + 1] = d;
            if (m < n_int - 1 && scan[i + 1] != 0xd0 + (m & 7)) status[img] = NERFHIP_E_DATA;
            ++m;
        } else if (cls == kStop) {
            if (m < n_int) atomicMin(&term[m], d);
        }
    }
}

// grid n: the markers' count, then the intervals cut into subsequences
__global__ void __launch_bounds__(kNT) jent_cut(Batch b, Layout L, Geom g, int32_t* __restrict__ status) {
    const int img = blockIdx.x, t = threadIdx.x;
    __shared__ int verdict;
    if (t == 0) {
        int v = status[img];
        if (v == 0) {
            const int n_int = (int)intervals_of(g, b.restart[img]);
            const int64_t n_data = L.totals[img] & 0xffffffff, n_markers = L.totals[img] >> 32;
            if (n_markers < n_int) L.int_start[(int64_t)img * (L.max_int + 1) + n_int] = (int32_t)n_data;
            if (n_markers < n_int - 1) v = NERFHIP_E_DATA;
            status[img] = v;
        }
        verdict = v;
    }
    __syncthreads();
    if (verdict != 0) return;
    const int n_int = (int)intervals_of(g, b.restart[img]);
    int64_t* fs = L.first_sub + (int64_t)img * (L.max_int + 1);
    const int64_t T = block_offsets_scan<kNT>(n_int, fs, [&](int64_t j) { return subs_of_interval(L, img, j); });
    for (int j = n_int + t; j <= L.max_int; j += kNT) fs[j] = T;
    if (t == 0) L.n_sub[img] = (int32_t)T;
}

__global__ void __launch_bounds__(kNT) jent_map(Layout L) {
    map_body(L, blockIdx.y, (int64_t)blockIdx.x * kNT + threadIdx.x);
}

__global__ void __launch_bounds__(kNT) jent_sync(Layout L, Geom g) {
    __shared__ uint32_t table_words[8 * sizeof(HuffTable) / 4];
    HuffTable* const tables = (HuffTable*)table_words;
    const int img = blockIdx.y, t = threadIdx.x;
    const int64_t T = L.n_sub[img], s = (int64_t)blockIdx.x * kNT + t;
    if ((int64_t)blockIdx.x * kNT >= T) return;          // (the whole workgroup)
    stage_tables(tables, L.tables + (int64_t)img * 8);
    const Segment seg = segment_of(L, img);
    const SlotTables tb = slot_tables(g, tables);
    uint64_t* rec = L.rec + (int64_t)img * L.cap;
    bool active = s < T;
    State st = {0, 0, 0};
    int64_t interval_end = 0;
    if (active) {
        const Sub u = sub_at(L, img, s);
        interval_end = s - u.q + u.n_in_interval;
        const uint64_t r = walk(seg, u.end, u.valid_end, tb, State{u.start, 0, 0});
        rec[s] = r;
        st = record_state(r);
    }
    __syncthreads();
    // Round r: thread t carries its state into subsequence s + r.  Only this thread writes that record in this round; all reads of
    // the round come before the barrier, all writes behind it.
    for (int r = 1; r < kNT; ++r) {
        active = active && t + r < kNT && s + r < interval_end;
        uint64_t now = 0, old = 0;
        if (active) {
            const Sub u = sub_at(L, img, s + r);
            now = walk(seg, u.end, u.valid_end, tb, st);
            old = rec[s + r];
        }
        __syncthreads();
        active = active && now != old;
        if (active) {
            rec[s + r] = now;
            st = record_state(now);
        }
        if (!__syncthreads_or(active ? 1 : 0)) break;
    }
    if (t == kNT - 1 && s < T) {
        L.tail[((int64_t)0 * L.n + img) * L.wgs + blockIdx.x] = rec[s];
        L.tail[((int64_t)1 * L.n + img) * L.wgs + blockIdx.x] = rec[s];
    }
}

// grid (ceil((wgs - 1) / 64), n).  Returns at once when the round before changed nothing.
__global__ void __launch_bounds__(64) jent_carry(Layout L, Geom g, int round, int32_t* __restrict__ progress) {
    if (*(volatile int32_t*)progress < round - 1) return;
    const int img = blockIdx.y, wg = blockIdx.x * 64 + threadIdx.x;
    if (wg >= L.wgs - 1) return;
    if (carry_body(L, g, L.tables + (int64_t)img * 8, img, wg, round)) atomicMax(progress, round);
}

__global__ void __launch_bounds__(kNT) jent_offsets(Layout L) {
    const int img = blockIdx.x;
    const uint64_t* rec = L.rec + (int64_t)img * L.cap;
    block_offsets_scan<kNT>(L.n_sub[img], L.blk_off + (int64_t)img * L.cap, [&](int64_t s) { return record_blocks(rec[s]); });
}

__global__ void __launch_bounds__(kNT) jent_emit(Layout L, Geom g, const int32_t* __restrict__ restart, int16_t* __restrict__ c0,
                                                 int16_t* __restrict__ c1, int16_t* __restrict__ c2, int32_t* __restrict__ status) {
    __shared__ uint32_t table_words[8 * sizeof(HuffTable) / 4];
    HuffTable* const tables = (HuffTable*)table_words;
    const int img = blockIdx.y;
    const int64_t T = L.n_sub[img], s = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if ((int64_t)blockIdx.x * kNT >= T) return;
    stage_tables(tables, L.tables + (int64_t)img * 8);
    if (s < T && emit_body(L, g, tables, restart, img, s, c0, c1, c2)) status[img] = NERFHIP_E_DATA;
}

// element e of component c in decode order -> its DC coefficient
NH_HD inline int16_t* dc_at(const Geom& g, int c, int16_t* coef, int img, int64_t e) {
    const int h = comp_h(g, c), bc = h * comp_v(g, c);
    const int b = (int)(e % bc);
    return coef + ((int64_t)img * comp_blocks(g, c) + raster_block(g, c, e / bc, b % h, b / h)) * 64;
}

__global__ void __launch_bounds__(kNT) jent_dc(Layout L, Geom g, const int32_t* __restrict__ restart, int16_t* __restrict__ c0,
                                               int16_t* __restrict__ c1, int16_t* __restrict__ c2, const int32_t* __restrict__ status) {
    const int img = blockIdx.x, t = threadIdx.x;
    if (status[img] != 0) return;
    const int64_t n_mcu = (int64_t)g.mcus_x * g.mcus_y;
    const int n_int = (int)intervals_of(g, restart[img]);
    const int64_t ri = restart[img] > 0 ? restart[img] : n_mcu;
    uint16_t* base = L.dc_base + (int64_t)img * L.max_int * 3;
    for (int c = 0; c < g.n_comp; ++c) {
        int16_t* coef = c == 0 ? c0 : (c == 1 ? c1 : c2);
        const int bc = comp_h(g, c) * comp_v(g, c);
        const int64_t count = n_mcu * bc;
        uint32_t carry = 0;              // sums modulo 2^16 are all that an int16 coefficient keeps
        for (int64_t first = 0; first < count; first += kNT) {
            const int64_t e = first + t;
            int16_t* at = e < count ? dc_at(g, c, coef, img, e) : nullptr;
            const uint32_t v = at ? (uint32_t)(uint16_t)*at : 0u;
            uint32_t total;
            const uint32_t ex = block_excl_scan<kNT, uint32_t>(v, total);
            if (at) *at = (int16_t)(uint16_t)(carry + ex + v);
            carry += total;
        }
        if (n_int > 1) {
            __syncthreads();
            for (int j = 1 + t; j < n_int; j += kNT) base[j * 3 + c] = (uint16_t)*dc_at(g, c, coef, img, (int64_t)j * ri * bc - 1);
            __syncthreads();
            for (int64_t e = ri * bc + t; e < count; e += kNT) {
                int16_t* at = dc_at(g, c, coef, img, e);
                *at = (int16_t)(uint16_t)((uint16_t)*at - base[(e / bc / ri) * 3 + c]);
            }
        }
        __syncthreads();
    }
}

// ---- argument checks shared by the entry points ---------------------------------------------------------------------------------------
int plan(const nerfhip_jpeg_batch* a, Layout& L, Geom& g, Batch& b) {
    NERFHIP_CHECK_ARG(a);
    size_t bytes;
    NERFHIP_CHECK_ARG(make_geom(a->n_comp, a->comp, a->mcus_x, a->mcus_y, g));
    NERFHIP_CHECK_ARG(a->workspace && make_layout(a->n_images, a->max_scan_bytes, a->max_intervals, a->subseq_bits, (char*)a->workspace, L, bytes));
    NERFHIP_CHECK_ARG(a->scans && a->offsets && a->huffman && a->huffman_masks && a->restart_intervals && a->status && a->progress);
    NERFHIP_CHECK_ARG(a->total_bytes >= 1);
    if (((uintptr_t)a->workspace & 255) || ((uintptr_t)a->offsets & 7) || (((uintptr_t)a->huffman_masks | (uintptr_t)a->restart_intervals |
                                                                           (uintptr_t)a->status | (uintptr_t)a->progress) & 3))
        return NERFHIP_E_ALIGN;
    b = Batch{a->scans, a->offsets, a->huffman, a->huffman_masks, a->restart_intervals, a->total_bytes, a->max_scan_bytes};
    return 0;
}

int check_coef(const Geom& g, int16_t* c0, int16_t* c1, int16_t* c2) {
    NERFHIP_CHECK_ARG(c0 && (g.n_comp == 1 || (c1 && c2)));
    if (((uintptr_t)c0 | (uintptr_t)c1 | (uintptr_t)c2) & 1) return NERFHIP_E_ALIGN;
    return 0;
}

void launch_rounds(const Layout& L, const Geom& g, int first, int count, int32_t* progress, hipStream_t s) {
    if (L.wgs < 2) return;
    for (int r = first; r < first + count; ++r)
        hipLaunchKernelGGL(jent_carry, dim3((unsigned)((L.wgs - 1 + 63) / 64), (unsigned)L.n), dim3(64), 0, s, L, g, r, progress);
}

}  // namespace

extern "C" size_t nerfhip_jpeg_entropy_workspace_bytes(int n_images, int64_t max_scan_bytes, int max_intervals, int subseq_bits) {
    Layout L;
    size_t bytes = 0;
    return make_layout(n_images, max_scan_bytes, max_intervals, subseq_bits, nullptr, L, bytes) ? bytes : 0;
}

extern "C" int nerfhip_jpeg_entropy_workgroups(int64_t max_scan_bytes, int max_intervals, int subseq_bits) {
    Layout L;
    size_t bytes = 0;
    return make_layout(1, max_scan_bytes, max_intervals, subseq_bits, nullptr, L, bytes) ? L.wgs : 0;
}

extern "C" int nerfhip_jpeg_entropy_sync(const nerfhip_jpeg_batch* a, int rounds, nerfhip_stream_t stream) {
    Layout L;
    Geom g;
    Batch b;
    const int e = plan(a, L, g, b);
    if (e) return e;
    NERFHIP_CHECK_ARG(rounds >= 0 && rounds <= 64);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 chunk_grid((unsigned)((L.chunks + kNT - 1) / kNT), (unsigned)L.n);
    hipLaunchKernelGGL(jent_count, chunk_grid, dim3(kNT), 0, s, b, L, g);
    hipLaunchKernelGGL(jent_prepare, dim3((unsigned)L.n), dim3(kNT), 0, s, b, L, g, a->status, a->progress);
    hipLaunchKernelGGL(jent_compact, chunk_grid, dim3(kNT), 0, s, b, L, g, a->status);
    hipLaunchKernelGGL(jent_cut, dim3((unsigned)L.n), dim3(kNT), 0, s, b, L, g, a->status);
    hipLaunchKernelGGL(jent_map, dim3((unsigned)L.wgs, (unsigned)L.n), dim3(kNT), 0, s, L);
    hipLaunchKernelGGL(jent_sync, dim3((unsigned)L.wgs, (unsigned)L.n), dim3(kNT), 0, s, L, g);
    launch_rounds(L, g, 1, rounds, a->progress, s);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_jpeg_entropy_rounds(const nerfhip_jpeg_batch* a, int first_round, int rounds, nerfhip_stream_t stream) {
    Layout L;
    Geom g;
    Batch b;
    const int e = plan(a, L, g, b);
    if (e) return e;
    NERFHIP_CHECK_ARG(first_round >= 1 && rounds >= 0 && rounds <= 64 && first_round <= (1 << 24));
    launch_rounds(L, g, first_round, rounds, a->progress, (hipStream_t)stream);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_jpeg_entropy_emit(const nerfhip_jpeg_batch* a, int16_t* coef_y, int16_t* coef_cb, int16_t* coef_cr,
                                         nerfhip_stream_t stream) {
    Layout L;
    Geom g;
    Batch b;
    int e = plan(a, L, g, b);
    if (e) return e;
    e = check_coef(g, coef_y, coef_cb, coef_cr);
    if (e) return e;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jent_offsets, dim3((unsigned)L.n), dim3(kNT), 0, s, L);
    hipLaunchKernelGGL(jent_emit, dim3((unsigned)L.wgs, (unsigned)L.n), dim3(kNT), 0, s, L, g, b.restart, coef_y, coef_cb, coef_cr, a->status);
    hipLaunchKernelGGL(jent_dc, dim3((unsigned)L.n), dim3(kNT), 0, s, L, g, b.restart, coef_y, coef_cb, coef_cr, (const int32_t*)a->status);
    return nerfhip_launch_status();
}

// ---- the host twin -------------------------------------------------------------------------------------------------------------------
namespace {

void host_prepare(const Batch& b, const Layout& L, const Geom& g, int img, int32_t* status) {
    L.n_sub[img] = 0;
    if (check_image(b, L, g, img) != 0) {
        status[img] = NERFHIP_E_BADARG;
        return;
    }
    const int64_t o0 = b.offsets[img], o1 = b.offsets[img + 1];
    const int32_t ri = b.restart[img];
    int verdict = 0;
    const uint8_t* scan = b.scans + o0;
    const int64_t n = o1 - o0;
    const int n_int = (int)intervals_of(g, ri);
    int32_t* is = L.int_start + (int64_t)img * (L.max_int + 1);
    int32_t* term = L.int_term + (int64_t)img * L.max_int;
    int64_t* fs = L.first_sub + (int64_t)img * (L.max_int + 1);
    HuffTable* tables = L.tables + (int64_t)img * 8;
    for (int t = 0; t < 8; ++t) {
        tables[t].present = false;
        if ((b.masks[img] >> t) & 1)
            if (!build_table(b.huffman + ((int64_t)img * 8 + t) * 272, tables[t])) verdict = NERFHIP_E_DATA;
    }
    for (int j = 0; j < n_int; ++j) term[j] = INT_MAX;
    uint8_t* out = (uint8_t*)(L.data + (int64_t)img * L.words);
    int32_t d = 0;
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int cls = classify(scan, n, i);
        if (cls == kData) {
            out[d++] = scan[i];
        } else if (cls == kRestart) {
            if (m < n_int) is[m + 1] = d;
            if (m < n_int - 1 && scan[i + 1] != 0xd0 + (m & 7)) verdict = NERFHIP_E_DATA;
            ++m;
        } else if (cls == kStop) {
            if (m < n_int && d < term[m]) term[m] = d;
        }
    }
    for (int64_t i = d; i < L.words * 4; ++i) out[i] = 0;        // (the device leaves them undefined: they are never delivered)
    is[0] = 0;
    if (m < n_int) is[n_int] = d;
    if (m < n_int - 1) verdict = NERFHIP_E_DATA;
    for (int c = 0; c < g.n_slots; ++c)
        if (!tables[(g.dc_ids >> (4 * c)) & 15].present || !tables[(g.ac_ids >> (4 * c)) & 15].present) verdict = NERFHIP_E_DATA;
    status[img] = verdict;
    if (verdict != 0) return;
    int64_t T = 0;
    for (int j = 0; j < n_int; ++j) {
        fs[j] = T;
        T += subs_of_interval(L, img, j);
    }
    for (int j = n_int; j <= L.max_int; ++j) fs[j] = T;
    L.n_sub[img] = (int32_t)T;
}

// jent_sync's workgroup `wg`, its threads in lockstep
void host_sync(const Layout& L, const Geom& g, int img, int wg) {
    const int64_t T = L.n_sub[img], base = (int64_t)wg * kNT;
    if (base >= T) return;
    const HuffTable* tables = L.tables + (int64_t)img * 8;
    const Segment seg = segment_of(L, img);
    const SlotTables tb = slot_tables(g, tables);
    uint64_t* rec = L.rec + (int64_t)img * L.cap;
    bool active[kNT];
    State st[kNT];
    int64_t interval_end[kNT];
    uint64_t now[kNT], old[kNT];
    for (int t = 0; t < kNT; ++t) {
        const int64_t s = base + t;
        active[t] = s < T;
        if (!active[t]) continue;
        const Sub u = sub_at(L, img, s);
        interval_end[t] = s - u.q + u.n_in_interval;
        rec[s] = walk(seg, u.end, u.valid_end, tb, State{u.start, 0, 0});
        st[t] = record_state(rec[s]);
    }
    for (int r = 1; r < kNT; ++r) {
        for (int t = 0; t < kNT; ++t) {
            const int64_t s = base + t;
            active[t] = active[t] && t + r < kNT && s + r < interval_end[t];
            if (!active[t]) continue;
            const Sub u = sub_at(L, img, s + r);
            now[t] = walk(seg, u.end, u.valid_end, tb, st[t]);
            old[t] = rec[s + r];
        }
        bool any = false;
        for (int t = 0; t < kNT; ++t) {
            active[t] = active[t] && now[t] != old[t];
            if (!active[t]) continue;
            rec[base + t + r] = now[t];
            st[t] = record_state(now[t]);
            any = true;
        }
        if (!any) break;
    }
    if (base + kNT - 1 < T)
        L.tail[((int64_t)0 * L.n + img) * L.wgs + wg] = L.tail[((int64_t)1 * L.n + img) * L.wgs + wg] = rec[base + kNT - 1];
}

void host_dc(const Layout& L, const Geom& g, const int32_t* restart, int img, int16_t* c0, int16_t* c1, int16_t* c2) {
    const int64_t n_mcu = (int64_t)g.mcus_x * g.mcus_y, ri = restart[img] > 0 ? restart[img] : n_mcu;
    for (int c = 0; c < g.n_comp; ++c) {
        int16_t* coef = c == 0 ? c0 : (c == 1 ? c1 : c2);
        const int bc = comp_h(g, c) * comp_v(g, c);
        uint32_t sum = 0;
        for (int64_t e = 0; e < n_mcu * bc; ++e) {
            if ((e / bc) % ri == 0 && e % bc == 0) sum = 0;
            int16_t* at = dc_at(g, c, coef, img, e);
            sum += (uint16_t)*at;
            *at = (int16_t)(uint16_t)sum;
        }
    }
}

}  // namespace

extern "C" int nerfhip_jpeg_entropy_decode_split(const nerfhip_jpeg_batch* a, int16_t* coef_y, int16_t* coef_cb, int16_t* coef_cr) {
    Layout L;
    Geom g;
    Batch b;
    int e = plan(a, L, g, b);
    if (e) return e;
    e = check_coef(g, coef_y, coef_cb, coef_cr);
    if (e) return e;
    int32_t* status = a->status;
    *a->progress = 0;
    for (int img = 0; img < L.n; ++img) {
        host_prepare(b, L, g, img, status);
        for (int64_t s = 0; s < L.cap; ++s) map_body(L, img, s);
        for (int wg = 0; wg < L.wgs; ++wg) host_sync(L, g, img, wg);
    }
    // the rounds between workgroups, every boundary of a round before the next round: at most (workgroups + 1) of them
    for (int round = 1; round <= L.wgs + 1 && *a->progress >= round - 1; ++round)
        for (int img = 0; img < L.n; ++img)
            for (int wg = 0; wg + 1 < L.wgs; ++wg)
                if (carry_body(L, g, L.tables + (int64_t)img * 8, img, wg, round)) *a->progress = round;
    for (int img = 0; img < L.n; ++img) {
        const int64_t T = L.n_sub[img];
        int64_t sum = 0;
        for (int64_t s = 0; s < T; ++s) {
            L.blk_off[(int64_t)img * L.cap + s] = sum;
            sum += record_blocks(L.rec[(int64_t)img * L.cap + s]);
        }
        for (int64_t s = 0; s < T; ++s)
            if (emit_body(L, g, L.tables + (int64_t)img * 8, b.restart, img, s, coef_y, coef_cb, coef_cr)) status[img] = NERFHIP_E_DATA;
        if (status[img] == 0) host_dc(L, g, b.restart, img, coef_y, coef_cb, coef_cr);
    }
    return 0;
}

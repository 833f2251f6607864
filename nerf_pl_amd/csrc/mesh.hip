// Mesh extraction from a sigma grid (extract_color_mesh.py:144-285): marching cubes, largest-cluster cleanup, vertex normals
// and per-view colour fusion.  Every kernel is one thread per lattice point / triangle / vertex; the only cross-block
// communication is the block-total scan (one workgroup, block_scan.h's offsets scan) between two launches.  Layouts and byte
// counts: DESIGN.md, mesh.
#include "block_scan.h"
#include "common.h"
#include "mc_tables.h"

namespace {

using nerfhip::block_excl_scan;
using nerfhip::carve;

constexpr int kBlock = 256;        // threads of every per-element kernel here (4 waves)
constexpr int kScanBlock = 1024;   // the single workgroup that scans the block totals

// Bourke edge e -> (offset of its lower corner in the cell, axis): mc_tables.h for the corner and edge numbering.
__constant__ const unsigned char kEdgeOwner[12][4] = {{0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1},
                                                      {0, 0, 1, 0}, {1, 0, 1, 1}, {0, 1, 1, 0}, {0, 0, 1, 1},
                                                      {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};
__constant__ const unsigned char kCorner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0},
                                                  {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};

__device__ __forceinline__ int tri_count(int c) {
    int n = 0;
    while (n < 5 && nerfhip::kMcTriTable[c][3 * n] >= 0) ++n;
    return n;
}

// ---- marching cubes -----------------------------------------------------------------------------------------------------------
struct McWs {
    unsigned char* mask;   // (npts) bit k: the +a_k edge of the point is crossed
    unsigned char* cube;   // (npts) Bourke case of the cell whose minimum corner is the point (0 where there is no cell)
    int32_t* vbase;        // (npts) id of the point's first vertex
    int32_t* blk_v;        // (nb) per-block vertex / triangle totals
    int32_t* blk_t;
    int64_t* off_v;        // (nb) exclusive block offsets
    int64_t* off_t;
};

__host__ __device__ inline McWs mc_ws(void* base, int64_t npts, size_t* bytes) {
    const int64_t nb = (npts + kBlock - 1) / kBlock;
    char* p = (char*)base;
    McWs w;
    w.mask = carve<unsigned char>(p, npts);
    w.cube = carve<unsigned char>(p, npts);
    w.vbase = carve<int32_t>(p, npts);
    w.blk_v = carve<int32_t>(p, nb);
    w.blk_t = carve<int32_t>(p, nb);
    w.off_v = carve<int64_t>(p, nb);
    w.off_t = carve<int64_t>(p, nb);
    if (bytes) *bytes = (size_t)(p - (char*)base);
    return w;
}

// Pass 1: per point its crossed-edge mask and cube case; per block the vertex and triangle totals.
__global__ void __launch_bounds__(kBlock) mc_count(const float* __restrict__ vol, int n0, int n1, int n2, double iso, McWs w) {
    const int64_t npts = (int64_t)n0 * n1 * n2;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int nv = 0, nt = 0;
    if (p < npts) {
        const int a2 = (int)(p % n2), a1 = (int)((p / n2) % n1), a0 = (int)(p / ((int64_t)n1 * n2));
        const int64_t s0 = (int64_t)n1 * n2, s1 = n2;
        const bool b = (double)vol[p] < iso;
        int m = 0;
        if (a0 + 1 < n0 && (((double)vol[p + s0] < iso) != b)) m |= 1;
        if (a1 + 1 < n1 && (((double)vol[p + s1] < iso) != b)) m |= 2;
        if (a2 + 1 < n2 && (((double)vol[p + 1] < iso) != b)) m |= 4;
        int c = 0;
        if (a0 + 1 < n0 && a1 + 1 < n1 && a2 + 1 < n2) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t q = p + kCorner[i][0] * s0 + kCorner[i][1] * s1 + kCorner[i][2];
                c |= ((double)vol[q] < iso) << i;
            }
            nt = tri_count(c);
        }
        nv = __popc(m);
        w.mask[p] = (unsigned char)m;
        w.cube[p] = (unsigned char)c;
    }
    int tv, tt;
    block_excl_scan<kBlock>(nv, tv);
    block_excl_scan<kBlock>(nt, tt);
    if (threadIdx.x == 0) {
        w.blk_v[blockIdx.x] = tv;
        w.blk_t[blockIdx.x] = tt;
    }
}

// One workgroup: exclusive offsets of two per-block total arrays (lengths na, nb) and their sums -> totals[0], totals[1].
__global__ void __launch_bounds__(kScanBlock) scan_totals(const int32_t* __restrict__ a, int64_t na, int64_t* __restrict__ off_a,
                                                          const int32_t* __restrict__ b, int64_t nb, int64_t* __restrict__ off_b,
                                                          int64_t* __restrict__ totals) {
    for (int which = 0; which < 2; ++which) {
        const int32_t* in = which ? b : a;
        const int64_t sum = nerfhip::block_offsets_scan<kScanBlock>(which ? nb : na, which ? off_b : off_a, [&](int64_t i) { return in[i]; });
        if (threadIdx.x == 0) totals[which] = sum;
    }
}

// Pass 2: vertex ids and positions.  Vertices are ordered by (owning point in C order, axis).
__global__ void __launch_bounds__(kBlock) mc_emit_vertices(const float* __restrict__ vol, int n0, int n1, int n2, double iso, McWs w,
                                                           const int64_t* __restrict__ totals, double* __restrict__ verts) {
    if (totals[0] > INT32_MAX || totals[1] > INT32_MAX) return;       // the caller refuses such a mesh; write nothing
    const int64_t npts = (int64_t)n0 * n1 * n2;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int m = p < npts ? w.mask[p] : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>((int)__popc(m), tot);
    if (p >= npts) return;
    const int64_t id0 = w.off_v[blockIdx.x] + ex;
    w.vbase[p] = (int32_t)id0;
    if (!m) return;
    const int a2 = (int)(p % n2), a1 = (int)((p / n2) % n1), a0 = (int)(p / ((int64_t)n1 * n2));
    const int64_t stride[3] = {(int64_t)n1 * n2, n2, 1};
    const double fa = (double)vol[p];
    int64_t id = id0;
    for (int k = 0; k < 3; ++k) {
        if (!((m >> k) & 1)) continue;
        const double fb = (double)vol[p + stride[k]];
        const double t = fa == fb ? 0.5 : (iso - fa) / (fb - fa);
        double x[3] = {(double)a0, (double)a1, (double)a2};
        x[k] = x[k] + t;
        verts[3 * id + 0] = x[0];
        verts[3 * id + 1] = x[1];
        verts[3 * id + 2] = x[2];
        ++id;
    }
}

// Pass 3: triangles, ordered by (cell in C order, table order); each corner is the id of the vertex on that lattice edge.
__global__ void __launch_bounds__(kBlock) mc_emit_triangles(int n0, int n1, int n2, McWs w, const int64_t* __restrict__ totals,
                                                            int32_t* __restrict__ tris) {
    if (totals[0] > INT32_MAX || totals[1] > INT32_MAX) return;
    const int64_t npts = (int64_t)n0 * n1 * n2;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int c = p < npts ? w.cube[p] : 0;
    const int nt = tri_count(c);
    int tot;
    const int ex = block_excl_scan<kBlock>(nt, tot);
    if (p >= npts || !nt) return;
    const int64_t s0 = (int64_t)n1 * n2, s1 = n2;
    int64_t t = w.off_t[blockIdx.x] + ex;
    for (int j = 0; j < nt; ++j, ++t) {
        for (int k = 0; k < 3; ++k) {
            const int e = nerfhip::kMcTriTable[c][3 * j + k];
            const int64_t q = p + kEdgeOwner[e][0] * s0 + kEdgeOwner[e][1] * s1 + kEdgeOwner[e][2];
            const int ax = kEdgeOwner[e][3];
            tris[3 * t + k] = w.vbase[q] + __popc(w.mask[q] & ((1 << ax) - 1));
        }
    }
}

// ---- largest connected cluster ------------------------------------------------------------------------------------------------
struct ClWs {
    int32_t* parent;      // (T) union-find forest over triangles (parents only point to lower ids)
    int32_t* label;       // (T) the cluster's root = its lowest triangle id.  Not flattened into `parent`: a path-halving store of
                          // another thread's find may land after the flattening store and leave a non-root there
    int32_t* count;       // (T) triangles per cluster root
    unsigned char* tflag; // (T) triangle kept
    unsigned char* vflag; // (V) vertex referenced by a kept triangle
    int32_t* vnew;        // (V) new vertex id (-1: dropped)
    int32_t* blk_t;
    int32_t* blk_v;
    int64_t* off_t;
    int64_t* off_v;
    uint64_t* best;       // (count << 32) | (0xffffffff - root) of the winning cluster
    unsigned long long* status;   // nonzero: a union gave up after its retry bound
};

__host__ __device__ inline ClWs cl_ws(void* base, int64_t V, int64_t T, size_t* bytes) {
    const int64_t bt = (T + kBlock - 1) / kBlock, bv = (V + kBlock - 1) / kBlock;
    char* p = (char*)base;
    ClWs w;
    w.parent = carve<int32_t>(p, T);
    w.label = carve<int32_t>(p, T);
    w.count = carve<int32_t>(p, T);
    w.tflag = carve<unsigned char>(p, T);
    w.vflag = carve<unsigned char>(p, V);
    w.vnew = carve<int32_t>(p, V);
    w.blk_t = carve<int32_t>(p, bt);
    w.blk_v = carve<int32_t>(p, bv);
    w.off_t = carve<int64_t>(p, bt);
    w.off_v = carve<int64_t>(p, bv);
    w.best = carve<uint64_t>(p, 1);
    w.status = carve<unsigned long long>(p, 1);
    if (bytes) *bytes = (size_t)(p - (char*)base);
    return w;
}

__device__ __forceinline__ int ld_relaxed(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(int32_t* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x with path halving.  Parents only ever point to lower ids (hooking puts the larger root under the smaller one),
// so the walk ends after at most x steps, and a halving store never touches a root.
__device__ int uf_find(int32_t* parent, int x) {
    int p = ld_relaxed(parent + x);
    while (p != x) {
        const int gp = ld_relaxed(parent + p);
        if (gp != p) st_relaxed(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

__global__ void __launch_bounds__(kBlock) mesh_edge_keys(const int32_t* __restrict__ tris, int64_t T, int64_t* __restrict__ keys) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int64_t v[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
    for (int j = 0; j < 3; ++j) {
        const int64_t a = v[j], b = v[(j + 1) % 3];
        keys[3 * t + j] = (a < b ? a : b) << 32 | (a < b ? b : a);
    }
}

__global__ void __launch_bounds__(kBlock) cl_init(int64_t V, int64_t T, ClWs w) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < T) {
        w.parent[i] = (int32_t)i;
        w.count[i] = 0;
        w.tflag[i] = 0;
    }
    if (i < V) w.vflag[i] = 0;
    if (i == 0) {
        *w.best = 0;
        *w.status = 0;
    }
}

// Union of the two triangles of every pair of equal consecutive sorted edge keys (an edge shared by k triangles chains k-1 unions).
__global__ void __launch_bounds__(kBlock) cl_union(const int64_t* __restrict__ keys, const int64_t* __restrict__ order, int64_t nE,
                                                   ClWs w) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x + 1;
    if (i >= nE || keys[i] != keys[i - 1]) return;
    int a = uf_find(w.parent, (int)(order[i] / 3)), b = uf_find(w.parent, (int)(order[i - 1] / 3));
    // Every failed hook means another thread hooked a root in between (the forest lost a root), so the retries are bounded by
    // the number of triangles; the explicit bound only turns a broken invariant into an error instead of a hang.
    for (int it = 0; a != b; ++it) {
        if (it >= (1 << 24)) {
            atomicOr(w.status, 1ull);
            return;
        }
        if (a > b) { const int t = a; a = b; b = t; }
        if (atomicCAS(w.parent + b, b, a) == b) return;
        a = uf_find(w.parent, a);
        b = uf_find(w.parent, b);
    }
}

__global__ void __launch_bounds__(kBlock) cl_flatten(int64_t T, ClWs w) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int r = uf_find(w.parent, (int)t);
    w.label[t] = r;
    atomicAdd(w.count + r, 1);
}

__global__ void __launch_bounds__(kBlock) cl_argmax(int64_t T, ClWs w) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T || w.label[t] != (int32_t)t) return;
    const unsigned long long key = ((unsigned long long)(uint32_t)w.count[t] << 32) | (0xffffffffull - (uint64_t)t);
    atomicMax((unsigned long long*)w.best, key);
}

// Mark kept triangles and the vertices they reference; per-block totals of both flag arrays.
__global__ void __launch_bounds__(kBlock) cl_mark(const int32_t* __restrict__ tris, int64_t T, ClWs w) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int32_t root = (int32_t)(0xffffffffull - (*w.best & 0xffffffffull));
    if (w.label[t] != root) return;
    w.tflag[t] = 1;
    w.vflag[tris[3 * t]] = 1;         // the same value from every writer
    w.vflag[tris[3 * t + 1]] = 1;
    w.vflag[tris[3 * t + 2]] = 1;
}

__global__ void __launch_bounds__(kBlock) flag_block_totals(const unsigned char* __restrict__ flag, int64_t n, int32_t* __restrict__ blk) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int tot;
    block_excl_scan<kBlock>(i < n ? (int)flag[i] : 0, tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kBlock) cl_compact_vertices(int64_t V, ClWs w, int64_t* __restrict__ kept_ids) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int f = v < V ? w.vflag[v] : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(f, tot);
    if (v >= V) return;
    const int64_t id = w.off_v[blockIdx.x] + ex;
    w.vnew[v] = f ? (int32_t)id : -1;
    if (f) kept_ids[id] = v;
}

__global__ void __launch_bounds__(kBlock) cl_compact_triangles(const int32_t* __restrict__ tris, int64_t T, ClWs w,
                                                               int32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int f = t < T ? w.tflag[t] : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(f, tot);
    if (!f) return;
    const int64_t id = w.off_t[blockIdx.x] + ex;
    for (int k = 0; k < 3; ++k) out[3 * id + k] = w.vnew[tris[3 * t + k]];
}

// ---- vertex normals and colour fusion -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) nrm_zero(double* __restrict__ n, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < count) n[i] = 0.0;
}

// open3d's ComputeTriangleNormals(false) + the scatter of ComputeVertexNormals, in fp64 on the float32 positions.
__global__ void __launch_bounds__(kBlock) nrm_scatter(const float* __restrict__ v, const int32_t* __restrict__ tris, int64_t T,
                                                      double* __restrict__ n) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int64_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    double p0[3], e1[3], e2[3];
    for (int k = 0; k < 3; ++k) p0[k] = (double)v[3 * i0 + k];
    for (int k = 0; k < 3; ++k) {
        e1[k] = (double)v[3 * i1 + k] - p0[k];
        e2[k] = (double)v[3 * i2 + k] - p0[k];
    }
    const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const int64_t ids[3] = {i0, i1, i2};
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) unsafeAtomicAdd(n + 3 * ids[j] + k, c[k]);
}

__global__ void __launch_bounds__(kBlock) nrm_normalize(int64_t V, double* __restrict__ n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    const double x = n[3 * i], y = n[3 * i + 1], z = n[3 * i + 2];
    const double s = x * x + y * y + z * z;
    if (s > 0.0) {
        const double r = sqrt(s);
        n[3 * i] = x / r;
        n[3 * i + 1] = y / r;
        n[3 * i + 2] = z / r;
    } else {
        n[3 * i] = 0.0;
        n[3 * i + 1] = 0.0;
        n[3 * i + 2] = 1.0;
    }
}

// extract_color_mesh.py:190-195: d = float32(normal), o = v - d * near * near_t, [o d near far].
__global__ void __launch_bounds__(kBlock) nrm_rays(const float* __restrict__ v, const double* __restrict__ n, int64_t V, float near,
                                                   float far, float near_t, float* __restrict__ rays) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    for (int k = 0; k < 3; ++k) {
        const float d = (float)n[3 * i + k];
        rays[8 * i + k] = nh_sub(v[3 * i + k], nh_mul(nh_mul(d, near), near_t));
        rays[8 * i + 3 + k] = d;
    }
    rays[8 * i + 6] = near;
    rays[8 * i + 7] = far;
}

struct ViewArgs {
    float w2c[12];      // float32 inverse of the 4x4 camera-to-world, top three rows
    float origin[3];    // camera centre (pose[:, 3])
    float focal, cx, cy, near;
    int W, H;
};

// One view of extract_color_mesh.py:223-264: fp64 projection, cv2.remap-exact bilinear colour, the camera->vertex occlusion ray.
__global__ void __launch_bounds__(kBlock) view_rays(const float* __restrict__ v, int64_t V, ViewArgs a, const unsigned char* __restrict__ img,
                                                    unsigned char* __restrict__ col, double* __restrict__ depth, float* __restrict__ rays) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    const float x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
    double cam[3];
    for (int r = 0; r < 3; ++r)
        cam[r] = (double)a.w2c[4 * r] * x + (double)a.w2c[4 * r + 1] * y + (double)a.w2c[4 * r + 2] * z + (double)a.w2c[4 * r + 3];
    cam[1] = -cam[1];
    cam[2] = -cam[2];
    const double px = (double)a.focal * cam[0] + (double)a.cx * cam[2];
    const double py = (double)a.focal * cam[1] + (double)a.cy * cam[2];
    const double d = cam[2] + 1e-5;
    float u = (float)(px / d), w = (float)(py / d);
    u = fminf(fmaxf(u, 0.0f), (float)(a.W - 1));        // np.clip keeps NaN; fmin/fmax would not, so test it below
    w = fminf(fmaxf(w, 0.0f), (float)(a.H - 1));
    const bool nan = !(px / d == px / d) || !(py / d == py / d);
    // cv2.remap(INTER_LINEAR) on float maps: positions rounded to 1/32 px, weights (32 - f) * f' * 32 of 2^15, rounded shift.
    int c0 = 0, c1 = 0, c2 = 0;
    if (!nan) {
        const int ix = (int)rintf(u * 32.0f), iy = (int)rintf(w * 32.0f);
        const int x0 = ix >> 5, fx = ix & 31, y0 = iy >> 5, fy = iy & 31;
        const int x1 = x0 + 1 < a.W ? x0 + 1 : x0, y1 = y0 + 1 < a.H ? y0 + 1 : y0;   // the clamped tap has weight 0
        const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
        const unsigned char* r0 = img + ((int64_t)y0 * a.W) * 3;
        const unsigned char* r1 = img + ((int64_t)y1 * a.W) * 3;
        int acc[3];
        for (int k = 0; k < 3; ++k)
            acc[k] = (r0[3 * x0 + k] * w00 + r0[3 * x1 + k] * w01 + r1[3 * x0 + k] * w10 + r1[3 * x1 + k] * w11 + (1 << 14)) >> 15;
        c0 = acc[0]; c1 = acc[1]; c2 = acc[2];
    }
    col[4 * i] = (unsigned char)c0;
    col[4 * i + 1] = (unsigned char)c1;
    col[4 * i + 2] = (unsigned char)c2;
    col[4 * i + 3] = 0;
    depth[i] = d;
    const float dx = nh_sub(x, a.origin[0]), dy = nh_sub(y, a.origin[1]), dz = nh_sub(z, a.origin[2]);
    const float nrm = sqrtf(nh_add(nh_add(nh_mul(dx, dx), nh_mul(dy, dy)), nh_mul(dz, dz)));
    float* r = rays + 8 * i;
    r[0] = a.origin[0]; r[1] = a.origin[1]; r[2] = a.origin[2];
    r[3] = nh_div(dx, nrm); r[4] = nh_div(dy, nrm); r[5] = nh_div(dz, nrm);
    r[6] = a.near;
    r[7] = (float)d;
}

// extract_color_mesh.py:266-272: w = 0.1 / depth + (opacity < occ); sum colour * w and w in fp64 (view after view: deterministic).
__global__ void __launch_bounds__(kBlock) color_accumulate(const unsigned char* __restrict__ col, const double* __restrict__ depth,
                                                           const float* __restrict__ opacity, int64_t V, float occ,
                                                           double* __restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    float op = opacity[i];
    if (op != op) op = 0.0f;                          // np.nan_to_num(opacity, 1): NaN -> 0 (the 1 is `copy`)
    const double w = 0.1 / depth[i] + (op < occ ? 1.0 : 0.0);
    for (int k = 0; k < 3; ++k) acc[4 * i + k] += (double)col[4 * i + k] * w;
    acc[4 * i + 3] += w;
}

__device__ __forceinline__ unsigned char to_u8(double x) {   // numpy's astype(uint8) on x86 for the values that occur (trunc)
    if (!(x == x)) return 0;
    return (unsigned char)(long long)x;
}

__global__ void __launch_bounds__(kBlock) color_finish(const double* __restrict__ acc, int64_t V, unsigned char* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    for (int k = 0; k < 3; ++k) out[3 * i + k] = to_u8(acc[4 * i + k] / acc[4 * i + 3]);
}

__global__ void __launch_bounds__(kBlock) rgb_to_u8(const float* __restrict__ rgb, int64_t n, unsigned char* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = to_u8((double)nh_mul(rgb[i], 255.0f));
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

inline bool mc_dims_ok(int64_t n0, int64_t n1, int64_t n2) {
    return n0 >= 2 && n1 >= 2 && n2 >= 2 && n0 <= INT32_MAX && n1 <= INT32_MAX && n2 <= INT32_MAX &&
           n0 * n1 <= INT32_MAX && n0 * n1 * n2 <= INT32_MAX;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" size_t nerfhip_marching_cubes_workspace_bytes(int64_t n0, int64_t n1, int64_t n2) {
    if (!mc_dims_ok(n0, n1, n2)) return 0;
    size_t bytes = 0;
    mc_ws(nullptr, n0 * n1 * n2, &bytes);
    return bytes;
}

extern "C" int nerfhip_marching_cubes_count(const float* volume, int64_t n0, int64_t n1, int64_t n2, double iso, void* workspace,
                                            int64_t* totals, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(volume && workspace && totals && mc_dims_ok(n0, n1, n2));
    const int64_t npts = n0 * n1 * n2;
    const McWs w = mc_ws(workspace, npts, nullptr);
    const unsigned nb = blocks(npts);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_count, dim3(nb), dim3(kBlock), 0, s, volume, (int)n0, (int)n1, (int)n2, iso, w);
    hipLaunchKernelGGL(scan_totals, dim3(1), dim3(kScanBlock), 0, s, w.blk_v, (int64_t)nb, w.off_v, w.blk_t, (int64_t)nb, w.off_t, totals);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_marching_cubes_emit(const float* volume, int64_t n0, int64_t n1, int64_t n2, double iso, void* workspace,
                                           const int64_t* totals, double* vertices, int32_t* triangles, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(volume && workspace && totals && vertices && triangles && mc_dims_ok(n0, n1, n2));
    const int64_t npts = n0 * n1 * n2;
    const McWs w = mc_ws(workspace, npts, nullptr);
    const unsigned nb = blocks(npts);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_emit_vertices, dim3(nb), dim3(kBlock), 0, s, volume, (int)n0, (int)n1, (int)n2, iso, w, totals, vertices);
    hipLaunchKernelGGL(mc_emit_triangles, dim3(nb), dim3(kBlock), 0, s, (int)n0, (int)n1, (int)n2, w, totals, triangles);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_edge_keys(const int32_t* triangles, int64_t T, int64_t* keys, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(triangles && keys && T > 0 && T <= INT32_MAX / 3);
    hipLaunchKernelGGL(mesh_edge_keys, dim3(blocks(T)), dim3(kBlock), 0, (hipStream_t)stream, triangles, T, keys);
    return nerfhip_launch_status();
}

extern "C" size_t nerfhip_mesh_cluster_workspace_bytes(int64_t V, int64_t T) {
    if (V <= 0 || T <= 0 || V > INT32_MAX || T > INT32_MAX / 3) return 0;
    size_t bytes = 0;
    cl_ws(nullptr, V, T, &bytes);
    return bytes;
}

extern "C" int nerfhip_mesh_largest_cluster(const int32_t* triangles, int64_t V, int64_t T, const int64_t* sorted_keys,
                                            const int64_t* order, void* workspace, int64_t* totals, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(triangles && sorted_keys && order && workspace && totals && V > 0 && T > 0 && V <= INT32_MAX &&
                      T <= INT32_MAX / 3);
    const ClWs w = cl_ws(workspace, V, T, nullptr);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cl_init, dim3(blocks(V > T ? V : T)), dim3(kBlock), 0, s, V, T, w);
    if (T > 1) hipLaunchKernelGGL(cl_union, dim3(blocks(3 * T - 1)), dim3(kBlock), 0, s, sorted_keys, order, 3 * T, w);
    hipLaunchKernelGGL(cl_flatten, dim3(blocks(T)), dim3(kBlock), 0, s, T, w);
    hipLaunchKernelGGL(cl_argmax, dim3(blocks(T)), dim3(kBlock), 0, s, T, w);
    hipLaunchKernelGGL(cl_mark, dim3(blocks(T)), dim3(kBlock), 0, s, triangles, T, w);
    hipLaunchKernelGGL(flag_block_totals, dim3(blocks(T)), dim3(kBlock), 0, s, w.tflag, T, w.blk_t);
    hipLaunchKernelGGL(flag_block_totals, dim3(blocks(V)), dim3(kBlock), 0, s, w.vflag, V, w.blk_v);
    hipLaunchKernelGGL(scan_totals, dim3(1), dim3(kScanBlock), 0, s, w.blk_t, (int64_t)blocks(T), w.off_t, w.blk_v, (int64_t)blocks(V),
                       w.off_v, totals);
    const hipError_t e = hipMemcpyAsync(totals + 2, w.status, sizeof(int64_t), hipMemcpyDeviceToDevice, s);
    return e != hipSuccess ? (int)e : nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_cluster_compact(const int32_t* triangles, int64_t V, int64_t T, void* workspace, int64_t* kept_vertex_ids,
                                            int32_t* kept_triangles, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(triangles && workspace && kept_vertex_ids && kept_triangles && V > 0 && T > 0 && V <= INT32_MAX &&
                      T <= INT32_MAX / 3);
    const ClWs w = cl_ws(workspace, V, T, nullptr);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cl_compact_vertices, dim3(blocks(V)), dim3(kBlock), 0, s, V, w, kept_vertex_ids);
    hipLaunchKernelGGL(cl_compact_triangles, dim3(blocks(T)), dim3(kBlock), 0, s, triangles, T, w, kept_triangles);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_vertex_normals(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, double* normals,
                                           nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(vertices && normals && V > 0 && T >= 0 && (T == 0 || triangles));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nrm_zero, dim3(blocks(3 * V)), dim3(kBlock), 0, s, normals, 3 * V);
    if (T > 0) hipLaunchKernelGGL(nrm_scatter, dim3(blocks(T)), dim3(kBlock), 0, s, vertices, triangles, T, normals);
    hipLaunchKernelGGL(nrm_normalize, dim3(blocks(V)), dim3(kBlock), 0, s, V, normals);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_normal_rays(const float* vertices, const double* normals, int64_t V, float near, float far, float near_t,
                                        float* rays, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(vertices && normals && rays && V > 0);
    hipLaunchKernelGGL(nrm_rays, dim3(blocks(V)), dim3(kBlock), 0, (hipStream_t)stream, vertices, normals, V, near, far, near_t, rays);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_view_rays(const float* vertices, int64_t V, const float* w2c_host, const float* origin_host, float focal,
                                      int W, int H, const uint8_t* image, float near, uint8_t* colors, double* depth, float* rays,
                                      nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(vertices && w2c_host && origin_host && image && colors && depth && rays && V > 0 && W > 0 && H > 0);
    ViewArgs a;
    for (int k = 0; k < 12; ++k) a.w2c[k] = w2c_host[k];
    for (int k = 0; k < 3; ++k) a.origin[k] = origin_host[k];
    a.focal = focal;
    a.cx = (float)W / 2.0f;      // K = [[f, 0, W/2], [0, f, H/2], [0, 0, 1]] as float32
    a.cy = (float)H / 2.0f;
    a.near = near;
    a.W = W;
    a.H = H;
    hipLaunchKernelGGL(view_rays, dim3(blocks(V)), dim3(kBlock), 0, (hipStream_t)stream, vertices, V, a, image, colors, depth, rays);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_color_accumulate(const uint8_t* colors, const double* depth, const float* opacity, int64_t V,
                                             float occ_threshold, double* accum, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(colors && depth && opacity && accum && V > 0);
    hipLaunchKernelGGL(color_accumulate, dim3(blocks(V)), dim3(kBlock), 0, (hipStream_t)stream, colors, depth, opacity, V, occ_threshold,
                       accum);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_color_finish(const double* accum, int64_t V, uint8_t* out, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(accum && out && V > 0);
    hipLaunchKernelGGL(color_finish, dim3(blocks(V)), dim3(kBlock), 0, (hipStream_t)stream, accum, V, out);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_mesh_rgb_to_u8(const float* rgb, int64_t n, uint8_t* out, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(rgb && out && n > 0);
    hipLaunchKernelGGL(rgb_to_u8, dim3(blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, rgb, n, out);
    return nerfhip_launch_status();
}

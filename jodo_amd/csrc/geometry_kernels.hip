// Sub-structure geometry of decoded molecules and the MMD between two sample sets, on the device.
//
//   jodo_geometry_count / jodo_geometry_write   bond lengths, bond angles and dihedral angles per symbol class, enumerated as
//                         evaluation/cal_geometry.py of the reference enumerates them (cal_bond_distance, cal_bond_angle,
//                         cal_dihedral_angle on the molecule check_2D_stability builds), multiplicities included
//   jodo_mmd_batched      evaluation/mmd.py: compute_mmd for a table of (source, target) segments in three launches
//
// Extraction runs one workgroup per molecule (one wave for N <= 64, four above).  The molecule's bonds are per-atom adjacency bit rows
// in LDS, as in eval_kernels.hip; a work unit is a cell (i, j) of the real n x n block, a bond when i < j and bit j of row i is set, and
// every thread owns a CONTIGUOUS run of cells, so thread order is the reference's bond order (row-major).  A pass counts per (thread,
// class), scans over the threads, and (write pass) enumerates again into the slots the scan assigned: the output is compact, its order
// fixed, and nothing depends on which thread ran first.  Plain C++, vector stores, integer atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"

namespace {
constexpr int GEO_MAX_N = 256;                                // atoms per molecule (eval_kernels.hip: EVAL_MAX_N)
constexpr int GEO_MAX_C = JODO_GEOMETRY_MAX_CLASSES;          // classes per group
constexpr float RAD2DEG = 57.29577951308232f;

struct Vec3 { float x, y, z; };
__device__ __forceinline__ Vec3 sub(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

struct GeoLds {
    float* px; float* py; float* pz;                          // [N]
    uint32_t* adj;                                            // [N][W]
    int* tcnt;                                                // [GEO_MAX_C][nt] per (class, thread): count, then running slot
    int* cls;                                                 // [GEO_MAX_C * 9] class tuples of the current group
    int* misc;                                                // [4] dropped values of the current group
    uint8_t* type;                                            // [N]
};

inline size_t geo_lds_bytes(int N, int W, int nt) {
    return (size_t)N * (12 + 4 * W) + (size_t)GEO_MAX_C * nt * 4 + (size_t)GEO_MAX_C * 9 * 4 + 16 + (size_t)((N + 3) & ~3);
}

__device__ __forceinline__ GeoLds geo_carve(unsigned char* base, int N, int W, int nt) {
    GeoLds L;
    float* f = (float*)base;
    L.px = f; L.py = f + N; L.pz = f + 2 * N;
    L.adj = (uint32_t*)(f + 3 * N);
    L.tcnt = (int*)(L.adj + (size_t)N * W);
    L.cls = L.tcnt + GEO_MAX_C * nt;
    L.misc = L.cls + GEO_MAX_C * 9;
    L.type = (uint8_t*)(L.misc + 4);
    return L;
}

// the reference's str(int(GetBondType())): 1, 2, 3, aromatic 12; an entry the decode cannot produce is a bond that matches no class
__device__ __forceinline__ int bond_code(int e) { return e <= 3 ? e : (e == 4 ? 12 : -1); }

__device__ __forceinline__ Vec3 at(const GeoLds& L, int i) { return {L.px[i], L.py[i], L.pz[i]}; }

// The three value formulas are NOT inlined: the count pass and the write pass must take the same finite / non-finite decision for the
// same atoms, so both call the one compiled body.
__device__ __noinline__ float length_of(Vec3 pi, Vec3 pj) {
    const Vec3 d = sub(pi, pj);
    return sqrtf(dot(d, d));
}

// degrees in [0, 180]; an arm of zero length has no direction: NaN (dropped by the caller)
__device__ __noinline__ float angle_of(Vec3 pi, Vec3 pj, Vec3 pk) {
    const Vec3 a = sub(pi, pj), b = sub(pk, pj);
    if (dot(a, a) == 0.f || dot(b, b) == 0.f) return NAN;
    const Vec3 c = cross(a, b);
    return atan2f(sqrtf(dot(c, c)), dot(a, b)) * RAD2DEG;
}

// degrees, signed; collinear or coincident atoms give 0 / 0 = NaN (dropped by the caller)
__device__ __noinline__ float dihedral_of(Vec3 pi, Vec3 pj, Vec3 pk, Vec3 pl) {
    const Vec3 rIJ = sub(pj, pi), rJK = sub(pk, pj), rKL = sub(pl, pk);
    const Vec3 nIJK = cross(rIJ, rJK), nJKL = cross(rJK, rKL), m = cross(nIJK, rJK);
    const float nn = dot(nJKL, nJKL);
    return -atan2f(dot(m, nJKL) / sqrtf(dot(m, m) * nn), dot(nIJK, nJKL) / sqrtf(dot(nIJK, nIJK) * nn)) * RAD2DEG;
}
__device__ __forceinline__ float bond_length(const GeoLds& L, int i, int j) { return length_of(at(L, i), at(L, j)); }
__device__ __forceinline__ float bond_angle(const GeoLds& L, int i, int j, int k) { return angle_of(at(L, i), at(L, j), at(L, k)); }
__device__ __forceinline__ float dihedral(const GeoLds& L, int i, int j, int k, int l) {
    return dihedral_of(at(L, i), at(L, j), at(L, k), at(L, l));
}

template <int LEN>
__device__ __forceinline__ int find_class(const int* __restrict__ cls, int C, const int (&t)[LEN]) {
    for (int c = 0; c < C; ++c) {
        bool same = true;
#pragma unroll
        for (int q = 0; q < LEN; ++q) same = same && cls[c * LEN + q] == t[q];
        if (same) return c;
    }
    return -1;
}

// bit c set = the three integers of class c at `at` (stride LEN) are (x, y, z): which classes one bond of a tuple leaves possible.  Only
// ever used to skip work that cannot match; the decision itself is find_class on the whole tuple.
template <int LEN>
__device__ __forceinline__ uint32_t bond_mask(const int* __restrict__ cls, int C, int at, int x, int y, int z) {
    uint32_t m = 0;
    for (int c = 0; c < C; ++c)
        if (cls[c * LEN + at] == x && cls[c * LEN + at + 1] == y && cls[c * LEN + at + 2] == z) m |= 1u << c;
    return m;
}

// One enumeration of group G over the calling thread's cells [u0, u1) of the molecule's n x n block.  emit(class, value) is called
// once per recorded value, in the reference's order.
template <int G, class Emit>
__device__ __forceinline__ void geo_enumerate(const GeoLds& L, const uint8_t* __restrict__ e, int N, int W, int n, int C, int u0, int u1,
                                              Emit&& emit) {
    for (int u = u0; u < u1; ++u) {
        const int i = u / n, j = u - i * n;
        if (j <= i || !((L.adj[(size_t)i * W + (j >> 5)] >> (j & 31)) & 1u)) continue;
        const int ti = L.type[i], tj = L.type[j], cm = bond_code(e[(size_t)i * N + j]);
        if (G == 0) {
            const int fwd[3] = {ti, cm, tj}, rev[3] = {tj, cm, ti};
            int c = find_class<3>(L.cls, C, fwd);
            if (c >= 0) { emit(c, bond_length(L, i, j)); continue; }
            c = find_class<3>(L.cls, C, rev);
            if (c >= 0) emit(c, bond_length(L, j, i));
        } else if (G == 1) {
            // no class has this bond as its first (forward) or its second, reversed (reverse): no partner can make a match
            if (!(bond_mask<6>(L.cls, C, 0, ti, cm, tj) | bond_mask<6>(L.cls, C, 3, tj, cm, ti))) continue;
            for (int w = 0; w < W; ++w) {                     // the other bonds at the end atom j, ascending
                uint32_t bits = L.adj[(size_t)j * W + w];
                while (bits) {
                    const int k = 32 * w + __ffs((int)bits) - 1;
                    bits &= bits - 1;
                    if (k == i) continue;
                    const int tk = L.type[k], c1 = bond_code(e[(size_t)min(j, k) * N + max(j, k)]);
                    const int fwd[6] = {ti, cm, tj, tj, c1, tk}, rev[6] = {tk, c1, tj, tj, cm, ti};
                    int c = find_class<6>(L.cls, C, fwd);
                    if (c >= 0) { emit(c, bond_angle(L, i, j, k)); continue; }
                    c = find_class<6>(L.cls, C, rev);
                    if (c >= 0) emit(c, bond_angle(L, k, j, i));
                }
            }
        } else {
            const uint32_t mid_f = bond_mask<9>(L.cls, C, 3, ti, cm, tj), mid_r = bond_mask<9>(L.cls, C, 3, tj, cm, ti);
            if (!(mid_f | mid_r)) continue;                   // no class has this central bond, in either direction
            for (int w = 0; w < W; ++w) {                     // right bonds at j (outer), left bonds at i (inner), both ascending
                uint32_t rbits = L.adj[(size_t)j * W + w];
                while (rbits) {
                    const int d = 32 * w + __ffs((int)rbits) - 1;
                    rbits &= rbits - 1;
                    if (d == i) continue;
                    const int td = L.type[d], cr = bond_code(e[(size_t)min(j, d) * N + max(j, d)]);
                    if (!((mid_f & bond_mask<9>(L.cls, C, 6, tj, cr, td)) | (mid_r & bond_mask<9>(L.cls, C, 0, td, cr, tj)))) continue;
                    for (int v = 0; v < W; ++v) {
                        uint32_t lbits = L.adj[(size_t)i * W + v];
                        while (lbits) {
                            const int a = 32 * v + __ffs((int)lbits) - 1;
                            lbits &= lbits - 1;
                            if (a == j) continue;
                            const int ta = L.type[a], cl = bond_code(e[(size_t)min(i, a) * N + max(i, a)]);
                            const int fwd[9] = {ta, cl, ti, ti, cm, tj, tj, cr, td}, rev[9] = {td, cr, tj, tj, cm, ti, ti, cl, ta};
                            int c = find_class<9>(L.cls, C, fwd);
                            if (c >= 0) { emit(c, dihedral(L, a, i, j, d)); continue; }
                            c = find_class<9>(L.cls, C, rev);
                            if (c >= 0) emit(c, dihedral(L, d, j, i, a));
                        }
                    }
                }
            }
        }
    }
}

// One group of one molecule: count per (class, thread), scan over the threads, then either the class totals (count pass) or the write.
template <int G, bool WRITE>
__device__ void geo_group(const GeoLds& L, const uint8_t* __restrict__ e, int B, int N, int W, int n, int b, int C, int cbase,
                          const int32_t* __restrict__ classes, int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                          float* __restrict__ out, long long total, unsigned long long* __restrict__ dropped) {
    constexpr int LEN = G == 0 ? 3 : (G == 1 ? 6 : 9);
    const int tid = threadIdx.x, nt = blockDim.x;
    __syncthreads();                                          // the previous group is done with tcnt / cls
    for (int q = tid; q < C * LEN; q += nt) L.cls[q] = classes[q];
    for (int q = tid; q < GEO_MAX_C * nt; q += nt) L.tcnt[q] = 0;
    if (tid == 0) L.misc[0] = 0;
    __syncthreads();
    const int cells = n * n, chunk = (cells + nt - 1) / nt;
    const int u0 = min(tid * chunk, cells), u1 = min(u0 + chunk, cells);
    int bad = 0;
    geo_enumerate<G>(L, e, N, W, n, C, u0, u1, [&](int c, float v) {
        if (isfinite(v)) L.tcnt[c * nt + tid] += 1; else ++bad;
    });
    if (!WRITE && bad) atomicAdd(&L.misc[0], bad);
    __syncthreads();
    if (tid < C) {                                            // exclusive scan of class `tid` over the threads
        int run = 0;
        for (int t = 0; t < nt; ++t) { const int v = L.tcnt[tid * nt + t]; L.tcnt[tid * nt + t] = run; run += v; }
        if (!WRITE) counts[(size_t)(cbase + tid) * B + b] = run;
    }
    if (!WRITE) {
        if (tid == 0 && L.misc[0]) atomicAdd(&dropped[G], (unsigned long long)L.misc[0]);
        return;
    }
    __syncthreads();
    geo_enumerate<G>(L, e, N, W, n, C, u0, u1, [&](int c, float v) {
        if (!isfinite(v)) return;
        const long long slot = offsets[(size_t)(cbase + c) * B + b] + (L.tcnt[c * nt + tid]++);
        if (slot >= 0 && slot < total) out[slot] = v;         // the count pass sized the array; never write past what it allocated
    });
}

template <bool WRITE>
__global__ void k_geometry(int B, int N, int W, int Cb, int Ca, int Cd, const int32_t* __restrict__ cls_b, const int32_t* __restrict__ cls_a,
                           const int32_t* __restrict__ cls_d, const int32_t* __restrict__ n_nodes, const uint8_t* __restrict__ keep,
                           const float* __restrict__ pos, const uint8_t* __restrict__ atom_type, const uint8_t* __restrict__ edge_type,
                           int32_t* __restrict__ counts, const int64_t* __restrict__ offsets, float* __restrict__ out_b,
                           float* __restrict__ out_a, float* __restrict__ out_d, long long tot_b, long long tot_a, long long tot_d,
                           unsigned long long* __restrict__ dropped) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const GeoLds L = geo_carve(lds_raw, N, W, nt);
    const int n = (keep && !keep[b]) ? 0 : min(max(n_nodes[b], 0), N);
    for (int i = tid; i < n; i += nt) {
        const float* p = pos + ((size_t)b * N + i) * 3;
        L.px[i] = p[0]; L.py[i] = p[1]; L.pz[i] = p[2];
        L.type[i] = atom_type[(size_t)b * N + i];
        for (int w = 0; w < W; ++w) L.adj[(size_t)i * W + w] = 0;
    }
    __syncthreads();
    const uint8_t* e = edge_type + (size_t)b * N * N;
    for (int c = tid; c < n * n; c += nt) {                   // AddBond(src, dst) for every nonzero edge_type[src, dst] with src < dst
        const int r = c / n, q = c - r * n;
        if (q <= r || !e[(size_t)r * N + q]) continue;
        atomicOr(&L.adj[(size_t)r * W + (q >> 5)], 1u << (q & 31));
        atomicOr(&L.adj[(size_t)q * W + (r >> 5)], 1u << (r & 31));
    }
    geo_group<0, WRITE>(L, e, B, N, W, n, b, Cb, 0, cls_b, counts, offsets, out_b, tot_b, dropped);
    geo_group<1, WRITE>(L, e, B, N, W, n, b, Ca, Cb, cls_a, counts, offsets, out_a, tot_a, dropped);
    geo_group<2, WRITE>(L, e, B, N, W, n, b, Cd, Cb + Ca, cls_d, counts, offsets, out_d, tot_d, dropped);
}

// counts i32 [Ctot][B] -> offsets i64 [Ctot][B]: the exclusive scan of each GROUP's rows (class-major, molecule-minor), relative to the
// group's own output array; sizes i64 [Ctot]: values per class.  One block per group.
__global__ void k_geometry_scan(int B, int Cb, int Ca, int Cd, const int32_t* __restrict__ counts, int64_t* __restrict__ offsets,
                                int64_t* __restrict__ sizes) {
    __shared__ long long part[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int C = g == 0 ? Cb : (g == 1 ? Ca : Cd), cbase = g == 0 ? 0 : (g == 1 ? Cb : Cb + Ca);
    const long long len = (long long)C * B, chunk = (len + 255) / 256;
    const int32_t* in = counts + (size_t)cbase * B;
    int64_t* o = offsets + (size_t)cbase * B;
    const long long q0 = min((long long)tid * chunk, len), q1 = min(q0 + chunk, len);
    long long sum = 0;
    for (long long q = q0; q < q1; ++q) sum += in[q];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 256; ++t) { const long long v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    long long run = part[tid];
    for (long long q = q0; q < q1; ++q) { o[q] = run; run += in[q]; }
    if (tid < C) {
        long long s = 0;
        for (int b = 0; b < B; ++b) s += in[(size_t)tid * B + b];
        sizes[cbase + tid] = s;
    }
}

int geo_check(const char* what, int B, int N, int Cb, int Ca, int Cd) {
    if (B <= 0 || N <= 0 || Cb < 0 || Ca < 0 || Cd < 0) return jodo_set_error(JODO_ERR_ARG, "%s: bad shape", what);
    if (N > GEO_MAX_N || Cb > GEO_MAX_C || Ca > GEO_MAX_C || Cd > GEO_MAX_C)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "%s: at most %d atoms per molecule and %d classes per group", what, GEO_MAX_N, GEO_MAX_C);
    return JODO_OK;
}

// ---- MMD ------------------------------------------------------------------------------------------------------------------------------
constexpr int MMD_TILE = JODO_MMD_TILE;                       // x values of a block (4 per thread) and y values of its LDS chunk
constexpr int MMD_NT = 256;
constexpr int MMD_RX = MMD_TILE / MMD_NT;
constexpr int MMD_SUB = 64;                                   // y values per float32 partial sum (64 terms of at most K each)
constexpr int MMD_PARAMS = 12;                                // per segment: mean, scale, c[8], 2 spare
constexpr int MMD_MAX_K = 8;
constexpr float MMD_PAD = 1e18f;                              // x pads +PAD, y pads -PAD: d^2 = 4e36 is finite and its kernel value is 0
constexpr double LOG2E = 1.4426950408889634;

struct Seg { long long so, ns, to, nt; };
__device__ __forceinline__ Seg load_seg(const int64_t* __restrict__ seg, int s) {
    return {seg[4 * s], seg[4 * s + 1], seg[4 * s + 2], seg[4 * s + 3]};
}

__device__ __forceinline__ double block_sum(double v, double* red) {      // fixed tree over the 256 threads; every thread gets the sum
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = MMD_NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// Per segment: the mean of the concatenation and the bandwidths.  The reference's sum over all ordered pairs of (t_a - t_b)^2 is
// 2 n sum (t - mean)^2, reduced here in float64.  params: [0] mean, [1] sqrt(log2 e / widest bandwidth) (the fast path's pre-scale),
// [2 + i] log2 e / bandwidth_i.
__global__ __launch_bounds__(MMD_NT) void k_mmd_params(int S, const int64_t* __restrict__ seg, const float* __restrict__ src,
                                                       const float* __restrict__ tgt, double kernel_mul, int K, double fix_sigma,
                                                       float* __restrict__ params) {
    __shared__ double red[MMD_NT];
    const int s = blockIdx.x, tid = threadIdx.x;
    const Seg g = load_seg(seg, s);
    const long long n = g.ns + g.nt;
    const float* a = src + g.so;
    const float* t = tgt + g.to;
    double sum = 0.;
    for (long long q = tid; q < n; q += MMD_NT) sum += (double)(q < g.ns ? a[q] : t[q - g.ns]);
    const double mean = block_sum(sum, red) / (double)n;
    double ss = 0.;
    for (long long q = tid; q < n; q += MMD_NT) { const double d = (double)(q < g.ns ? a[q] : t[q - g.ns]) - mean; ss += d * d; }
    ss = block_sum(ss, red);
    if (tid == 0) {
        const double nn = (double)n;
        double bw = fix_sigma != 0. ? fix_sigma : (2. * nn * ss) / (nn * nn - nn);
        for (int q = 0; q < K / 2; ++q) bw /= kernel_mul;
        float* p = params + (size_t)s * MMD_PARAMS;
        p[0] = (float)mean;
        double w = bw;
        for (int q = 0; q < MMD_MAX_K; ++q) {
            p[2 + q] = q < K ? (float)(LOG2E / w) : 0.f;
            if (q == K - 1) p[1] = (float)sqrt(LOG2E / w);
            w *= kernel_mul;
        }
    }
}

// One tile: 1024 x values in registers (4 per thread) against a chunk of up to 1024 y values in LDS, read as broadcast float4.
// FAST (kernel_mul 2, K = 5): values pre-scaled so that u = exp2(-(x - y)^2) is the widest kernel and the others are u^2 .. u^16.
// Otherwise one exp2 per kernel with c_i = log2 e / bandwidth_i.  Per-thread float32 sums run over 64 y values, then float64.
template <bool FAST>
__global__ __launch_bounds__(MMD_NT) void k_mmd_tiles(int S, int T, int K, const int64_t* __restrict__ seg, const int32_t* __restrict__ tiles,
                                                      const float* __restrict__ params, const float* __restrict__ src,
                                                      const float* __restrict__ tgt, double* __restrict__ partials) {
    __shared__ __align__(16) float ys[MMD_TILE];
    __shared__ double red[MMD_NT];
    const int tile = blockIdx.x, tid = threadIdx.x;
    const int s = tiles[4 * tile], kind = tiles[4 * tile + 1];
    const long long x0 = tiles[4 * tile + 2], y0 = tiles[4 * tile + 3];
    if (s < 0 || s >= S || kind < 0 || kind > 2 || x0 < 0 || y0 < 0) { if (tid == 0) partials[tile] = 0.; return; }
    const Seg g = load_seg(seg, s);
    const float* xa = kind == 1 ? tgt + g.to : src + g.so;    // 0: source x source, 1: target x target, 2: source x target
    const float* ya = kind == 0 ? src + g.so : tgt + g.to;
    const long long nx = kind == 1 ? g.nt : g.ns, ny = kind == 0 ? g.ns : g.nt;
    const float* p = params + (size_t)s * MMD_PARAMS;
    const float mean = p[0], scale = FAST ? p[1] : 1.f;
    float c[MMD_MAX_K];
#pragma unroll
    for (int q = 0; q < MMD_MAX_K; ++q) c[q] = p[2 + q];
    float x[MMD_RX];
#pragma unroll
    for (int r = 0; r < MMD_RX; ++r) {
        const long long q = x0 + tid + MMD_NT * r;
        x[r] = q < nx ? (xa[q] - mean) * scale : MMD_PAD;
        const long long y = y0 + tid + MMD_NT * r;
        ys[tid + MMD_NT * r] = y < ny ? (ya[y] - mean) * scale : -MMD_PAD;
    }
    __syncthreads();
    const long long left = ny - y0;
    const int jmax = left >= MMD_TILE ? MMD_TILE : (int)((left + MMD_SUB - 1) / MMD_SUB) * MMD_SUB;
    double acc = 0.;
    for (int j0 = 0; j0 < jmax; j0 += MMD_SUB) {
        float a32[MMD_RX];
#pragma unroll
        for (int r = 0; r < MMD_RX; ++r) a32[r] = 0.f;
#pragma unroll 4
        for (int j = j0; j < j0 + MMD_SUB; j += 4) {
            const float4 y4 = *(const float4*)&ys[j];
            const float yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int r = 0; r < MMD_RX; ++r) {
                    const float d = x[r] - yy[q], a = d * d;
                    if (FAST) {
                        const float u = __builtin_amdgcn_exp2f(-a), u2 = u * u, u4 = u2 * u2, u8 = u4 * u4, u16 = u8 * u8;
                        a32[r] += (u + u2) + (u4 + u8) + u16;
                    } else {
                        float k = 0.f;
#pragma unroll
                        for (int i = 0; i < MMD_MAX_K; ++i) k += i < K ? __builtin_amdgcn_exp2f(-(a * c[i])) : 0.f;
                        a32[r] += k;
                    }
                }
            }
        }
        acc += (double)((a32[0] + a32[1]) + (a32[2] + a32[3]));
    }
    const double sum = block_sum(acc, red);
    if (tid == 0) partials[tile] = (kind != 2 && y0 > x0) ? 2. * sum : sum;      // a tile above the diagonal stands for its mirror too
}

// Per segment: the tile partials of its range in a fixed order, then XX / ns^2 + YY / nt^2 - 2 XY / (ns nt).
__global__ __launch_bounds__(MMD_NT) void k_mmd_final(int S, int T, const int64_t* __restrict__ seg, const int32_t* __restrict__ tiles,
                                                      const int32_t* __restrict__ tile_start, const double* __restrict__ partials,
                                                      double* __restrict__ out) {
    __shared__ double red[MMD_NT];
    const int s = blockIdx.x, tid = threadIdx.x;
    const Seg g = load_seg(seg, s);
    double part[3] = {0., 0., 0.};
    for (int t = max(tile_start[s], 0) + tid; t < min(tile_start[s + 1], T); t += MMD_NT) {
        const int kind = tiles[4 * t + 1];
        if (kind >= 0 && kind <= 2) part[kind] += partials[t];
    }
    const double xx = block_sum(part[0], red), yy = block_sum(part[1], red), xy = block_sum(part[2], red);
    if (tid == 0) {
        const double ns = (double)g.ns, nt = (double)g.nt;
        out[s] = xx / (ns * ns) + yy / (nt * nt) - 2. * (xy / (ns * nt));
    }
}
}  // namespace

extern "C" int jodo_geometry_count(int B, int N, int Cb, int Ca, int Cd, const int32_t* cls_b_dev, const int32_t* cls_a_dev,
                                   const int32_t* cls_d_dev, const int32_t* n_nodes_dev, const uint8_t* keep, const float* pos,
                                   const uint8_t* atom_type, const uint8_t* edge_type, int32_t* counts_out, int64_t* offsets_out,
                                   int64_t* sizes_out, int64_t* dropped_out, void* stream) {
    int rc = geo_check("geometry_count", B, N, Cb, Ca, Cd);
    if (rc != JODO_OK) return rc;
    if ((Cb && !cls_b_dev) || (Ca && !cls_a_dev) || (Cd && !cls_d_dev) || !n_nodes_dev || !pos || !atom_type || !edge_type || !counts_out ||
        !offsets_out || !sizes_out || !dropped_out)
        return jodo_set_error(JODO_ERR_ARG, "geometry_count: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(dropped_out, 0, 3 * sizeof(int64_t), st) != hipSuccess) return jodo_set_error(JODO_ERR_LAUNCH, "geometry_count: memset failed");
    const int W = (N + 31) / 32, nt = N <= 64 ? 64 : 256;
    hipLaunchKernelGGL(k_geometry<false>, dim3(B), dim3(nt), geo_lds_bytes(N, W, nt), st, B, N, W, Cb, Ca, Cd, cls_b_dev, cls_a_dev, cls_d_dev,
                       n_nodes_dev, keep, pos, atom_type, edge_type, counts_out, (const int64_t*)nullptr, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr, 0ll, 0ll, 0ll, (unsigned long long*)dropped_out);
    rc = jodo_check_launch("k_geometry<count>");
    if (rc != JODO_OK) return rc;
    hipLaunchKernelGGL(k_geometry_scan, dim3(3), dim3(256), 0, st, B, Cb, Ca, Cd, counts_out, offsets_out, sizes_out);
    return jodo_check_launch("k_geometry_scan");
}

extern "C" int jodo_geometry_write(int B, int N, int Cb, int Ca, int Cd, const int32_t* cls_b_dev, const int32_t* cls_a_dev,
                                   const int32_t* cls_d_dev, const int32_t* n_nodes_dev, const uint8_t* keep, const float* pos,
                                   const uint8_t* atom_type, const uint8_t* edge_type, const int64_t* offsets, float* out_b, float* out_a,
                                   float* out_d, int64_t n_b, int64_t n_a, int64_t n_d, void* stream) {
    int rc = geo_check("geometry_write", B, N, Cb, Ca, Cd);
    if (rc != JODO_OK) return rc;
    if ((Cb && !cls_b_dev) || (Ca && !cls_a_dev) || (Cd && !cls_d_dev) || !n_nodes_dev || !pos || !atom_type || !edge_type || !offsets ||
        n_b < 0 || n_a < 0 || n_d < 0 || (n_b && !out_b) || (n_a && !out_a) || (n_d && !out_d))
        return jodo_set_error(JODO_ERR_ARG, "geometry_write: null argument");
    const int W = (N + 31) / 32, nt = N <= 64 ? 64 : 256;
    hipLaunchKernelGGL(k_geometry<true>, dim3(B), dim3(nt), geo_lds_bytes(N, W, nt), (hipStream_t)stream, B, N, W, Cb, Ca, Cd, cls_b_dev,
                       cls_a_dev, cls_d_dev, n_nodes_dev, keep, pos, atom_type, edge_type, (int32_t*)nullptr, offsets, out_b, out_a, out_d,
                       (long long)n_b, (long long)n_a, (long long)n_d, (unsigned long long*)nullptr);
    return jodo_check_launch("k_geometry<write>");
}

extern "C" int jodo_mmd_batched(int S, int T, const int64_t* seg_dev, const int32_t* tiles_dev, const int32_t* tile_start_dev,
                                const float* src, const float* tgt, double kernel_mul, int kernel_num, double fix_sigma, float* params_ws,
                                double* partials_ws, double* out_dev, void* stream) {
    if (S <= 0 || T < 0) return jodo_set_error(JODO_ERR_ARG, "mmd_batched: bad shape");
    if (kernel_num < 1 || kernel_num > MMD_MAX_K)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "mmd_batched: kernel_num is 1 .. %d", MMD_MAX_K);
    if (!(kernel_mul > 0.) || !(fix_sigma >= 0.)) return jodo_set_error(JODO_ERR_ARG, "mmd_batched: kernel_mul > 0 and fix_sigma >= 0");
    if (!seg_dev || !tile_start_dev || !src || !tgt || !params_ws || !out_dev || (T && (!tiles_dev || !partials_ws)))
        return jodo_set_error(JODO_ERR_ARG, "mmd_batched: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mmd_params, dim3(S), dim3(MMD_NT), 0, st, S, seg_dev, src, tgt, kernel_mul, kernel_num, fix_sigma, params_ws);
    int rc = jodo_check_launch("k_mmd_params");
    if (rc != JODO_OK) return rc;
    if (T) {
        if (kernel_mul == 2. && kernel_num == 5)
            hipLaunchKernelGGL(k_mmd_tiles<true>, dim3(T), dim3(MMD_NT), 0, st, S, T, kernel_num, seg_dev, tiles_dev, params_ws, src, tgt, partials_ws);
        else
            hipLaunchKernelGGL(k_mmd_tiles<false>, dim3(T), dim3(MMD_NT), 0, st, S, T, kernel_num, seg_dev, tiles_dev, params_ws, src, tgt, partials_ws);
        rc = jodo_check_launch("k_mmd_tiles");
        if (rc != JODO_OK) return rc;
    }
    hipLaunchKernelGGL(k_mmd_final, dim3(S), dim3(MMD_NT), 0, st, S, T, seg_dev, tiles_dev, tile_start_dev, partials_ws, out_dev);
    return jodo_check_launch("k_mmd_final");
}

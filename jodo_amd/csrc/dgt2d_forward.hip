// jodo_dgt2d_forward: one evaluation of the 2-D score network DGT_concat_2D (include/jodo_hip.h), and the 2-D sampler update.
//
// Layout.  Real atoms are compact: node row = noff_b + i.  The edge state lives in memory between blocks as rows of De = 64 floats,
// row(b, r, c) = eoff_b + r n_b + c (n_b^2 rows per molecule).  With symmetric inputs (device flag 0) only the rows r < c are live:
// embedding, pair update, readout and heads run once per unordered pair, and the attention kernel reads row (min, max).  With
// asymmetric inputs every ordered pair is its own row (directed fallback, twice the pair work).
//
// Per block:  k2d_ln_mod (LN1 + modulate) -> k2d_gemm (q | k | v) -> k2d_attn -> k2d_gemm (node2edge) -> k2d_ln_mod (residual, LN2,
// modulate) -> k2d_gemm x 2 (node FFN) -> k2d_gemm (node readout) -> k2d_pair (edge residual, LN, FFN, readout).
// jodo_dgt2d_forward_walk with the pair walk puts k2d_attn_pair in k2d_attn's place when the inputs are symmetric: one evaluation of both
// tanh projections per unordered pair, groups of whole molecules per workgroup, LDS hand-over between the two atoms of a pair.
// Every projection is exact fp32 on v_mfma_f32_32x32x2_f32 in the strip model of dgt_device.h (32 items per wave, weights as A operand,
// packed by csrc/dgt2d_pack.cpp).  The two per-edge kernels are persistent: a workgroup of four waves copies the block's weights
// (128 KiB lin_edge0 | lin_edge1; 72 KiB edge FFN + readout) into LDS once and its waves then walk over the items.
#include "dgt_split.h"
#include <vector>
#include "jodo_hip_internal.h"
#include "../../include/jodo_hip.h"

using namespace jd;

extern "C" int jodo_dgt2d_check_cfg(const jodo_cfg2d* cfg);

namespace {

constexpr int D2 = 256, DE = 64, T2 = 1024, L2 = 8, MODB = 6 * D2 + 6 * DE, MODW = L2 * MODB, EHW = DE + L2 * 16, NHW = D2 + L2 * 64;

#define L2D(kern, grid, block, ...)                                               \
    do {                                                                          \
        auto kf_ = kern;                                                          \
        hipLaunchKernelGGL(kf_, dim3(grid), dim3(block), 0, st, __VA_ARGS__);     \
        int rc_ = jodo_check_launch(#kern);                                       \
        if (rc_ != JODO_OK) return rc_;                                           \
    } while (0)

struct Lay {                     // sizes and workspace offsets (in floats)
    int B, N, Nn, P;
    int64_t R;
    size_t hid1, tembs, mods, h, hm, qkv, hn, u, f1, ahid, nh1, nh2, nh3, e, ehid, total;
    int off_n, off_noff, off_eoff, off_node, off_pair, words;
};

int make_lay(int B, int N, const int32_t* n, Lay* o) {
    if (B <= 0 || N <= 0 || !n) return jodo_set_error(JODO_ERR_ARG, "dgt2d: bad batch");
    if (N > 64) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: padded width %d above 64", N);
    if (B >= (1 << 19)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: batch %d too large", B);
    int64_t Nn = 0, R = 0, P = 0;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 1 || n[b] > N) return jodo_set_error(JODO_ERR_ARG, "dgt2d: n_nodes[%d]=%d outside [1,%d]", b, n[b], N);
        Nn += n[b]; R += (int64_t)n[b] * n[b]; P += (int64_t)n[b] * (n[b] - 1) / 2;
    }
    if (R >= ((int64_t)1 << 30) / 48) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: batch too large (%lld edge rows)", (long long)R);
    o->B = B; o->N = N; o->Nn = (int)Nn; o->P = (int)P; o->R = R;
    const size_t Bp = (size_t)(B + 63) / 64 * 64, Np = (size_t)(Nn + 63) / 64 * 64, Rp = (size_t)(R + 63) / 64 * 64;
    size_t at = 0;
    auto take = [&](size_t cnt) { size_t a = at; at += (cnt + 63) / 64 * 64; return a; };
    o->hid1 = take(Bp * T2); o->tembs = take(Bp * T2); o->mods = take(Bp * MODW);
    o->h = take(Np * D2); o->hm = take(Np * D2); o->qkv = take(Np * 3 * D2); o->hn = take(Np * D2); o->u = take(Np * DE);
    o->f1 = take(Np * 2 * D2); o->ahid = take(Np * NHW); o->nh1 = take(Np * D2); o->nh2 = take(Np * (D2 / 2)); o->nh3 = take(Np * 32);
    o->e = take(Rp * DE); o->ehid = take(Rp * EHW);
    o->total = at;
    o->off_n = 0; o->off_noff = B; o->off_eoff = 2 * B; o->off_node = 3 * B; o->off_pair = 3 * B + (int)Nn;
    o->words = 3 * B + (int)Nn + (int)P + 1;
    return JODO_OK;
}

struct K2 {                      // kernel arguments
    const int *mol_n, *mol_noff, *mol_eoff, *node_b, *pair;
    int B, N, Nn, P, nd, ch, layer;
    float th;
    const float* W;
    const int32_t* flags;        // [0] symmetric inputs, [1] shared noise level, [2] pair walk ran, [3] split-bf16 form ran
    const float *xh, *edge_x, *cond_x, *cond_edge_x, *noise;
    float *out_xh, *out_edge;
    float *hid1, *tembs, *mods, *h, *hm, *qkv, *hn, *u, *f1, *ahid, *nh1, *nh2, *nh3, *e, *ehid;
    int64_t wg[J2_GLOBAL_COUNT], wb[J2B_BLOCK_COUNT];
    const char* T;               // split tape (bf16x3 form) or NULL; tb: byte offsets of this block's ff_linear3 | ff_linear4 | readout in it
    int64_t tb[3];
};

__device__ __forceinline__ float half_max(float v) {          // over the 32 lanes of a half
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// Sum of 16 per-lane values over the 32 lanes of a half, transposed: lane j ends with the total of value j % 16 (31 exchanges
// instead of 80: after the first full exchange every step halves the values a lane still carries).
__device__ __forceinline__ float half_sum16(const float (&v)[16], int j) {
    float a[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) a[s] = v[s] + __shfl_xor(v[s], 16);
    float b8[8], b4[4], b2[2];
    const bool u8 = (j & 8) != 0, u4 = (j & 4) != 0, u2 = (j & 2) != 0, u1 = (j & 1) != 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) b8[s] = (u8 ? a[s + 8] : a[s]) + __shfl_xor(u8 ? a[s] : a[s + 8], 8);
#pragma unroll
    for (int s = 0; s < 4; ++s) b4[s] = (u4 ? b8[s + 4] : b8[s]) + __shfl_xor(u4 ? b8[s] : b8[s + 4], 4);
#pragma unroll
    for (int s = 0; s < 2; ++s) b2[s] = (u2 ? b4[s + 2] : b4[s]) + __shfl_xor(u2 ? b4[s] : b4[s + 2], 2);
    return (u1 ? b2[1] : b2[0]) + __shfl_xor(u1 ? b2[0] : b2[1], 1);
}

// ---- prologue ------------------------------------------------------------------------------------------------------------------
__global__ void k2d_flags_init(int32_t* flags, int force_directed, int split) {
    if (threadIdx.x == 0) { flags[0] = force_directed ? 0 : 1; flags[1] = 1; flags[3] = split; }
}
__global__ void k2d_flags(K2 A, int32_t* flags) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (size_t)A.B && A.noise[idx] != A.noise[0]) flags[1] = 0;
    const size_t tot = (size_t)A.B * A.N * A.N;
    if (idx >= tot) return;
    const int c = (int)(idx % A.N), r = (int)((idx / A.N) % A.N), b = (int)(idx / ((size_t)A.N * A.N));
    const int n = A.mol_n[b];
    if (!(r < c && c < n)) return;
    const size_t t = (((size_t)b * A.N + c) * A.N + r) * A.ch;
    bool same = true;
    for (int k = 0; k < A.ch; ++k) {
        same = same && A.edge_x[idx * A.ch + k] == A.edge_x[t + k];
        if (A.cond_edge_x) same = same && A.cond_edge_x[idx * A.ch + k] == A.cond_edge_x[t + k];
    }
    if (!same) flags[0] = 0;
}

// time_mlp.0 / .1: [x, sin, cos] (17) -> Linear -> GELU(erf)
__global__ __launch_bounds__(256) void k2d_time1(K2 A) {
    const int b = blockIdx.x;
    if (A.flags[1] && b > 0) return;
    __shared__ float ft[17];
    if (threadIdx.x < 8) {
        const float x = A.noise[b];
        const float fr = x * A.W[A.wg[J2_TIME_FREQ] + threadIdx.x] * 2.f * 3.14159265358979323846f;
        ft[1 + threadIdx.x] = sinf(fr);
        ft[9 + threadIdx.x] = cosf(fr);
        if (threadIdx.x == 0) ft[0] = x;
    }
    __syncthreads();
    const float* W1 = A.W + A.wg[J2_TIME_W1];
    const float* b1 = A.W + A.wg[J2_TIME_B1];
    for (int j = threadIdx.x; j < T2; j += 256) {
        float s = b1[j];
#pragma unroll
        for (int k = 0; k < 17; ++k) s = fmaf(W1[j * 17 + k], ft[k], s);
        A.hid1[(size_t)b * T2 + j] = 0.5f * s * (1.f + erff(s * 0.70710678118654752f));
    }
}

// ---- row GEMM: Y[rows, 32 NB] = epi(X[rows, 64 nk] W^T + bias) ----------------------------------------------------------------------
struct Gemm2 {
    const float* X; int ldx; float* Y; int ldy; const float* W; const float* bias; int rows, nk, NB, act;    // act 1: SiLU
    const float* R; int ldr; const float* gate; int gate_ld; const int* node_b; const int32_t* flags; int uni_rows;
};
// bias, SiLU, R + gate y (per-row molecule gate, or the shared row under flags[1]) and the store of a strip's 32 x 32 accumulator images
template <int NOB, int MT>
__device__ __forceinline__ void gemm_epilogue(const Gemm2& G, const f32x16 (&acc)[NOB][MT], const int (&row)[MT], int ob0, int h) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (row[m] >= G.rows) continue;
        int mrow = 0;
        if (G.R && !G.flags[1]) mrow = G.node_b[row[m]] >> 8;
#pragma unroll
        for (int o = 0; o < NOB; ++o) {
            if (ob0 + o >= G.NB) continue;
            const int col0 = (ob0 + o) * 32 + 16 * h;
            float v[16], bb[16];
            if (G.bias) load16(G.bias + col0, bb);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                v[s] = acc[o][m][s] + (G.bias ? bb[s] : 0.f);
                if (G.act == 1) v[s] = silu_f(v[s]);
            }
            if (G.R) {
                float rr[16], gg[16];
                load16(G.R + (size_t)row[m] * G.ldr + col0, rr);
                load16(G.gate + (size_t)mrow * G.gate_ld + col0, gg);
#pragma unroll
                for (int s = 0; s < 16; ++s) v[s] = fmaf(gg[s], v[s], rr[s]);
            }
            store16(G.Y + (size_t)row[m] * G.ldy + col0, v);
        }
    }
}
template <int NOB, int MT>
__global__ __launch_bounds__(64) void k2d_gemm(Gemm2 G) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int strip = blockIdx.x, ob0 = blockIdx.y * NOB;
    if (G.uni_rows && G.flags[1] && strip > 0) return;
    f32x16 acc[NOB][MT];
    int row[MT];
    const float* xr[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        row[m] = (strip * MT + m) * 32 + j;
        xr[m] = G.X + (size_t)min(row[m], G.rows - 1) * G.ldx;
#pragma unroll
        for (int o = 0; o < NOB; ++o) acc[o][m] = zero16();
    }
    for (int kc = 0; kc < G.nk; ++kc) {
        float act[MT][32];
#pragma unroll
        for (int m = 0; m < MT; ++m) load_nat<2>(xr[m] + kc * 64, h, act[m]);
#pragma unroll
        for (int o = 0; o < NOB; ++o) {
            if (ob0 + o >= G.NB) continue;
            const float4* w = reinterpret_cast<const float4*>(G.W) + ((size_t)(ob0 + o) * G.nk + kc) * 512 + lane;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 a = w[q * 64];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, act[m][4 * q + 0], acc[o][m], 0, 0, 0);
                    acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, act[m][4 * q + 1], acc[o][m], 0, 0, 0);
                    acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, act[m][4 * q + 2], acc[o][m], 0, 0, 0);
                    acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, act[m][4 * q + 3], acc[o][m], 0, 0, 0);
                }
            }
        }
    }
    gemm_epilogue<NOB, MT>(G, acc, row, ob0, h);
}

// ---- row GEMM, split-bf16 form (opt-in; dgt_split.h): same contract, same accumulator image, same epilogue -----------------------------
// G.W points at the matrix's slot of the split tape (csrc/dgt2d_pack.cpp): [out block][nk * 4 K16 steps][hi, mid, lo][64 lanes][8 bf16].
// Per K chunk of 64 the activations of a tile become four Split8; a "group" is one (output block, K chunk) = 4 K16 steps = 12 KiB of
// tape, whose 24 * MT MFMAs run while the next group's twelve 16-byte loads are in flight (WPipeS<4>); the next chunk's activation rows
// are requested before the chunk's first group.  With MT > 1 neighbouring MFMAs alternate between the tiles.  Output blocks past NB (NB
// not a multiple of NOB) read the last block's tape again and are dropped by the epilogue.
// Shape, by measurement (ZINC250k B = 2000, ms per sampling step, exact form 21.5): NOB x MT = 4 x 2 18.33, 8 x 1 17.95 - one tile per wave
// halves the splits per MFMA and doubles the tape traffic per row, and the splits cost more; 8 x 1 with the next chunk's split issued
// between the last group's MFMAs (sched_group_barrier) 17.95: nothing, not kept.  DESIGN.md 4j has the kernel tables.
constexpr int K2S_NOB = 8, K2S_MT = 1;
template <int NOB, int MT>
__global__ __launch_bounds__(64) void k2d_gemm_s(Gemm2 G) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int strip = blockIdx.x, ob0 = blockIdx.y * NOB;
    f32x16 acc[NOB][MT];
    int row[MT];
    const float* xr[MT];
    float nxt[MT][32];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        row[m] = (strip * MT + m) * 32 + j;
        xr[m] = G.X + (size_t)min(row[m], G.rows - 1) * G.ldx;
        load_nat<2>(xr[m], h, nxt[m]);
#pragma unroll
        for (int o = 0; o < NOB; ++o) acc[o][m] = zero16();
    }
    const WSrc ws = make_wsrc(G.W, lane);
    const unsigned blk = (unsigned)G.nk * 12288u;
    unsigned boff[NOB];
#pragma unroll
    for (int o = 0; o < NOB; ++o) boff[o] = (unsigned)min(ob0 + o, G.NB - 1) * blk;
    WPipeS<4> wp;
    wpipe_prime_s(wp, ws, boff[0]);
    for (int kc = 0; kc < G.nk; ++kc) {
        Split8 xs[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) xs[m][g] = split8(&nxt[m][8 * g]);
        if (kc + 1 < G.nk) {
#pragma unroll
            for (int m = 0; m < MT; ++m) load_nat<2>(xr[m] + (kc + 1) * 64, h, nxt[m]);
        }
#pragma unroll
        for (int o = 0; o < NOB; ++o) {
            u32x4 cur[4][3];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < 3; ++t) cur[i][t] = wp.q[i][t];
            // (behind the last group the ring re-reads that group: a live address, never consumed)
            const unsigned nof = o + 1 < NOB ? boff[o + 1] + (unsigned)kc * 12288u : boff[0] + (unsigned)min(kc + 1, G.nk - 1) * 12288u;
            wpipe_prime_s(wp, ws, nof);
            pipeline_fence();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16x8 wh = as_bf16x8(cur[i][0]), wm = as_bf16x8(cur[i][1]), wl = as_bf16x8(cur[i][2]);
                // the six products of mfma_step_s, small terms first, dealt over the tiles
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xs[m][i].l, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xs[m][i].h, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, xs[m][i].m, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xs[m][i].m, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, xs[m][i].h, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xs[m][i].h, acc[o][m], 0, 0, 0);
            }
            pipeline_fence();
        }
    }
    gemm_epilogue<NOB, MT>(G, acc, row, ob0, h);
}

// ---- embeddings ------------------------------------------------------------------------------------------------------------------
__global__ void k2d_embed_nodes(K2 A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.Nn * D2) return;
    const int node = idx >> 8, f = idx & 255;
    const int nb = A.node_b[node], b = nb >> 8, i = nb & 255;
    const float* w = A.W + A.wg[J2_NODE_EMB_W] + (size_t)f * 2 * A.nd;
    const float* x = A.xh + ((size_t)b * A.N + i) * A.nd;
    float s = A.W[A.wg[J2_NODE_EMB_B] + f];
    for (int k = 0; k < A.nd; ++k) s = fmaf(w[k], x[k], s);
    if (A.cond_x) {
        const float* cx = A.cond_x + ((size_t)b * A.N + i) * A.nd;
        for (int k = 0; k < A.nd; ++k) s = fmaf(w[A.nd + k], cx[k], s);
    }
    A.h[(size_t)node * D2 + f] = s;
    A.ahid[(size_t)node * NHW + f] = s;
}

// item < P: pair (r, c) with r < c; item >= P: its mirror (c, r) (directed fallback only)
__device__ __forceinline__ void item_rc(const K2& A, int item, int& b, int& r, int& c) {
    const int pr = A.pair[item < A.P ? item : item - A.P];
    b = pr >> 12;
    r = (pr >> 6) & 63;
    c = pr & 63;
    if (item >= A.P) { const int t = r; r = c; c = t; }
}

__global__ void k2d_embed_edges(K2 A) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int item = (int)(idx >> 6), f = (int)(idx & 63);
    if (item >= (A.flags[0] ? A.P : 2 * A.P)) return;
    int b, r, c;
    item_rc(A, item, b, r, c);
    const int n = A.mol_n[b];
    const size_t row = (size_t)A.mol_eoff[b] + (size_t)r * n + c;
    const size_t in = (((size_t)b * A.N + r) * A.N + c) * A.ch;
    const float* w = A.W + A.wg[J2_EDGE_EMB_W] + (size_t)f * 2 * A.ch;
    float s = A.W[A.wg[J2_EDGE_EMB_B] + f];
    for (int k = 0; k < A.ch; ++k) s = fmaf(w[k], A.edge_x[in + k], s);
    if (A.cond_edge_x)
        for (int k = 0; k < A.ch; ++k) s = fmaf(w[A.ch + k], A.cond_edge_x[in + k], s);
    A.e[row * DE + f] = s;
    A.ehid[row * EHW + f] = s;
}

// ---- node LayerNorm + modulate: Y = LN(X + gate R) (1 + scale) + shift; one wave per node row -------------------------------------
__global__ __launch_bounds__(256) void k2d_ln_mod(K2 A, const float* X, const float* R, float* Y, int gate_off, int shift_off, int scale_off) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= A.Nn) return;
    const int mrow = A.flags[1] ? 0 : (A.node_b[row] >> 8);
    const float* md = A.mods + (size_t)mrow * MODW + (size_t)A.layer * MODB;
    float4 v = reinterpret_cast<const float4*>(X + (size_t)row * D2)[lane];
    if (R) {
        const float4 r = reinterpret_cast<const float4*>(R + (size_t)row * D2)[lane];
        const float4 g = reinterpret_cast<const float4*>(md + gate_off)[lane];
        v.x = fmaf(g.x, r.x, v.x); v.y = fmaf(g.y, r.y, v.y); v.z = fmaf(g.z, r.z, v.z); v.w = fmaf(g.w, r.w, v.w);
    }
    float s = (v.x + v.y) + (v.z + v.w);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    const float mean = s * (1.f / D2);
    v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
    float q = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) q += __shfl_xor(q, m);
    const float rstd = 1.f / sqrtf(q * (1.f / D2) + 1e-6f);
    const float4 sh = reinterpret_cast<const float4*>(md + shift_off)[lane], sc = reinterpret_cast<const float4*>(md + scale_off)[lane];
    float4 y;
    y.x = fmaf(v.x * rstd, 1.f + sc.x, sh.x); y.y = fmaf(v.y * rstd, 1.f + sc.y, sh.y);
    y.z = fmaf(v.z * rstd, 1.f + sc.z, sh.z); y.w = fmaf(v.w * rstd, 1.f + sc.w, sh.w);
    reinterpret_cast<float4*>(Y + (size_t)row * D2)[lane] = y;
}

// one 32-row output block from LDS-resident tiles: acc += W_tile act (tile = 8 quads x 64 lanes of float4)
__device__ __forceinline__ f32x16 mfma_lds(const float4* tile, int lane, const float* act, f32x16 acc) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float4 a = tile[q * 64 + lane];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, act[4 * q + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, act[4 * q + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, act[4 * q + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, act[4 * q + 3], acc, 0, 0, 0);
    }
    return acc;
}

// ---- 2-D attention: one wave per target atom, sources in chunks of 32 (one per lane pair), running softmax ---------------------------
// Lane (j, h): source r0 + j, half h.  Scores: half 0 holds attention heads 0 (adjacency) .. 7, half 1 heads 8 .. 15; the value /
// lin_edge1 channels of block ob on half h are those of head 8 h + ob (row maps of csrc/dgt2d_pack.cpp).
// DEFER (the pair-walk entry launches both attention kernels): leave at once when the inputs are symmetric, k2d_attn_pair does the
// work then; otherwise record in flags[2] that the directed walk ran.
template <bool DEFER>
__global__ __launch_bounds__(256, 1) void k2d_attn(K2 A) {
    if (DEFER) {
        if (A.flags[0]) return;
        if (blockIdx.x == 0 && threadIdx.x == 0) const_cast<int32_t*>(A.flags)[2] = 0;
    }
    __shared__ float4 wl[16 * 512];
    {
        const float4* src = reinterpret_cast<const float4*>(A.W + A.wb[J2B_LE_W]);
        for (int i = threadIdx.x; i < 16 * 512; i += 256) wl[i] = src[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int sym = A.flags[0], uni = A.flags[1];
    for (int t = blockIdx.x * 4 + wave; t < A.Nn; t += gridDim.x * 4) {
        const int nb = A.node_b[t], b = nb >> 8, c = nb & 255;
        const int n = A.mol_n[b], noff = A.mol_noff[b];
        const size_t eoff = (size_t)A.mol_eoff[b];
        float* out_row = A.hn + (size_t)t * D2;
        if (n == 1) {                                        // no sources: the block's attention output is zero
            reinterpret_cast<float4*>(out_row)[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float* md = A.mods + (size_t)(uni ? 0 : b) * MODW + (size_t)A.layer * MODB + 6 * D2;
        const float* qrow = A.qkv + (size_t)t * 3 * D2 + h * 128;
        float mx[8], den[8], out[8];             // out[ob]: channel j % 16 of attention head 8 h + ob
#pragma unroll
        for (int i = 0; i < 8; ++i) { mx[i] = -INFINITY; den[i] = 0.f; }
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = 0.f;
        for (int r0 = 0; r0 < n; r0 += 32) {
            const int r = r0 + j;
            const bool valid = r < n && r != c;
            const int rs = valid ? r : (c == 0 ? 1 : 0);     // a live row for masked lanes (their weight is zero)
            const size_t row = sym ? eoff + (size_t)min(rs, c) * n + max(rs, c) : eoff + (size_t)rs * n + c;
            float et[32];
            load_nat<2>(A.e + row * DE, h, et);
            layer_norm<32>(et);
            modulate<2>(et, md, md + DE, h);
            const float* krow = A.qkv + (size_t)(noff + rs) * 3 * D2 + D2 + h * 128;
            const float* qr = launder(qrow);                 // (re-read per chunk instead of 128 hoisted registers)
            float seg[7], tail = 0.f;
#pragma unroll
            for (int g = 0; g < 7; ++g) seg[g] = 0.f;
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) {
                const f32x16 acc = mfma_lds(wl + ob * 512, lane, et, zero16());
                float tt[16], kk[16], qq[16];
                tanh16(acc, tt);
                load16(krow + ob * 16, kk);
                load16(qr + ob * 16, qq);
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int slot = ob * 16 + s;
                    const float p = qq[s] * kk[s] * tt[s];
                    if (slot < 119) seg[slot / 17] += p; else tail += p;
                }
                pipeline_fence();                            // keeps the next block's loads from being hoisted above this block (registers)
            }
            tail = pair_sum(tail);
            float S[8];
            if (h == 0) {
                float adj = 1.f;
                if (A.cond_edge_x) adj = A.cond_edge_x[(((size_t)b * A.N + rs) * A.N + c) * A.ch] >= A.th ? 1.f : -1e10f;
                S[0] = adj;
            } else {
                S[0] = tail * 0.25f;
            }
#pragma unroll
            for (int g = 0; g < 7; ++g) S[1 + g] = seg[g] * 0.25f;
            float wgt[8], fsc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float si = valid ? S[i] : -INFINITY;
                const float mnew = fmaxf(mx[i], half_max(si));
                const float muse = mnew == -INFINITY ? 0.f : mnew;
                wgt[i] = valid ? fast_exp(si - muse) : 0.f;
                fsc[i] = fast_exp(mx[i] - muse);
                den[i] = den[i] * fsc[i] + half_sum(wgt[i]);
                mx[i] = mnew;
            }
            const float* vrow = A.qkv + (size_t)(noff + rs) * 3 * D2 + 2 * D2 + h * 128;
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) {
                const f32x16 acc = mfma_lds(wl + (8 + ob) * 512, lane, et, zero16());
                float tt[16], vv[16];
                tanh16(acc, tt);
                load16(vrow + ob * 16, vv);
#pragma unroll
                for (int s = 0; s < 16; ++s) tt[s] = wgt[ob] * vv[s] * tt[s];
                out[ob] = fmaf(out[ob], fsc[ob], half_sum16(tt, j));
                pipeline_fence();
            }
        }
        if (j < 16) {
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) out_row[(8 * h + ob) * 16 + j] = den[ob] > 0.f ? out[ob] / den[ob] : 0.f;
        }
    }
}

// ---- 2-D attention, pair-symmetric walk (opt-in; symmetric inputs only) ---------------------------------------------------------------
// A workgroup of four waves owns a group of whole molecules in 128 atom slots (jodo_dgt2d_pair_fill_desc).  Lane pair (j, h) of wave w
// owns the atom in slot 32 w + j as a TARGET; half h scores heads 8 h .. 8 h + 7 as in k2d_attn.  The waves walk the circulant offsets
// d = 1 .. n / 2: at offset d the lane of atom i evaluates the unordered pair {i, p = (i + d) mod n} once (row (min, max) of the edge
// state: LayerNorm, modulate, both tanh projections) and forms both directions from it: source p into its own softmax, and source i
// into p's, which it hands over through LDS (8 scores per half, then the unweighted message v_i * T1 block by block).  It receives the
// same from the lane of (i - d) mod n.  At d = n / 2 of an even n both lanes meet the same pair: each acts as target only.
// The running (max, sum) and the 128 message accumulators are per lane, so there is no cross-lane reduction, no atomic and no
// scatter; a target's sum order is the offset order, own source before received source, whatever its slot, group or batch.
// The 128 message accumulators of a lane wait in accumulation registers while a pass does not touch them (the vector ALU reaches 256
// of the 512 registers of a wave; left alone the compiler sends part of them to scratch instead).
__device__ __forceinline__ void park(float (&out)[8][16]) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int s = 0; s < 16; ++s) asm volatile("" : "+a"(out[k][s]));
}
struct Pair2 {
    const int* items;            // [n_items][4]: group, first offset, last offset, 0; longest first
    const int* slots;            // [groups][128]: (molecule << 8) | atom, or -1
    int n_items;
};
constexpr int GS = 128;

__global__ __launch_bounds__(256, 1) void k2d_attn_pair(K2 A, Pair2 Q) {
    if (!A.flags[0]) return;                                 // asymmetric inputs / force_directed: k2d_attn<true> does the work
    if (blockIdx.x == 0 && threadIdx.x == 0) const_cast<int32_t*>(A.flags)[2] = 1;
    __shared__ float4 wl[16 * 512];                          // lin_edge0 | lin_edge1, 128 KiB
    __shared__ float4 hs[2 * 2 * GS];                        // hand-over, scores:  [quad][half][slot], 8 KiB
    __shared__ float4 hm[4 * 2 * GS];                        // hand-over, one message block: [quad][half][slot], 16 KiB
    {
        const float4* src = reinterpret_cast<const float4*>(A.W + A.wb[J2B_LE_W]);
        for (int i = threadIdx.x; i < 16 * 512; i += 256) wl[i] = src[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int slot = wave * 32 + j, uni = A.flags[1];
    const int rounds = (Q.n_items + (int)gridDim.x - 1) / (int)gridDim.x;
    for (int rd = 0; rd < rounds; ++rd) {
        // items are sorted longest first; odd rounds run backwards so that a workgroup's long item is followed by a short one
        const int it = rd * (int)gridDim.x + ((rd & 1) ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x);
        if (it >= Q.n_items) continue;                       // (uniform over the workgroup)
        const int g = Q.items[4 * it], d_first = Q.items[4 * it + 1], d_last = Q.items[4 * it + 2];
        const int code = Q.slots[(size_t)g * GS + slot];
        const bool used = code >= 0;
        const int b = used ? code >> 8 : 0, i = used ? code & 255 : 0;
        const int n = A.mol_n[b], noff = A.mol_noff[b];
        const size_t eoff = (size_t)A.mol_eoff[b];
        const int t = noff + i;
        const float* md = A.mods + (size_t)(uni ? 0 : b) * MODW + (size_t)A.layer * MODB + 6 * D2;
        const float* own = A.qkv + (size_t)t * 3 * D2 + h * 128;             // q | k | v of this atom at +0 | +D2 | +2 D2
        float mx[8], den[8], out[8][16];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            mx[k] = -INFINITY; den[k] = 0.f;
#pragma unroll
            for (int s = 0; s < 16; ++s) out[k][s] = 0.f;
        }
        for (int d = d_first; d <= d_last; ++d) {
            const bool act = used && 2 * d <= n;             // this lane has a pair at this offset
            const bool recv = used && 2 * d < n;             // ... and is the partner of another lane's pair
            int p = i + d, s_at = i - d;
            if (p >= n) p -= n;
            if (s_at < 0) s_at += n;
            if (!act) p = i;                                 // idle lanes read a live address (the diagonal row) and drop the result
            const int sslot = recv ? slot - i + s_at : slot; // the slot of the lane that sends to this one
            const size_t row = eoff + (size_t)min(i, p) * n + max(i, p);
            float et[32];
            load_nat<2>(A.e + row * DE, h, et);
            layer_norm<32>(et);
            modulate<2>(et, md, md + DE, h);
            const float* par = A.qkv + (size_t)(noff + p) * 3 * D2 + h * 128;
            float so[7], to = 0.f, ss[7], ts = 0.f;
#pragma unroll
            for (int k = 0; k < 7; ++k) { so[k] = 0.f; ss[k] = 0.f; }
            park(out);                                       // the score pass needs the vector registers
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) {
                const f32x16 acc = mfma_lds(wl + ob * 512, lane, et, zero16());
                float tt[16];
                tanh16(acc, tt);
                const float* pb = launder(par) + ob * 16;    // (opaque per block: keeps the loads of later blocks below this one)
                const float* ib = launder(own) + ob * 16;
                {                                            // source p -> target i
                    float qi[16], kp[16];
                    load16(ib, qi);
                    load16(pb + D2, kp);
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const int c = ob * 16 + s;
                        const float po = qi[s] * kp[s] * tt[s];
                        if (c < 119) so[c / 17] += po; else to += po;
                    }
                }
                {                                            // source i -> target p
                    float qp[16], ki[16];
                    load16(pb, qp);
                    load16(ib + D2, ki);
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const int c = ob * 16 + s;
                        const float ps = qp[s] * ki[s] * tt[s];
                        if (c < 119) ss[c / 17] += ps; else ts += ps;
                    }
                }
                // (the sums are pinned here: instruction selection otherwise defers the eight blocks' tanh and products behind all
                // eight MFMA chains, with eight accumulator blocks and every row load live at once)
#pragma unroll
                for (int k = 0; k < 7; ++k) asm volatile("" : "+v"(so[k]), "+v"(ss[k]));
                asm volatile("" : "+v"(to), "+v"(ts));
                pipeline_fence();
            }
            to = pair_sum(to);
            ts = pair_sum(ts);
            float So[8], Ss[8];
            if (h == 0) {
                float ao = 1.f, as = 1.f;
                if (A.cond_edge_x) {
                    ao = A.cond_edge_x[(((size_t)b * A.N + p) * A.N + i) * A.ch] >= A.th ? 1.f : -1e10f;
                    as = A.cond_edge_x[(((size_t)b * A.N + i) * A.N + p) * A.ch] >= A.th ? 1.f : -1e10f;
                }
                So[0] = ao; Ss[0] = as;
            } else {
                So[0] = to * 0.25f; Ss[0] = ts * 0.25f;
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) { So[1 + k] = so[k] * 0.25f; Ss[1 + k] = ss[k] * 0.25f; }
            hs[h * GS + slot] = make_float4(Ss[0], Ss[1], Ss[2], Ss[3]);
            hs[2 * GS + h * GS + slot] = make_float4(Ss[4], Ss[5], Ss[6], Ss[7]);
            __syncthreads();
            float Sr[8];
            {
                const float4 a0 = hs[h * GS + sslot], a1 = hs[2 * GS + h * GS + sslot];
                Sr[0] = a0.x; Sr[1] = a0.y; Sr[2] = a0.z; Sr[3] = a0.w; Sr[4] = a1.x; Sr[5] = a1.y; Sr[6] = a1.z; Sr[7] = a1.w;
            }
            float w1[8], w2[8], fsc[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float s1 = act ? So[k] : -INFINITY, s2 = recv ? Sr[k] : -INFINITY;
                const float mnew = fmaxf(mx[k], fmaxf(s1, s2));
                const float muse = mnew == -INFINITY ? 0.f : mnew;
                w1[k] = act ? fast_exp(s1 - muse) : 0.f;
                w2[k] = recv ? fast_exp(s2 - muse) : 0.f;
                fsc[k] = fast_exp(mx[k] - muse);
                den[k] = (den[k] * fsc[k] + w1[k]) + w2[k];
                mx[k] = mnew;
            }
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) {
                const f32x16 acc = mfma_lds(wl + (8 + ob) * 512, lane, et, zero16());
                float tt[16], vp[16], vi[16];
                tanh16(acc, tt);
                load16(launder(par) + 2 * D2 + ob * 16, vp);
                load16(launder(own) + 2 * D2 + ob * 16, vi);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    hm[(q * 2 + h) * GS + slot] = make_float4(vi[4 * q] * tt[4 * q], vi[4 * q + 1] * tt[4 * q + 1], vi[4 * q + 2] * tt[4 * q + 2],
                                                              vi[4 * q + 3] * tt[4 * q + 3]);
#pragma unroll
                for (int s = 0; s < 16; ++s) out[ob][s] = fmaf(out[ob][s], fsc[ob], w1[ob] * (vp[s] * tt[s]));
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 m = hm[(q * 2 + h) * GS + sslot];
                    out[ob][4 * q + 0] = fmaf(w2[ob], m.x, out[ob][4 * q + 0]);
                    out[ob][4 * q + 1] = fmaf(w2[ob], m.y, out[ob][4 * q + 1]);
                    out[ob][4 * q + 2] = fmaf(w2[ob], m.z, out[ob][4 * q + 2]);
                    out[ob][4 * q + 3] = fmaf(w2[ob], m.w, out[ob][4 * q + 3]);
                }
#pragma unroll
                for (int s = 0; s < 16; ++s) asm volatile("" : "+a"(out[ob][s]));
                if (ob < 7) __syncthreads();                 // (after block 7 the next offset's score barrier separates the reuse)
            }
        }
        if (used) {                                          // n == 1: no offsets, den = 0, a zero row
            float* out_row = A.hn + (size_t)t * D2 + h * 128;
#pragma unroll
            for (int ob = 0; ob < 8; ++ob) {
                float v[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) v[s] = den[ob] > 0.f ? out[ob][s] / den[ob] : 0.f;
                store16(out_row + ob * 16, v);
            }
        }
    }
}

// per-lane modulation vector in natural-half order (lanes of a strip may belong to different molecules)
__device__ __forceinline__ void lane_vec(const float* p, int h, float (&x)[32]) { load_nat<2>(p, h, x); }

// ---- 2-D pair update: e1 = e + gate_msa (W_n2e (hn_r + hn_c) + b); e2 = modulate(LN(e1)); e' = e2 + gate_mlp FFN(e2); readout ------
__global__ __launch_bounds__(256, 1) void k2d_pair(K2 A) {
    __shared__ float4 wl[9 * 512];                           // ff_linear3 (4 tiles) | ff_linear4 (2 x 2 tiles) | readout (1 tile)
    {
        const float4* s3 = reinterpret_cast<const float4*>(A.W + A.wb[J2B_FF3_W]);
        const float4* s4 = reinterpret_cast<const float4*>(A.W + A.wb[J2B_FF4_W]);
        const float4* sr = reinterpret_cast<const float4*>(A.W + A.wb[J2B_ERO_W]);
        for (int i = threadIdx.x; i < 4 * 512; i += 256) { wl[i] = s3[i]; wl[4 * 512 + i] = s4[i]; }
        for (int i = threadIdx.x; i < 512; i += 256) wl[8 * 512 + i] = sr[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int uni = A.flags[1];
    const int items = A.flags[0] ? A.P : 2 * A.P;
    const float* b2e = A.W + A.wb[J2B_N2E_B];
    const float* b3 = A.W + A.wb[J2B_FF3_B];
    const float* b4 = A.W + A.wb[J2B_FF4_B];
    const float* bro = A.W + A.wb[J2B_ERO_B];
    for (int strip = blockIdx.x * 4 + wave; strip * 32 < items; strip += gridDim.x * 4) {
        const int item = strip * 32 + j;
        const bool live = item < items;
        int b, r, c;
        item_rc(A, live ? item : items - 1, b, r, c);
        const int n = A.mol_n[b], noff = A.mol_noff[b];
        const size_t row = (size_t)A.mol_eoff[b] + (size_t)r * n + c;
        const float* md = A.mods + (size_t)(uni ? 0 : b) * MODW + (size_t)A.layer * MODB + 6 * D2;
        float e[32];
        load_nat<2>(A.e + row * DE, h, e);
        {
            float ur[32], uc[32], g[32], bb[32];
            load_nat<2>(A.u + (size_t)(noff + r) * DE, h, ur);
            load_nat<2>(A.u + (size_t)(noff + c) * DE, h, uc);
            lane_vec(md + 2 * DE, h, g);
            lane_vec(b2e, h, bb);
#pragma unroll
            for (int i = 0; i < 32; ++i) e[i] = fmaf(g[i], (ur[i] + uc[i]) + bb[i], e[i]);
        }
        layer_norm<32>(e);
        {
            float sh[32], sc[32];
            lane_vec(md + 3 * DE, h, sh);
            lane_vec(md + 4 * DE, h, sc);
#pragma unroll
            for (int i = 0; i < 32; ++i) e[i] = fmaf(e[i], 1.f + sc[i], sh[i]);
        }
        float hid[64];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
            const f32x16 acc = mfma_lds(wl + ob * 512, lane, e, zero16());
            float bb[16], o16[16];
            load16(b3 + ob * 32 + 16 * h, bb);
            silu_bias16(acc, bb, o16);
#pragma unroll
            for (int s = 0; s < 16; ++s) hid[ob * 16 + s] = o16[s];
            pipeline_fence();
        }
        float gm[32];
        lane_vec(md + 5 * DE, h, gm);
#pragma unroll
        for (int ob = 0; ob < 2; ++ob) {
            f32x16 acc = mfma_lds(wl + (4 + ob * 2) * 512, lane, hid, zero16());
            acc = mfma_lds(wl + (5 + ob * 2) * 512, lane, hid + 32, acc);
            float bb[16];
            load16(b4 + ob * 32 + 16 * h, bb);
#pragma unroll
            for (int s = 0; s < 16; ++s) e[ob * 16 + s] = fmaf(gm[ob * 16 + s], acc[s] + bb[s], e[ob * 16 + s]);
        }
        const f32x16 racc = mfma_lds(wl + 8 * 512, lane, e, zero16());
        if (live) {
            store_nat<2>(A.e + row * DE, h, e);
            if (h == 0) {
                float bb[16], o16[16];
                load16(bro, bb);
#pragma unroll
                for (int s = 0; s < 16; ++s) o16[s] = racc[s] + bb[s];
                store16(A.ehid + row * EHW + DE + 16 * A.layer, o16);
            }
        }
    }
}

// ---- 2-D pair update, split-bf16 form (opt-in): the same item walk, LayerNorm, modulation and in-place update; the nine tiles on the
// bf16 MFMA from an LDS copy of the block's tape slots (108 KiB: one workgroup of eight waves per compute unit, two waves per SIMD) -----
__device__ __forceinline__ f32x16 mfma_lds_s(const u32x4* tile, int lane, const Split8* x, f32x16 acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const bf16x8 wh = as_bf16x8(tile[(g * 3 + 0) * 64 + lane]), wm = as_bf16x8(tile[(g * 3 + 1) * 64 + lane]);
        const bf16x8 wl = as_bf16x8(tile[(g * 3 + 2) * 64 + lane]);
        acc = mfma_step_s(wh, wm, wl, x[g], acc);
    }
    return acc;
}
constexpr int TS16 = 768;                                    // 16-byte words of a tile in split form (4 K16 steps x 3 terms x 64 lanes)

__global__ __launch_bounds__(512, 1) void k2d_pair_s(K2 A) {
    __shared__ u32x4 wl[9 * TS16];                           // ff_linear3 (4 tiles) | ff_linear4 (2 x 2 tiles) | readout (1 tile)
    {
        const u32x4* s3 = reinterpret_cast<const u32x4*>(A.T + A.tb[0]);
        const u32x4* s4 = reinterpret_cast<const u32x4*>(A.T + A.tb[1]);
        const u32x4* sr = reinterpret_cast<const u32x4*>(A.T + A.tb[2]);
        for (int i = threadIdx.x; i < 4 * TS16; i += 512) { wl[i] = s3[i]; wl[4 * TS16 + i] = s4[i]; }
        for (int i = threadIdx.x; i < TS16; i += 512) wl[8 * TS16 + i] = sr[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int uni = A.flags[1];
    const int items = A.flags[0] ? A.P : 2 * A.P;
    const float* b2e = A.W + A.wb[J2B_N2E_B];
    const float* b3 = A.W + A.wb[J2B_FF3_B];
    const float* b4 = A.W + A.wb[J2B_FF4_B];
    const float* bro = A.W + A.wb[J2B_ERO_B];
    for (int strip = blockIdx.x * 8 + wave; strip * 32 < items; strip += gridDim.x * 8) {
        const int item = strip * 32 + j;
        const bool live = item < items;
        int b, r, c;
        item_rc(A, live ? item : items - 1, b, r, c);
        const int n = A.mol_n[b], noff = A.mol_noff[b];
        const size_t row = (size_t)A.mol_eoff[b] + (size_t)r * n + c;
        const float* md = A.mods + (size_t)(uni ? 0 : b) * MODW + (size_t)A.layer * MODB + 6 * D2;
        float e[32];
        load_nat<2>(A.e + row * DE, h, e);
        {
            float ur[32], uc[32], g[32], bb[32];
            load_nat<2>(A.u + (size_t)(noff + r) * DE, h, ur);
            load_nat<2>(A.u + (size_t)(noff + c) * DE, h, uc);
            lane_vec(md + 2 * DE, h, g);
            lane_vec(b2e, h, bb);
#pragma unroll
            for (int i = 0; i < 32; ++i) e[i] = fmaf(g[i], (ur[i] + uc[i]) + bb[i], e[i]);
        }
        layer_norm<32>(e);
        {
            float sh[32], sc[32];
            lane_vec(md + 3 * DE, h, sh);
            lane_vec(md + 4 * DE, h, sc);
#pragma unroll
            for (int i = 0; i < 32; ++i) e[i] = fmaf(e[i], 1.f + sc[i], sh[i]);
        }
        Split8 xs[4], hs[8];                                 // the hidden layer's f32 accumulators are split once, block by block
#pragma unroll
        for (int g = 0; g < 4; ++g) xs[g] = split8(&e[8 * g]);
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
            const f32x16 acc = mfma_lds_s(wl + ob * TS16, lane, xs, zero16());
            float bb[16], o16[16];
            load16(b3 + ob * 32 + 16 * h, bb);
            silu_bias16(acc, bb, o16);
            hs[2 * ob] = split8(&o16[0]);
            hs[2 * ob + 1] = split8(&o16[8]);
            pipeline_fence();
        }
        float gm[32];
        lane_vec(md + 5 * DE, h, gm);
#pragma unroll
        for (int ob = 0; ob < 2; ++ob) {
            f32x16 acc = mfma_lds_s(wl + (4 + ob * 2) * TS16, lane, hs, zero16());
            acc = mfma_lds_s(wl + (5 + ob * 2) * TS16, lane, hs + 4, acc);
            float bb[16];
            load16(b4 + ob * 32 + 16 * h, bb);
#pragma unroll
            for (int s = 0; s < 16; ++s) e[ob * 16 + s] = fmaf(gm[ob * 16 + s], acc[s] + bb[s], e[ob * 16 + s]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) xs[g] = split8(&e[8 * g]);
        const f32x16 racc = mfma_lds_s(wl + 8 * TS16, lane, xs, zero16());
        if (live) {
            store_nat<2>(A.e + row * DE, h, e);
            if (h == 0) {
                float bb[16], o16[16];
                load16(bro, bb);
#pragma unroll
                for (int s = 0; s < 16; ++s) o16[s] = racc[s] + bb[s];
                store16(A.ehid + row * EHW + DE + 16 * A.layer, o16);
            }
        }
    }
}

// ---- edge heads: exist / type MLPs on [e0 | 8 readouts] (192), one evaluation per unordered pair (two when directed), 0.5 (E + E^T) --
__global__ __launch_bounds__(64) void k2d_edge_head(K2 A) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int item = blockIdx.x * 32 + j;
    const bool live = item < A.P;
    const int sym = A.flags[0];
    int b, r, c;
    item_rc(A, live ? item : A.P - 1, b, r, c);
    const int n = A.mol_n[b];
    const size_t eoff = (size_t)A.mol_eoff[b];
    const float4* w1 = reinterpret_cast<const float4*>(A.W + A.wg[J2_EH1_W]);
    const float4* w2 = reinterpret_cast<const float4*>(A.W + A.wg[J2_EH2_W]);
    const float* b1 = A.W + A.wg[J2_EH1_B];
    const float* b2 = A.W + A.wg[J2_EH2_B];
    const float* w3 = A.W + A.wg[J2_EH3_W];
    const float* b3 = A.W + A.wg[J2_EH3_B];
    float res[4] = {0.f, 0.f, 0.f, 0.f};
    for (int dir = 0; dir < (sym ? 1 : 2); ++dir) {
        const size_t row = dir == 0 ? eoff + (size_t)r * n + c : eoff + (size_t)c * n + r;
        f32x16 a1[4];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) a1[ob] = zero16();
#pragma unroll
        for (int kc = 0; kc < 3; ++kc) {
            float x[32];
            load_nat<2>(A.ehid + row * EHW + kc * 64, h, x);
#pragma unroll
            for (int ob = 0; ob < 4; ++ob) {
                a1[ob] = mfma_block<8>(w1 + (size_t)(ob * 3 + kc) * 512 + lane, x, a1[ob]);
                pipeline_fence();
            }
        }
        float h1[64];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
            float bb[16], o16[16];
            load16(b1 + ob * 32 + 16 * h, bb);
            silu_bias16(a1[ob], bb, o16);
#pragma unroll
            for (int s = 0; s < 16; ++s) h1[ob * 16 + s] = o16[s];
        }
#pragma unroll
        for (int mlp = 0; mlp < 2; ++mlp) {                  // 0 = edge_exist_mlp, 1 = edge_type_mlp
            const f32x16 acc = mfma_block<8>(w2 + (size_t)mlp * 512 + lane, *reinterpret_cast<const float(*)[32]>(h1 + mlp * 32), zero16());
            float bb[16], h2[16];
            load16(b2 + mlp * 32 + 16 * h, bb);
            silu_bias16(acc, bb, h2);
            const int k0 = mlp == 0 ? 0 : 1, k1 = mlp == 0 ? 1 : A.ch;
            for (int k = k0; k < k1; ++k) {
                float wv[16], s = 0.f;
                load16(w3 + k * 32 + 16 * h, wv);
#pragma unroll
                for (int i = 0; i < 16; ++i) s = fmaf(wv[i], h2[i], s);
                res[k] += pair_sum(s) + b3[k];
            }
        }
    }
    if (live && h == 0) {
        float* o1 = A.out_edge + (((size_t)b * A.N + r) * A.N + c) * A.ch;
        float* o2 = A.out_edge + (((size_t)b * A.N + c) * A.N + r) * A.ch;
        for (int k = 0; k < A.ch; ++k) {
            const float v = sym ? res[k] : 0.5f * res[k];
            o1[k] = v;
            o2[k] = v;
        }
    }
}

__global__ void k2d_finalize_nodes(K2 A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.Nn * A.nd) return;
    const int node = idx / A.nd, k = idx % A.nd;
    const int nb = A.node_b[node], b = nb >> 8, i = nb & 255;
    A.out_xh[((size_t)b * A.N + i) * A.nd + k] = A.nh3[(size_t)node * 32 + k];
}

// ---- the 2-D sampler's ancestral update -------------------------------------------------------------------------------------------
__global__ void k2d_sampler_step(int B, int N, int nd, int ch, const int32_t* n_nodes, float cx, float cp, float sigma, const float* x,
                                 const float* ex, const float* pred, const float* epred, const float* eps, const float* eeps, float* x_next,
                                 float* e_next, float* x_mean, float* e_mean) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n_node = (size_t)B * N * nd, n_edge = (size_t)B * N * N * ch;
    if (idx < n_node) {
        const int i = (int)((idx / nd) % N), b = (int)(idx / ((size_t)nd * N));
        const float m = cx * x[idx] + cp * pred[idx];
        x_mean[idx] = m;
        x_next[idx] = m + (i < n_nodes[b] ? sigma * eps[idx] : 0.f);
    } else if (idx < n_node + n_edge) {
        const size_t q = idx - n_node;
        const int k = (int)(q % ch), c = (int)((q / ch) % N), r = (int)((q / ((size_t)ch * N)) % N), b = (int)(q / ((size_t)ch * N * N));
        const float m = cx * ex[q] + cp * epred[q];
        e_mean[q] = m;
        const int n = n_nodes[b];
        // the noise of pair {r, c} is the entry of the strict lower triangle (row max, column min), as the reference mirrors it
        const size_t src = (((size_t)b * N + max(r, c)) * N + min(r, c)) * ch + k;
        e_next[q] = m + ((r != c && r < n && c < n) ? sigma * eeps[src] : 0.f);
    }
}

// WS != NULL: the matrix's slot of the split tape, split-bf16 form (never with uni_rows)
int gemm(hipStream_t st, const float* X, int ldx, float* Y, int ldy, const float* W, const float* bias, int rows, int K, int NB, int act,
         const K2& A, const float* R = nullptr, int ldr = 0, const float* gate = nullptr, bool uni_rows = false, const void* WS = nullptr) {
    if (K % 64) return jodo_set_error(JODO_ERR_ARG, "dgt2d gemm: K=%d not a multiple of 64", K);
    Gemm2 G{X, ldx, Y, ldy, W, bias, rows, K / 64, NB, act, R, ldr, gate, MODW, A.node_b, A.flags, uni_rows ? 1 : 0};
    if (WS && !uni_rows) {
        G.W = static_cast<const float*>(WS);
        const int strips = (rows + 32 * K2S_MT - 1) / (32 * K2S_MT);
        if (NB >= 3) { L2D((k2d_gemm_s<K2S_NOB, K2S_MT>), dim3(strips, (NB + K2S_NOB - 1) / K2S_NOB), 64, G); }
        else if (NB == 2) { L2D((k2d_gemm_s<2, K2S_MT>), dim3(strips, 1), 64, G); }
        else { L2D((k2d_gemm_s<1, K2S_MT>), dim3(strips, 1), 64, G); }
    }
    else if (uni_rows) { L2D((k2d_gemm<1, 1>), dim3((rows + 31) / 32, NB), 64, G); }
    else { L2D((k2d_gemm<4, 2>), dim3((rows + 63) / 64, (NB + 3) / 4), 64, G); }
    return JODO_OK;
}

// ---- groups of whole molecules for the pair walk (host) -----------------------------------------------------------------------------
// Molecules by descending size; a group takes the largest remaining molecule, then keeps taking the largest remaining one that still
// fits its 128 slots (the 3-D plan's rule).  N <= 64: every molecule fits a group.  One work item per group, carrying the offsets
// 1 .. max n / 2 of its molecules: a lane's running softmax lives in registers across all offsets of its atom, so a group's offset
// range is not split (splitting it needs a merge pass; unmeasured).  Items are sorted longest first.
struct PairLay {
    int groups, items, off_items, off_slots, words;
};
struct PairGroup { int first, count, dmax; };               // range of `order`, largest n / 2

int make_pair_groups(int B, int N, const int32_t* n, std::vector<int>* order, std::vector<PairGroup>* groups) {
    if (B <= 0 || N <= 0 || !n) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pair: bad batch");
    if (N > 64) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d_pair: padded width %d above 64", N);
    if (B >= (1 << 19)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d_pair: batch %d too large", B);
    std::vector<int> head(66, 0), next_at(66, 0);
    for (int b = 0; b < B; ++b) {
        if (n[b] < 1 || n[b] > N) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pair: n_nodes[%d]=%d outside [1,%d]", b, n[b], N);
        ++head[n[b] + 1];
    }
    for (int s = 1; s < 66; ++s) head[s] += head[s - 1];    // head[s] .. head[s + 1]: molecules of size s, ascending index
    std::vector<int> by_size(B);
    next_at = head;
    for (int b = 0; b < B; ++b) by_size[next_at[n[b]]++] = b;
    next_at = head;                                          // next unplaced molecule of each size
    order->clear(); groups->clear();
    order->reserve(B);
    int left = B, top = 64;
    while (left > 0) {
        PairGroup g{(int)order->size(), 0, 0};
        int room = GS;
        for (;;) {
            while (top > 0 && next_at[top] == head[top + 1]) --top;
            int s = top < room ? top : room;
            while (s > 0 && next_at[s] == head[s + 1]) --s;
            if (s == 0) break;
            order->push_back(by_size[next_at[s]++]);
            if (g.count == 0) g.dmax = s / 2;
            ++g.count; room -= s; --left;
        }
        groups->push_back(g);
    }
    return JODO_OK;
}

PairLay pair_lay(int groups) {
    PairLay l;
    l.groups = groups; l.items = groups; l.off_items = 0; l.off_slots = 4 * groups; l.words = 4 * groups + GS * groups;
    return l;
}

}  // namespace

extern "C" int jodo_dgt2d_layout(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, int64_t* out8) {
    if (!out8) return jodo_set_error(JODO_ERR_ARG, "dgt2d_layout: null argument");
    if (int rc = jodo_dgt2d_check_cfg(cfg)) return rc;
    Lay l;
    if (int rc = make_lay(B, N, n_nodes, &l)) return rc;
    out8[0] = l.words; out8[1] = (int64_t)(l.total * sizeof(float)); out8[2] = l.Nn; out8[3] = l.R;
    out8[4] = (int64_t)(l.h * sizeof(float)); out8[5] = (int64_t)(l.e * sizeof(float)); out8[6] = l.P; out8[7] = 0;
    return JODO_OK;
}

extern "C" int jodo_dgt2d_fill_desc(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, int32_t* desc, int64_t n_words) {
    if (!desc) return jodo_set_error(JODO_ERR_ARG, "dgt2d_fill_desc: null argument");
    if (int rc = jodo_dgt2d_check_cfg(cfg)) return rc;
    Lay l;
    if (int rc = make_lay(B, N, n_nodes, &l)) return rc;
    if (n_words < l.words) return jodo_set_error(JODO_ERR_ARG, "dgt2d_fill_desc: %lld words, need %d", (long long)n_words, l.words);
    int noff = 0, eoff = 0, node = 0, pair = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_nodes[b];
        desc[l.off_n + b] = n; desc[l.off_noff + b] = noff; desc[l.off_eoff + b] = eoff;
        for (int i = 0; i < n; ++i) desc[l.off_node + node++] = (b << 8) | i;
        for (int r = 0; r < n; ++r)
            for (int c = r + 1; c < n; ++c) desc[l.off_pair + pair++] = (b << 12) | (r << 6) | c;
        noff += n; eoff += n * n;
    }
    desc[l.off_pair + pair] = 0;
    return JODO_OK;
}

// pair_desc_dev != NULL: the pair-walk entry (both attention kernels are launched, the flags decide on the device which one works)
static int forward_2d(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev, const void* pair_desc_dev,
                      const float* packed_w, const int64_t* woff, int n_woff, const float* xh, const float* edge_x, const float* cond_x,
                      const float* cond_edge_x, const float* noise_level, float* out_xh, float* out_edge, int32_t* flags_dev,
                      void* workspace, int force_directed, int max_blocks, void* stream, const void* tape_dev = nullptr,
                      const int64_t* toff = nullptr) {
    if (!desc_dev || !packed_w || !woff || !xh || !edge_x || !noise_level || !out_xh || !out_edge || !flags_dev || !workspace)
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward: null argument");
    if (int rc = jodo_dgt2d_check_cfg(cfg)) return rc;
    if ((cond_x == nullptr) != (cond_edge_x == nullptr))
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward: cond_x and cond_edge_x must both be given or both NULL");
    if (n_woff != J2_GLOBAL_COUNT + cfg->n_layers * J2B_BLOCK_COUNT)
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward: weight table has %d slots, expected %d", n_woff, J2_GLOBAL_COUNT + cfg->n_layers * J2B_BLOCK_COUNT);
    static const int split_global[] = {J2_NH1_W, J2_NH2_W, J2_NH3_W};
    static const int split_block[] = {J2B_QKV_W, J2B_N2E_W, J2B_FF1_W, J2B_FF2_W, J2B_NRO_W, J2B_FF3_W, J2B_FF4_W, J2B_ERO_W};
    if (tape_dev) {                                          // split-bf16 form: every covered slot needs its place in the tape
        if (!toff) return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward: split tape without its offset table");
        bool ok = true;
        for (int s : split_global) ok = ok && toff[s] >= 0 && toff[s] % 16 == 0;
        for (int lyr = 0; lyr < cfg->n_layers; ++lyr)
            for (int s : split_block) { const int64_t t = toff[J2_GLOBAL_COUNT + lyr * J2B_BLOCK_COUNT + s]; ok = ok && t >= 0 && t % 16 == 0; }
        if (!ok) return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward: the split tape's offset table misses a covered slot");
    }
    const char* T = static_cast<const char*>(tape_dev);
    auto TG = [&](int slot) -> const void* { return T ? T + toff[slot] : nullptr; };
    Lay l;
    if (int rc = make_lay(B, N, n_nodes, &l)) return rc;
    Pair2 Q{nullptr, nullptr, 0};
    if (pair_desc_dev) {
        std::vector<int> order;
        std::vector<PairGroup> groups;
        if (int rc = make_pair_groups(B, N, n_nodes, &order, &groups)) return rc;
        const PairLay pl = pair_lay((int)groups.size());
        const int* pd = static_cast<const int*>(pair_desc_dev);
        Q.items = pd + pl.off_items; Q.slots = pd + pl.off_slots; Q.n_items = pl.items;
    }
    hipStream_t st = (hipStream_t)stream;
    const int* dsc = static_cast<const int*>(desc_dev);
    float* ws = static_cast<float*>(workspace);
    K2 A;
    A.mol_n = dsc + l.off_n; A.mol_noff = dsc + l.off_noff; A.mol_eoff = dsc + l.off_eoff; A.node_b = dsc + l.off_node; A.pair = dsc + l.off_pair;
    A.B = B; A.N = N; A.Nn = l.Nn; A.P = l.P; A.nd = cfg->in_node_dim; A.ch = cfg->edge_ch; A.layer = 0; A.th = cfg->edge_quan_th;
    A.W = packed_w; A.flags = flags_dev; A.T = T; A.tb[0] = A.tb[1] = A.tb[2] = 0;
    A.xh = xh; A.edge_x = edge_x; A.cond_x = cond_x; A.cond_edge_x = cond_edge_x; A.noise = noise_level; A.out_xh = out_xh; A.out_edge = out_edge;
    A.hid1 = ws + l.hid1; A.tembs = ws + l.tembs; A.mods = ws + l.mods; A.h = ws + l.h; A.hm = ws + l.hm; A.qkv = ws + l.qkv; A.hn = ws + l.hn;
    A.u = ws + l.u; A.f1 = ws + l.f1; A.ahid = ws + l.ahid; A.nh1 = ws + l.nh1; A.nh2 = ws + l.nh2; A.nh3 = ws + l.nh3; A.e = ws + l.e; A.ehid = ws + l.ehid;
    for (int i = 0; i < J2_GLOBAL_COUNT; ++i) A.wg[i] = woff[i];
    for (int i = 0; i < J2B_BLOCK_COUNT; ++i) A.wb[i] = 0;
    const float* W = packed_w;
    const size_t n_out_x = (size_t)B * N * A.nd, n_out_e = (size_t)B * N * N * A.ch;
    if (hipMemsetAsync(out_xh, 0, n_out_x * sizeof(float), st) != hipSuccess || hipMemsetAsync(out_edge, 0, n_out_e * sizeof(float), st) != hipSuccess)
        return jodo_set_error(JODO_ERR_LAUNCH, "dgt2d_forward: clearing the outputs failed");

    // ---- flags, time embedding, modulation rows ----
    L2D(k2d_flags_init, 1, 64, flags_dev, force_directed, T ? 1 : 0);
    L2D(k2d_flags, (unsigned)(((size_t)B * N * N + 255) / 256), 256, A, flags_dev);
    L2D(k2d_time1, B, 256, A);
    int rc;
    if ((rc = gemm(st, A.hid1, T2, A.tembs, T2, W + A.wg[J2_TIME_W3], W + A.wg[J2_TIME_B3], B, T2, T2 / 32, 1, A, nullptr, 0, nullptr, true))) return rc;
    if ((rc = gemm(st, A.tembs, T2, A.mods, MODW, W + A.wg[J2_MOD_W], W + A.wg[J2_MOD_B], B, T2, MODW / 32, 0, A, nullptr, 0, nullptr, true))) return rc;
    // ---- embeddings ----
    L2D(k2d_embed_nodes, (l.Nn * D2 + 255) / 256, 256, A);
    if (l.P > 0) L2D(k2d_embed_edges, (unsigned)(((size_t)2 * l.P * 64 + 255) / 256), 256, A);
    // ---- blocks ----
    const int nblocks = (max_blocks >= 0 && max_blocks < cfg->n_layers) ? max_blocks : cfg->n_layers;
    const int persist = 256;                                 // one workgroup of four waves per compute unit
    for (int lyr = 0; lyr < nblocks; ++lyr) {
        A.layer = lyr;
        const int slot0 = J2_GLOBAL_COUNT + lyr * J2B_BLOCK_COUNT;
        for (int i = 0; i < J2B_BLOCK_COUNT; ++i) A.wb[i] = woff[slot0 + i];
        if (T) { A.tb[0] = toff[slot0 + J2B_FF3_W]; A.tb[1] = toff[slot0 + J2B_FF4_W]; A.tb[2] = toff[slot0 + J2B_ERO_W]; }
        const float* gate_mlp = A.mods + (size_t)lyr * MODB + 5 * D2;
        L2D(k2d_ln_mod, (l.Nn + 3) / 4, 256, A, A.h, (const float*)nullptr, A.hm, 0, 0, D2);
        if ((rc = gemm(st, A.hm, D2, A.qkv, 3 * D2, W + A.wb[J2B_QKV_W], W + A.wb[J2B_QKV_B], l.Nn, D2, 24, 0, A, nullptr, 0, nullptr, false, TG(slot0 + J2B_QKV_W)))) return rc;
        if (pair_desc_dev) {
            L2D(k2d_attn_pair, persist, 256, A, Q);
            L2D(k2d_attn<true>, persist, 256, A);
        } else {
            L2D(k2d_attn<false>, persist, 256, A);
        }
        if ((rc = gemm(st, A.hn, D2, A.u, DE, W + A.wb[J2B_N2E_W], nullptr, l.Nn, D2, 2, 0, A, nullptr, 0, nullptr, false, TG(slot0 + J2B_N2E_W)))) return rc;
        L2D(k2d_ln_mod, (l.Nn + 3) / 4, 256, A, A.h, (const float*)A.hn, A.hm, 2 * D2, 3 * D2, 4 * D2);
        if ((rc = gemm(st, A.hm, D2, A.f1, 2 * D2, W + A.wb[J2B_FF1_W], W + A.wb[J2B_FF1_B], l.Nn, D2, 16, 1, A, nullptr, 0, nullptr, false, TG(slot0 + J2B_FF1_W)))) return rc;
        if ((rc = gemm(st, A.f1, 2 * D2, A.h, D2, W + A.wb[J2B_FF2_W], W + A.wb[J2B_FF2_B], l.Nn, 2 * D2, 8, 0, A, A.hm, D2, gate_mlp, false, TG(slot0 + J2B_FF2_W)))) return rc;
        if ((rc = gemm(st, A.h, D2, A.ahid + D2 + 64 * lyr, NHW, W + A.wb[J2B_NRO_W], W + A.wb[J2B_NRO_B], l.Nn, D2, 2, 0, A, nullptr, 0, nullptr, false, TG(slot0 + J2B_NRO_W)))) return rc;
        if (l.P > 0) {
            if (T) L2D(k2d_pair_s, persist, 512, A);
            else L2D(k2d_pair, 2 * persist, 256, A);
        }
    }
    // ---- heads ----
    if ((rc = gemm(st, A.ahid, NHW, A.nh1, D2, W + A.wg[J2_NH1_W], W + A.wg[J2_NH1_B], l.Nn, NHW, 8, 1, A, nullptr, 0, nullptr, false, TG(J2_NH1_W)))) return rc;
    if ((rc = gemm(st, A.nh1, D2, A.nh2, D2 / 2, W + A.wg[J2_NH2_W], W + A.wg[J2_NH2_B], l.Nn, D2, 4, 1, A, nullptr, 0, nullptr, false, TG(J2_NH2_W)))) return rc;
    if ((rc = gemm(st, A.nh2, D2 / 2, A.nh3, 32, W + A.wg[J2_NH3_W], W + A.wg[J2_NH3_B], l.Nn, D2 / 2, 1, 0, A, nullptr, 0, nullptr, false, TG(J2_NH3_W)))) return rc;
    L2D(k2d_finalize_nodes, (l.Nn * A.nd + 255) / 256, 256, A);
    if (l.P > 0) L2D(k2d_edge_head, (l.P + 31) / 32, 64, A);
    return JODO_OK;
}

extern "C" int jodo_dgt2d_forward(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev, const float* packed_w,
                                  const int64_t* woff, int n_woff, const float* xh, const float* edge_x, const float* cond_x,
                                  const float* cond_edge_x, const float* noise_level, float* out_xh, float* out_edge, int32_t* flags_dev,
                                  void* workspace, int force_directed, int max_blocks, void* stream) {
    return forward_2d(cfg, B, N, n_nodes, desc_dev, nullptr, packed_w, woff, n_woff, xh, edge_x, cond_x, cond_edge_x, noise_level, out_xh,
                      out_edge, flags_dev, workspace, force_directed, max_blocks, stream);
}

extern "C" int jodo_dgt2d_forward_walk(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev,
                                       const void* pair_desc_dev, int walk, const float* packed_w, const int64_t* woff, int n_woff,
                                       const float* xh, const float* edge_x, const float* cond_x, const float* cond_edge_x,
                                       const float* noise_level, float* out_xh, float* out_edge, int32_t* flags_dev, void* workspace,
                                       int force_directed, int max_blocks, void* stream) {
    if (walk != JODO_2D_WALK_DIRECTED && walk != JODO_2D_WALK_PAIR)
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward_walk: walk %d is neither directed (0) nor pair (1)", walk);
    if (walk == JODO_2D_WALK_PAIR && !pair_desc_dev)
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward_walk: the pair walk needs the group descriptor");
    return forward_2d(cfg, B, N, n_nodes, desc_dev, walk == JODO_2D_WALK_PAIR ? pair_desc_dev : nullptr, packed_w, woff, n_woff, xh, edge_x,
                      cond_x, cond_edge_x, noise_level, out_xh, out_edge, flags_dev, workspace, force_directed, max_blocks, stream);
}

// jodo_dgt2d_forward_walk with the split-bf16 form of the node GEMMs and the pair update: tape_dev / toff from jodo_dgt2d_split_size and
// jodo_dgt2d_pack_split_host (the device copy of the tape, the host offset table).  Records flags_dev[3] = 1.
extern "C" int jodo_dgt2d_forward_split(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev,
                                        const void* pair_desc_dev, int walk, const float* packed_w, const int64_t* woff, int n_woff,
                                        const void* tape_dev, const int64_t* toff, const float* xh, const float* edge_x, const float* cond_x,
                                        const float* cond_edge_x, const float* noise_level, float* out_xh, float* out_edge, int32_t* flags_dev,
                                        void* workspace, int force_directed, int max_blocks, void* stream) {
    if (walk != JODO_2D_WALK_DIRECTED && walk != JODO_2D_WALK_PAIR)
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward_split: walk %d is neither directed (0) nor pair (1)", walk);
    if (walk == JODO_2D_WALK_PAIR && !pair_desc_dev)
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward_split: the pair walk needs the group descriptor");
    if (!tape_dev || !toff) return jodo_set_error(JODO_ERR_ARG, "dgt2d_forward_split: null split tape");
    return forward_2d(cfg, B, N, n_nodes, desc_dev, walk == JODO_2D_WALK_PAIR ? pair_desc_dev : nullptr, packed_w, woff, n_woff, xh, edge_x,
                      cond_x, cond_edge_x, noise_level, out_xh, out_edge, flags_dev, workspace, force_directed, max_blocks, stream, tape_dev,
                      toff);
}

// tests: the production row GEMM on caller-packed weights, Y [rows, n_out] = epi(X [rows, K] W^T + bias).  split = 0: w_dev is the f32
// packing, k2d_gemm<4, 2>; split = 1: the split packing (both as jodo_debug_pack_split emits them), k2d_gemm_s as forward_2d launches it.
extern "C" int jodo_debug_gemm2d(int split, const float* x, int rows, int K, int n_out, const void* w_dev, const float* bias, int act,
                                 float* y, void* stream) {
    if (!x || !w_dev || !y || rows <= 0 || K <= 0 || n_out <= 0 || n_out % 32 || (act != 0 && act != 1))
        return jodo_set_error(JODO_ERR_ARG, "debug_gemm2d: bad argument");
    K2 A{};
    return gemm((hipStream_t)stream, x, K, y, n_out, static_cast<const float*>(w_dev), bias, rows, K, n_out / 32, act, A, nullptr, 0, nullptr,
                false, split ? w_dev : nullptr);
}

extern "C" int jodo_dgt2d_pair_layout(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, int64_t* out8) {
    if (!out8) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pair_layout: null argument");
    if (int rc = jodo_dgt2d_check_cfg(cfg)) return rc;
    std::vector<int> order;
    std::vector<PairGroup> groups;
    if (int rc = make_pair_groups(B, N, n_nodes, &order, &groups)) return rc;
    const PairLay pl = pair_lay((int)groups.size());
    out8[0] = pl.words; out8[1] = pl.groups; out8[2] = pl.items; out8[3] = pl.off_items; out8[4] = pl.off_slots; out8[5] = GS;
    out8[6] = 4; out8[7] = 0;
    return JODO_OK;
}

extern "C" int jodo_dgt2d_pair_fill_desc(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, int32_t* desc, int64_t n_words) {
    if (!desc) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pair_fill_desc: null argument");
    if (int rc = jodo_dgt2d_check_cfg(cfg)) return rc;
    std::vector<int> order;
    std::vector<PairGroup> groups;
    if (int rc = make_pair_groups(B, N, n_nodes, &order, &groups)) return rc;
    const PairLay pl = pair_lay((int)groups.size());
    if (n_words < pl.words) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pair_fill_desc: %lld words, need %d", (long long)n_words, pl.words);
    // groups come out in descending order of their largest molecule, which is the order of their offset counts: longest items first
    for (int g = 0; g < pl.groups; ++g) {
        int32_t* item = desc + pl.off_items + 4 * g;
        item[0] = g; item[1] = 1; item[2] = groups[g].dmax; item[3] = 0;
        int32_t* slots = desc + pl.off_slots + (size_t)GS * g;
        int at = 0;
        for (int m = 0; m < groups[g].count; ++m) {
            const int b = order[groups[g].first + m];
            for (int i = 0; i < n_nodes[b]; ++i) slots[at++] = (b << 8) | i;
        }
        for (; at < GS; ++at) slots[at] = -1;
    }
    return JODO_OK;
}

extern "C" int jodo_sampler_step_2d(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float cx, float cp, float sigma,
                                    const float* x, const float* edge_x, const float* pred, const float* edge_pred, const float* eps_node,
                                    const float* eps_edge, float* x_next, float* edge_next, float* x_mean, float* edge_mean, void* stream) {
    if (B <= 0 || N <= 0 || node_feats <= 0 || edge_ch <= 0 || !n_nodes_dev || !x || !edge_x || !pred || !edge_pred || !eps_node || !eps_edge ||
        !x_next || !edge_next || !x_mean || !edge_mean)
        return jodo_set_error(JODO_ERR_ARG, "sampler_step_2d: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const size_t tot = (size_t)B * N * node_feats + (size_t)B * N * N * edge_ch;
    L2D(k2d_sampler_step, (unsigned)((tot + 255) / 256), 256, B, N, node_feats, edge_ch, n_nodes_dev, cx, cp, sigma, x, edge_x, pred, edge_pred,
        eps_node, eps_edge, x_next, edge_next, x_mean, edge_mean);
    return JODO_OK;
}

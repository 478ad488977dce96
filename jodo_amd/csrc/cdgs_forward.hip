// jodo_cdgs_forward: one evaluation of the 2-D graph noise-prediction network CDGS (include/jodo_hip.h, section "CDGS").
//
// Layout.  Real atoms are compact: node row = noff_b + i.  The edge state keeps n_b^2 rows of 256 floats per molecule, row(b, r, c) =
// eoff_b + r n_b + c, every ordered pair its own row (the directed walk: nothing assumes symmetric inputs).  The diagonal rows are zero
// between blocks; inside a block they hold FF(2 h_i), which the reference's dense edge GroupNorm sees on the diagonal.
//
// Every projection is exact fp32 on v_mfma_f32_32x32x2_f32 in the strip model of dgt_device.h (kc_gemm: 32 rows per wave, weights as A
// operand, packed by csrc/cdgs_pack.cpp); three forms of the row load: a plain row, a row plus its molecule's time shift, and h_r + h_c
// of an edge row.  Per block:
//   kc_addt (h + t_node) -> kc_gine (GINE aggregation over the thresholded adjacency) -> kc_gemm x 2 (gin_nn)
//   kc_gemm (q | k | v) -> kc_gemm over edge rows (tanh(E0 (e + t_edge)) | tanh(E1 (e + t_edge))) -> kc_attn (softmax over sources)
//   kc_gn2 (GroupNorm(h + local) + GroupNorm(h + attn)) -> kc_gemm x 2 (node FF) -> kc_gn2 (norm2_node) -> kc_gemm (node readout)
//   kc_gemm x 2 over edge rows (e + FF(h_r + h_c), in place) and over the Nn + 1 rows [h ; 0] (the padded partners' FF(h_i), FF(0))
//   kc_estats (per (molecule, group) moments over 8 channels x N x N positions of the PADDED batch, double accumulators, fixed order)
//   kc_enorm (normalise, affine, mask; second pass in place) -> kc_gemm (edge readout)
// No float atomics anywhere: every reduction has one owner and a fixed order.
//
// jodo_cdgs_forward_split (opt-in, model.bf16x3): the same launch sequence with every kc_gemm over node rows or edge rows replaced by
// kc_gemm_s, the split-bf16 form (dgt_split.h) reading a weight tape derived from the packed blob; the three GEMMs over the B
// time-embedding rows and every other kernel are the exact-fp32 ones above.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"
#include "dgt_device.h"
#include "dgt_split.h"
#include "cdgs_common.h"

using namespace jd;

namespace {

constexpr int DC = 256, HC = 16;               // width, heads (16 channels each)

#define LCD(kern, grid, block, ...)                                               \
    do {                                                                          \
        auto kf_ = kern;                                                          \
        hipLaunchKernelGGL(kf_, dim3(grid), dim3(block), 0, st, __VA_ARGS__);     \
        int rc_ = jodo_check_launch(#kern);                                       \
        if (rc_ != JODO_OK) return rc_;                                           \
    } while (0)

struct Lay {                     // sizes and workspace offsets (in floats)
    int B, N, Nn, L, cat, catp, KA, KE;
    int64_t R;
    size_t tin, t1, temb, tmod, land, nin, h, hs, agg, g1, g2, qkv, att, hc, f1, f2, x1, xff, ahid, a1, a2, a3;
    size_t ad, pa, pb, cnt, e, tmp, ehid, eh3, mean, rstd, total;
    int off_n, off_noff, off_eoff, off_node, off_pair;
    int64_t words;
};

int make_lay(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n, Lay* o) {
    if (B <= 0 || N <= 0 || !n) return jodo_set_error(JODO_ERR_ARG, "cdgs: bad batch");
    if (N > JODO_CDGS_MAX_N) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: padded width %d above the limit %d", N, JODO_CDGS_MAX_N);
    if (B >= (1 << 20)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: batch %d too large", B);
    int64_t Nn = 0, R = 0;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 1 || n[b] > N) return jodo_set_error(JODO_ERR_ARG, "cdgs: n_nodes[%d]=%d outside [1,%d]", b, n[b], N);
        Nn += n[b]; R += (int64_t)n[b] * n[b];
    }
    if (R >= ((int64_t)1 << 26)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: batch too large (%lld edge rows)", (long long)R);
    o->B = B; o->N = N; o->Nn = (int)Nn; o->R = R; o->L = cfg->n_layers;
    o->cat = 2 * DC / o->L; o->catp = (o->cat + 31) / 32 * 32;
    o->KA = (o->L * o->catp + 154 + 63) / 64 * 64; o->KE = (o->L * o->catp + 192 + 63) / 64 * 64;
    const size_t Bp = (size_t)(B + 63) / 64 * 64, Np = (size_t)(Nn + 1 + 63) / 64 * 64, Rp = (size_t)(R + 63) / 64 * 64;
    size_t at = 0;
    auto take = [&](size_t cnt) { size_t a = at; at += (cnt + 63) / 64 * 64; return a; };
    o->tin = take(Bp * DC); o->t1 = take(Bp * 2 * DC); o->temb = take(Bp * DC); o->tmod = take(Bp * 2 * DC * o->L);
    o->land = take(Np * 16); o->nin = take(Np * DC); o->h = take(Np * DC); o->hs = take(Np * DC); o->agg = take(Np * DC);
    o->g1 = take(Np * DC); o->g2 = take(Np * DC); o->qkv = take(Np * 3 * DC); o->att = take(Np * DC); o->hc = take(Np * DC);
    o->f1 = take(Np * 2 * DC); o->f2 = take(Np * DC); o->x1 = take(Np * 2 * DC); o->xff = take(Np * DC);
    o->ahid = take(Np * o->KA); o->a1 = take(Np * DC); o->a2 = take(Np * (DC / 2)); o->a3 = take(Np * 32);
    o->ad = take(Rp); o->pa = take(Rp); o->pb = take(Rp); o->cnt = take(Rp);
    o->e = take(Rp * DC); o->tmp = take(Rp * 2 * DC); o->ehid = take(Rp * o->KE); o->eh3 = take(Rp * 32);
    o->mean = take(Bp * 32); o->rstd = take(Bp * 32);
    o->total = at;
    o->off_n = 0; o->off_noff = B; o->off_eoff = 2 * B; o->off_node = 3 * B; o->off_pair = 3 * B + (int)Nn;
    o->words = (int64_t)3 * B + Nn + R;
    return JODO_OK;
}

struct KC {                      // kernel arguments
    const int *mol_n, *mol_noff, *mol_eoff, *node_b, *pair_b;
    int B, N, Nn, ach, ch, K, L, catp, KA, KE;
    int64_t R;
    const float* W;
    const float *t, *x, *edge_x;
    float *out_x, *out_e;
    float *tin, *land, *nin, *h, *hs, *agg, *qkv, *att, *hc, *xff, *ahid, *a3, *ad, *pa, *pb, *e, *tmp, *ehid, *eh3, *mean, *rstd, *tmod;
    int* cnt;
    int64_t wg[JCG_GLOBAL_COUNT], wb[JCB_BLOCK_COUNT];
};

// ---- row GEMM: Y[rows, 32 NB] = R + act(X'[rows, 64 nk] W^T + bias) ---------------------------------------------------------------------
// X' by MODE: 0 the row of X; 1 the row of X plus row `rowmol[row]` of xadd (an edge row and its molecule's time shift); 2 the sum of two
// rows of X, those of the atoms r and c of edge row `row` (h_r + h_c).  act: 0 none, 1 SiLU, 2 ReLU, 3 tanh.  R may alias Y.
struct GemmC {
    const float* X; int ldx; float* Y; int ldy; const float* W; const float* bias; int rows, nk, NB, act;
    const float* R; int ldr;
    const float* xadd; int ldadd; const int* rowmol; const int *mol_n, *mol_noff, *mol_eoff;
};
constexpr int GC_NOB = 4, GC_MT = 2;
// bias, activation, residual and the store of a strip's 32 x 32 accumulator images: the one epilogue of both forms of the row GEMM
template <int NOB, int MT>
__device__ __forceinline__ void gemmc_epilogue(const GemmC& G, const f32x16 (&acc)[NOB][MT], const int (&row)[MT], int ob0, int h) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (row[m] >= G.rows) continue;
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
                else if (G.act == 2) v[s] = fmaxf(v[s], 0.f);
                else if (G.act == 3) v[s] = tanh_f(v[s]);
            }
            if (G.R) {
                float rr[16];
                load16(G.R + (size_t)row[m] * G.ldr + col0, rr);
#pragma unroll
                for (int s = 0; s < 16; ++s) v[s] += rr[s];
            }
            store16(G.Y + (size_t)row[m] * G.ldy + col0, v);
        }
    }
}
// the source rows of output row rw: xs is the second row of modes 1 and 2 (NULL in mode 0)
template <int MODE>
__device__ __forceinline__ void gemmc_src(const GemmC& G, int rw, const float*& xr, const float*& xs) {
    if (MODE == 2) {
        const int b = G.rowmol[rw], n = G.mol_n[b], loc = rw - G.mol_eoff[b];
        xr = G.X + (size_t)(G.mol_noff[b] + loc / n) * G.ldx;
        xs = G.X + (size_t)(G.mol_noff[b] + loc % n) * G.ldx;
    } else {
        xr = G.X + (size_t)rw * G.ldx;
        xs = MODE == 1 ? G.xadd + (size_t)G.rowmol[rw] * G.ldadd : nullptr;
    }
}
template <int MODE>
__global__ __launch_bounds__(64) void kc_gemm(GemmC G) {
    constexpr int NOB = GC_NOB, MT = GC_MT;
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int strip = blockIdx.x, ob0 = blockIdx.y * NOB;
    f32x16 acc[NOB][MT];
    int row[MT];
    const float *xr[MT], *xs[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        row[m] = (strip * MT + m) * 32 + j;
        gemmc_src<MODE>(G, min(row[m], G.rows - 1), xr[m], xs[m]);
#pragma unroll
        for (int o = 0; o < NOB; ++o) acc[o][m] = zero16();
    }
    for (int kc = 0; kc < G.nk; ++kc) {
        float act[MT][32];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            load_nat<2>(xr[m] + kc * 64, h, act[m]);
            if (MODE != 0) {
                float add[32];
                load_nat<2>(xs[m] + kc * 64, h, add);
#pragma unroll
                for (int s = 0; s < 32; ++s) act[m][s] += add[s];
            }
        }
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
    gemmc_epilogue<NOB, MT>(G, acc, row, ob0, h);
}

// ---- row GEMM, split-bf16 form (opt-in; dgt_split.h): same contract, same accumulator image, same epilogue ----------------------------
// The counterpart of k2d_gemm_s (csrc/dgt2d_forward.hip) with the three row loads of kc_gemm.  G.W points at the matrix's slot of the split
// tape (csrc/cdgs_pack.cpp): [out block][nk * 4 K16 steps][hi, mid, lo][64 lanes][8 bf16].  Per K chunk of 64 the activations of a tile
// become four Split8; in modes 1 and 2 the two source rows are added in fp32 first, as kc_gemm adds them before its MFMAs, and the sum is
// split.  A group is one (output block, K chunk) = 4 K16 steps = 12 KiB of tape, whose 24 MT MFMAs run while the next group's twelve
// 16-byte loads are in flight (WPipeS<4>); the next chunk's rows (both of them in modes 1 and 2) are requested before the chunk's first
// group.  Output blocks past NB read the last block's tape again and are dropped by the epilogue.  DESIGN.md 4n has the shape table.
constexpr int GCS_NOB = 8, GCS_MT = 1;
template <int MODE, int NOB, int MT>
__global__ __launch_bounds__(64) void kc_gemm_s(GemmC G) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int strip = blockIdx.x, ob0 = blockIdx.y * NOB;
    f32x16 acc[NOB][MT];
    int row[MT];
    const float *xr[MT], *xs[MT];
    float nxt[MT][32], nad[MT][32];                          // nad: the second row of modes 1 and 2 (dead in mode 0)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        row[m] = (strip * MT + m) * 32 + j;
        gemmc_src<MODE>(G, min(row[m], G.rows - 1), xr[m], xs[m]);
        load_nat<2>(xr[m], h, nxt[m]);
        if (MODE != 0) load_nat<2>(xs[m], h, nad[m]);
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
        Split8 xv[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (MODE != 0) {
#pragma unroll
                for (int s = 0; s < 32; ++s) nxt[m][s] += nad[m][s];
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) xv[m][g] = split8(&nxt[m][8 * g]);
        }
        if (kc + 1 < G.nk) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                load_nat<2>(xr[m] + (kc + 1) * 64, h, nxt[m]);
                if (MODE != 0) load_nat<2>(xs[m] + (kc + 1) * 64, h, nad[m]);
            }
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
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xv[m][i].l, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xv[m][i].h, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, xv[m][i].m, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xv[m][i].m, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, xv[m][i].h, acc[o][m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xv[m][i].h, acc[o][m], 0, 0, 0);
            }
            pipeline_fence();
        }
    }
    gemmc_epilogue<NOB, MT>(G, acc, row, ob0, h);
}

// GroupNorm of one 256-wide row held one channel per thread: groups of 8 consecutive lanes, biased variance around the mean, eps 1e-6
__device__ __forceinline__ float gn8(float v, float gamma, float beta) {
    float s = v;
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
    const float mean = s * 0.125f, d = v - mean;
    float q = d * d;
    q += __shfl_xor(q, 1); q += __shfl_xor(q, 2); q += __shfl_xor(q, 4);
    return d * rsqrtf(q * 0.125f + 1e-6f) * gamma + beta;
}

// ---- prologue -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kc_time(KC A) {                       // sinusoid of t * 999: [sin (128) | cos (128)]
    const int b = blockIdx.x, c = threadIdx.x;
    A.tin[(size_t)b * DC + c] = jcdgs::sinusoid(A.t[b], A.W + A.wg[JCG_FREQ], c, DC / 2);
}

// Random-walk features of one molecule: AD = adj / (deg + 1e-8), powers AD^2 .. AD^(K+1) through two buffers, the landing probabilities
// (their diagonals) and per ordered pair the count of powers with no walk.  Padded atoms have empty rows and columns in the reference's
// padded matrices, so the n x n corner is the whole computation.
__global__ __launch_bounds__(256) void kc_rw(KC A) {
    const int b = blockIdx.x, n = A.mol_n[b], noff = A.mol_noff[b], eoff = A.mol_eoff[b], nn = n * n;
    __shared__ float deg[JODO_CDGS_MAX_N + 3];
    float *ad = A.ad + eoff, *pa = A.pa + eoff, *pb = A.pb + eoff;
    int* cnt = A.cnt + eoff;
    for (int idx = threadIdx.x; idx < nn; idx += 256) {
        const int r = idx / n, c = idx % n;
        ad[idx] = jcdgs::adjacent(r != c, A.edge_x[(((size_t)b * A.N + r) * A.N + c) * A.ch]) ? 1.f : 0.f;
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += 256) {
        float s = 0.f;
        for (int c = 0; c < n; ++c) s += ad[r * n + c];
        deg[r] = s + 1e-8f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nn; idx += 256) {
        const float v = ad[idx] / deg[idx / n];
        ad[idx] = v; pa[idx] = v; cnt[idx] = 0;
    }
    __syncthreads();
    for (int m = 0; m < A.K; ++m) {
        const float* src = (m & 1) ? pb : pa;
        float* dst = (m & 1) ? pa : pb;
        for (int idx = threadIdx.x; idx < nn; idx += 256) {
            const int r = idx / n, c = idx % n;
            float s = 0.f;
            for (int k = 0; k < n; ++k) s = fmaf(src[r * n + k], ad[k * n + c], s);
            dst[idx] = s;
            if (s <= 0.f) cnt[idx] += 1;
            if (r == c) A.land[(size_t)(noff + r) * 16 + m] = s;
        }
        __syncthreads();
    }
}

// the 256-wide input row of the node embedding [degree (51) | atom_cate (154) | rw landing (51)]; atom_cate also goes to the head input
__global__ __launch_bounds__(256) void kc_embed_nodes(KC A) {
    const int node = blockIdx.x, c = threadIdx.x, b = A.node_b[node], i = node - A.mol_noff[b];
    __shared__ float dsum[4];
    if (c < A.ch) {                                   // the reference sums edge_x over the whole padded row, unmasked
        float s = 0.f;
        const float* p = A.edge_x + (((size_t)b * A.N + i) * A.N) * A.ch + c;
        for (int jn = 0; jn < A.N; ++jn) s += p[(size_t)jn * A.ch];
        dsum[c] = s;
    }
    __syncthreads();
    float v;
    if (c < 51) {
        v = A.W[A.wg[JCG_AD_B] + c];
        for (int k = 0; k < A.ch; ++k) v = fmaf(A.W[A.wg[JCG_AD_W] + c * A.ch + k], dsum[k], v);
    } else if (c < 205) {
        const int o = c - 51;
        v = A.W[A.wg[JCG_AC_B] + o];
        const float* xp = A.x + ((size_t)b * A.N + i) * A.ach;
        for (int k = 0; k < A.ach; ++k) v = fmaf(A.W[A.wg[JCG_AC_W] + o * A.ach + k], xp[k], v);
        A.ahid[(size_t)node * A.KA + A.L * A.catp + o] = v;
    } else {
        const int o = c - 205;
        v = A.W[A.wg[JCG_AR_B] + o];
        for (int k = 0; k < A.K; ++k) v = fmaf(A.W[A.wg[JCG_AR_W] + o * A.K + k], A.land[(size_t)node * 16 + k], v);
    }
    A.nin[(size_t)node * DC + c] = v;
}

// the 256-wide input row of the edge embedding [dense_cate (77) | dense_exist (77) | dense_spd (102)] per edge row; the first two also
// go to the head input
__global__ __launch_bounds__(256) void kc_embed_edges(KC A) {
    const size_t row = blockIdx.x;
    const int c = threadIdx.x, b = A.pair_b[row], n = A.mol_n[b], loc = (int)(row - A.mol_eoff[b]), r = loc / n, cc = loc % n;
    const float* ex = A.edge_x + (((size_t)b * A.N + r) * A.N + cc) * A.ch;
    float v;
    if (c < 77) {
        v = A.W[A.wg[JCG_EC_B] + c];
        for (int k = 0; k < A.ch - 1; ++k) v = fmaf(A.W[A.wg[JCG_EC_W] + c * (A.ch - 1) + k], ex[1 + k], v);
        A.ehid[row * A.KE + A.L * A.catp + c] = v;
    } else if (c < 154) {
        const int o = c - 77;
        v = fmaf(A.W[A.wg[JCG_EX_W] + o], ex[0], A.W[A.wg[JCG_EX_B] + o]);
        A.ehid[row * A.KE + A.L * A.catp + 96 + o] = v;
    } else {
        const int o = c - 154;
        v = A.W[A.wg[JCG_SPD_W] + o * (A.K + 1) + A.cnt[row]] + A.W[A.wg[JCG_SPD_B] + o];
    }
    A.tmp[row * DC + c] = v;
}

__global__ __launch_bounds__(256) void kc_zero_diag(KC A) {
    const int node = blockIdx.x, b = A.node_b[node], n = A.mol_n[b], i = node - A.mol_noff[b];
    A.e[((size_t)A.mol_eoff[b] + (size_t)i * n + i) * DC + threadIdx.x] = 0.f;
    // row Nn of hc: the "0" of the [h ; 0] rows whose FF(0) the padded partners read; no kernel of a block writes it, so it is
    // written here on every forward instead of being left to the workspace's first zero fill
    if (node == 0) A.hc[(size_t)A.Nn * DC + threadIdx.x] = 0.f;
}

// ---- block -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kc_addt(KC A, int layer) {             // hs = h + t_node(SiLU(temb))
    const int node = blockIdx.x, c = threadIdx.x, b = A.node_b[node];
    A.hs[(size_t)node * DC + c] = A.h[(size_t)node * DC + c] + A.tmod[((size_t)b * A.L + layer) * 2 * DC + c];
}

// GINE aggregation at target i: (1 + eps) hs_i + sum over sources j with adj[j, i] of relu(hs_j + e[j, i] + t_edge)
__global__ __launch_bounds__(256) void kc_gine(KC A, int layer) {
    const int node = blockIdx.x, c = threadIdx.x, b = A.node_b[node], n = A.mol_n[b], noff = A.mol_noff[b], i = node - noff;
    const size_t eoff = (size_t)A.mol_eoff[b];
    const float te = A.tmod[((size_t)b * A.L + layer) * 2 * DC + DC + c];
    float s = (1.f + A.W[A.wb[JCB_EPS]]) * A.hs[(size_t)node * DC + c];
    for (int jn = 0; jn < n; ++jn) {
        const size_t row = eoff + (size_t)jn * n + i;
        if (A.ad[row] > 0.f) s += fmaxf(A.hs[(size_t)(noff + jn) * DC + c] + (A.e[row * DC + c] + te), 0.f);
    }
    A.agg[(size_t)node * DC + c] = s;
}

// EdgeGateTransLayer at target i, one thread per (head, channel): logits over the sources j != i, softmax (max, exp, sum + 1e-16),
// messages.  tmp holds tanh(E0 e') | tanh(E1 e') per edge row.
__global__ __launch_bounds__(256) void kc_attn(KC A) {
    const int node = blockIdx.x, t = threadIdx.x, hd = t >> 4, b = A.node_b[node], n = A.mol_n[b], noff = A.mol_noff[b], i = node - noff;
    const size_t eoff = (size_t)A.mol_eoff[b];
    __shared__ float lg[JODO_CDGS_MAX_N * HC];
    const float q = A.qkv[(size_t)node * 3 * DC + t];
    for (int jn = 0; jn < n; ++jn) {
        if (jn == i) continue;
        const size_t row = eoff + (size_t)jn * n + i;
        float p = q * A.qkv[(size_t)(noff + jn) * 3 * DC + DC + t] * A.tmp[row * 2 * DC + t];
        p += __shfl_xor(p, 8); p += __shfl_xor(p, 4); p += __shfl_xor(p, 2); p += __shfl_xor(p, 1);
        if ((t & 15) == 0) lg[jn * HC + hd] = p * 0.25f;
    }
    __syncthreads();
    float mx = -INFINITY, sum = 0.f, out = 0.f;
    for (int jn = 0; jn < n; ++jn)
        if (jn != i) mx = fmaxf(mx, lg[jn * HC + hd]);
    for (int jn = 0; jn < n; ++jn)
        if (jn != i) sum += expf(lg[jn * HC + hd] - mx);
    const float inv = 1.f / (sum + 1e-16f);
    for (int jn = 0; jn < n; ++jn) {
        if (jn == i) continue;
        const size_t row = eoff + (size_t)jn * n + i;
        const float alpha = expf(lg[jn * HC + hd] - mx) * inv;
        out = fmaf(A.qkv[(size_t)(noff + jn) * 3 * DC + 2 * DC + t] * A.tmp[row * 2 * DC + DC + t], alpha, out);
    }
    A.att[(size_t)node * DC + t] = out;
}

// Y = GroupNorm(X1 + A1; g1, b1) [+ GroupNorm(X2 + A2; g2, b2)] per node row
__global__ __launch_bounds__(256) void kc_gn2(int Nn, const float* X1, const float* A1, const float* g1, const float* b1, const float* X2,
                                              const float* A2, const float* g2, const float* b2, float* Y) {
    const size_t at = (size_t)blockIdx.x * DC + threadIdx.x;
    const int c = threadIdx.x;
    float v = gn8(X1[at] + A1[at], g1[c], b1[c]);
    if (X2) v += gn8(X2[at] + A2[at], g2[c], b2[c]);
    Y[at] = v;
}

// Moments of the edge GroupNorm of one molecule, over 8 channels x N x N positions of the padded batch: the n^2 rows of e (diagonal
// included), 2 (N - n) times FF(h_i) per real atom (xff rows noff .. noff + n - 1) and (N - n)^2 times FF(0) (xff row Nn).  One thread
// per (channel, quarter of the rows), double sums in a fixed order.
__global__ __launch_bounds__(1024) void kc_estats(KC A) {
    const int b = blockIdx.x, c = threadIdx.x & 255, part = threadIdx.x >> 8, n = A.mol_n[b], noff = A.mol_noff[b], nn = n * n;
    const float* e = A.e + (size_t)A.mol_eoff[b] * DC;
    __shared__ double ss[4][DC], sq[4][DC];
    double s = 0.0, q = 0.0;
    for (int r = part; r < nn; r += 4) { const double v = e[(size_t)r * DC + c]; s += v; q += v * v; }
    const double pad = (double)(A.N - n);
    double s1 = 0.0, q1 = 0.0;
    for (int r = part; r < n; r += 4) { const double v = A.xff[(size_t)(noff + r) * DC + c]; s1 += v; q1 += v * v; }
    s += 2.0 * pad * s1; q += 2.0 * pad * q1;
    if (part == 0) { const double v = A.xff[(size_t)A.Nn * DC + c]; s += pad * pad * v; q += pad * pad * v * v; }
    ss[part][c] = s; sq[part][c] = q;
    __syncthreads();
    if (threadIdx.x < 32) {
        const int g = threadIdx.x;
        double S = 0.0, Q = 0.0;
        for (int k = 0; k < 8; ++k)
            for (int p = 0; p < 4; ++p) { S += ss[p][g * 8 + k]; Q += sq[p][g * 8 + k]; }
        const double cntv = 8.0 * (double)A.N * (double)A.N, mean = S / cntv;
        double var = Q / cntv - mean * mean;
        if (var < 0.0) var = 0.0;
        A.mean[(size_t)b * 32 + g] = (float)mean;
        A.rstd[(size_t)b * 32 + g] = (float)(1.0 / sqrt(var + 1e-6));
    }
}

__global__ __launch_bounds__(256) void kc_enorm(KC A) {
    const size_t row = blockIdx.x;
    const int c = threadIdx.x, b = A.pair_b[row], n = A.mol_n[b], loc = (int)(row - A.mol_eoff[b]);
    float v = 0.f;
    if (loc / n != loc % n)
        v = (A.e[row * DC + c] - A.mean[(size_t)b * 32 + (c >> 3)]) * A.rstd[(size_t)b * 32 + (c >> 3)] * A.W[A.wb[JCB_NE_G] + c] + A.W[A.wb[JCB_NE_B] + c];
    A.e[row * DC + c] = v;
}

// ---- epilogue ----------------------------------------------------------------------------------------------------------------------
__global__ void kc_out_nodes(KC A) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)A.B * A.N * A.ach) return;
    const int c = (int)(idx % A.ach), i = (int)((idx / A.ach) % A.N), b = (int)(idx / ((size_t)A.ach * A.N));
    A.out_x[idx] = i < A.mol_n[b] ? A.a3[(size_t)(A.mol_noff[b] + i) * 32 + c] : 0.f;
}
__global__ void kc_out_edges(KC A) {                   // (s + s^T) / 2 over the two directed rows of a pair, masked
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)A.B * A.N * A.N * A.ch) return;
    const int c = (int)(idx % A.ch);
    const size_t p = idx / A.ch;
    const int j = (int)(p % A.N), i = (int)((p / A.N) % A.N), b = (int)(p / ((size_t)A.N * A.N)), n = A.mol_n[b];
    float v = 0.f;
    if (i < n && j < n && i != j) {
        const size_t eoff = (size_t)A.mol_eoff[b];
        v = (A.eh3[(eoff + (size_t)i * n + j) * 32 + c] + A.eh3[(eoff + (size_t)j * n + i) * 32 + c]) * 0.5f;
    }
    A.out_e[idx] = v;
}

__global__ void kc_flags_init(int32_t* flags) {            // the 2-D model's flag words: [3] = the split-bf16 form ran; the others unused here
    if (threadIdx.x < 4) flags[threadIdx.x] = threadIdx.x == 3 ? 1 : 0;
}

struct Ctx { hipStream_t st; const KC* A; };

// the split form of one row-load mode, dispatched on NB as the 2-D launcher does
template <int MODE>
int gemm_split(hipStream_t st, const GemmC& G) {
    const unsigned strips = (unsigned)((G.rows + 32 * GCS_MT - 1) / (32 * GCS_MT));
    if (G.NB >= 3) LCD((kc_gemm_s<MODE, GCS_NOB, GCS_MT>), dim3(strips, (unsigned)((G.NB + GCS_NOB - 1) / GCS_NOB)), 64, G);
    else if (G.NB == 2) LCD((kc_gemm_s<MODE, 2, GCS_MT>), dim3(strips, 1), 64, G);
    else LCD((kc_gemm_s<MODE, 1, GCS_MT>), dim3(strips, 1), 64, G);
    return JODO_OK;
}

// WS != NULL: the matrix's slot of the split tape, split-bf16 form (kc_gemm_s); W is then not read
int gemm(const Ctx& C, int mode, const float* X, int ldx, int64_t rows, int Kc, const float* W, const float* bias, int n_out, int act,
         float* Y, int ldy, const float* R = nullptr, int ldr = 0, const float* xadd = nullptr, int ldadd = 0, const void* WS = nullptr) {
    if (rows <= 0) return JODO_OK;
    hipStream_t st = C.st;
    GemmC G;
    G.X = X; G.ldx = ldx; G.Y = Y; G.ldy = ldy; G.W = W; G.bias = bias; G.rows = (int)rows; G.nk = (Kc + 63) / 64; G.NB = (n_out + 31) / 32;
    G.act = act; G.R = R; G.ldr = ldr; G.xadd = xadd; G.ldadd = ldadd; G.rowmol = C.A->pair_b; G.mol_n = C.A->mol_n;
    G.mol_noff = C.A->mol_noff; G.mol_eoff = C.A->mol_eoff;
    if (WS) {
        G.W = static_cast<const float*>(WS);
        return mode == 0 ? gemm_split<0>(st, G) : mode == 1 ? gemm_split<1>(st, G) : gemm_split<2>(st, G);
    }
    const dim3 grid((unsigned)((rows + 32 * GC_MT - 1) / (32 * GC_MT)), (unsigned)((G.NB + GC_NOB - 1) / GC_NOB));
    if (mode == 0) LCD(kc_gemm<0>, grid, 64, G);
    else if (mode == 1) LCD(kc_gemm<1>, grid, 64, G);
    else LCD(kc_gemm<2>, grid, 64, G);
    return JODO_OK;
}

}  // namespace

extern "C" int jodo_cdgs_layout(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes, int64_t* out8) {
    if (!out8) return jodo_set_error(JODO_ERR_ARG, "cdgs_layout: null argument");
    if (int rc = jodo_cdgs_check_cfg(cfg)) return rc;
    Lay l;
    if (int rc = make_lay(cfg, B, N, n_nodes, &l)) return rc;
    out8[0] = l.words; out8[1] = (int64_t)(l.total * sizeof(float)); out8[2] = l.Nn; out8[3] = l.R;
    out8[4] = (int64_t)(l.h * sizeof(float)); out8[5] = (int64_t)(l.e * sizeof(float)); out8[6] = (int64_t)(l.cnt * sizeof(float));
    out8[7] = (int64_t)(l.land * sizeof(float));
    return JODO_OK;
}

extern "C" int jodo_cdgs_fill_desc(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes, int32_t* desc, int64_t n_words) {
    if (!desc) return jodo_set_error(JODO_ERR_ARG, "cdgs_fill_desc: null argument");
    if (int rc = jodo_cdgs_check_cfg(cfg)) return rc;
    Lay l;
    if (int rc = make_lay(cfg, B, N, n_nodes, &l)) return rc;
    if (n_words < l.words) return jodo_set_error(JODO_ERR_ARG, "cdgs_fill_desc: %lld words, need %lld", (long long)n_words, (long long)l.words);
    int noff = 0, eoff = 0;
    int64_t node = 0, pair = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_nodes[b];
        desc[l.off_n + b] = n; desc[l.off_noff + b] = noff; desc[l.off_eoff + b] = eoff;
        for (int i = 0; i < n; ++i) desc[l.off_node + node++] = b;
        for (int i = 0; i < n * n; ++i) desc[l.off_pair + pair++] = b;
        noff += n; eoff += n * n;
    }
    return JODO_OK;
}

// the covered slots of the split tape (csrc/cdgs_pack.cpp split_slots): every row GEMM over node rows or edge rows
static const int split_global[] = {JCG_NEMB_W, JCG_EEMB_W, JCG_AH1_W, JCG_AH2_W, JCG_AH3_W, JCG_EH1_W, JCG_EH2_W, JCG_EH3_W};
static const int split_block[] = {JCB_GIN1_W, JCB_GIN2_W, JCB_QKV_W, JCB_E01_W, JCB_FF1_W, JCB_FF2_W, JCB_FF3_W, JCB_FF4_W, JCB_RN_W, JCB_RE_W};

// tape_dev != NULL: the split-bf16 form of the node-row and edge-row GEMMs (flags_dev then receives {0, 0, 0, 1}); the launch sequence
// is the same either way
static int forward_cdgs(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev, const float* packed_w,
                        const int64_t* woff, int n_woff, const float* t, const float* x, const float* edge_x, float* out_x, float* out_e,
                        void* workspace, int max_blocks, void* stream, const void* tape_dev = nullptr, const int64_t* toff = nullptr,
                        int32_t* flags_dev = nullptr) {
    if (!desc_dev || !packed_w || !woff || !t || !x || !edge_x || !out_x || !out_e || !workspace)
        return jodo_set_error(JODO_ERR_ARG, "cdgs_forward: null argument");
    if (int rc = jodo_cdgs_check_cfg(cfg)) return rc;
    if (n_woff != JCG_GLOBAL_COUNT + cfg->n_layers * JCB_BLOCK_COUNT)
        return jodo_set_error(JODO_ERR_ARG, "cdgs_forward: weight table has %d slots, expected %d", n_woff, JCG_GLOBAL_COUNT + cfg->n_layers * JCB_BLOCK_COUNT);
    if (tape_dev) {                                          // split-bf16 form: every covered slot needs its place in the tape
        if (!toff || !flags_dev) return jodo_set_error(JODO_ERR_ARG, "cdgs_forward: split tape without its offset table or the flag words");
        bool ok = true;
        for (int s : split_global) ok = ok && toff[s] >= 0 && toff[s] % 16 == 0;
        for (int lyr = 0; lyr < cfg->n_layers; ++lyr)
            for (int s : split_block) { const int64_t o = toff[JCG_GLOBAL_COUNT + lyr * JCB_BLOCK_COUNT + s]; ok = ok && o >= 0 && o % 16 == 0; }
        if (!ok) return jodo_set_error(JODO_ERR_ARG, "cdgs_forward: the split tape's offset table misses a covered slot");
    }
    const char* T = static_cast<const char*>(tape_dev);
    Lay l;
    if (int rc = make_lay(cfg, B, N, n_nodes, &l)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int* dsc = static_cast<const int*>(desc_dev);
    float* ws = static_cast<float*>(workspace);
    KC A;
    A.mol_n = dsc + l.off_n; A.mol_noff = dsc + l.off_noff; A.mol_eoff = dsc + l.off_eoff; A.node_b = dsc + l.off_node; A.pair_b = dsc + l.off_pair;
    A.B = B; A.N = N; A.Nn = l.Nn; A.R = l.R; A.ach = cfg->atom_ch; A.ch = cfg->edge_ch; A.K = cfg->rw_depth; A.L = l.L; A.catp = l.catp;
    A.KA = l.KA; A.KE = l.KE; A.W = packed_w; A.t = t; A.x = x; A.edge_x = edge_x; A.out_x = out_x; A.out_e = out_e;
    A.tin = ws + l.tin; A.land = ws + l.land; A.nin = ws + l.nin; A.h = ws + l.h; A.hs = ws + l.hs; A.agg = ws + l.agg; A.qkv = ws + l.qkv;
    A.att = ws + l.att; A.hc = ws + l.hc; A.xff = ws + l.xff; A.ahid = ws + l.ahid; A.a3 = ws + l.a3; A.ad = ws + l.ad; A.pa = ws + l.pa;
    A.pb = ws + l.pb; A.cnt = reinterpret_cast<int*>(ws + l.cnt); A.e = ws + l.e; A.tmp = ws + l.tmp; A.ehid = ws + l.ehid; A.eh3 = ws + l.eh3;
    A.mean = ws + l.mean; A.rstd = ws + l.rstd; A.tmod = ws + l.tmod;
    for (int i = 0; i < JCG_GLOBAL_COUNT; ++i) A.wg[i] = woff[i];
    for (int i = 0; i < JCB_BLOCK_COUNT; ++i) A.wb[i] = 0;
    float *t1 = ws + l.t1, *temb = ws + l.temb, *g1 = ws + l.g1, *g2 = ws + l.g2, *f1 = ws + l.f1, *f2 = ws + l.f2, *x1 = ws + l.x1,
          *a1 = ws + l.a1, *a2 = ws + l.a2;
    const float* W = packed_w;
    const Ctx C{st, &A};
    const int Nn = l.Nn, L = l.L, D = DC;
    const unsigned R = (unsigned)l.R;
    int rc;
    // a row GEMM over node rows or edge rows: weights of woff slot `slot`, from the split tape when there is one
    auto mm = [&](int mode, const float* X, int ldx, int64_t rows, int Kc, int slot, const float* bias, int n_out, int act, float* Y, int ldy,
                  const float* Rs = nullptr, int ldr = 0, const float* xadd = nullptr, int ldadd = 0) {
        return gemm(C, mode, X, ldx, rows, Kc, W + woff[slot], bias, n_out, act, Y, ldy, Rs, ldr, xadd, ldadd, T ? T + toff[slot] : nullptr);
    };
    if (T) LCD(kc_flags_init, 1, 64, flags_dev);
    // ---- time embedding and every block's time shifts (the blocks read temb only through SiLU; exact fp32 in both forms) ----
    LCD(kc_time, B, 256, A);
    if ((rc = gemm(C, 0, A.tin, D, B, D, W + A.wg[JCG_T1_W], W + A.wg[JCG_T1_B], 2 * D, 1, t1, 2 * D))) return rc;
    if ((rc = gemm(C, 0, t1, 2 * D, B, 2 * D, W + A.wg[JCG_T2_W], W + A.wg[JCG_T2_B], D, 1, temb, D))) return rc;
    if ((rc = gemm(C, 0, temb, D, B, D, W + A.wg[JCG_TMOD_W], W + A.wg[JCG_TMOD_B], 2 * D * L, 0, A.tmod, 2 * D * L))) return rc;
    // ---- random-walk features and embeddings ----
    LCD(kc_rw, B, 256, A);
    LCD(kc_embed_nodes, Nn, 256, A);
    if ((rc = mm(0, A.nin, D, Nn, D, JCG_NEMB_W, W + A.wg[JCG_NEMB_B], D, 0, A.h, D))) return rc;
    LCD(kc_embed_edges, R, 256, A);
    if ((rc = mm(0, A.tmp, D, l.R, D, JCG_EEMB_W, W + A.wg[JCG_EEMB_B], D, 0, A.e, D))) return rc;
    LCD(kc_zero_diag, Nn, 256, A);
    // ---- blocks ----
    const bool stop = max_blocks >= 0 && max_blocks <= L;
    const int nblocks = stop ? max_blocks : L;
    for (int lyr = 0; lyr < nblocks; ++lyr) {
        const int slot0 = JCG_GLOBAL_COUNT + lyr * JCB_BLOCK_COUNT;
        for (int i = 0; i < JCB_BLOCK_COUNT; ++i) A.wb[i] = woff[slot0 + i];
        const float* te = A.tmod + (size_t)lyr * 2 * D + D;          // row b of the time shifts: stride 2 D L
        LCD(kc_addt, Nn, 256, A, lyr);
        LCD(kc_gine, Nn, 256, A, lyr);
        if ((rc = mm(0, A.agg, D, Nn, D, slot0 + JCB_GIN1_W, W + A.wb[JCB_GIN1_B], D, 2, g1, D))) return rc;
        if ((rc = mm(0, g1, D, Nn, D, slot0 + JCB_GIN2_W, W + A.wb[JCB_GIN2_B], D, 0, g2, D))) return rc;
        if ((rc = mm(0, A.hs, D, Nn, D, slot0 + JCB_QKV_W, W + A.wb[JCB_QKV_B], 3 * D, 0, A.qkv, 3 * D))) return rc;
        if ((rc = mm(1, A.e, D, l.R, D, slot0 + JCB_E01_W, nullptr, 2 * D, 3, A.tmp, 2 * D, nullptr, 0, te, 2 * D * L))) return rc;
        LCD(kc_attn, Nn, 256, A);
        LCD(kc_gn2, Nn, 256, Nn, (const float*)A.h, (const float*)g2, W + A.wb[JCB_NL_G], W + A.wb[JCB_NL_B], (const float*)A.h,
            (const float*)A.att, W + A.wb[JCB_NA_G], W + A.wb[JCB_NA_B], A.hc);
        if ((rc = mm(0, A.hc, D, Nn, D, slot0 + JCB_FF1_W, W + A.wb[JCB_FF1_B], 2 * D, 1, f1, 2 * D))) return rc;
        if ((rc = mm(0, f1, 2 * D, Nn, 2 * D, slot0 + JCB_FF2_W, W + A.wb[JCB_FF2_B], D, 0, f2, D))) return rc;
        LCD(kc_gn2, Nn, 256, Nn, (const float*)A.hc, (const float*)f2, W + A.wb[JCB_NN_G], W + A.wb[JCB_NN_B], (const float*)nullptr,
            (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, A.h);
        if ((rc = mm(0, A.h, D, Nn, D, slot0 + JCB_RN_W, W + A.wb[JCB_RN_B], l.catp, 0, A.ahid + lyr * l.catp, l.KA))) return rc;
        // edge path: e <- e + FF(h_r + h_c) in place; FF(h_i) and FF(0) for the padded positions (row Nn of hc is the zero row: kc_zero_diag writes it, no block does)
        if ((rc = mm(2, A.hc, D, l.R, D, slot0 + JCB_FF3_W, W + A.wb[JCB_FF3_B], 2 * D, 1, A.tmp, 2 * D))) return rc;
        if ((rc = mm(0, A.tmp, 2 * D, l.R, 2 * D, slot0 + JCB_FF4_W, W + A.wb[JCB_FF4_B], D, 0, A.e, D, A.e, D))) return rc;
        if ((rc = mm(0, A.hc, D, Nn + 1, D, slot0 + JCB_FF3_W, W + A.wb[JCB_FF3_B], 2 * D, 1, x1, 2 * D))) return rc;
        if ((rc = mm(0, x1, 2 * D, Nn + 1, 2 * D, slot0 + JCB_FF4_W, W + A.wb[JCB_FF4_B], D, 0, A.xff, D))) return rc;
        LCD(kc_estats, B, 1024, A);
        LCD(kc_enorm, R, 256, A);
        if ((rc = mm(0, A.e, D, l.R, D, slot0 + JCB_RE_W, W + A.wb[JCB_RE_B], l.catp, 0, A.ehid + lyr * l.catp, l.KE))) return rc;
    }
    if (stop) return JODO_OK;                                        // debug stop: h and e stay in the workspace (the heads reuse e)
    // ---- heads ----
    if ((rc = mm(0, A.ahid, l.KA, Nn, l.KA, JCG_AH1_W, W + A.wg[JCG_AH1_B], D, 1, a1, D))) return rc;
    if ((rc = mm(0, a1, D, Nn, D, JCG_AH2_W, W + A.wg[JCG_AH2_B], D / 2, 1, a2, D / 2))) return rc;
    if ((rc = mm(0, a2, D / 2, Nn, D / 2, JCG_AH3_W, W + A.wg[JCG_AH3_B], 32, 0, A.a3, 32))) return rc;
    if ((rc = mm(0, A.ehid, l.KE, l.R, l.KE, JCG_EH1_W, W + A.wg[JCG_EH1_B], 2 * D, 1, A.tmp, 2 * D))) return rc;
    if ((rc = mm(0, A.tmp, 2 * D, l.R, 2 * D, JCG_EH2_W, W + A.wg[JCG_EH2_B], D, 1, A.e, D))) return rc;
    if ((rc = mm(0, A.e, D, l.R, D, JCG_EH3_W, W + A.wg[JCG_EH3_B], 32, 0, A.eh3, 32))) return rc;
    LCD(kc_out_nodes, (unsigned)(((size_t)B * N * A.ach + 255) / 256), 256, A);
    LCD(kc_out_edges, (unsigned)(((size_t)B * N * N * A.ch + 255) / 256), 256, A);
    return JODO_OK;
}

extern "C" int jodo_cdgs_forward(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev, const float* packed_w,
                                 const int64_t* woff, int n_woff, const float* t, const float* x, const float* edge_x, float* out_x,
                                 float* out_e, void* workspace, int max_blocks, void* stream) {
    return forward_cdgs(cfg, B, N, n_nodes, desc_dev, packed_w, woff, n_woff, t, x, edge_x, out_x, out_e, workspace, max_blocks, stream);
}

// jodo_cdgs_forward with the split-bf16 form of every row GEMM over node rows and edge rows: tape_dev / toff from jodo_cdgs_split_size and
// jodo_cdgs_pack_split_host (the device copy of the tape, the host offset table).  Its first launch writes flags_dev[0..3] = {0, 0, 0, 1}.
extern "C" int jodo_cdgs_forward_split(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev,
                                       const float* packed_w, const int64_t* woff, int n_woff, const float* t, const float* x,
                                       const float* edge_x, float* out_x, float* out_e, void* workspace, int max_blocks, void* stream,
                                       const void* tape_dev, const int64_t* toff, int32_t* flags_dev) {
    if (!tape_dev || !toff || !flags_dev) return jodo_set_error(JODO_ERR_ARG, "cdgs_forward_split: null split tape, offset table or flag words");
    return forward_cdgs(cfg, B, N, n_nodes, desc_dev, packed_w, woff, n_woff, t, x, edge_x, out_x, out_e, workspace, max_blocks, stream,
                        tape_dev, toff, flags_dev);
}

// tests: the production row GEMM on caller-packed device weights, y [rows, n_out] = residual + act(x' [rows, K] W^T + bias) with x' by
// mode as in GemmC.  split = 0: w_dev is the f32 packing, kc_gemm; split = 1: the split packing (both as jodo_debug_pack_split emits
// them), kc_gemm_s as forward_cdgs launches it.  Modes 1 and 2 read the descriptor of (cfg, B, N, n_nodes) and need rows = its edge rows.
extern "C" int jodo_debug_gemm_cdgs(int split, int mode, const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev,
                                    const float* x, int ldx, int rows, int K, int n_out, const void* w_dev, const float* bias, int act,
                                    const float* xadd, int ldadd, const float* residual, float* y, int ldy, void* stream) {
    if (!x || !w_dev || !y || rows <= 0 || K <= 0 || K % 64 || n_out <= 0 || n_out % 32 || act < 0 || act > 3 || mode < 0 || mode > 2 ||
        ldx < K || ldy < n_out)
        return jodo_set_error(JODO_ERR_ARG, "debug_gemm_cdgs: bad argument");
    KC A{};
    if (mode != 0) {
        if (!desc_dev || (mode == 1 && (!xadd || ldadd < K))) return jodo_set_error(JODO_ERR_ARG, "debug_gemm_cdgs: mode %d needs its descriptor and rows", mode);
        if (int rc = jodo_cdgs_check_cfg(cfg)) return rc;
        Lay l;
        if (int rc = make_lay(cfg, B, N, n_nodes, &l)) return rc;
        if (rows != l.R) return jodo_set_error(JODO_ERR_ARG, "debug_gemm_cdgs: %d rows, the descriptor has %lld edge rows", rows, (long long)l.R);
        const int* dsc = static_cast<const int*>(desc_dev);
        A.mol_n = dsc + l.off_n; A.mol_noff = dsc + l.off_noff; A.mol_eoff = dsc + l.off_eoff; A.node_b = dsc + l.off_node; A.pair_b = dsc + l.off_pair;
    }
    const Ctx C{(hipStream_t)stream, &A};
    return gemm(C, mode, x, ldx, rows, K, static_cast<const float*>(w_dev), bias, n_out, act, y, ldy, residual, ldy, xadd, ldadd,
                split ? w_dev : nullptr);
}

// Forward of the property classifier (the masked EGNN of the conditional evaluation: cond_gen/model.py EGNN / E_GCL_mask) for gfx950.
// Exact fp32 on v_mfma_f32_32x32x2_f32 in the strip model of dgt_device.h; real atoms compact at noff_b + i, prefix masks, no scatter,
// no atomics.  Positions are never updated, so the radial |x_i - x_j|^2 is recomputed from the compact positions in every layer.
//
// Per layer:
//   kegnn_gemm   P = h [W_src ; W_tgt]^T + [b1 ; 0]        (edge_mlp.0 = [W_src | W_tgt | w_r] hoisted to the nodes; the radial term is rank 1)
//   kegnn_edge   agg_i = sum_{j != i} gate_ij m_ij,  m_ij = SiLU(W2 SiLU(P_src[i] + P_tgt[j] + r_ij w_r) + b2),
//                gate_ij = sigmoid(w_a . m_ij + b_a) with attention, 1 without          (the message never reaches memory)
//   kegnn_gemm   t = SiLU([h | agg (| h0)] N0^T + b)
//   kegnn_gemm   h = h + t N2^T + b
// Readout: node_dec (two row GEMMs), kegnn_molsum (per-molecule sum in atom order, one wave per molecule), graph_dec.0 (row GEMM over
// molecules), kegnn_out (graph_dec.2: one dot product per molecule).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"
#include "dgt_device.h"
#include "egnn_internal.h"

using namespace jd;
using jegnn::half_sum16;

namespace {

#define LEG(kern, grid, block, ...)                                               \
    do {                                                                          \
        auto kf_ = kern;                                                          \
        hipLaunchKernelGGL(kf_, dim3(grid), dim3(block), 0, st, __VA_ARGS__);     \
        int rc_ = jodo_check_launch(#kern);                                       \
        if (rc_ != JODO_OK) return rc_;                                           \
    } while (0)

struct Lay {                     // sizes and workspace offsets (in floats)
    int B, N, Nn, words;
    size_t h, p, agg, t, a0, xc, g, g1, total;
};

int make_lay(const jodo_egnn_cfg* c, int B, int N, const int32_t* n, Lay* o) {
    if (B <= 0 || N <= 0 || !n) return jodo_set_error(JODO_ERR_ARG, "egnn: bad batch");
    if (N > 255) return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: padded width %d above 255", N);
    if (B >= (1 << 22)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: batch %d too large", B);
    int64_t Nn = 0;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 1 || n[b] > N) return jodo_set_error(JODO_ERR_ARG, "egnn: n_nodes[%d]=%d outside [1,%d]", b, n[b], N);
        Nn += n[b];
    }
    if (Nn >= ((int64_t)1 << 31) / (2 * c->hidden_nf)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: batch too large (%lld atoms)", (long long)Nn);
    o->B = B; o->N = N; o->Nn = (int)Nn; o->words = 2 * B + (int)Nn;
    const size_t nf = (size_t)c->hidden_nf, Np = (size_t)(Nn + 63) / 64 * 64, Bp = (size_t)(B + 63) / 64 * 64;
    size_t at = 0;
    auto take = [&](size_t cnt) { size_t a = at; at += (cnt + 63) / 64 * 64; return a; };
    o->h = take(Np * nf); o->p = take(Np * 2 * nf); o->agg = take(Np * nf); o->t = take(Np * nf); o->a0 = take(Np * 64); o->xc = take(Np * 4);
    o->g = take(Bp * nf); o->g1 = take(Bp * nf);
    o->total = at;
    return JODO_OK;
}

// ---- inputs -> compact rows: a0 [Nn, 64] = h0 zero-padded to a K chunk, xc [Nn, 4] = positions ---------------------------------------
__global__ void kegnn_gather(const int* node_b, int Nn, int N, int in_nf, const float* h0, const float* x, float* a0, float* xc) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int t = (int)(idx >> 6), k = (int)(idx & 63);
    if (t >= Nn) return;
    const int nb = node_b[t], b = nb >> 8, i = nb & 255;
    const size_t src = (size_t)b * N + i;
    a0[(size_t)t * 64 + k] = k < in_nf ? h0[src * in_nf + k] : 0.f;
    if (k < 4) xc[(size_t)t * 4 + k] = k < 3 ? x[src * 3 + k] : 0.f;
}

// ---- row GEMM: Y[rows, 32 NB] = epi([X0 | X1 | X2][rows, 64 (nk0 + nk1 + nk2)] W^T + bias) ---------------------------------------------
// The row GEMM of the 2-D model (k2d_gemm) with the K range gathered from up to three row arrays (the node MLP reads [h | agg | h0]
// without a concatenated copy); epilogue: bias, SiLU (act 1), residual R.  W tiled [NB][nk][8 quads][64 lanes][4].
struct EGemm {
    const float *X0, *X1, *X2; int ld0, ld1, ld2, nk0, nk1, nk2;
    float* Y; int ldy; const float* W; const float* bias; int rows, NB, act; const float* R; int ldr;
};
template <int NOB, int MT>
__global__ __launch_bounds__(64) void kegnn_gemm(EGemm G) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int strip = blockIdx.x, ob0 = blockIdx.y * NOB;
    const int nk = G.nk0 + G.nk1 + G.nk2;
    f32x16 acc[NOB][MT];
    int row[MT];
    size_t rr[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        row[m] = (strip * MT + m) * 32 + j;
        rr[m] = (size_t)min(row[m], G.rows - 1);
#pragma unroll
        for (int o = 0; o < NOB; ++o) acc[o][m] = zero16();
    }
    for (int kc = 0; kc < nk; ++kc) {
        const float* xb; int ld, c;
        if (kc < G.nk0) { xb = G.X0; ld = G.ld0; c = kc; }
        else if (kc < G.nk0 + G.nk1) { xb = G.X1; ld = G.ld1; c = kc - G.nk0; }
        else { xb = G.X2; ld = G.ld2; c = kc - G.nk0 - G.nk1; }
        float act[MT][32];
#pragma unroll
        for (int m = 0; m < MT; ++m) load_nat<2>(xb + rr[m] * ld + c * 64, h, act[m]);
#pragma unroll
        for (int o = 0; o < NOB; ++o) {
            if (ob0 + o >= G.NB) continue;
            const float4* w = reinterpret_cast<const float4*>(G.W) + ((size_t)(ob0 + o) * nk + kc) * 512 + lane;
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
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (row[m] >= G.rows) continue;
#pragma unroll
        for (int o = 0; o < NOB; ++o) {
            if (ob0 + o >= G.NB) continue;
            const int col0 = (ob0 + o) * 32 + 16 * h;
            float v[16], bb[16];
            load16(G.bias + col0, bb);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                v[s] = acc[o][m][s] + bb[s];
                if (G.act == 1) v[s] = silu_f(v[s]);
            }
            if (G.R) {
                float r0[16];
                load16(G.R + (size_t)row[m] * G.ldr + col0, r0);
#pragma unroll
                for (int s = 0; s < 16; ++s) v[s] += r0[s];
            }
            store16(G.Y + (size_t)row[m] * G.ldy + col0, v);
        }
    }
}

// ---- fused edge kernel ----------------------------------------------------------------------------------------------------------------
using jegnn::EEdge;                  // egnn_internal.h

// One wave per row atom i; sources j in chunks of 32, lane pair (j, h): source r0 + j, half h of its features (natural-half slots).
// The first edge layer is formed in registers (the B operand of the second), the second runs on the MFMA with W2 as A operand from LDS
// (LDSW: the whole matrix is staged once per persistent workgroup) or streamed from L2 (widths whose W2 does not fit), then bias, SiLU,
// the attention gate (a dot product over the lane's 16 NB features, the two halves joined by one exchange), the mask j < n, j != i, and
// the sum over the 32 sources: lane (j, h) ends with feature 32 ob + 16 h + j % 16 of block ob.  Chunks ascending: a fixed order.
// Registers: act and m are 16 NB floats each, agg is NB floats per lane; at the streamed widths (nf 192, 256) act + m would pass the
// 256 vector registers, so m waits in LDS there (the LDS that W2 does not use), each lane reading back only what it wrote.
template <int NB, bool LDSW>
__global__ __launch_bounds__(256, 1) void kegnn_edge(EEdge A) {
    constexpr int nf = NB * 32, NK = NB / 2;
    constexpr bool MLDS = !LDSW;                             // the streamed widths park m in LDS (lane-private columns, no exchange)
    __shared__ float4 wl[LDSW ? NB * NK * 512 : 1];
    __shared__ float ml[MLDS ? 4 * NB * 16 * 64 : 1];
    if (LDSW) {
        const float4* src = reinterpret_cast<const float4*>(A.W2);
        for (int i = threadIdx.x; i < NB * NK * 512; i += 256) wl[i] = src[i];
        __syncthreads();
    }
    const float4* wsrc = LDSW ? wl : reinterpret_cast<const float4*>(A.W2);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    for (int t = blockIdx.x * 4 + wave; t < A.Nn; t += gridDim.x * 4) {
        const int nb = A.node_b[t], b = nb >> 8, c = nb & 255;
        const int n = A.mol_n[b], noff = A.mol_noff[b];
        float* out_row = A.agg + (size_t)t * nf;
        if (n == 1) {                                        // no sources
            for (int k = lane; k < nf; k += 64) out_row[k] = 0.f;
            continue;
        }
        const float4 xi = reinterpret_cast<const float4*>(A.xc)[t];
        const float* psrc = A.P + (size_t)t * 2 * nf + h * 16;
        float agg[NB];
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) agg[ob] = 0.f;
        for (int r0 = 0; r0 < n; r0 += 32) {
            const int r = r0 + j;
            const bool valid = r < n && r != c;
            const int rs = valid ? r : c;                    // a live row for masked lanes (their weight is zero)
            const float4 xj = reinterpret_cast<const float4*>(A.xc)[noff + rs];
            const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            const float rad = dx * dx + dy * dy + dz * dz;
            const float* ptgt = A.P + (size_t)(noff + rs) * 2 * nf + nf + h * 16;
            const float* ps = launder(psrc);                 // (re-read per chunk instead of 16 NB hoisted registers)
            const float* wr = launder(A.wr) + h * 16;
            const float4* wt = LDSW ? wsrc : launder(wsrc);   // (loop-invariant streams: re-read per chunk, never hoisted into registers)
            const float* b2 = launder(A.b2) + h * 16;
            const float* wa = A.wa ? launder(A.wa) + h * 16 : nullptr;
            float act[NB * 16];
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) {
                float a[16], bq[16], w[16];
                load16(ps + kb * 32, a);
                load16(ptgt + kb * 32, bq);
                load16(wr + kb * 32, w);
#pragma unroll
                for (int s = 0; s < 16; ++s) act[kb * 16 + s] = silu_f(fmaf(rad, w[s], a[s] + bq[s]));
                pipeline_fence();                            // keeps the next block's loads from being hoisted above this one (registers)
            }
            float m[MLDS ? 1 : NB * 16];
            float* mw = ml + (size_t)(MLDS ? wave * NB * 16 * 64 + lane : 0);
            float dot = 0.f;
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) {
                f32x16 acc = zero16();
#pragma unroll
                for (int kc = 0; kc < NK; ++kc) {
                    const float4* tile = wt + (ob * NK + kc) * 512 + lane;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const float4 a = tile[q * 64];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, act[kc * 32 + 4 * q + 0], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, act[kc * 32 + 4 * q + 1], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, act[kc * 32 + 4 * q + 2], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, act[kc * 32 + 4 * q + 3], acc, 0, 0, 0);
                    }
                    if constexpr (!LDSW) pipeline_fence();   // one tile (32 registers) of the L2 stream in flight, not the whole block's
                }
                float bb[16];
                load16(b2 + ob * 32, bb);
                float mo[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    mo[s] = silu_f(acc[s] + bb[s]);
                    if constexpr (MLDS) mw[(ob * 16 + s) * 64] = mo[s]; else m[ob * 16 + s] = mo[s];
                }
                if (wa) {
                    float wv[16];
                    load16(wa + ob * 32, wv);
#pragma unroll
                    for (int s = 0; s < 16; ++s) dot = fmaf(wv[s], mo[s], dot);
                }
                pipeline_fence();
            }
            float scale = valid ? 1.f : 0.f;
            if (A.wa) {
                const float gte = pair_sum(dot) + A.ba[0];
                scale = valid ? fast_rcp(1.f + fast_exp(-gte)) : 0.f;
            }
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) {
                float tt[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) tt[s] = (MLDS ? mw[(ob * 16 + s) * 64] : m[ob * 16 + s]) * scale;
                agg[ob] += half_sum16(tt, j);
                pipeline_fence();
            }
        }
        if (j < 16) {
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) out_row[ob * 32 + h * 16 + j] = agg[ob];
        }
    }
}

// ---- readout ---------------------------------------------------------------------------------------------------------------------------
// g[b] = sum over the molecule's atoms, in atom order, of hd rows: one wave per molecule
__global__ __launch_bounds__(64) void kegnn_molsum(const int* mol_n, const int* mol_noff, int B, int nf, const float* hd, float* g) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const int n = mol_n[b], noff = mol_noff[b];
    for (int k = lane; k < nf; k += 64) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += hd[(size_t)(noff + i) * nf + k];
        g[(size_t)b * nf + k] = s;
    }
}
// out[b] = w . g1[b] + bias: one wave per molecule, a fixed exchange tree
__global__ __launch_bounds__(64) void kegnn_out(int B, int nf, const float* g1, const float* w, const float* bias, float* out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int k = lane; k < nf; k += 64) s = fmaf(w[k], g1[(size_t)b * nf + k], s);
#pragma unroll
    for (int msk = 1; msk < 64; msk <<= 1) s += __shfl_xor(s, msk);
    if (lane == 0) out[b] = s + bias[0];
}

int gemm(hipStream_t st, EGemm G) {
    LEG((kegnn_gemm<4, 2>), dim3((G.rows + 63) / 64, (G.NB + 3) / 4), 64, G);
    return JODO_OK;
}

template <int NB, bool LDSW>
int edge_launch(hipStream_t st, const EEdge& A, int grid_cap) {
    const int grid = (A.Nn + 3) / 4 < grid_cap ? (A.Nn + 3) / 4 : grid_cap;      // persistent: a workgroup stages W2 once and walks its atoms
    LEG((kegnn_edge<NB, LDSW>), grid, 256, A);
    return JODO_OK;
}

}  // namespace

extern "C" int jodo_egnn_layout(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes, int64_t* out8) {
    if (!out8) return jodo_set_error(JODO_ERR_ARG, "egnn_layout: null argument");
    if (int rc = jodo_egnn_check_cfg(cfg)) return rc;
    Lay l;
    if (int rc = make_lay(cfg, B, N, n_nodes, &l)) return rc;
    out8[0] = l.words; out8[1] = (int64_t)(l.total * sizeof(float)); out8[2] = l.Nn; out8[3] = (int64_t)(l.h * sizeof(float));
    out8[4] = out8[5] = out8[6] = out8[7] = 0;
    return JODO_OK;
}

extern "C" int jodo_egnn_fill_desc(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes, int32_t* desc, int64_t n_words) {
    if (!desc) return jodo_set_error(JODO_ERR_ARG, "egnn_fill_desc: null argument");
    if (int rc = jodo_egnn_check_cfg(cfg)) return rc;
    Lay l;
    if (int rc = make_lay(cfg, B, N, n_nodes, &l)) return rc;
    if (n_words < l.words) return jodo_set_error(JODO_ERR_ARG, "egnn_fill_desc: %lld words, need %d", (long long)n_words, l.words);
    int noff = 0, node = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_nodes[b];
        desc[b] = n; desc[B + b] = noff;
        for (int i = 0; i < n; ++i) desc[2 * B + node++] = (b << 8) | i;
        noff += n;
    }
    return JODO_OK;
}

int jegnn::edge_forward(hipStream_t st, int NB, const EEdge& A, int grid_cap) {
    switch (NB) {
        case 2: return edge_launch<2, true>(st, A, grid_cap);
        case 4: return edge_launch<4, true>(st, A, grid_cap);
        case 6: return edge_launch<6, false>(st, A, grid_cap);
        default: return edge_launch<8, false>(st, A, grid_cap);
    }
}

int jegnn::row_gemm(hipStream_t st, const float* X0, int ld0, int nk0, const float* X1, int ld1, int nk1, const float* X2, int ld2, int nk2, float* Y,
                    int ldy, const float* W, const float* bias, int rows, int nb, int act, const float* R) {
    EGemm G{X0, X1, X2, ld0, ld1, ld2, nk0, nk1, nk2, Y, ldy, W, bias, rows, nb, act, R, ldy};
    return gemm(st, G);
}

int jegnn::run(const jodo_egnn_cfg* cfg, int B, int N, int Nn, const void* desc_dev, const float* packed_w, const int64_t* woff, const float* h0,
               const float* x, float* out, const Bufs& bf, int max_layers, hipStream_t st) {
    const int nf = cfg->hidden_nf, NB = nf / 32, NK = nf / 64;
    const int* desc = (const int*)desc_dev;
    const int *mol_n = desc, *mol_noff = desc + B, *node_b = desc + 2 * B;
    float *a0 = bf.a0, *xc = bf.xc;
    auto W = [&](int64_t off) { return packed_w + off; };

    LEG(kegnn_gather, (unsigned)(((size_t)Nn * 64 + 255) / 256), 256, node_b, Nn, N, cfg->in_node_nf, h0, x, a0, xc);
    auto row_gemm = [&](const float* X0, int ld0, int nk0, const float* X1, int ld1, int nk1, const float* X2, int ld2, int nk2, float* Y,
                        int ldy, int64_t w, int64_t bias, int rows, int nb, int act, const float* R) {
        EGemm G{X0, X1, X2, ld0, ld1, ld2, nk0, nk1, nk2, Y, ldy, W(w), W(bias), rows, nb, act, R, ldy};
        return gemm(st, G);
    };
    if (int rc = row_gemm(a0, 64, 1, nullptr, 0, 0, nullptr, 0, 0, bf.h[0], nf, woff[JE_EMB_W], woff[JE_EMB_B], Nn, NB, 0, nullptr)) return rc;
    const int layers = max_layers < 0 || max_layers > cfg->n_layers ? cfg->n_layers : max_layers;
    for (int ly = 0; ly < layers; ++ly) {
        const int64_t* wl = woff + JE_GLOBAL_COUNT + (size_t)ly * JEL_LAYER_COUNT;
        const float* h = bf.h[ly];
        float *p = bf.p[ly], *agg = bf.agg[ly], *t = bf.t[ly];
        if (int rc = row_gemm(h, nf, NK, nullptr, 0, 0, nullptr, 0, 0, p, 2 * nf, wl[JEL_P_W], wl[JEL_P_B], Nn, 2 * NB, 0, nullptr)) return rc;
        EEdge E{mol_n, mol_noff, node_b, Nn, p, xc, W(wl[JEL_WR]), W(wl[JEL_W2]), W(wl[JEL_B2]),
                cfg->attention ? W(wl[JEL_ATT_W]) : nullptr, cfg->attention ? W(wl[JEL_ATT_B]) : nullptr, agg};
        if (int rc = edge_forward(st, NB, E)) return rc;
        if (int rc2 = row_gemm(h, nf, NK, agg, nf, NK, a0, 64, cfg->node_attr ? 1 : 0, t, nf, wl[JEL_N0_W], wl[JEL_N0_B], Nn, NB, 1, nullptr)) return rc2;
        if (int rc2 = row_gemm(t, nf, NK, nullptr, 0, 0, nullptr, 0, 0, bf.h[ly + 1], nf, wl[JEL_N2_W], wl[JEL_N2_B], Nn, NB, 0, h)) return rc2;
    }
    if (max_layers >= 0) return JODO_OK;
    const float* h = bf.h[layers];
    if (int rc = row_gemm(h, nf, NK, nullptr, 0, 0, nullptr, 0, 0, bf.tnd, nf, woff[JE_ND0_W], woff[JE_ND0_B], Nn, NB, 1, nullptr)) return rc;
    if (int rc = row_gemm(bf.tnd, nf, NK, nullptr, 0, 0, nullptr, 0, 0, bf.hd, nf, woff[JE_ND2_W], woff[JE_ND2_B], Nn, NB, 0, nullptr)) return rc;
    LEG(kegnn_molsum, B, 64, mol_n, mol_noff, B, nf, bf.hd, bf.g);
    if (int rc = row_gemm(bf.g, nf, NK, nullptr, 0, 0, nullptr, 0, 0, bf.g1, nf, woff[JE_GD0_W], woff[JE_GD0_B], B, NB, 1, nullptr)) return rc;
    LEG(kegnn_out, B, 64, B, nf, bf.g1, W(woff[JE_GD2_W]), W(woff[JE_GD2_B]), out);
    return JODO_OK;
}

extern "C" int jodo_egnn_forward(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes, const void* desc_dev, const float* packed_w,
                                 const int64_t* woff, int n_woff, const float* h0, const float* x, float* out, void* workspace,
                                 int max_layers, void* stream) {
    if (!desc_dev || !packed_w || !woff || !h0 || !x || !workspace || (max_layers < 0 && !out))
        return jodo_set_error(JODO_ERR_ARG, "egnn_forward: null argument");
    if (int rc = jodo_egnn_check_cfg(cfg)) return rc;
    if (n_woff != JE_GLOBAL_COUNT + cfg->n_layers * JEL_LAYER_COUNT)
        return jodo_set_error(JODO_ERR_ARG, "egnn_forward: offset table of %d slots, expected %d", n_woff, JE_GLOBAL_COUNT + cfg->n_layers * JEL_LAYER_COUNT);
    Lay l;
    if (int rc = make_lay(cfg, B, N, n_nodes, &l)) return rc;
    float* ws = (float*)workspace;
    jegnn::Bufs bf;                                          // inference: one array of each kind, every layer overwrites the last one's
    bf.a0 = ws + l.a0; bf.xc = ws + l.xc;
    for (int ly = 0; ly <= cfg->n_layers; ++ly) bf.h[ly] = ws + l.h;
    for (int ly = 0; ly < cfg->n_layers; ++ly) { bf.p[ly] = ws + l.p; bf.agg[ly] = ws + l.agg; bf.t[ly] = ws + l.t; }
    bf.tnd = ws + l.t; bf.hd = ws + l.agg; bf.g = ws + l.g; bf.g1 = ws + l.g1;
    return jegnn::run(cfg, B, N, l.Nn, desc_dev, packed_w, woff, h0, x, out, bf, max_layers, (hipStream_t)stream);
}

// Training of the property classifier (the masked EGNN of cond_gen/model.py) behind the C ABI jodo_egnn_train_*: the forward keeps
// per-atom and per-molecule tensors only (O(L Nn nf)), the backward returns d <d_out, out> / d parameter for every tensor of the
// state_dict.  Gradients with respect to h0 and x are not computed.
//
// Forward: the inference forward (egnn_forward.hip: the same kernels in the same order through jegnn::run) with one destination per
// layer.  The tiled weight image those kernels read is rebuilt on the device from the live parameter pointers on every call
// (kegnn_pack over the slots of jodo_egnn_wslot_*, plus a transposed tile image of every edge_mlp.2 for the backward), so the result
// is bit-identical to jodo_egnn_forward on the same weights and follows `.data` writes and flat-buffer optimisers.
//
// Backward of layer l (d h_{l+1} given):
//   node_mlp.2 / node_mlp.0      jt::gemm on the PyTorch-layout parameters (weight gradients with the bias-gradient epilogue); the
//                                pre-activation of node_mlp.0 is recomputed by kegnn_gemm (act 0) from h_l, agg_l, h0
//   kegnn_edge_bwd               one wave per row atom i, sources j in chunks of 32 (the walk of kegnn_edge): recomputes z1, a = SiLU(z1),
//                                z2 = W2 a + b2 on the fp32 MFMA, m = SiLU(z2) and the gate g with the forward's instruction forms, then
//                                dm = g dagg_i + (dagg_i . m) g (1 - g) w_a, dz2 = dm SiLU'(z2), da = W2^T dz2 (MFMA, transposed tile
//                                image), dz1 = da SiLU'(z1).  Inside the wave: dP_src[i] = sum_j dz1, and the row atom's partial sums
//                                of dw_r (sum_j r_ij dz1), dw_a (sum_j c_ij m), db_a (sum_j c_ij).  To memory per edge: a, dz2, dz1
//                                (3 nf floats, compact edge rows e = eoff_b + i (n - 1) + (j < i ? j : j - 1))
//   kegnn_tgt_sum                dP_tgt[j] = sum_{i != j} dz1[(i, j)] in ascending i
//   jt::gemm (tA)                dW2 = dz2^T a over the edge rows, db2 its column sums (split-K in fixed slices)
//   kegnn_colsum_part / _fin     dw_r, dw_a, db_a: column sums of the per-atom partial rows in 64-row chunks, then over chunks
//   jt::gemm                     dW_src / dW_tgt / db1 from dP and h_l; d h_l = d h_{l+1} + dt N0_h + dP_src W_src + dP_tgt W_tgt
// No floating-point atomics, no scatter: every sum has a fixed order, two runs give the same bits.
// Tests: jodo_egnn_debug_edge (at the end) runs kegnn_edge or kegnn_edge_bwd + kegnn_tgt_sum alone on caller-owned arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"
#include "dgt_device.h"
#include "egnn_internal.h"
#include "train_gemm.h"

using namespace jd;
using jegnn::half_sum16;

namespace {

#define LEGT(kern, grid, block, ...)                                              \
    do {                                                                          \
        auto kf_ = kern;                                                          \
        hipLaunchKernelGGL(kf_, dim3(grid), dim3(block), 0, st, __VA_ARGS__);     \
    } while (0)

struct Lin { int w = -1, b = -1; };
struct LayIx { Lin e0, e2, n0, n2, att; };

struct Arena {
    char* base; size_t off;
    float* f(size_t n) { const size_t o = off; off += (n * 4 + 255) / 256 * 256; return base ? reinterpret_cast<float*>(base + o) : nullptr; }
};

struct TBufs {
    float* tape; float* w2t;
    jegnn::Bufs fw;
    // backward scratch
    float *zs, *dh, *dt, *dagg, *dP, *Q, *qb, *part, *zg, *dzg, *dg, *ea, *ez1, *ez2, *splitk;
    size_t splitk_floats;
};

__device__ __forceinline__ float sigm_f(float x) { return fast_rcp(1.f + fast_exp(-x)); }       // the factor inside silu_f
__device__ __forceinline__ float silu_grad_f(float x) { const float s = sigm_f(x); return s * (1.f + x * (1.f - s)); }

// ---- weight image from the live parameters -------------------------------------------------------------------------------------------
// kind 0: tiled [nb][nk][8 quads][64 lanes][4] of the rows of s0 (rows0) stacked on s1 (rows1), element (r, col) = s[r ld + c + col],
//         zero beyond the rows and beyond K (the layout of egnn_pack.cpp `tiled`);  kind 1: the same of the TRANSPOSE of s0 [K, rows0];
// kind 2: vector of n floats, dst[i] = s0[i ld] for i < rows0, zero behind
struct PackJob { const float *s0, *s1; float* dst; int rows0, rows1, ld, c0, c1, K, nb, nk, kind, n; };
#define PACK_MAX 12
struct PackTable { int n; PackJob j[PACK_MAX]; };

__global__ void kegnn_pack(PackTable T) {
    const PackJob& J = T.j[blockIdx.y];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (J.kind == 2) {
        if (idx < J.n) J.dst[idx] = idx < J.rows0 ? J.s0[(size_t)idx * J.ld] : 0.f;
        return;
    }
    if (idx >= J.nb * J.nk * 2048) return;
    const int i = idx & 3, l = (idx >> 2) & 63, q = (idx >> 8) & 7, rest = idx >> 11, kc = rest % J.nk, b = rest / J.nk;
    const int a = 4 * q + i, m = l % 32;
    const int col = kc * 64 + (a / 16) * 32 + (l / 32) * 16 + a % 16;
    int r = b * 32 + 16 * ((m / 4) % 2) + 4 * (m / 8) + m % 4;
    float v = 0.f;
    if (col < J.K) {
        if (J.kind == 1) { if (r < J.rows0) v = J.s0[(size_t)col * J.ld + r]; }
        else if (r < J.rows0) v = J.s0[(size_t)r * J.ld + J.c0 + col];
        else if (r - J.rows0 < J.rows1) v = J.s1[(size_t)(r - J.rows0) * J.ld + J.c1 + col];
    }
    J.dst[idx] = v;
}

// ---- fused edge backward ----------------------------------------------------------------------------------------------------------------
using jegnn::EBwd;                   // egnn_internal.h

// One wave per row atom i, sources in chunks of 32, lane pair (j, h) as in kegnn_edge.  LDSW: W2 and its transposed image are staged
// in LDS once per persistent workgroup (nf 64: 32 KiB, nf 128: 128 KiB); otherwise both stream from L2 and z2 / dz2 wait in LDS
// (lane-private columns) like the forward's m at those widths.  Masked lanes (j >= n, j == i) compute on the row atom's own row with
// gate 0 and c 0, so every one of their gradients is exactly zero; they store nothing.
template <int NB, bool LDSW>
__global__ __launch_bounds__(256, 1) void kegnn_edge_bwd(EBwd A) {
    constexpr int nf = NB * 32, NK = NB / 2, TILE = NB * NK * 512;
    constexpr bool ZL = !LDSW;
    __shared__ float4 wl[LDSW ? 2 * TILE : 1];
    __shared__ float zl[ZL ? 4 * NB * 16 * 64 : 1];
    if (LDSW) {
        const float4* s0 = reinterpret_cast<const float4*>(A.W2);
        const float4* s1 = reinterpret_cast<const float4*>(A.W2T);
        for (int i = threadIdx.x; i < TILE; i += 256) { wl[i] = s0[i]; wl[TILE + i] = s1[i]; }
        __syncthreads();
    }
    const float4* wsrc = LDSW ? wl : reinterpret_cast<const float4*>(A.W2);
    const float4* wsrcT = LDSW ? wl + TILE : reinterpret_cast<const float4*>(A.W2T);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    for (int t = blockIdx.x * 4 + wave; t < A.Nn; t += gridDim.x * 4) {
        const int nb = A.node_b[t], b = nb >> 8, c = nb & 255;
        const int n = A.mol_n[b], noff = A.mol_noff[b];
        float* dps_row = A.dP + (size_t)t * 2 * nf;
        float* q_row = A.Q + (size_t)t * 2 * nf;
        if (n == 1) {                                        // no sources
            for (int k = lane; k < nf; k += 64) dps_row[k] = 0.f;
            for (int k = lane; k < 2 * nf; k += 64) q_row[k] = 0.f;
            if (lane == 0) A.qb[t] = 0.f;
            continue;
        }
        const size_t erow0 = (size_t)A.eoff[b] + (size_t)c * (n - 1);
        const float4 xi = reinterpret_cast<const float4*>(A.xc)[t];
        const float* psrc = A.P + (size_t)t * 2 * nf + h * 16;
        const float* dag = A.dagg + (size_t)t * nf + h * 16;
        float dps[NB], dwr[NB], dwa[NB], dba = 0.f;
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) dps[ob] = dwr[ob] = dwa[ob] = 0.f;
        for (int r0 = 0; r0 < n; r0 += 32) {
            const int r = r0 + j;
            const bool valid = r < n && r != c;
            const int rs = valid ? r : c;                    // a live row for masked lanes (their gradients are zero)
            const size_t eo = (erow0 + (size_t)(rs < c ? rs : rs - 1)) * nf + h * 16;      // (used by valid lanes only)
            const float4 xj = reinterpret_cast<const float4*>(A.xc)[noff + rs];
            const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            const float rad = dx * dx + dy * dy + dz * dz;
            const float* ptgt = A.P + (size_t)(noff + rs) * 2 * nf + nf + h * 16;
            const float* ps = launder(psrc);
            const float* wr = launder(A.wr) + h * 16;
            const float4* wt = LDSW ? wsrc : launder(wsrc);
            const float4* wtT = LDSW ? wsrcT : launder(wsrcT);
            const float* b2 = launder(A.b2) + h * 16;
            const float* wa = A.wa ? launder(A.wa) + h * 16 : nullptr;
            const float* dg = launder(dag);
            float act[NB * 16];
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) {
                float a[16], bq[16], w[16], av[16];
                load16(ps + kb * 32, a);
                load16(ptgt + kb * 32, bq);
                load16(wr + kb * 32, w);
#pragma unroll
                for (int s = 0; s < 16; ++s) av[s] = act[kb * 16 + s] = silu_f(fmaf(rad, w[s], a[s] + bq[s]));
                if (valid) store16(A.ea + eo + kb * 32, av);
                pipeline_fence();
            }
            // z2 = W2 a + b2; the gate's dot product and dagg . m
            float zr[NB * 16];
            float* zw = zl + (size_t)(ZL ? wave * NB * 16 * 64 + lane : 0);
            float dot = 0.f, dd = 0.f;
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
                    if constexpr (!LDSW) pipeline_fence();
                }
                float bb[16], dgv[16];
                load16(b2 + ob * 32, bb);
                load16(dg + ob * 32, dgv);
                float mo[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const float z = acc[s] + bb[s];
                    mo[s] = silu_f(z);
                    if constexpr (ZL) zw[(ob * 16 + s) * 64] = z; else zr[ob * 16 + s] = z;
                    dd = fmaf(dgv[s], mo[s], dd);
                }
                if (wa) {
                    float wv[16];
                    load16(wa + ob * 32, wv);
#pragma unroll
                    for (int s = 0; s < 16; ++s) dot = fmaf(wv[s], mo[s], dot);
                }
                pipeline_fence();
            }
            float g = valid ? 1.f : 0.f, cc = 0.f;
            if (A.wa) {
                const float gte = pair_sum(dot) + A.ba[0];
                const float gs = fast_rcp(1.f + fast_exp(-gte));
                g = valid ? gs : 0.f;
                cc = valid ? pair_sum(dd) * gs * (1.f - gs) : 0.f;
                dba += cc;
            }
            // dz2 = (g dagg + c w_a) SiLU'(z2), in place of z2; the row atom's dw_a partial sum_j c m
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) {
                float dgv[16], wv[16], dzv[16], tw[16];
                load16(dg + ob * 32, dgv);
                if (wa) load16(wa + ob * 32, wv);
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const float z = ZL ? zw[(ob * 16 + s) * 64] : zr[ob * 16 + s];
                    const float sg = sigm_f(z);
                    const float dm = wa ? fmaf(cc, wv[s], g * dgv[s]) : g * dgv[s];
                    dzv[s] = dm * (sg * (1.f + z * (1.f - sg)));
                    tw[s] = cc * (z * sg);
                    if constexpr (ZL) zw[(ob * 16 + s) * 64] = dzv[s]; else zr[ob * 16 + s] = dzv[s];
                }
                if (wa) dwa[ob] += half_sum16(tw, j);
                if (valid) store16(A.ez2 + eo + ob * 32, dzv);
                pipeline_fence();
            }
            if constexpr (ZL) {
#pragma unroll
                for (int i = 0; i < NB * 16; ++i) zr[i] = zw[i * 64];
            }
            // da = W2^T dz2, dz1 = da SiLU'(z1) (z1 recomputed), the wave's sums over sources
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) {
                f32x16 acc = zero16();
#pragma unroll
                for (int kc = 0; kc < NK; ++kc) {
                    const float4* tile = wtT + (kb * NK + kc) * 512 + lane;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const float4 a = tile[q * 64];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, zr[kc * 32 + 4 * q + 0], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, zr[kc * 32 + 4 * q + 1], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, zr[kc * 32 + 4 * q + 2], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, zr[kc * 32 + 4 * q + 3], acc, 0, 0, 0);
                    }
                    if constexpr (!LDSW) pipeline_fence();
                }
                float a[16], bq[16], w[16], d1[16], tw[16];
                load16(ps + kb * 32, a);
                load16(ptgt + kb * 32, bq);
                load16(wr + kb * 32, w);
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    d1[s] = acc[s] * silu_grad_f(fmaf(rad, w[s], a[s] + bq[s]));
                    tw[s] = rad * d1[s];
                }
                if (valid) store16(A.ez1 + eo + kb * 32, d1);
                dps[kb] += half_sum16(d1, j);
                dwr[kb] += half_sum16(tw, j);
                pipeline_fence();
            }
        }
        if (j < 16) {
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) {
                dps_row[ob * 32 + h * 16 + j] = dps[ob];
                q_row[ob * 32 + h * 16 + j] = dwr[ob];
                q_row[nf + ob * 32 + h * 16 + j] = dwa[ob];
            }
        }
#pragma unroll
        for (int msk = 1; msk < 32; msk <<= 1) dba += __shfl_xor(dba, msk);      // over the 32 sources' lanes of a half: a fixed tree
        if (lane == 0) A.qb[t] = dba;
    }
}

// dP[t, nf + k] = sum over row atoms i != j (ascending) of dz1[(i, j), k]: one workgroup per atom t = (b, j), one thread per feature
__global__ void kegnn_tgt_sum(const int* mol_n, const int* mol_noff, const int* node_b, const int* eoff, int nf, const float* ez1, float* dP) {
    const int t = blockIdx.x, k = threadIdx.x;
    const int nb = node_b[t], b = nb >> 8, j = nb & 255, n = mol_n[b];
    const size_t e0 = (size_t)eoff[b];
    float s = 0.f;
    for (int i = 0; i < n; ++i) {
        if (i == j) continue;
        s += ez1[(e0 + (size_t)i * (n - 1) + (j < i ? j : j - 1)) * nf + k];
    }
    dP[(size_t)t * 2 * nf + nf + k] = s;
}

// column sums in two fixed levels: part[c, k] = sum of rows 64 c .. 64 c + 63, then dst[k stride] = sum over c (ascending)
__global__ void kegnn_colsum_part(int rows, int F, const float* src, int ld, float* part) {
    const int c = blockIdx.x, k = blockIdx.y * 64 + threadIdx.x;
    if (k >= F) return;
    const int r1 = min(rows, (c + 1) * 64);
    float s = 0.f;
    for (int r = c * 64; r < r1; ++r) s += src[(size_t)r * ld + k];
    part[(size_t)c * F + k] = s;
}
__global__ void kegnn_colsum_fin(int nchunk, int F, const float* part, int pld, float* dst, int dstride) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= F) return;
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) s += part[(size_t)c * pld + k];
    dst[(size_t)k * dstride] = s;
}

__global__ void kegnn_out_bwd(int B, int nf, const float* d_out, const float* w, const float* zg, float* dzg) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * nf) return;
    dzg[i] = d_out[i / nf] * w[i % nf] * silu_grad_f(zg[i]);
}
__global__ void kegnn_silu_bwd(size_t n, const float* z, float* d) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] *= silu_grad_f(z[i]);
}
__global__ void kegnn_bcast_mol(int Nn, int nf, const int* node_b, const float* dg, float* dhd) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Nn * nf) return;
    dhd[i] = dg[(size_t)(node_b[i / nf] >> 8) * nf + i % nf];
}

template <int NB, bool LDSW>
void edge_bwd_launch(hipStream_t st, const EBwd& A, int grid_cap) {
    const int grid = (A.Nn + 3) / 4 < grid_cap ? (A.Nn + 3) / 4 : grid_cap;     // the forward's persistent grid
    LEGT((kegnn_edge_bwd<NB, LDSW>), grid, 256, A);
}

// the three pieces of the weight image that a call of the edge kernels needs, as pack_tape makes them
PackJob tiled_job(float* dst, const float* s0, int rows0, int ld, int c0, int K, const float* s1 = nullptr, int rows1 = 0, int c1 = 0) {
    PackJob J{s0, s1, dst, rows0, rows1, ld, c0, c1, K, (rows0 + rows1 + 31) / 32, (K + 63) / 64, 0, 0};
    return J;
}
PackJob transposed_job(float* dst, const float* w, int nf) {     // the transposed image of edge_mlp.2 for da = W2^T dz2
    PackJob J{w, nullptr, dst, nf, 0, nf, 0, 0, nf, nf / 32, nf / 64, 1, 0};
    return J;
}
void launch_pack(hipStream_t st, const PackTable& T) {
    int most = 0;
    for (int i = 0; i < T.n; ++i) { const int cnt = T.j[i].kind == 2 ? T.j[i].n : T.j[i].nb * T.j[i].nk * 2048; most = cnt > most ? cnt : most; }
    LEGT(kegnn_pack, dim3((most + 255) / 256, T.n), 256, T);
}

// n_b [B] | noff_b [B] | (b << 8 | i) [Nn] | eoff_b [B]: the descriptor of the training path (3 B + Nn ints)
void fill_tables(int B, const int32_t* n_nodes, long Nn, int* tables) {
    int noff = 0, node = 0;
    long eo = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_nodes[b];
        tables[b] = n; tables[B + b] = noff; tables[(size_t)2 * B + Nn + b] = (int)eo;
        for (int i = 0; i < n; ++i) tables[2 * B + node++] = (b << 8) | i;
        noff += n; eo += (long)n * (n - 1);
    }
}

}  // namespace

int jegnn::edge_backward(hipStream_t st, int NB, const EBwd& A, int grid_cap) {
    switch (NB) {
        case 2: edge_bwd_launch<2, true>(st, A, grid_cap); break;
        case 4: edge_bwd_launch<4, true>(st, A, grid_cap); break;
        case 6: edge_bwd_launch<6, false>(st, A, grid_cap); break;
        default: edge_bwd_launch<8, false>(st, A, grid_cap); break;
    }
    LEGT(kegnn_tgt_sum, A.Nn, NB * 32, A.mol_n, A.mol_noff, A.node_b, A.eoff, NB * 32, (const float*)A.ez1, A.dP);
    return JODO_OK;
}

struct jodo_egnn_train {
    jodo_egnn_cfg cfg;
    int B, N, Nn;
    long E;
    std::vector<int> tables;              // n_b [B] | noff_b [B] | (b << 8 | i) [Nn] | eoff_b [B]
    int n_params;
    std::vector<size_t> numel;
    Lin emb, nd0, nd2, gd0, gd2;
    std::vector<LayIx> lay;
    std::vector<int64_t> woff;
    size_t tape_floats;
    size_t ws_bytes;
};

namespace {

void layout(const jodo_egnn_train& t, Arena& a, TBufs& b) {
    const size_t nf = t.cfg.hidden_nf, L = t.cfg.n_layers, Np = ((size_t)t.Nn + 63) / 64 * 64, Bp = ((size_t)t.B + 63) / 64 * 64;
    const size_t E = (size_t)t.E;
    b.tape = a.f(t.tape_floats);
    b.w2t = a.f(L * nf * nf);
    b.fw.a0 = a.f(Np * 64); b.fw.xc = a.f(Np * 4);
    for (size_t l = 0; l <= L; ++l) b.fw.h[l] = a.f(Np * nf);
    for (size_t l = 0; l < L; ++l) { b.fw.p[l] = a.f(Np * 2 * nf); b.fw.agg[l] = a.f(Np * nf); b.fw.t[l] = a.f(Np * nf); }
    b.fw.tnd = a.f(Np * nf); b.fw.hd = a.f(Np * nf); b.fw.g = a.f(Bp * nf); b.fw.g1 = a.f(Bp * nf);
    b.zs = a.f(Np * nf); b.dh = a.f(Np * nf); b.dt = a.f(Np * nf); b.dagg = a.f(Np * nf); b.dP = a.f(Np * 2 * nf); b.Q = a.f(Np * 2 * nf);
    b.qb = a.f(Np);
    b.part = a.f((Np / 64 + 1) * 2 * nf);
    b.zg = a.f(Bp * nf); b.dzg = a.f(Bp * nf); b.dg = a.f(Bp * nf);
    b.ea = a.f(E * nf + 64); b.ez1 = a.f(E * nf + 64); b.ez2 = a.f(E * nf + 64);        // the per-edge scratch of ONE layer: 3 E nf floats
    const size_t rows = E > (size_t)t.Nn ? E : (size_t)t.Nn;
    size_t slices = rows / 64 + 2;
    if (slices > 512) slices = 512;
    b.splitk_floats = slices * (nf * nf + nf);
    b.splitk = a.f(b.splitk_floats);
}

struct Ctx {
    const jodo_egnn_train& t; const float* const* P; float* const* G; TBufs& b; hipStream_t s;
    const float* p(int i) const { return P[i]; }
    float* g(int i) const { return G[i]; }
    // dX[rows, K] (ldx) (+)= dY[rows, N] (ldy) W[N, K] (ldw)
    void lin_dx(const float* dY, int ldy, int rows, int N, const float* W, int ldw, int K, float* dX, int ldx, int acc) const {
        jt::gemm(s, 0, 0, rows, K, N, dY, ldy, W, ldw, dX, ldx, nullptr, acc, b.splitk, b.splitk_floats);
    }
    // dW[N, K] (lddw) += dY[rows, N]^T X[rows, K]; db[N] += column sums of dY
    void lin_dw(const float* dY, int ldy, long rows, int N, const float* X, int ldx, int K, float* dW, int lddw, float* db = nullptr) const {
        jt::GemmEpi e; e.act = 0; e.out2 = nullptr; e.drop.p = 0.f; e.drop.seed = 0; e.drop.site = 0; e.dbias = db;
        jt::gemm(s, 1, 0, N, K, (int)rows, dY, ldy, X, ldx, dW, lddw, nullptr, 1, b.splitk, b.splitk_floats, &e);
    }
    void colsum(int rows, int F, const float* src, int ld) const {
        hipStream_t st = s;
        LEGT(kegnn_colsum_part, dim3((rows + 63) / 64, (F + 63) / 64), 64, rows, F, src, ld, b.part);
    }
    void colsum_fin(int rows, int F, const float* part, int pld, float* dst, int dstride) const {
        hipStream_t st = s;
        LEGT(kegnn_colsum_fin, (F + 63) / 64, 64, (rows + 63) / 64, F, part, pld, dst, dstride);
    }
};

void pack_tape(const Ctx& c) {
    const jodo_egnn_train& t = c.t; hipStream_t st = c.s;
    const int nf = t.cfg.hidden_nf, in = t.cfg.in_node_nf, L = t.cfg.n_layers;
    float* tape = c.b.tape;
    const int64_t* wo = t.woff.data();
    auto tiled = [&](int64_t off, const float* s0, int rows0, int ld, int c0, int K, const float* s1 = nullptr, int rows1 = 0, int c1 = 0) {
        return tiled_job(tape + off, s0, rows0, ld, c0, K, s1, rows1, c1);
    };
    auto vec = [&](int64_t off, const float* s0, int len, int stride, int n) {
        PackJob J{s0, nullptr, tape + off, len, 0, stride, 0, 0, 0, 0, 0, 2, n};
        return J;
    };
    auto launch = [&](const PackTable& T) { launch_pack(st, T); };
    PackTable T;
    T.n = 0;
    T.j[T.n++] = tiled(wo[JE_EMB_W], c.p(t.emb.w), nf, in, 0, in);
    T.j[T.n++] = vec(wo[JE_EMB_B], c.p(t.emb.b), nf, 1, nf);
    T.j[T.n++] = tiled(wo[JE_ND0_W], c.p(t.nd0.w), nf, nf, 0, nf);
    T.j[T.n++] = vec(wo[JE_ND0_B], c.p(t.nd0.b), nf, 1, nf);
    T.j[T.n++] = tiled(wo[JE_ND2_W], c.p(t.nd2.w), nf, nf, 0, nf);
    T.j[T.n++] = vec(wo[JE_ND2_B], c.p(t.nd2.b), nf, 1, nf);
    T.j[T.n++] = tiled(wo[JE_GD0_W], c.p(t.gd0.w), nf, nf, 0, nf);
    T.j[T.n++] = vec(wo[JE_GD0_B], c.p(t.gd0.b), nf, 1, nf);
    T.j[T.n++] = vec(wo[JE_GD2_W], c.p(t.gd2.w), nf, 1, nf);
    T.j[T.n++] = vec(wo[JE_GD2_B], c.p(t.gd2.b), 1, 1, 1);
    launch(T);
    for (int l = 0; l < L; ++l) {
        const int64_t* wl = wo + JE_GLOBAL_COUNT + (size_t)l * JEL_LAYER_COUNT;
        const LayIx& ix = t.lay[l];
        const int K0 = 2 * nf + 1, KN = 2 * nf + (t.cfg.node_attr ? in : 0);
        T.n = 0;
        T.j[T.n++] = tiled(wl[JEL_P_W], c.p(ix.e0.w), nf, K0, 0, nf, c.p(ix.e0.w), nf, nf);
        T.j[T.n++] = vec(wl[JEL_P_B], c.p(ix.e0.b), nf, 1, 2 * nf);
        T.j[T.n++] = vec(wl[JEL_WR], c.p(ix.e0.w) + 2 * nf, nf, K0, nf);
        T.j[T.n++] = tiled(wl[JEL_W2], c.p(ix.e2.w), nf, nf, 0, nf);
        T.j[T.n++] = vec(wl[JEL_B2], c.p(ix.e2.b), nf, 1, nf);
        T.j[T.n++] = transposed_job(c.b.w2t + (size_t)l * nf * nf, c.p(ix.e2.w), nf);      // outside the forward's slot table
        if (t.cfg.attention) {
            T.j[T.n++] = vec(wl[JEL_ATT_W], c.p(ix.att.w), nf, 1, nf);
            T.j[T.n++] = vec(wl[JEL_ATT_B], c.p(ix.att.b), 1, 1, 1);
        }
        T.j[T.n++] = tiled(wl[JEL_N0_W], c.p(ix.n0.w), nf, KN, 0, KN);
        T.j[T.n++] = vec(wl[JEL_N0_B], c.p(ix.n0.b), nf, 1, nf);
        T.j[T.n++] = tiled(wl[JEL_N2_W], c.p(ix.n2.w), nf, nf, 0, nf);
        T.j[T.n++] = vec(wl[JEL_N2_B], c.p(ix.n2.b), nf, 1, nf);
        launch(T);
    }
}

int forward(const Ctx& c, const void* desc_dev, const float* h0, const float* x, float* out) {
    pack_tape(c);
    const jodo_egnn_train& t = c.t;
    return jegnn::run(&t.cfg, t.B, t.N, t.Nn, desc_dev, c.b.tape, t.woff.data(), h0, x, out, c.b.fw, -1, c.s);
}

int backward(const Ctx& c, const void* desc_dev, const float* d_out) {
    const jodo_egnn_train& t = c.t; TBufs& b = c.b; hipStream_t st = c.s;
    const int B = t.B, Nn = t.Nn, nf = t.cfg.hidden_nf, in = t.cfg.in_node_nf, L = t.cfg.n_layers, NB = nf / 32, NK = nf / 64;
    const int* desc = static_cast<const int*>(desc_dev);
    const int *mol_n = desc, *mol_noff = desc + B, *node_b = desc + 2 * B, *eoff = desc + 2 * B + Nn;
    const float* tape = b.tape;
    const int64_t* wo = t.woff.data();
    // gradients are accumulated below: zero them first — adjacent buffers (and gaps under 16 bytes between them) in one fill
    for (int i = 0; i < t.n_params;) {
        char* beg = reinterpret_cast<char*>(c.g(i));
        size_t bytes = t.numel[i] * 4;
        int j = i + 1;
        while (j < t.n_params && reinterpret_cast<char*>(c.g(j)) >= beg + bytes && reinterpret_cast<char*>(c.g(j)) - (beg + bytes) < 16) {
            bytes = (size_t)(reinterpret_cast<char*>(c.g(j)) - beg) + t.numel[j] * 4;
            ++j;
        }
        (void)hipMemsetAsync(beg, 0, bytes, st);
        i = j;
    }
    const unsigned gB = (unsigned)(((size_t)B * nf + 255) / 256), gN = (unsigned)(((size_t)Nn * nf + 255) / 256);
    // ---- readout: out = w . SiLU(graph_dec.0 g) + bias, g = per-molecule sum of node_dec.2 SiLU(node_dec.0 h_L)
    c.lin_dw(d_out, 1, B, 1, b.fw.g1, nf, nf, c.g(t.gd2.w), nf, c.g(t.gd2.b));
    if (int rc = jegnn::row_gemm(st, b.fw.g, nf, NK, nullptr, 0, 0, nullptr, 0, 0, b.zg, nf, tape + wo[JE_GD0_W], tape + wo[JE_GD0_B], B, NB, 0, nullptr)) return rc;
    LEGT(kegnn_out_bwd, gB, 256, B, nf, d_out, c.p(t.gd2.w), (const float*)b.zg, b.dzg);
    c.lin_dw(b.dzg, nf, B, nf, b.fw.g, nf, nf, c.g(t.gd0.w), nf, c.g(t.gd0.b));
    c.lin_dx(b.dzg, nf, B, nf, c.p(t.gd0.w), nf, nf, b.dg, nf, 0);
    float *dhd = b.dagg, *dh = b.dh, *dt = b.dt;
    LEGT(kegnn_bcast_mol, gN, 256, Nn, nf, node_b, (const float*)b.dg, dhd);
    c.lin_dw(dhd, nf, Nn, nf, b.fw.tnd, nf, nf, c.g(t.nd2.w), nf, c.g(t.nd2.b));
    c.lin_dx(dhd, nf, Nn, nf, c.p(t.nd2.w), nf, nf, dt, nf, 0);
    if (int rc = jegnn::row_gemm(st, b.fw.h[L], nf, NK, nullptr, 0, 0, nullptr, 0, 0, b.zs, nf, tape + wo[JE_ND0_W], tape + wo[JE_ND0_B], Nn, NB, 0, nullptr)) return rc;
    LEGT(kegnn_silu_bwd, gN, 256, (size_t)Nn * nf, (const float*)b.zs, dt);
    c.lin_dw(dt, nf, Nn, nf, b.fw.h[L], nf, nf, c.g(t.nd0.w), nf, c.g(t.nd0.b));
    c.lin_dx(dt, nf, Nn, nf, c.p(t.nd0.w), nf, nf, dh, nf, 0);
    // ---- layers
    for (int l = L - 1; l >= 0; --l) {
        const int64_t* wl = wo + JE_GLOBAL_COUNT + (size_t)l * JEL_LAYER_COUNT;
        const LayIx& ix = t.lay[l];
        const int K0 = 2 * nf + 1, KN = 2 * nf + (t.cfg.node_attr ? in : 0);
        const float *h = b.fw.h[l], *agg = b.fw.agg[l], *tl = b.fw.t[l], *a0 = b.fw.a0;
        // h_{l+1} = h_l + node_mlp.2 SiLU(node_mlp.0 [h_l | agg | h0])
        c.lin_dw(dh, nf, Nn, nf, tl, nf, nf, c.g(ix.n2.w), nf, c.g(ix.n2.b));
        c.lin_dx(dh, nf, Nn, nf, c.p(ix.n2.w), nf, nf, dt, nf, 0);
        if (int rc = jegnn::row_gemm(st, h, nf, NK, agg, nf, NK, a0, 64, t.cfg.node_attr ? 1 : 0, b.zs, nf, tape + wl[JEL_N0_W], tape + wl[JEL_N0_B], Nn, NB, 0,
                                     nullptr))
            return rc;
        LEGT(kegnn_silu_bwd, gN, 256, (size_t)Nn * nf, (const float*)b.zs, dt);
        c.lin_dw(dt, nf, Nn, nf, h, nf, nf, c.g(ix.n0.w), KN, c.g(ix.n0.b));
        c.lin_dw(dt, nf, Nn, nf, agg, nf, nf, c.g(ix.n0.w) + nf, KN);
        if (t.cfg.node_attr) c.lin_dw(dt, nf, Nn, nf, a0, 64, in, c.g(ix.n0.w) + 2 * nf, KN);
        c.lin_dx(dt, nf, Nn, nf, c.p(ix.n0.w) + nf, KN, nf, b.dagg, nf, 0);
        c.lin_dx(dt, nf, Nn, nf, c.p(ix.n0.w), KN, nf, dh, nf, 1);                      // dh is now d h_l without the edge path
        // the edge path
        EBwd A{mol_n, mol_noff, node_b, eoff, Nn, b.fw.p[l], b.fw.xc, b.dagg, tape + wl[JEL_WR], tape + wl[JEL_W2], b.w2t + (size_t)l * nf * nf,
               tape + wl[JEL_B2], t.cfg.attention ? tape + wl[JEL_ATT_W] : nullptr, t.cfg.attention ? tape + wl[JEL_ATT_B] : nullptr,
               b.dP, b.Q, b.qb, b.ea, b.ez1, b.ez2};
        if (int rc = jegnn::edge_backward(st, NB, A)) return rc;      // kegnn_edge_bwd, then kegnn_tgt_sum
        if (t.E > 0) c.lin_dw(b.ez2, nf, t.E, nf, b.ea, nf, nf, c.g(ix.e2.w), nf, c.g(ix.e2.b));
        c.colsum(Nn, 2 * nf, b.Q, 2 * nf);
        c.colsum_fin(Nn, nf, b.part, 2 * nf, c.g(ix.e0.w) + 2 * nf, K0);
        if (t.cfg.attention) {
            c.colsum_fin(Nn, nf, b.part + nf, 2 * nf, c.g(ix.att.w), 1);
            c.colsum(Nn, 1, b.qb, 1);
            c.colsum_fin(Nn, 1, b.part, 1, c.g(ix.att.b), 1);
        }
        // P = h [W_src ; W_tgt]^T + [b1 ; 0]
        c.lin_dw(b.dP, 2 * nf, Nn, nf, h, nf, nf, c.g(ix.e0.w), K0, c.g(ix.e0.b));
        c.lin_dw(b.dP + nf, 2 * nf, Nn, nf, h, nf, nf, c.g(ix.e0.w) + nf, K0);
        c.lin_dx(b.dP, 2 * nf, Nn, nf, c.p(ix.e0.w), K0, nf, dh, nf, 1);
        c.lin_dx(b.dP + nf, 2 * nf, Nn, nf, c.p(ix.e0.w) + nf, K0, nf, dh, nf, 1);
    }
    // h_0 = embedding(h0)
    c.lin_dw(dh, nf, Nn, nf, b.fw.a0, 64, in, c.g(t.emb.w), in, c.g(t.emb.b));
    return JODO_OK;
}

}  // namespace

extern "C" {

int jodo_egnn_train_create(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes, const jodo_tensor* params, int n_params, jodo_egnn_train** out) {
    if (!cfg || !n_nodes || !params || !out || B <= 0 || N <= 0) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_create: null / non-positive argument");
    if (int rc = jodo_egnn_check_cfg(cfg)) return rc;
    if (N > 255) return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_egnn_train_create: padded width %d above 255", N);
    if (B >= (1 << 22)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_egnn_train_create: batch %d too large", B);
    long Nn = 0, E = 0;
    for (int b = 0; b < B; ++b) {
        if (n_nodes[b] < 1 || n_nodes[b] > N) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_create: n_nodes[%d] = %d outside 1..%d", b, n_nodes[b], N);
        Nn += n_nodes[b]; E += (long)n_nodes[b] * (n_nodes[b] - 1);
    }
    if (Nn >= (1L << 31) / (2 * cfg->hidden_nf) || E > (1L << 30))
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_egnn_train_create: batch too large (%ld atoms, %ld edges)", Nn, E);
    jodo_egnn_train* t = new jodo_egnn_train();
    t->cfg = *cfg; t->B = B; t->N = N; t->Nn = (int)Nn; t->E = E;
    t->tables.assign((size_t)3 * B + Nn, 0);
    fill_tables(B, n_nodes, Nn, t->tables.data());
    std::unordered_map<std::string, int> ix;
    t->n_params = n_params; t->numel.resize(n_params);
    for (int i = 0; i < n_params; ++i) {
        std::string nm = params[i].name ? params[i].name : "";
        if (nm.rfind("module.", 0) == 0) nm = nm.substr(7);
        size_t ne = 1;
        for (int d = 0; d < params[i].ndim; ++d) ne *= (size_t)params[i].shape[d];
        t->numel[i] = ne; ix[nm] = i;
    }
    std::string missing;
    auto find = [&](const std::string& nm, size_t numel) -> int {
        auto it = ix.find(nm);
        if (it == ix.end() || t->numel[it->second] != numel) { if (missing.empty()) missing = nm; return -1; }
        return it->second;
    };
    auto lin = [&](const std::string& nm, size_t out_f, size_t in_f) { Lin l; l.w = find(nm + ".weight", out_f * in_f); l.b = find(nm + ".bias", out_f); return l; };
    const size_t nf = cfg->hidden_nf, in = cfg->in_node_nf;
    t->emb = lin("embedding", nf, in);
    t->lay.resize(cfg->n_layers);
    for (int l = 0; l < cfg->n_layers; ++l) {
        const std::string p = "gcl_" + std::to_string(l) + ".";
        LayIx& k = t->lay[l];
        k.e0 = lin(p + "edge_mlp.0", nf, 2 * nf + 1); k.e2 = lin(p + "edge_mlp.2", nf, nf);
        k.n0 = lin(p + "node_mlp.0", nf, 2 * nf + (cfg->node_attr ? in : 0)); k.n2 = lin(p + "node_mlp.2", nf, nf);
        if (cfg->attention) k.att = lin(p + "att_mlp.0", 1, nf);
    }
    t->nd0 = lin("node_dec.0", nf, nf); t->nd2 = lin("node_dec.2", nf, nf);
    t->gd0 = lin("graph_dec.0", nf, nf); t->gd2 = lin("graph_dec.2", 1, nf);
    if (!missing.empty()) { delete t; return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_create: parameter '%s' missing or mis-sized", missing.c_str()); }
    t->woff.assign((size_t)JE_GLOBAL_COUNT + (size_t)cfg->n_layers * JEL_LAYER_COUNT, 0);
    if (int rc = jodo_egnn_packed_layout(cfg, t->woff.data(), (int)t->woff.size(), &t->tape_floats)) { delete t; return rc; }
    Arena a{nullptr, 0}; TBufs bufs;
    layout(*t, a, bufs);
    t->ws_bytes = a.off;
    *out = t;
    return JODO_OK;
}

void jodo_egnn_train_destroy(jodo_egnn_train* t) { delete t; }
size_t jodo_egnn_train_desc_bytes(const jodo_egnn_train* t) { return t ? t->tables.size() * sizeof(int) : 0; }
size_t jodo_egnn_train_workspace_bytes(const jodo_egnn_train* t) { return t ? t->ws_bytes : 0; }
const void* jodo_egnn_train_desc_host(const jodo_egnn_train* t) { return t ? t->tables.data() : nullptr; }
int jodo_egnn_train_upload(jodo_egnn_train* t, void* desc_dev, void* stream) {
    if (!t || !desc_dev) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_upload: null argument");
    (void)hipMemcpyAsync(desc_dev, t->tables.data(), t->tables.size() * sizeof(int), hipMemcpyHostToDevice, static_cast<hipStream_t>(stream));
    (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));
    return jodo_check_launch("jodo_egnn_train_upload");
}
// option 2 (the numbering of jodo_train2d_set_option): 1 (default) / 0 = the following forwards are (not) followed by a backward.  The
// forward keeps the same per-atom tensors either way, so the value changes nothing; options 0 / 1 (fused chains) do not exist here.
int jodo_egnn_train_set_option(jodo_egnn_train* t, int option, int value) {
    if (!t) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_set_option: null handle");
    if (option != 2 || (value != 0 && value != 1)) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_set_option: option %d value %d", option, value);
    return JODO_OK;
}
// tests: where a kept tensor of layer `layer` lives in the workspace.  0 = h_layer [Nn, nf] (layer 0 .. L: L = the last hidden state),
// 1 = P [Nn, 2 nf], 2 = agg [Nn, nf], 3 = SiLU(node_mlp.0) [Nn, nf]
int jodo_egnn_train_debug_locate(const jodo_egnn_train* t, int what, int layer, size_t* byte_offset, size_t* count) {
    if (!t || !byte_offset || !count) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_debug_locate: null argument");
    const int L = t->cfg.n_layers;
    if (layer < 0 || layer > L || (what != 0 && layer == L)) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_debug_locate: layer %d of %d", layer, L);
    Arena a{reinterpret_cast<char*>(256), 0};
    TBufs b;
    layout(*t, a, b);
    const size_t Nn = t->Nn, nf = t->cfg.hidden_nf;
    const float* ptr = nullptr;
    size_t n = 0;
    switch (what) {
        case 0: ptr = b.fw.h[layer]; n = Nn * nf; break;
        case 1: ptr = b.fw.p[layer]; n = Nn * 2 * nf; break;
        case 2: ptr = b.fw.agg[layer]; n = Nn * nf; break;
        case 3: ptr = b.fw.t[layer]; n = Nn * nf; break;
        default: return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_debug_locate: unknown selector %d", what);
    }
    *byte_offset = (size_t)(reinterpret_cast<const char*>(ptr) - reinterpret_cast<const char*>(256));
    *count = n;
    return JODO_OK;
}

int jodo_egnn_train_forward(jodo_egnn_train* t, const void* desc_dev, const float* const* params_dev, int n_params, const float* h0, const float* x,
                            float* out, void* workspace, void* stream) {
    if (!t || !desc_dev || !params_dev || !h0 || !x || !out || !workspace) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_forward: null argument");
    if (n_params != t->n_params) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_forward: %d parameters, handle was created with %d", n_params, t->n_params);
    Arena a{static_cast<char*>(workspace), 0}; TBufs bufs;
    layout(*t, a, bufs);
    Ctx c{*t, params_dev, nullptr, bufs, static_cast<hipStream_t>(stream)};
    if (int rc = forward(c, desc_dev, h0, x, out)) return rc;
    return jodo_check_launch("jodo_egnn_train_forward");
}

int jodo_egnn_train_backward(jodo_egnn_train* t, const void* desc_dev, const float* const* params_dev, float* const* grads_dev, int n_params,
                             const float* d_out, void* workspace, void* stream) {
    if (!t || !desc_dev || !params_dev || !grads_dev || !d_out || !workspace) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_backward: null argument");
    if (n_params != t->n_params) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_train_backward: %d parameters, handle was created with %d", n_params, t->n_params);
    Arena a{static_cast<char*>(workspace), 0}; TBufs bufs;
    layout(*t, a, bufs);
    Ctx c{*t, params_dev, grads_dev, bufs, static_cast<hipStream_t>(stream)};
    if (int rc = backward(c, desc_dev, d_out)) return rc;
    return jodo_check_launch("jodo_egnn_train_backward");
}

// tests: one edge kernel on caller-owned arrays (include/jodo_hip.h).  No kernel lives here; the entry is the safety boundary of
// tests/test_egnn_kernels_gpu.py: everything is checked on the host before anything is launched.
int jodo_egnn_debug_edge(const jodo_egnn_edge_test_args* args, void* stream) {
    static const char* const SLOT[JODO_ET_N_SLOTS] = {"p", "xc", "dagg", "wr", "w2", "b2", "wa", "ba", "desc", "img", "agg", "ea", "ez2", "ez1",
                                                     "dp", "q", "qb"};
    if (!args) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: args is a null pointer");
    const jodo_egnn_edge_test_args& a = *args;
    if (a.op < 0 || a.op >= JODO_ET_N_OPS) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: unknown op %d", a.op);
    if (a.nf != 64 && a.nf != 128 && a.nf != 192 && a.nf != 256)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_egnn_debug_edge: hidden_nf %d is not one of 64, 128, 192, 256", a.nf);
    if (a.B <= 0 || a.B >= (1 << 22) || !a.n_nodes) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: B %d or a null n_nodes", a.B);
    if (a.grid_cap < 0) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: grid_cap %d", a.grid_cap);
    long Nn = 0, E = 0;
    for (int b = 0; b < a.B; ++b) {
        const int n = a.n_nodes[b];
        if (n < 1) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: n_nodes[%d] = %d below 1", b, n);
        if (n > 255) return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_egnn_debug_edge: n_nodes[%d] = %d above 255", b, n);
        Nn += n; E += (long)n * (n - 1);
    }
    if (Nn >= (1L << 31) / (2 * a.nf) || E > (1L << 30))
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_egnn_debug_edge: batch too large (%ld atoms, %ld edges)", Nn, E);
    const size_t nf = (size_t)a.nf, N = (size_t)Nn, Ee = (size_t)E, words = (size_t)3 * a.B + N;
    const bool bwd = a.op == JODO_ET_OP_BWD, att = a.a[JODO_ET_WA] || a.a[JODO_ET_BA];
    // slot -> element count the op touches (exact for the arrays, a minimum for the scratch); -1: not used
    long need[JODO_ET_N_SLOTS];
    for (int s = 0; s < JODO_ET_N_SLOTS; ++s) need[s] = -1;
    need[JODO_ET_P] = (long)(N * 2 * nf); need[JODO_ET_XC] = (long)(N * 4); need[JODO_ET_WR] = need[JODO_ET_B2] = (long)nf;
    need[JODO_ET_W2] = (long)(nf * nf); need[JODO_ET_DESC] = (long)words; need[JODO_ET_IMG] = (long)(2 * nf * nf);
    if (att) { need[JODO_ET_WA] = (long)nf; need[JODO_ET_BA] = 1; }
    if (bwd) {
        need[JODO_ET_DAGG] = (long)(N * nf);
        need[JODO_ET_EA] = need[JODO_ET_EZ2] = need[JODO_ET_EZ1] = (long)(Ee * nf);
        need[JODO_ET_DP] = need[JODO_ET_Q] = (long)(N * 2 * nf); need[JODO_ET_QB] = (long)N;
    } else {
        need[JODO_ET_AGG] = (long)(N * nf);
    }
    for (int s = 0; s < JODO_ET_N_SLOTS; ++s) {
        if (need[s] < 0) continue;
        const bool scratch = s == JODO_ET_DESC || s == JODO_ET_IMG;
        if (scratch ? a.n[s] < (size_t)need[s] : a.n[s] != (size_t)need[s])
            return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: array %s has %zu elements, the op touches %ld", SLOT[s], a.n[s], need[s]);
        if (need[s] == 0) continue;
        if (!a.a[s]) return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: array %s is a null pointer", SLOT[s]);
        const uintptr_t align = s == JODO_ET_BA ? 4 : 16;
        if (((uintptr_t)a.a[s] & (align - 1)) != 0)
            return jodo_set_error(JODO_ERR_ARG, "jodo_egnn_debug_edge: array %s is not %d-byte aligned", SLOT[s], (int)align);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_egnn_debug_edge: no HIP device");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<int> tables(words, 0);
    fill_tables(a.B, a.n_nodes, Nn, tables.data());
    int* desc = reinterpret_cast<int*>(a.a[JODO_ET_DESC]);
    if (hipMemcpyAsync(desc, tables.data(), words * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return jodo_set_error(JODO_ERR_LAUNCH, "jodo_egnn_debug_edge: upload of the descriptor failed");      // (tables is pageable and local: wait)
    float *img = a.a[JODO_ET_IMG], *imgT = img + nf * nf;
    PackTable T;
    T.n = 0;
    T.j[T.n++] = tiled_job(img, a.a[JODO_ET_W2], a.nf, a.nf, 0, a.nf);
    if (bwd) T.j[T.n++] = transposed_job(imgT, a.a[JODO_ET_W2], a.nf);
    launch_pack(st, T);
    const int B = a.B, NB = a.nf / 32, cap = a.grid_cap > 0 ? a.grid_cap : jegnn::EDGE_GRID_MAX;
    const int *mol_n = desc, *mol_noff = desc + B, *node_b = desc + 2 * B, *eoff = desc + 2 * B + Nn;
    const float *wa = att ? a.a[JODO_ET_WA] : nullptr, *ba = att ? a.a[JODO_ET_BA] : nullptr;
    if (bwd) {
        EBwd A{mol_n, mol_noff, node_b, eoff, (int)Nn, a.a[JODO_ET_P], a.a[JODO_ET_XC], a.a[JODO_ET_DAGG], a.a[JODO_ET_WR], img, imgT, a.a[JODO_ET_B2],
               wa, ba, a.a[JODO_ET_DP], a.a[JODO_ET_Q], a.a[JODO_ET_QB], a.a[JODO_ET_EA], a.a[JODO_ET_EZ1], a.a[JODO_ET_EZ2]};
        if (int rc = jegnn::edge_backward(st, NB, A, cap)) return rc;
    } else {
        jegnn::EEdge A{mol_n, mol_noff, node_b, (int)Nn, a.a[JODO_ET_P], a.a[JODO_ET_XC], a.a[JODO_ET_WR], img, a.a[JODO_ET_B2], wa, ba, a.a[JODO_ET_AGG]};
        if (int rc = jegnn::edge_forward(st, NB, A, cap)) return rc;
    }
    return jodo_check_launch("jodo_egnn_debug_edge");
}

}  // extern "C"

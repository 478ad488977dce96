// Shared by the property classifier's forward (egnn_forward.hip) and its training path (egnn_train.hip): the device helper both edge
// kernels use, and the host side of the forward with one destination per layer, so that the training forward runs the very same
// kernels in the same order and only keeps what inference overwrites.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/jodo_hip.h"

namespace jegnn {

// lane j ends with the total of value j % 16 over the 32 lanes of its half (as in csrc/dgt2d_forward.hip): a fixed exchange tree
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

constexpr int EDGE_GRID_MAX = 512, EDGE_WAVES = 4;      // persistent edge kernels: grid cap, waves per workgroup

// Where one evaluation writes.  Inference points every layer at the same arrays (h is then updated in place); the training forward
// gives each layer its own.  h has n_layers + 1 entries (h[0] = the embedding), the others n_layers.
struct Bufs {
    float *a0, *xc;                  // [Nn, 64] gathered input, [Nn, 4] positions
    float* h[17];                    // [Nn, nf]
    float *p[16], *agg[16], *t[16];  // [Nn, 2 nf], [Nn, nf], [Nn, nf] = SiLU(node_mlp.0)
    float *tnd, *hd, *g, *g1;        // SiLU(node_dec.0) [Nn, nf], node_dec [Nn, nf], molecule sums [B, nf], SiLU(graph_dec.0) [B, nf]
};

// the evaluation of jodo_egnn_forward on the destinations given; desc_dev = n_b [B] | noff_b [B] | (b << 8 | i) [Nn]
int run(const jodo_egnn_cfg* cfg, int B, int N, int Nn, const void* desc_dev, const float* packed_w, const int64_t* woff, const float* h0,
        const float* x, float* out, const Bufs& bufs, int max_layers, hipStream_t st);

// Arguments of the two fused edge kernels (kegnn_edge in egnn_forward.hip, kegnn_edge_bwd in egnn_train.hip).
struct EEdge {
    const int *mol_n, *mol_noff, *node_b;
    int Nn;
    const float *P, *xc;         // P [Nn, 2 nf] = [P_src + b1 | P_tgt], xc [Nn, 4]
    const float *wr, *W2, *b2, *wa, *ba;     // wa NULL: no attention
    float* agg;                  // [Nn, nf]
};
struct EBwd {
    const int *mol_n, *mol_noff, *node_b, *eoff;
    int Nn;
    const float *P, *xc, *dagg;              // P [Nn, 2 nf] = [P_src + b1 | P_tgt], xc [Nn, 4], dagg [Nn, nf]
    const float *wr, *W2, *W2T, *b2, *wa, *ba;       // wa NULL: no attention
    float *dP, *Q, *qb;                      // dP [Nn, 2 nf] (columns 0 .. nf written here), Q [Nn, 2 nf] = dw_r | dw_a partial rows, qb [Nn]
    float *ea, *ez1, *ez2;                   // compact edge rows [E, nf]
};

// The host launchers of the edge kernels: the instantiation for NB = nf / 32 (2, 4: W2 in LDS; 6, 8: streamed) on a persistent grid of
// at most grid_cap workgroups.  jegnn::run and the training backward call them at the default; the test entry jodo_egnn_debug_edge
// (egnn_train.hip) also with smaller caps.  edge_backward is kegnn_edge_bwd followed by kegnn_tgt_sum (the second half of dP).
int edge_forward(hipStream_t st, int NB, const EEdge& A, int grid_cap = EDGE_GRID_MAX);
int edge_backward(hipStream_t st, int NB, const EBwd& A, int grid_cap = EDGE_GRID_MAX);

// kegnn_gemm on its own: Y[rows, 32 nb] = epi([X0 | X1 | X2] W^T + bias), K chunks of 64 (nk0 + nk1 + nk2), act 1 = SiLU, R = residual
int row_gemm(hipStream_t st, const float* X0, int ld0, int nk0, const float* X1, int ld1, int nk1, const float* X2, int ld2, int nk2, float* Y,
             int ldy, const float* W, const float* bias, int rows, int nb, int act, const float* R);

}  // namespace jegnn

// slot offsets of the packed blob without any data (egnn_pack.cpp): what jodo_egnn_pack_weights_host writes into woff_out
extern "C" int jodo_egnn_packed_layout(const jodo_egnn_cfg* cfg, int64_t* woff_out, int n_woff, size_t* n_floats);

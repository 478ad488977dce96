// Fused caller-side kernels of the sampling loop: HBM-bound elementwise
// work on the dense API tensors, one pass each instead of ~25 small framework launches per step.
//
//   jodo_sampler_step   the ancestral update of AncestralSampler.sampling (sampling.py:536-589):
//                         mean = c_x * x_t + c_pred * pred          (nodes and edges)
//                         x_s  = mean + sigma * eps
//                       with eps built from raw N(0,1) draws exactly as the reference's noise samplers do
//                       (models/utils.py:67-99): node noise masked, its 3 position channels made
//                       centre-of-mass free per molecule; edge noise = strict lower triangle of a
//                       [B,ch,N,N] draw mirrored to the upper triangle, masked, diagonal zero.
//   jodo_decode         post_process + the per-molecule part of mol_process (sampling.py:53-97, :12-32,
//                       utils.py:71-105): undo the normalisation, atom type = argmax, formal charge =
//                       round, bond order by thresholds; compact u8/i8 outputs for ONE device->host copy.
//
// Both take the atom counts as a device int32[B] (masks are prefix masks, sampling.py:193-201); all
// tensors are the reference's dense row-major layouts.  Coalescing: one thread per innermost element,
// consecutive threads walk the contiguous last dimensions.
#include <hip/hip_runtime.h>
#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"

namespace {

// ---- counter-based normal draws (SURVEY.md §8f row 1 "device noise"): Philox4x32-10 (Salmon et al., SC'11) keyed by the
// caller's 64-bit seed, counter = (element lo, element hi, draw index, stream id); four uniforms -> four normals by
// Box-Muller.  A value depends only on (seed, draw, stream, element): no generator state, so the same call replays in a
// captured hipGraph (draw index from a device counter), both triangle halves of the edge noise evaluate the SAME
// counter (exactly symmetric), and ranks with different seeds never share a stream.  oracle/philox_ref.py restates
// it in numpy (tests only).
struct Rng { unsigned long long seed; unsigned draw; unsigned draw_mul; int on; };
enum { RNG_POS = 0, RNG_FEAT = 1, RNG_EDGE = 2 };

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// four N(0,1) draws of element `elem` of stream `stream` at draw index `draw`
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned draw, unsigned stream, unsigned long long elem,
                                               float z[4]) {
    unsigned u[4];
    philox4x32_10((unsigned)elem, (unsigned)(elem >> 32), draw, stream, (unsigned)seed, (unsigned)(seed >> 32), u);
    // u1 in (0, 1], u2 in [0, 1): r = sqrt(-2 ln u1), angle = 2 pi u2
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = ((float)(u[2 * p] >> 8) + 1.0f) * (1.0f / 16777216.0f);
        const float u2 = (float)(u[2 * p + 1] >> 8) * (1.0f / 16777216.0f);
        const float r = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);
        z[2 * p] = r * cs; z[2 * p + 1] = r * sn;
    }
}
__device__ __forceinline__ unsigned rng_draw(const Rng& g, const int* step) { return g.draw + (step ? (unsigned)(*step) * g.draw_mul : 0u); }
// raw position draw of atom (b, i): component f in 0..2
__device__ __forceinline__ void rng_pos3(const Rng& g, unsigned draw, size_t atom, float e[3]) {
    float z[4];
    philox_normal4(g.seed, draw, RNG_POS, atom, z);
    e[0] = z[0]; e[1] = z[1]; e[2] = z[2];
}
__device__ __forceinline__ float rng_feat(const Rng& g, unsigned draw, size_t atom, int k) {
    float z[4];
    philox_normal4(g.seed, draw, RNG_FEAT, atom * 64 + (size_t)(k >> 2), z);       // up to 256 feature channels per atom
    return z[k & 3];
}
// raw edge draw of the unordered pair (lo > hi) of molecule b, channel f < 4
__device__ __forceinline__ float rng_edge(const Rng& g, unsigned draw, size_t cell_lower, int f) {
    float z[4];
    philox_normal4(g.seed, draw, RNG_EDGE, cell_lower, z);
    return z[f & 3];
}

// one workgroup per molecule: mean / next state of the node tensor [N, F] (F = 3 + nd)
// coef (optional): device table [steps][4] = (c_x, c_pred, sigma, noise_level), row *step — lets a captured
// HIP graph of one sampling step be replayed for every step (host scalars would be baked into the graph)
__global__ __launch_bounds__(256) void k_step_nodes(int N, int F, const int* __restrict__ n_nodes, float c_x, float c_pred,
                                                    float sigma, const float* __restrict__ coef, const int* __restrict__ step,
                                                    const float* __restrict__ x, const float* __restrict__ pred,
                                                    const float* __restrict__ eps_pos, const float* __restrict__ eps_feat,
                                                    Rng rng, float* __restrict__ x_next, float* __restrict__ x_mean) {
    const int b = blockIdx.x, n = n_nodes[b], nd = F - 3;
    if (coef) { const float* c = coef + 4 * (size_t)(*step); c_x = c[0]; c_pred = c[1]; sigma = c[2]; }
    const unsigned draw = rng.on ? rng_draw(rng, coef ? step : nullptr) : 0u;
    __shared__ float red[3][256];
    // centre of mass of the masked position noise: sum over real atoms / n  (remove_mean_with_mask)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float ev[3];
        if (rng.on) rng_pos3(rng, draw, (size_t)b * N + i, ev);
        else { const float* e = eps_pos + ((size_t)b * N + i) * 3; ev[0] = e[0]; ev[1] = e[1]; ev[2] = e[2]; }
        s0 += ev[0]; s1 += ev[1]; s2 += ev[2];
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
            red[2][threadIdx.x] += red[2][threadIdx.x + w];
        }
        __syncthreads();
    }
    const float inv = 1.f / (float)n;
    const float m[3] = {red[0][0] * inv, red[1][0] * inv, red[2][0] * inv};
    for (int idx = threadIdx.x; idx < N * F; idx += blockDim.x) {
        const int i = idx / F, f = idx % F;
        const size_t g = (size_t)b * N * F + idx;
        // products rounded separately, then added: the op order of the framework expression c_x*x + c_pred*pred
        const float mean = __fadd_rn(__fmul_rn(c_x, x[g]), __fmul_rn(c_pred, pred[g]));
        float e = 0.f;
        if (i < n) {
            if (rng.on) {
                if (f < 3) { float ev[3]; rng_pos3(rng, draw, (size_t)b * N + i, ev); e = ev[f] - m[f]; }
                else e = rng_feat(rng, draw, (size_t)b * N + i, f - 3);
            } else e = f < 3 ? eps_pos[((size_t)b * N + i) * 3 + f] - m[f] : eps_feat[((size_t)b * N + i) * nd + (f - 3)];
        }
        x_mean[g] = mean;
        x_next[g] = __fadd_rn(mean, __fmul_rn(sigma, e));
    }
}

// one thread per (b, a, c, f) of the edge tensor [B, N, N, ch]; eps_edge is the raw draw [B, ch, N, N]
__global__ __launch_bounds__(256) void k_step_edges(int B, int N, int ch, const int* __restrict__ n_nodes, float c_x, float c_pred,
                                                    float sigma, const float* __restrict__ coef, const int* __restrict__ step,
                                                    const float* __restrict__ ex, const float* __restrict__ epred,
                                                    const float* __restrict__ eps, Rng rng, float* __restrict__ e_next,
                                                    float* __restrict__ e_mean) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t NN = (size_t)N * N, tot = (size_t)B * NN * ch;
    if (g >= tot) return;
    if (coef) { const float* c = coef + 4 * (size_t)(*step); c_x = c[0]; c_pred = c[1]; sigma = c[2]; }
    const int f = (int)(g % ch);
    const size_t cell = g / ch;
    const int c = (int)(cell % N), a = (int)((cell / N) % N), b = (int)(cell / NN);
    const int n = n_nodes[b];
    const float mean = __fadd_rn(__fmul_rn(c_x, ex[g]), __fmul_rn(c_pred, epred[g]));
    float e = 0.f;
    if (a < n && c < n && a != c) {
        const int lo = a > c ? a : c, hi = a > c ? c : a;          // strict lower triangle entry (row lo, col hi)
        e = rng.on ? rng_edge(rng, rng_draw(rng, coef ? step : nullptr), ((size_t)b * N + lo) * N + hi, f)
                   : eps[(((size_t)b * ch + f) * N + lo) * N + hi];
    }
    e_mean[g] = mean;
    e_next[g] = __fadd_rn(mean, __fmul_rn(sigma, e));
}

// ---- the 2-D sampler's update with both draws generated in the kernel (jodo_sampler_step_2d_rng): node tensor [B,N,nd] WITHOUT
// position channels, edge tensor [B,N,N,ch].  ONE launch over two index ranges: a thread of the first owns the four node channels
// 4q .. 4q+3 of one atom (one Philox evaluation: element atom * 64 + q of stream RNG_FEAT, the numbering of rng_feat above), a
// thread of the second owns all channels of one cell (b, r, c) (one evaluation: cell (b, max, min) of stream RNG_EDGE, as
// rng_edge; both orientations of a pair evaluate the same counter, so the edge noise is exactly symmetric).  Every output
// element is written by exactly one thread with plain stores; padding and the diagonal get mean + sigma * 0.
__global__ __launch_bounds__(256) void k_step_2d_rng(int B, int N, int nd, int ch, const int* __restrict__ n_nodes, float c_x, float c_pred,
                                                     float sigma, const float* __restrict__ coef, const int* __restrict__ step, Rng rng,
                                                     const float* __restrict__ x, const float* __restrict__ ex,
                                                     const float* __restrict__ pred, const float* __restrict__ epred,
                                                     float* __restrict__ x_next, float* __restrict__ e_next, float* __restrict__ x_mean,
                                                     float* __restrict__ e_mean) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = (nd + 3) >> 2;
    const size_t n_quad = (size_t)B * N * nq, n_cell = (size_t)B * N * N;
    if (g >= n_quad + n_cell) return;
    if (coef) { const float* c = coef + 4 * (size_t)(*step); c_x = c[0]; c_pred = c[1]; sigma = c[2]; }
    const unsigned draw = rng_draw(rng, coef ? step : nullptr);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (g < n_quad) {
        const int q = (int)(g % nq);
        const size_t atom = g / nq;
        const int i = (int)(atom % N), b = (int)(atom / N);
        if (i < n_nodes[b]) philox_normal4(rng.seed, draw, RNG_FEAT, atom * 64 + (size_t)q, z);
        const int k1 = min(4 * q + 4, nd);
        for (int k = 4 * q; k < k1; ++k) {
            const size_t o = atom * nd + k;
            const float mean = __fadd_rn(__fmul_rn(c_x, x[o]), __fmul_rn(c_pred, pred[o]));
            x_mean[o] = mean;
            x_next[o] = __fadd_rn(mean, __fmul_rn(sigma, z[k & 3]));
        }
    } else {
        const size_t cell = g - n_quad;
        const int c = (int)(cell % N), r = (int)((cell / N) % N), b = (int)(cell / ((size_t)N * N));
        const int n = n_nodes[b];
        if (r < n && c < n && r != c) {
            const int lo = r > c ? r : c, hi = r > c ? c : r;          // strict lower triangle entry (row lo, col hi)
            philox_normal4(rng.seed, draw, RNG_EDGE, ((size_t)b * N + lo) * N + hi, z);
        }
        for (int f = 0; f < ch; ++f) {
            const size_t o = cell * ch + f;
            const float mean = __fadd_rn(__fmul_rn(c_x, ex[o]), __fmul_rn(c_pred, epred[o]));
            e_mean[o] = mean;
            e_next[o] = __fadd_rn(mean, __fmul_rn(sigma, z[f]));
        }
    }
}

struct DecodeArgs {
    int B, N, atom_types, include_fc, ch, compress_edge, centered;
    float pos_norm, atom_norm, fc_norm, edge_norm;
};

// the inverse scaler in the framework's fp32 operation order (utils.py:71-105): x * norm, then (x + 1) / 2 when centred — each
// operation rounded on its own (no fused multiply-add), so that a value on a decision threshold falls on the framework's side
__device__ __forceinline__ float inv_scale(float v, float norm, int centered) {
    v = __fmul_rn(v, norm);
    return centered ? __fadd_rn(v, 1.f) * 0.5f : v;
}

// one thread per (b, i): positions (P = 3; P = 0: the 2-D models' node tensor without them, pos unused), atom type, formal charge
template <int P>
__global__ __launch_bounds__(256) void k_decode_nodes(DecodeArgs A, const int* __restrict__ n_nodes, const float* __restrict__ xh,
                                                      float* __restrict__ pos, uint8_t* __restrict__ atom_type,
                                                      int8_t* __restrict__ fc) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.B * A.N) return;
    const int b = idx / A.N, i = idx % A.N;
    const int F = P + A.atom_types + (A.include_fc ? 1 : 0);
    const float* r = xh + (size_t)idx * F;
    const bool real = i < n_nodes[b];
    if (P) {
        float* p = pos + (size_t)idx * P;
        for (int k = 0; k < P; ++k) p[k] = real ? r[k] * A.pos_norm : 0.f;
    }
    // argmax over the inverse-scaled categories (an increasing affine map: same argmax; first maximum wins)
    int best = 0;
    float bv = -INFINITY;
    for (int k = 0; k < A.atom_types; ++k) {
        float v = inv_scale(r[P + k], A.atom_norm, A.centered);
        if (!real) v = 0.f;
        if (v > bv) { bv = v; best = k; }
    }
    atom_type[idx] = (uint8_t)best;
    float q = 0.f;
    if (A.include_fc && real) q = rintf(r[F - 1] * A.fc_norm);       // torch.round = round-half-to-even
    fc[idx] = (int8_t)q;
}

// one thread per (b, a, c): bond type
__global__ __launch_bounds__(256) void k_decode_edges(DecodeArgs A, const int* __restrict__ n_nodes, const float* __restrict__ ex,
                                                      uint8_t* __restrict__ edge_type) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t NN = (size_t)A.N * A.N;
    if (idx >= (size_t)A.B * NN) return;
    const int b = (int)(idx / NN), a = (int)((idx % NN) / A.N), c = (int)(idx % A.N);
    const int n = n_nodes[b];
    const bool real = a < n && c < n && a != c;
    const float* r = ex + idx * A.ch;
    float h[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < A.ch && k < 4; ++k) {
        const float v = inv_scale(r[k], A.edge_norm, A.centered);
        h[k] = real ? v : 0.f;
    }
    int t = 0;
    if (A.compress_edge) {
        const bool exist = h[0] >= 0.5f;
        const float o = h[1] * 3.f;
        int order = 0;
        if (o >= 0.5f) order = 1;
        if (o >= 1.5f) order = 2;
        if (o >= 2.5f) order = 3;
        t = exist ? order : 0;
        if (A.ch == 3 && exist && h[2] >= 0.5f && t == 0) t = 4;
    } else {
        bool any = false;
        int best = 0;
        float bv = -INFINITY;
        for (int k = 0; k < A.ch && k < 4; ++k) {
            any |= h[k] > 0.5f;
            if (h[k] > bv) { bv = h[k]; best = k; }
        }
        t = any ? best + 1 : 0;
    }
    edge_type[idx] = (uint8_t)t;
}

}  // namespace

namespace {
__global__ void k_step_begin(int B, const float* __restrict__ coef, const int* __restrict__ step, float* __restrict__ noise_level) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) noise_level[b] = coef[4 * (size_t)(*step) + 3];
}
__global__ void k_step_end(int* step) { *step += 1; }

int sampler_step_launch(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float c_x, float c_pred, float sigma,
                        const float* coef, const int32_t* step, Rng rng, const float* x, const float* edge_x, const float* pred,
                        const float* edge_pred, const float* eps_pos, const float* eps_feat, const float* eps_edge, float* x_next,
                        float* edge_next, float* x_mean, float* edge_mean, void* stream) {
    if (B <= 0 || N <= 0 || node_feats < 4 || edge_ch < 1) return jodo_set_error(JODO_ERR_ARG, "sampler_step: bad shape");
    if (!n_nodes_dev || !x || !edge_x || !pred || !edge_pred || !x_next || !edge_next || !x_mean || !edge_mean)
        return jodo_set_error(JODO_ERR_ARG, "sampler_step: null argument");
    if (!rng.on && (!eps_pos || !eps_feat || !eps_edge)) return jodo_set_error(JODO_ERR_ARG, "sampler_step: null noise draw");
    if (rng.on && (edge_ch > 4 || node_feats - 3 > 256))
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "sampler_step_rng: at most 4 edge channels and 256 node feature channels");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_step_nodes, dim3(B), dim3(256), 0, st, N, node_feats, n_nodes_dev, c_x, c_pred, sigma, coef, step, x, pred,
                       eps_pos, eps_feat, rng, x_next, x_mean);
    int rc = jodo_check_launch("k_step_nodes");
    if (rc != JODO_OK) return rc;
    const size_t tot = (size_t)B * N * N * edge_ch;
    hipLaunchKernelGGL(k_step_edges, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, B, N, edge_ch, n_nodes_dev, c_x, c_pred,
                       sigma, coef, step, edge_x, edge_pred, eps_edge, rng, edge_next, edge_mean);
    return jodo_check_launch("k_step_edges");
}
const Rng kNoRng{0ull, 0u, 0u, 0};
}  // namespace

extern "C" int jodo_sampler_step(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float c_x, float c_pred,
                                 float sigma, const float* x, const float* edge_x, const float* pred, const float* edge_pred,
                                 const float* eps_pos, const float* eps_feat, const float* eps_edge, float* x_next,
                                 float* edge_next, float* x_mean, float* edge_mean, void* stream) {
    return sampler_step_launch(B, N, node_feats, edge_ch, n_nodes_dev, c_x, c_pred, sigma, nullptr, nullptr, kNoRng, x, edge_x, pred,
                               edge_pred, eps_pos, eps_feat, eps_edge, x_next, edge_next, x_mean, edge_mean, stream);
}

extern "C" int jodo_sampler_step_tab(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef_tab_dev,
                                     const int32_t* step_dev, const float* x, const float* edge_x, const float* pred,
                                     const float* edge_pred, const float* eps_pos, const float* eps_feat, const float* eps_edge,
                                     float* x_next, float* edge_next, float* x_mean, float* edge_mean, void* stream) {
    if (!coef_tab_dev || !step_dev) return jodo_set_error(JODO_ERR_ARG, "sampler_step_tab: null table");
    return sampler_step_launch(B, N, node_feats, edge_ch, n_nodes_dev, 0.f, 0.f, 0.f, coef_tab_dev, step_dev, kNoRng, x, edge_x, pred,
                               edge_pred, eps_pos, eps_feat, eps_edge, x_next, edge_next, x_mean, edge_mean, stream);
}

extern "C" int jodo_sampler_step_rng(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float c_x, float c_pred,
                                     float sigma, const float* coef_tab_dev, const int32_t* step_dev, uint64_t seed, uint32_t draw,
                                     const float* x, const float* edge_x, const float* pred, const float* edge_pred, float* x_next,
                                     float* edge_next, float* x_mean, float* edge_mean, void* stream) {
    if ((coef_tab_dev == nullptr) != (step_dev == nullptr))
        return jodo_set_error(JODO_ERR_ARG, "sampler_step_rng: pass both the device table and the step counter, or neither");
    return sampler_step_launch(B, N, node_feats, edge_ch, n_nodes_dev, c_x, c_pred, sigma, coef_tab_dev, step_dev, Rng{seed, draw, 1u, 1},
                               x, edge_x, pred, edge_pred, nullptr, nullptr, nullptr, x_next, edge_next, x_mean, edge_mean, stream);
}

extern "C" int jodo_sampler_step_2d_rng(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float c_x, float c_pred,
                                        float sigma, const float* coef_tab_dev, const int32_t* step_dev, uint64_t seed, uint32_t draw,
                                        const float* x, const float* edge_x, const float* pred, const float* edge_pred, float* x_next,
                                        float* edge_next, float* x_mean, float* edge_mean, void* stream) {
    if (B <= 0 || N <= 0 || node_feats < 1 || edge_ch < 1) return jodo_set_error(JODO_ERR_ARG, "sampler_step_2d_rng: bad shape");
    if (!n_nodes_dev || !x || !edge_x || !pred || !edge_pred || !x_next || !edge_next || !x_mean || !edge_mean)
        return jodo_set_error(JODO_ERR_ARG, "sampler_step_2d_rng: null argument");
    if ((coef_tab_dev == nullptr) != (step_dev == nullptr))
        return jodo_set_error(JODO_ERR_ARG, "sampler_step_2d_rng: pass both the device table and the step counter, or neither");
    if (edge_ch > 4 || node_feats > 256)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "sampler_step_2d_rng: at most 4 edge channels and 256 node channels");
    const size_t tot = (size_t)B * N * ((node_feats + 3) / 4) + (size_t)B * N * N;
    if ((tot + 255) / 256 > 0x7fffffffull) return jodo_set_error(JODO_ERR_UNSUPPORTED, "sampler_step_2d_rng: batch too large for one launch");
    hipLaunchKernelGGL(k_step_2d_rng, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, N, node_feats, edge_ch,
                       n_nodes_dev, c_x, c_pred, sigma, coef_tab_dev, step_dev, Rng{seed, draw, 1u, 1}, x, edge_x, pred, edge_pred, x_next,
                       edge_next, x_mean, edge_mean);
    return jodo_check_launch("k_step_2d_rng");
}

extern "C" int jodo_step_begin(int B, const float* coef_tab_dev, const int32_t* step_dev, float* noise_level_out, void* stream) {
    if (B <= 0 || !coef_tab_dev || !step_dev || !noise_level_out) return jodo_set_error(JODO_ERR_ARG, "step_begin: bad argument");
    hipLaunchKernelGGL(k_step_begin, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, coef_tab_dev, step_dev, noise_level_out);
    return jodo_check_launch("k_step_begin");
}

extern "C" int jodo_step_end(int32_t* step_dev, void* stream) {
    if (!step_dev) return jodo_set_error(JODO_ERR_ARG, "step_end: null");
    hipLaunchKernelGGL(k_step_end, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev);
    return jodo_check_launch("k_step_end");
}

// ---- hybrid DPM-Solver++ update (mix_dpm_solver.py:44-59 positions, :61-265 atom / charge / bond channels) ----------
//   positions   pos_out = cx * pos + cp * pos_pred + sigma * eps          (ancestral; eps: masked, centre-of-mass free)
//   the rest    out     = a * base - b * P - c * (c2 * (DA - DB))         (data-prediction DPM-Solver++; c = 0: first order)
// coefficients: {cx, cp, sigma, a, b, c, c2, noise_level} by value, or row (*step) * stride + col of a device table
// (captured HIP graphs).  Products are rounded one by one in the order of the framework expressions.
namespace {
struct DpmCoef { float cx, cp, sigma, a, b, c, c2, nl; };

__device__ __forceinline__ DpmCoef dpm_coef(DpmCoef k, const float* tab, const int* step, int stride, int col) {
    if (tab) {
        const float* r = tab + (size_t)(*step) * stride + col;
        k.cx = r[0]; k.cp = r[1]; k.sigma = r[2]; k.a = r[3]; k.b = r[4]; k.c = r[5]; k.c2 = r[6]; k.nl = r[7];
    }
    return k;
}
__device__ __forceinline__ float dpm_value(const DpmCoef& k, float base, float p, float da, float db) {
    float v = __fsub_rn(__fmul_rn(k.a, base), __fmul_rn(k.b, p));
    if (k.c != 0.f) {
        float d = __fsub_rn(da, db);
        if (k.c2 != 1.f) d = __fmul_rn(k.c2, d);
        v = __fsub_rn(v, __fmul_rn(k.c, d));
    }
    return v;
}

// one workgroup per molecule, node tensor [N, F]
__global__ __launch_bounds__(256) void k_dpm_nodes(int N, int F, const int* __restrict__ n_nodes, DpmCoef k, const float* __restrict__ tab,
                                                   const int* __restrict__ step, int stride, int col, const float* __restrict__ x_pos,
                                                   const float* __restrict__ x_base, const float* __restrict__ P,
                                                   const float* __restrict__ DA, const float* __restrict__ DB,
                                                   const float* __restrict__ PP, const float* __restrict__ eps_pos,
                                                   Rng rng, float* __restrict__ out) {
    const int b = blockIdx.x, n = n_nodes[b];
    k = dpm_coef(k, tab, step, stride, col);
    const unsigned draw = rng.on ? rng_draw(rng, tab ? step : nullptr) : 0u;
    __shared__ float red[3][256];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (k.sigma != 0.f)
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            float ev[3];
            if (rng.on) rng_pos3(rng, draw, (size_t)b * N + i, ev);
            else { const float* e = eps_pos + ((size_t)b * N + i) * 3; ev[0] = e[0]; ev[1] = e[1]; ev[2] = e[2]; }
            s0 += ev[0]; s1 += ev[1]; s2 += ev[2];
        }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
            red[2][threadIdx.x] += red[2][threadIdx.x + w];
        }
        __syncthreads();
    }
    const float inv = 1.f / (float)n;
    const float m[3] = {red[0][0] * inv, red[1][0] * inv, red[2][0] * inv};
    for (int idx = threadIdx.x; idx < N * F; idx += blockDim.x) {
        const int i = idx / F, f = idx % F;
        const size_t g = (size_t)b * N * F + idx;
        float v;
        if (f < 3) {
            v = __fadd_rn(__fmul_rn(k.cx, x_pos[g]), __fmul_rn(k.cp, PP[g]));
            if (k.sigma != 0.f) {                               // last update of a round: no noise (last_step)
                float e = 0.f;
                if (i < n) {
                    if (rng.on) { float ev[3]; rng_pos3(rng, draw, (size_t)b * N + i, ev); e = ev[f] - m[f]; }
                    else e = eps_pos[((size_t)b * N + i) * 3 + f] - m[f];
                }
                v = __fadd_rn(v, __fmul_rn(k.sigma, e));
            }
        } else {
            v = dpm_value(k, x_base[g], P[g], DA[g], DB[g]);
        }
        out[g] = v;
    }
}

__global__ __launch_bounds__(256) void k_dpm_edges(size_t tot, DpmCoef k, const float* __restrict__ tab, const int* __restrict__ step,
                                                   int stride, int col, const float* __restrict__ base, const float* __restrict__ P,
                                                   const float* __restrict__ DA, const float* __restrict__ DB, float* __restrict__ out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tot) return;
    k = dpm_coef(k, tab, step, stride, col);
    out[g] = dpm_value(k, base[g], P[g], DA[g], DB[g]);
}

__global__ void k_step_begin_at(int B, const float* __restrict__ tab, const int* __restrict__ step, int stride, int col,
                                float* __restrict__ noise_level) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) noise_level[b] = tab[(size_t)(*step) * stride + col + 7];
}
}  // namespace

namespace {
int dpm_update_launch(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef8_host,
                      const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, Rng rng, const float* x_pos,
                      const float* x_base, const float* edge_base, const float* P, const float* eP, const float* DA, const float* eDA,
                      const float* DB, const float* eDB, const float* PP, const float* eps_pos, float* x_out, float* edge_out,
                      void* stream) {
    if (B <= 0 || N <= 0 || node_feats < 4 || edge_ch < 1) return jodo_set_error(JODO_ERR_ARG, "dpm_update: bad shape");
    if (!n_nodes_dev || !x_pos || !x_base || !edge_base || !P || !eP || !DA || !eDA || !DB || !eDB || !PP || !x_out || !edge_out)
        return jodo_set_error(JODO_ERR_ARG, "dpm_update: null argument");
    if (!rng.on && !eps_pos) return jodo_set_error(JODO_ERR_ARG, "dpm_update: null noise draw");
    if ((coef8_host == nullptr) == (coef_tab_dev == nullptr) || (coef_tab_dev && !step_dev))
        return jodo_set_error(JODO_ERR_ARG, "dpm_update: pass either host coefficients or a device table + step counter");
    DpmCoef k{0, 0, 0, 0, 0, 0, 1, 0};
    if (coef8_host) k = DpmCoef{coef8_host[0], coef8_host[1], coef8_host[2], coef8_host[3], coef8_host[4], coef8_host[5], coef8_host[6], coef8_host[7]};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dpm_nodes, dim3(B), dim3(256), 0, st, N, node_feats, n_nodes_dev, k, coef_tab_dev, step_dev, tab_stride, tab_col,
                       x_pos, x_base, P, DA, DB, PP, eps_pos, rng, x_out);
    int rc = jodo_check_launch("k_dpm_nodes");
    if (rc != JODO_OK) return rc;
    const size_t tot = (size_t)B * N * N * edge_ch;
    hipLaunchKernelGGL(k_dpm_edges, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, tot, k, coef_tab_dev, step_dev, tab_stride,
                       tab_col, edge_base, eP, eDA, eDB, edge_out);
    return jodo_check_launch("k_dpm_edges");
}
}  // namespace

extern "C" int jodo_dpm_update(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef8_host,
                               const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, const float* x_pos,
                               const float* x_base, const float* edge_base, const float* P, const float* eP, const float* DA,
                               const float* eDA, const float* DB, const float* eDB, const float* PP, const float* eps_pos,
                               float* x_out, float* edge_out, void* stream) {
    return dpm_update_launch(B, N, node_feats, edge_ch, n_nodes_dev, coef8_host, coef_tab_dev, step_dev, tab_stride, tab_col, kNoRng,
                             x_pos, x_base, edge_base, P, eP, DA, eDA, DB, eDB, PP, eps_pos, x_out, edge_out, stream);
}

extern "C" int jodo_dpm_update_rng(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef8_host,
                                   const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, uint64_t seed,
                                   uint32_t draw, uint32_t draw_mul, const float* x_pos, const float* x_base, const float* edge_base,
                                   const float* P, const float* eP, const float* DA, const float* eDA, const float* DB,
                                   const float* eDB, const float* PP, float* x_out, float* edge_out, void* stream) {
    return dpm_update_launch(B, N, node_feats, edge_ch, n_nodes_dev, coef8_host, coef_tab_dev, step_dev, tab_stride, tab_col,
                             Rng{seed, draw, draw_mul, 1}, x_pos, x_base, edge_base, P, eP, DA, eDA, DB, eDB, PP, nullptr, x_out,
                             edge_out, stream);
}

extern "C" int jodo_step_begin_at(int B, const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col,
                                  float* noise_level_out, void* stream) {
    if (B <= 0 || !coef_tab_dev || !step_dev || !noise_level_out) return jodo_set_error(JODO_ERR_ARG, "step_begin_at: bad argument");
    hipLaunchKernelGGL(k_step_begin_at, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, coef_tab_dev, step_dev, tab_stride,
                       tab_col, noise_level_out);
    return jodo_check_launch("k_step_begin_at");
}

// ---- DPM-Solver++ update of the 2-D models (jodo_dpm_update_2d): the data-prediction update of jodo_dpm_update on a node tensor
// [B,N,nd] WITHOUT position channels and the edge tensor [B,N,N,ch]; no ancestral part, so nothing is drawn and the coefficient row
// {a, b, c, c2, -, -, -, noise_level} has no sigma (noise_level stays in column 7: jodo_step_begin_at reads it unchanged).  ONE launch
// over two index ranges: a thread of the first owns the four node channels 4q .. 4q+3 of one atom; a thread of the second owns one
// entry (r >= c) of the lower triangle of one molecule — for r > c it computes every channel ONCE from cell (b, r, c) and stores the
// value to (b, r, c) and (b, c, r), so the output is symmetric bit for bit whatever the upper triangle of the inputs holds; for r == c it
// stores the diagonal's zeros.  Padded atoms and cells get exact zeros.  Every output element is written by exactly one thread with
// plain stores, and a thread reads only elements it also writes: an output may be one of its own inputs (in-place update), hence no
// __restrict__ on the tensors.
namespace {
__device__ __forceinline__ DpmCoef dpm2d_coef(DpmCoef k, const float* __restrict__ tab, const int* __restrict__ step, int stride, int col) {
    if (tab) {
        const float* r = tab + (size_t)(*step) * stride + col;
        k.a = r[0]; k.b = r[1]; k.c = r[2]; k.c2 = r[3];
    }
    return k;
}

// dpm_value with contraction switched off for the function: the __f*_rn intrinsics are plain operators to this compiler (compiled
// under its default -ffp-contract=fast, so a product may still be fused into the following sum: v_fma_f32); here every product and
// every sum is rounded on its own, in the order of the framework expression a * base - b * P - c * (c2 * (DA - DB)), so the result equals it bit for bit
__device__ __forceinline__ float dpm_value_2d(const DpmCoef& k, float base, float p, float da, float db) {
#pragma clang fp contract(off)
    const float t0 = k.a * base, t1 = k.b * p;           // plain operators: the pragma governs the operations written in this function
    float v = t0 - t1;
    if (k.c != 0.f) {
        float d = da - db;
        if (k.c2 != 1.f) d = k.c2 * d;
        const float t2 = k.c * d;
        v = v - t2;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_dpm_2d(int B, int N, int nd, int ch, const int* __restrict__ n_nodes, DpmCoef k,
                                                const float* __restrict__ tab, const int* __restrict__ step, int stride, int col,
                                                const float* x_base, const float* e_base, const float* P, const float* eP,
                                                const float* DA, const float* eDA, const float* DB, const float* eDB, float* x_out,
                                                float* e_out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = (nd + 3) >> 2;
    const size_t tri = (size_t)N * (N + 1) / 2;
    const size_t n_quad = (size_t)B * N * nq, n_tri = (size_t)B * tri;
    if (g >= n_quad + n_tri) return;
    k = dpm2d_coef(k, tab, step, stride, col);
    if (g < n_quad) {
        const int q = (int)(g % nq);
        const size_t atom = g / nq;
        const int i = (int)(atom % N), b = (int)(atom / N);
        const bool real = i < n_nodes[b];
        const int k1 = min(4 * q + 4, nd);
        for (int f = 4 * q; f < k1; ++f) {
            const size_t o = atom * nd + f;
            x_out[o] = real ? dpm_value_2d(k, x_base[o], P[o], DA[o], DB[o]) : 0.f;
        }
    } else {
        const size_t pg = g - n_quad;
        const int b = (int)(pg / tri);
        const size_t t = pg % tri;
        // row of triangle entry t: the largest r with r (r + 1) / 2 <= t; the float root is corrected to the exact integer
        int r = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
        r = min(max(r, 0), N - 1);
        while ((size_t)r * (r + 1) / 2 > t) --r;
        while ((size_t)(r + 1) * (r + 2) / 2 <= t) ++r;
        const int c = (int)(t - (size_t)r * (r + 1) / 2);
        const int n = n_nodes[b];
        const size_t lo = (((size_t)b * N + r) * N + c) * ch;           // cell (b, r, c): the one that is read
        if (r == c) {
            for (int f = 0; f < ch; ++f) e_out[lo + f] = 0.f;
            return;
        }
        const size_t up = (((size_t)b * N + c) * N + r) * ch;           // its mirror (b, c, r)
        const bool real = r < n;                                        // c < r
        for (int f = 0; f < ch; ++f) {
            const float v = real ? dpm_value_2d(k, e_base[lo + f], eP[lo + f], eDA[lo + f], eDB[lo + f]) : 0.f;
            e_out[lo + f] = v;
            e_out[up + f] = v;
        }
    }
}
}  // namespace

extern "C" int jodo_dpm_update_2d(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef8_host,
                                  const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, const float* x_base,
                                  const float* edge_base, const float* P, const float* eP, const float* DA, const float* eDA,
                                  const float* DB, const float* eDB, float* x_out, float* edge_out, void* stream) {
    if (B <= 0 || N <= 0 || node_feats < 1 || edge_ch < 1) return jodo_set_error(JODO_ERR_ARG, "dpm_update_2d: bad shape");
    if (!n_nodes_dev || !x_base || !edge_base || !P || !eP || !DA || !eDA || !DB || !eDB || !x_out || !edge_out)
        return jodo_set_error(JODO_ERR_ARG, "dpm_update_2d: null argument");
    if ((coef8_host == nullptr) == (coef_tab_dev == nullptr) || (coef_tab_dev && !step_dev))
        return jodo_set_error(JODO_ERR_ARG, "dpm_update_2d: pass either host coefficients or a device table + step counter");
    if (coef_tab_dev && (tab_stride < 8 || tab_col < 0 || tab_col + 8 > tab_stride))
        return jodo_set_error(JODO_ERR_ARG, "dpm_update_2d: the 8 columns from tab_col do not fit a table row of tab_stride floats");
    DpmCoef k{0, 0, 0, 0, 0, 0, 1, 0};
    if (coef8_host) { k.a = coef8_host[0]; k.b = coef8_host[1]; k.c = coef8_host[2]; k.c2 = coef8_host[3]; }
    const size_t tot = (size_t)B * N * ((node_feats + 3) / 4) + (size_t)B * ((size_t)N * (N + 1) / 2);
    if ((tot + 255) / 256 > 0x7fffffffull) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dpm_update_2d: batch too large for one launch");
    hipLaunchKernelGGL(k_dpm_2d, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, N, node_feats, edge_ch,
                       n_nodes_dev, k, coef_tab_dev, step_dev, tab_stride, tab_col, x_base, edge_base, P, eP, DA, eDA, DB, eDB, x_out,
                       edge_out);
    return jodo_check_launch("k_dpm_2d");
}

// ---- noise prediction -> data prediction for the 2-D models (jodo_eps_to_data_2d): DPM_Solver_2D on a noise-predicting network (CDGS)
// turns every network output eps into d = (x - sigma * eps) / alpha before the data-prediction update above.  (alpha, sigma) by value,
// or columns tab_col + 5 / tab_col + 6 of row *step of a device table: the noise-form rows {a, b, c, c2, t, alpha_t, sigma_t,
// noise_level} fill the three columns that k_dpm_2d does not read.  The index ranges, the ownership of elements and hence the aliasing
// rule are k_dpm_2d's: a thread of the first range owns four node channels of one atom, a thread of the second one entry (r >= c) of
// the lower triangle of one molecule, computed once from cell (b, r, c) and stored to both orientations; zeros on the diagonal and on
// padding; every output element written by exactly one thread with plain stores; a thread reads only elements it also writes, so d_x
// may be x or eps_x and d_e may be edge_x or eps_e (no __restrict__ on the tensors).
namespace {
// __fmul_rn, __fsub_rn, __fdiv_rn in that order: three operations, each rounded on its own, as the framework expression
// (x - sigma * eps) / alpha rounds them.  Written with plain operators under contract(off), as dpm_value_2d is: the intrinsics are
// inline functions of the runtime's headers, compiled under the default -ffp-contract=fast, and the pragma governs only the operations
// written in THIS function — with the intrinsics the product went into the difference as one v_fma_f32.  The quotient is the
// compiler's correctly rounded fp32 division (v_div_scale / v_div_fmas / v_div_fixup), fp32 denormals kept.
__device__ __forceinline__ float eps_to_data(float alpha, float sigma, float x, float eps) {
#pragma clang fp contract(off)
    const float t0 = sigma * eps;
    const float t1 = x - t0;
    return t1 / alpha;
}

__global__ __launch_bounds__(256) void k_eps_to_data_2d(int B, int N, int nd, int ch, const int* __restrict__ n_nodes, float alpha,
                                                        float sigma, const float* __restrict__ tab, const int* __restrict__ step,
                                                        int stride, int col, const float* x, const float* e, const float* eps_x,
                                                        const float* eps_e, float* d_x, float* d_e) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = (nd + 3) >> 2;
    const size_t tri = (size_t)N * (N + 1) / 2;
    const size_t n_quad = (size_t)B * N * nq, n_tri = (size_t)B * tri;
    if (g >= n_quad + n_tri) return;
    if (tab) {
        const float* r = tab + (size_t)(*step) * stride + col;
        alpha = r[5]; sigma = r[6];
    }
    if (g < n_quad) {
        const int q = (int)(g % nq);
        const size_t atom = g / nq;
        const int i = (int)(atom % N), b = (int)(atom / N);
        const bool real = i < n_nodes[b];
        const int k1 = min(4 * q + 4, nd);
        for (int f = 4 * q; f < k1; ++f) {
            const size_t o = atom * nd + f;
            d_x[o] = real ? eps_to_data(alpha, sigma, x[o], eps_x[o]) : 0.f;
        }
    } else {
        const size_t pg = g - n_quad;
        const int b = (int)(pg / tri);
        const size_t t = pg % tri;
        // row of triangle entry t, as in k_dpm_2d: the float root corrected to the exact integer
        int r = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
        r = min(max(r, 0), N - 1);
        while ((size_t)r * (r + 1) / 2 > t) --r;
        while ((size_t)(r + 1) * (r + 2) / 2 <= t) ++r;
        const int c = (int)(t - (size_t)r * (r + 1) / 2);
        const size_t lo = (((size_t)b * N + r) * N + c) * ch;           // cell (b, r, c): the one that is read
        if (r == c) {
            for (int f = 0; f < ch; ++f) d_e[lo + f] = 0.f;
            return;
        }
        const size_t up = (((size_t)b * N + c) * N + r) * ch;           // its mirror (b, c, r)
        const bool real = r < n_nodes[b];                               // c < r
        for (int f = 0; f < ch; ++f) {
            const float v = real ? eps_to_data(alpha, sigma, e[lo + f], eps_e[lo + f]) : 0.f;
            d_e[lo + f] = v;
            d_e[up + f] = v;
        }
    }
}

__global__ void k_step_begin_t(int B, const float* __restrict__ tab, const int* __restrict__ step, int stride, int col,
                               float* __restrict__ t_out, float* __restrict__ noise_level) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* r = tab + (size_t)(*step) * stride + col;
    t_out[b] = r[4];
    if (noise_level) noise_level[b] = r[7];
}
}  // namespace

extern "C" int jodo_eps_to_data_2d(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float alpha, float sigma,
                                   const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, const float* x,
                                   const float* edge_x, const float* eps_x, const float* eps_e, float* d_x, float* d_e, void* stream) {
    if (B <= 0 || N <= 0 || node_feats < 1 || edge_ch < 1) return jodo_set_error(JODO_ERR_ARG, "eps_to_data_2d: bad shape");
    if (!n_nodes_dev || !x || !edge_x || !eps_x || !eps_e || !d_x || !d_e) return jodo_set_error(JODO_ERR_ARG, "eps_to_data_2d: null argument");
    if ((coef_tab_dev == nullptr) != (step_dev == nullptr))
        return jodo_set_error(JODO_ERR_ARG, "eps_to_data_2d: pass both the device table and the step counter, or neither");
    if (coef_tab_dev && (tab_stride < 8 || tab_col < 0 || tab_col + 8 > tab_stride))
        return jodo_set_error(JODO_ERR_ARG, "eps_to_data_2d: the 8 columns from tab_col do not fit a table row of tab_stride floats");
    if (edge_ch > 4 || node_feats > 256)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "eps_to_data_2d: at most 4 edge channels and 256 node channels");
    const size_t tot = (size_t)B * N * ((node_feats + 3) / 4) + (size_t)B * ((size_t)N * (N + 1) / 2);
    if ((tot + 255) / 256 > 0x7fffffffull) return jodo_set_error(JODO_ERR_UNSUPPORTED, "eps_to_data_2d: batch too large for one launch");
    hipLaunchKernelGGL(k_eps_to_data_2d, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, N, node_feats, edge_ch,
                       n_nodes_dev, alpha, sigma, coef_tab_dev, step_dev, tab_stride, tab_col, x, edge_x, eps_x, eps_e, d_x, d_e);
    return jodo_check_launch("k_eps_to_data_2d");
}

extern "C" int jodo_step_begin_t(int B, const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, float* t_out,
                                 float* noise_level_out, void* stream) {
    if (B <= 0 || !coef_tab_dev || !step_dev || !t_out) return jodo_set_error(JODO_ERR_ARG, "step_begin_t: bad argument");
    if (tab_stride < 8 || tab_col < 0 || tab_col + 8 > tab_stride)
        return jodo_set_error(JODO_ERR_ARG, "step_begin_t: the 8 columns from tab_col do not fit a table row of tab_stride floats");
    hipLaunchKernelGGL(k_step_begin_t, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, coef_tab_dev, step_dev, tab_stride,
                       tab_col, t_out, noise_level_out);
    return jodo_check_launch("k_step_begin_t");
}

// ---- the property prior's draw (jodo_prop_sample; contract in include/jodo_hip.h): one thread per (molecule, property) ------------
// Per thread: one Philox evaluation (or two words of the test form), a binary search over one row of the cumulative table (at most
// 17 dependent 4-byte loads: n_bins <= 65536) and the reference's bin -> value expression.  tests/prop_dist_common.py restates it.
namespace {
enum { RNG_PROP = 3 };

// the reference's _idx2value + normalize_tensor (cond_gen/property_distribution.py:69-73, :93-98) with u2 for torch.rand.  Plain
// operators under contract(off), as eps_to_data above: every product, sum and quotient is rounded on its own.  fl32(idx / n_bins):
// the reference forms the quotient in double and the product rounds it to fp32; for integers below 2^24 that double rounding is
// innocuous (53 >= 2 * 24 + 2 bits), so the correctly rounded fp32 quotient is the same number.
__device__ __forceinline__ float prop_value(unsigned idx, int n_bins, float mn, float mx, float u2, float mean, float mad) {
#pragma clang fp contract(off)
    const float range = mx - mn;
    const float fl = (float)idx / (float)n_bins;
    const float fr = (float)(idx + 1u) / (float)n_bins;
    const float tl = fl * range;
    const float left = tl + mn;
    const float tr = fr * range;
    const float right = tr + mn;
    const float width = right - left;
    const float t = u2 * width;
    const float val = t + left;
    const float c = val - mean;
    return c / mad;
}

__global__ __launch_bounds__(256) void k_prop_sample(int B, int n_prop, int n_bins, int n_slots, const unsigned* __restrict__ cum,
                                                     const float* __restrict__ minmax, const float* __restrict__ norm,
                                                     const int* __restrict__ slots, const long long* __restrict__ indices,
                                                     unsigned long long first_index, unsigned long long seed,
                                                     const unsigned* __restrict__ words, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * n_prop) return;
    const int b = (int)(t / n_prop), p = (int)(t % n_prop);
    const int slot = slots[b];
    if (slot < 0 || slot >= n_slots) { out[t] = __int_as_float(0x7fc00000); return; }   // (the host entry has refused it already)
    unsigned w0, w1;
    if (words) { w0 = words[2 * t]; w1 = words[2 * t + 1]; }
    else {
        const unsigned long long g = indices ? (unsigned long long)indices[b] : first_index + (unsigned long long)b;
        unsigned w[4];
        philox4x32_10((unsigned)g, (unsigned)(g >> 32), (unsigned)p, RNG_PROP, (unsigned)seed, (unsigned)(seed >> 32), w);
        w0 = w[0]; w1 = w[1];
    }
    const size_t row = (size_t)p * n_slots + slot;
    const unsigned* c = cum + row * n_bins;
    const unsigned T = c[n_bins - 1];
    const unsigned r = (unsigned)(((unsigned long long)(w0 >> 8) * T) >> 24);         // r < T
    int lo = 0, hi = n_bins - 1;                              // the smallest bin whose cumulative weight exceeds r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] > r) hi = mid; else lo = mid + 1;
    }
    const float u2 = (float)(w1 >> 8) * (1.0f / 16777216.0f);
    out[t] = prop_value((unsigned)lo, n_bins, minmax[2 * row], minmax[2 * row + 1], u2, norm[2 * p], norm[2 * p + 1]);
}
}  // namespace

extern "C" int jodo_prop_sample(int B, int n_prop, int n_bins, int n_slots, const uint32_t* cum_dev, const float* minmax_dev,
                                const float* norm_dev, const int32_t* slots_host, const int32_t* slots_dev, const int64_t* indices_dev,
                                uint64_t first_index, uint64_t seed, const uint32_t* words_dev, float* out, void* stream) {
    if (B < 1 || n_prop < 1 || n_bins < 1 || n_slots < 1) return jodo_set_error(JODO_ERR_ARG, "prop_sample: bad shape");
    if (!cum_dev || !minmax_dev || !norm_dev || !slots_host || !slots_dev || !out)
        return jodo_set_error(JODO_ERR_ARG, "prop_sample: null argument");
    if (n_prop > JODO_PROP_MAX_PROPS) return jodo_set_error(JODO_ERR_UNSUPPORTED, "prop_sample: at most 16 properties");
    if (n_bins > JODO_PROP_MAX_BINS) return jodo_set_error(JODO_ERR_UNSUPPORTED, "prop_sample: at most 65536 bins");
    for (int b = 0; b < B; ++b)
        if (slots_host[b] < 0 || slots_host[b] >= n_slots) return jodo_set_error(JODO_ERR_ARG, "prop_sample: slot outside the table");
    const size_t tot = (size_t)B * n_prop;
    hipLaunchKernelGGL(k_prop_sample, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, n_prop, n_bins, n_slots,
                       cum_dev, minmax_dev, norm_dev, slots_dev, (const long long*)indices_dev, (unsigned long long)first_index,
                       (unsigned long long)seed, words_dev, out);
    return jodo_check_launch("k_prop_sample");
}

extern "C" int jodo_decode(int B, int N, int atom_types, int include_fc, int edge_ch, int compress_edge, int centered,
                           float pos_norm, float atom_norm, float fc_norm, float edge_norm, const int32_t* n_nodes_dev,
                           const float* xh, const float* edge_x, float* pos_out, uint8_t* atom_type_out, int8_t* fc_out,
                           uint8_t* edge_type_out, void* stream) {
    if (B <= 0 || N <= 0 || atom_types < 1 || atom_types > 255 || edge_ch < 1 || edge_ch > 4)
        return jodo_set_error(JODO_ERR_ARG, "decode: bad shape");
    if (!n_nodes_dev || !xh || !edge_x || !pos_out || !atom_type_out || !fc_out || !edge_type_out)
        return jodo_set_error(JODO_ERR_ARG, "decode: null argument");
    DecodeArgs A{B, N, atom_types, include_fc, edge_ch, compress_edge, centered, pos_norm, atom_norm, fc_norm, edge_norm};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_decode_nodes<3>, dim3((B * N + 255) / 256), dim3(256), 0, st, A, n_nodes_dev, xh, pos_out, atom_type_out, fc_out);
    int rc = jodo_check_launch("k_decode_nodes");
    if (rc != JODO_OK) return rc;
    const size_t tot = (size_t)B * N * N;
    hipLaunchKernelGGL(k_decode_edges, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, A, n_nodes_dev, edge_x, edge_type_out);
    return jodo_check_launch("k_decode_edges");
}

extern "C" int jodo_decode_2d(int B, int N, int atom_types, int include_fc, int edge_ch, int compress_edge, int centered, float atom_norm,
                              float fc_norm, float edge_norm, const int32_t* n_nodes_dev, const float* xh, const float* edge_x,
                              uint8_t* atom_type_out, int8_t* fc_out, uint8_t* edge_type_out, void* stream) {
    if (B <= 0 || N <= 0 || atom_types < 1 || atom_types > 255 || edge_ch < 1 || edge_ch > 4)
        return jodo_set_error(JODO_ERR_ARG, "decode_2d: bad shape");
    if (!n_nodes_dev || !xh || !edge_x || !atom_type_out || !fc_out || !edge_type_out)
        return jodo_set_error(JODO_ERR_ARG, "decode_2d: null argument");
    DecodeArgs A{B, N, atom_types, include_fc, edge_ch, compress_edge, centered, 1.f, atom_norm, fc_norm, edge_norm};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_decode_nodes<0>, dim3((B * N + 255) / 256), dim3(256), 0, st, A, n_nodes_dev, xh, (float*)nullptr, atom_type_out,
                       fc_out);
    int rc = jodo_check_launch("k_decode_nodes");
    if (rc != JODO_OK) return rc;
    const size_t tot = (size_t)B * N * N;
    hipLaunchKernelGGL(k_decode_edges, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, A, n_nodes_dev, edge_x, edge_type_out);
    return jodo_check_launch("k_decode_edges");
}

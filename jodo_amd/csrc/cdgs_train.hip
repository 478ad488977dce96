// Training step of the CDGS noise-prediction network behind the C ABI (include/jodo_hip.h, "CDGS training"): jodo_cdgs_train_forward
// evaluates the network with every activation the backward needs kept in the caller's workspace (dropout active when p > 0, as under
// model.train()), jodo_cdgs_train_backward returns d loss / d parameter for every parameter of the state_dict given d loss / d outputs.
//
// Layout: the reference's own dense padded tensors.  Node row = b N + i, edge row = (b N + r) N + c, padded and diagonal rows included,
// masks applied where the reference applies them.  The reference normalises the edge state over the PADDED tile (8 channels x N x N
// positions per group), and under model.train() draws the edge feed-forward's dropout masks at every one of the N x N positions, so the
// edge feed-forward, its residual and norm2_edge run over all B N^2 rows for every dropout probability; gates, attention and GINE walk
// the same tile under the mask.  The flat index of an element of these tensors is the reference's own, which is the dropout numbering:
// site = 8 l + {1 h_local, 2 h_attn, 3 node FF hidden, 4 node FF out, 5 edge FF hidden, 6 edge FF out}, element = row * width + f.
//
// Every projection and both of its gradient products are jt::gemm (train_gemm.hip); everything else is below, in the style of
// train_ops.h: one thread per output element or per reduced (row | atom | molecule, feature), plain loops in a fixed order, no LDS, no
// barriers, no atomics: bit-deterministic, and the host emulation build of the CPU suite runs these very kernels.
// Gradient buffers are fully written (zeroed, then accumulated in a fixed launch order).  No gradient flows through the random-walk
// features or the thresholded adjacency (torch.no_grad in the reference); the GINE eps buffers are inputs without a gradient.
// Tests: jodo_cdgs_train_debug_op (at the end) runs one launch sequence of the step ("launch sequences" below) on caller-owned arrays.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <unordered_map>
#include <vector>

#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"
#include "train_gemm.h"
#include "cdgs_common.h"
#define JT_OPS_NS jtc         // this translation unit's own copy of the train_ops.h kernels
#include "train_ops.h"

using namespace jt;
using namespace jtc;

namespace {

constexpr int COLSUM_PER = 32;    // chunks per group of the column sums' second level
constexpr int GW = 8;             // channels per GroupNorm group (nf / min(nf / 4, 32) at nf = 256)

struct Lin { int w = -1, b = -1; };
struct BlkIx {
    Lin t_node, t_edge, gin0, gin2, key, query, value, ff1, ff2, ff3, ff4, nl, na, nn, ne, ro_n, ro_e;    // (the norms: w = weight, b = bias)
    int le0 = -1, le1 = -1, eps = -1;
};

struct Arena {
    char* base; size_t off;
    float* f(size_t n) { const size_t o = off; off += (n * 4 + 255) / 256 * 256; return base ? reinterpret_cast<float*>(base + o) : nullptr; }
};

struct BlkBuf {
    float *te, *tn, *hs, *agg, *g1, *xh1, *rs1, *xh2, *rs2, *xh3, *rs3, *q, *k, *v, *t0, *t1, *alpha, *hc, *f1p, *a1, *f3p, *a3, *xhe, *rse;
};
struct HeadBuf { float *p1, *a1, *p2, *a2; };
struct Bufs {
    float *tin, *t1p, *t1a, *temb, *tact;
    float *adj, *AD, *pa, *pb, *cnt, *onehot, *land, *deg, *ein, *nin, *ahid, *bhid, *a3, *Ep;
    std::vector<float*> h, e;
    std::vector<BlkBuf> blk;
    HeadBuf hd[3];                 // atom | bond | exist
    float *sE[5], *sE_F, *sE_H, *sN[6], *sN_F, *sB[2], *dtact, *dein, *dnin, *dah, *dbh, *dEp, *da3, *part, *gsum, *splitk;
    size_t splitk_floats;
};

// batch geometry: everything else follows from the row index
struct Geo { int B, N; const int* nn; };
__device__ __forceinline__ bool node_live(const Geo& g, long row) { return (int)(row % g.N) < g.nn[row / g.N]; }
__device__ __forceinline__ bool edge_live(const Geo& g, long row) {
    const int c = (int)(row % g.N), r = (int)((row / g.N) % g.N), n = g.nn[row / ((long)g.N * g.N)];
    return r < n && c < n && r != c;
}
// mode 0: every row; 1: node rows inside the molecule; 2: edge rows of real ordered pairs
__device__ __forceinline__ bool row_live(const Geo& g, int mode, long row) { return mode == 0 || (mode == 1 ? node_live(g, row) : edge_live(g, row)); }

// ================================================================ prologue ====================================================
__global__ void kc_time(int B, int D, const float* __restrict__ t, const float* __restrict__ freq, float* __restrict__ tin) {
    JT_IDX((long)B * D);
    tin[i_] = jcdgs::sinusoid(t[i_ / D], freq, (int)(i_ % D), D / 2);
}
__global__ void kc_adj(Geo g, int ch, const float* __restrict__ edge_x, float* __restrict__ adj) {
    JT_IDX((long)g.B * g.N * g.N);
    adj[i_] = jcdgs::adjacent(edge_live(g, i_), edge_x[i_ * ch]) ? 1.f : 0.f;
}
// AD = adj / (deg + 1e-8); the first power and the walk counters
__global__ void kc_adnorm(Geo g, const float* __restrict__ adj, float* __restrict__ AD, float* __restrict__ pa, float* __restrict__ cnt) {
    JT_IDX((long)g.B * g.N * g.N);
    const long row0 = i_ / g.N * g.N;
    float s = 0.f;
    for (int c = 0; c < g.N; ++c) s += adj[row0 + c];
    const float v = adj[i_] / (s + 1e-8f);
    AD[i_] = v; pa[i_] = v; cnt[i_] = 0.f;
}
// dst = src AD (power m + 2); its diagonal is landing probability m, the pairs it leaves without a walk are counted
__global__ void kc_rw_step(Geo g, int K, int m, const float* __restrict__ src, const float* __restrict__ AD, float* __restrict__ dst,
                           float* __restrict__ cnt, float* __restrict__ land) {
    JT_IDX((long)g.B * g.N * g.N);
    const int N = g.N, c = (int)(i_ % N), r = (int)((i_ / N) % N);
    const long b = i_ / ((long)N * N), base = b * N * N;
    float s = 0.f;
    for (int k = 0; k < N; ++k) s = fmaf(src[base + (long)r * N + k], AD[base + (long)k * N + c], s);
    dst[i_] = s;
    if (s <= 0.f) cnt[i_] += 1.f;
    if (r == c) land[(b * N + r) * K + m] = s;
}
__global__ void kc_onehot(long R, int K1, const float* __restrict__ cnt, float* __restrict__ onehot) {
    JT_IDX(R * K1);
    onehot[i_] = (int)cnt[i_ / K1] == (int)(i_ % K1) ? 1.f : 0.f;
}
// the reference sums edge_x over the whole padded row, unmasked
__global__ void kc_deg(Geo g, int ch, const float* __restrict__ edge_x, float* __restrict__ deg) {
    JT_IDX((long)g.B * g.N * ch);
    const long row = i_ / ch; const int k = (int)(i_ % ch);
    float s = 0.f;
    for (int j = 0; j < g.N; ++j) s += edge_x[(row * g.N + j) * ch + k];
    deg[i_] = s;
}

// ================================================================ elementwise =================================================
// dst[row, f] (+)= src[row, f] * dropout(row F + f) * mask(row)      (dst may alias src when acc = 0)
__global__ void kc_scale(Geo g, int mode, long rows, int F, const float* src, Drop d, float* dst, int acc) {
    JT_IDX(rows * F);
    const float v = row_live(g, mode, i_ / F) ? src[i_] * drop_mul(d, (unsigned long long)i_) : 0.f;
    dst[i_] = acc ? dst[i_] + v : v;
}
// out = (x + tb[molecule]) * mask
__global__ void kc_addt(Geo g, int mode, long rows, int F, const float* __restrict__ x, const float* __restrict__ tb, float* __restrict__ out) {
    JT_IDX(rows * F);
    const long row = i_ / F;
    const long b = mode == 1 ? row / g.N : row / ((long)g.N * g.N);
    out[i_] = row_live(g, mode, row) ? x[i_] + tb[b * F + i_ % F] : 0.f;
}
// tests: the multipliers of rows row0 .. row0 + rows - 1 of a [., F] tensor, element index row * F + f as kc_scale and the GEMM epilogue form it
__global__ void kc_drop_rows(long row0, long rows, int F, Drop d, float* __restrict__ out) {
    JT_IDX(rows * F);
    const long row = row0 + i_ / F;
    out[i_] = drop_mul(d, (unsigned long long)(row * F + i_ % F));
}
__global__ void kc_relu(long n, const float* x, float* y) {
    JT_IDX(n);
    y[i_] = fmaxf(x[i_], 0.f);
}
__global__ void kc_relu_bwd(long n, const float* __restrict__ y, float* __restrict__ d) {
    JT_IDX(n);
    if (!(y[i_] > 0.f)) d[i_] = 0.f;
}
// pair[(b, r, c)] = hc[b, r] + hc[b, c]
__global__ void kc_pair(Geo g, int D, const float* __restrict__ hc, float* __restrict__ pair) {
    JT_IDX((long)g.B * g.N * g.N * D);
    const long row = i_ / D; const int f = (int)(i_ % D);
    const long c = row % g.N, br = row / g.N, b = br / g.N;
    pair[i_] = hc[br * D + f] + hc[(b * g.N + c) * D + f];
}
// dhc[b, i] (+)= sum_c dpair[b, i, c] + sum_r dpair[b, r, i]: one owner per atom and channel
__global__ void kc_pair_bwd(Geo g, int D, const float* __restrict__ dpair, float* __restrict__ dhc) {
    JT_IDX((long)g.B * g.N * D);
    const long row = i_ / D; const int f = (int)(i_ % D);
    const long b = row / g.N, i = row % g.N;
    float s = 0.f;
    for (int c = 0; c < g.N; ++c) s += dpair[(row * g.N + c) * D + f];
    for (int r = 0; r < g.N; ++r) s += dpair[((b * g.N + r) * g.N + i) * D + f];
    dhc[i_] = s;
}

// ================================================================ GINE =========================================================
// agg[b, i] = (1 + eps) hs[b, i] + sum over sources j with adj[j, i] of relu(hs[b, j] + he[b, j, i])
__global__ void kc_gine(Geo g, int D, const float* __restrict__ eps, const float* __restrict__ hs, const float* __restrict__ he,
                        const float* __restrict__ adj, float* __restrict__ agg) {
    JT_IDX((long)g.B * g.N * D);
    const long row = i_ / D; const int f = (int)(i_ % D);
    const long b = row / g.N, i = row % g.N;
    float s = (1.f + eps[0]) * hs[i_];
    for (int j = 0; j < g.N; ++j) {
        const long er = (b * g.N + j) * g.N + i;
        if (adj[er] > 0.f) s += fmaxf(hs[(b * g.N + j) * D + f] + he[er * D + f], 0.f);
    }
    agg[i_] = s;
}
// d he[b, j, i] = adj[j, i] relu'(hs_j + he_ji) dagg[b, i]     (written at every row)
__global__ void kc_gine_bwd_e(Geo g, int D, const float* __restrict__ hs, const float* __restrict__ he, const float* __restrict__ adj,
                              const float* __restrict__ dagg, float* __restrict__ dhe) {
    JT_IDX((long)g.B * g.N * g.N * D);
    const long er = i_ / D; const int f = (int)(i_ % D);
    const long i = er % g.N, bj = er / g.N, b = bj / g.N;
    float v = 0.f;
    if (adj[er] > 0.f && hs[bj * D + f] + he[i_] > 0.f) v = dagg[(b * g.N + i) * D + f];
    dhe[i_] = v;
}
// d hs[b, j] = (1 + eps) dagg[b, j] + sum_i d he[b, j, i]      (dhe as kc_gine_bwd_e left it)
__global__ void kc_gine_bwd_n(Geo g, int D, const float* __restrict__ eps, const float* __restrict__ dagg, const float* __restrict__ dhe,
                              float* __restrict__ dhs) {
    JT_IDX((long)g.B * g.N * D);
    const long row = i_ / D; const int f = (int)(i_ % D);
    float s = (1.f + eps[0]) * dagg[i_];
    for (int i = 0; i < g.N; ++i) s += dhe[(row * g.N + i) * D + f];
    dhs[i_] = s;
}

// ================================================================ per-row GroupNorm (nodes) ====================================
// x = h + a * dropout * (amask ? node mask : 1); xhat, rstd kept; y (+)= (xhat gamma + beta) * node mask.  One thread per (row, group).
__global__ void kc_gn_fwd(Geo g, long rows, int D, const float* __restrict__ h, const float* __restrict__ a, Drop d, int amask,
                          const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ xhat, float* __restrict__ rstd,
                          float* __restrict__ y, int acc) {
    const int G = D / GW;
    JT_IDX(rows * G);
    const long row = i_ / G; const int c0 = (int)(i_ % G) * GW;
    const bool live = node_live(g, row);
    float v[GW], s = 0.f;
    for (int k = 0; k < GW; ++k) {
        const long at = row * D + c0 + k;
        const float add = (amask && !live) ? 0.f : a[at] * drop_mul(d, (unsigned long long)at);
        v[k] = h[at] + add; s += v[k];
    }
    const float mean = s / GW;
    float q = 0.f;
    for (int k = 0; k < GW; ++k) { v[k] -= mean; q += v[k] * v[k]; }
    const float rs = 1.f / sqrtf(q / GW + 1e-6f);
    rstd[i_] = rs;
    for (int k = 0; k < GW; ++k) {
        const long at = row * D + c0 + k;
        const float xh = v[k] * rs, o = live ? xh * gamma[c0 + k] + beta[c0 + k] : 0.f;
        xhat[at] = xh;
        y[at] = acc ? y[at] + o : o;
    }
}
// dx (+)= rstd (gamma dy - mean(gamma dy) - xhat mean(gamma dy xhat)), dy = node mask * dyin
__global__ void kc_gn_bwd(Geo g, long rows, int D, const float* __restrict__ dyin, const float* __restrict__ xhat, const float* __restrict__ rstd,
                          const float* __restrict__ gamma, float* __restrict__ dx, int acc) {
    const int G = D / GW;
    JT_IDX(rows * G);
    const long row = i_ / G; const int c0 = (int)(i_ % G) * GW;
    const bool live = node_live(g, row);
    float gd[GW], s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < GW; ++k) {
        const long at = row * D + c0 + k;
        gd[k] = live ? gamma[c0 + k] * dyin[at] : 0.f;
        s1 += gd[k]; s2 += gd[k] * xhat[at];
    }
    s1 /= GW; s2 /= GW;
    for (int k = 0; k < GW; ++k) {
        const long at = row * D + c0 + k;
        const float v = rstd[i_] * (gd[k] - s1 - xhat[at] * s2);
        dx[at] = acc ? dx[at] + v : v;
    }
}

// ================================================================ edge GroupNorm over the padded tile ==========================
// per (molecule, tile row, group): double sums of a and a b over the N positions of the row and the group's channels, taken where
// mode says (0 every position, 2 real pairs only); b = nullptr: sums of a and a^2
__global__ void kc_egn_part(Geo g, int mode, int D, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gamma,
                            double* __restrict__ part) {
    const int G = D / GW;
    JT_IDX((long)g.B * g.N * G);
    const long br = i_ / G; const int c0 = (int)(i_ % G) * GW;
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < g.N; ++c) {
        const long er = br * g.N + c;
        if (!row_live(g, mode, er)) continue;
        for (int k = 0; k < GW; ++k) {
            const double va = (double)a[er * D + c0 + k] * (gamma ? (double)gamma[c0 + k] : 1.0);
            s1 += va; s2 += va * (b ? (double)b[er * D + c0 + k] : va);
        }
    }
    part[2 * i_] = s1; part[2 * i_ + 1] = s2;
}
// per (molecule, group): the rows' sums in order
__global__ void kc_egn_fin(Geo g, int G, const double* __restrict__ part, double* __restrict__ sums) {
    JT_IDX((long)g.B * G);
    const long b = i_ / G; const int gi = (int)(i_ % G);
    double s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < g.N; ++r) { s1 += part[2 * ((b * g.N + r) * G + gi)]; s2 += part[2 * ((b * g.N + r) * G + gi) + 1]; }
    sums[2 * i_] = s1; sums[2 * i_ + 1] = s2;
}
// x -> xhat in place over every position; e_out = (xhat gamma + beta) on real pairs, 0 elsewhere; rstd kept per (molecule, group)
__global__ void kc_egn_apply(Geo g, int D, const double* __restrict__ sums, float* __restrict__ x, const float* __restrict__ gamma,
                             const float* __restrict__ beta, float* __restrict__ rstd, float* __restrict__ eout) {
    JT_IDX((long)g.B * g.N * g.N * D);
    const int G = D / GW, f = (int)(i_ % D);
    const long er = i_ / D, bg = er / ((long)g.N * g.N) * G + f / GW;
    const double cnt = (double)GW * g.N * g.N, mean = sums[2 * bg] / cnt;
    double var = sums[2 * bg + 1] / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rs = (float)(1.0 / sqrt(var + 1e-6));
    if (er % ((long)g.N * g.N) == 0 && f % GW == 0) rstd[bg] = rs;
    const float xh = (x[i_] - (float)mean) * rs;
    x[i_] = xh;
    eout[i_] = edge_live(g, er) ? xh * gamma[f] + beta[f] : 0.f;
}
// d pre at EVERY position of the tile: rstd (gamma dy - (S1 + xhat S2) / cnt), dy = de on real pairs, 0 elsewhere; S1, S2 the sums of
// gamma dy and gamma dy xhat over the real pairs (kc_egn_part mode 2 + kc_egn_fin)
__global__ void kc_egn_bwd(Geo g, int D, const double* __restrict__ sums, const float* __restrict__ de, const float* __restrict__ xhat,
                           const float* __restrict__ rstd, const float* __restrict__ gamma, float* __restrict__ dpre) {
    JT_IDX((long)g.B * g.N * g.N * D);
    const int G = D / GW, f = (int)(i_ % D);
    const long er = i_ / D, bg = er / ((long)g.N * g.N) * G + f / GW;
    const double cnt = (double)GW * g.N * g.N;
    const float m1 = (float)(sums[2 * bg] / cnt), m2 = (float)(sums[2 * bg + 1] / cnt);
    const float gd = edge_live(g, er) ? gamma[f] * de[i_] : 0.f;
    dpre[i_] = rstd[bg] * (gd - m1 - xhat[i_] * m2);
}

// ================================================================ column sums (norm weights) ===================================
// part[chunk, f] = sums over the chunk's live rows of a and of a b, in double, rows in order; 64 rows per chunk
__global__ void kc_colsum_part(Geo g, int mode, long rows, int F, const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ part) {
    const long nchunk = (rows + 63) / 64;
    JT_IDX(nchunk * F);
    const long ck = i_ / F; const int f = (int)(i_ % F);
    const long r1 = (ck + 1) * 64 < rows ? (ck + 1) * 64 : rows;
    double s1 = 0.0, s2 = 0.0;
    for (long r = ck * 64; r < r1; ++r) {
        if (!row_live(g, mode, r)) continue;
        const double va = a[r * F + f];
        s1 += va; s2 += va * (double)b[r * F + f];
    }
    part[2 * i_] = s1; part[2 * i_ + 1] = s2;
}
// second level: mid[g, f] = the sums of chunks g per .. (g + 1) per - 1 in order (doubles)
__global__ void kc_colsum_mid(long nchunk, int per, int F, const double* __restrict__ part, double* __restrict__ mid) {
    const long ngroup = (nchunk + per - 1) / per;
    JT_IDX(ngroup * F);
    const long gi = i_ / F; const int f = (int)(i_ % F);
    const long c1 = (gi + 1) * per < nchunk ? (gi + 1) * per : nchunk;
    double s1 = 0.0, s2 = 0.0;
    for (long ck = gi * per; ck < c1; ++ck) { s1 += part[2 * (ck * F + f)]; s2 += part[2 * (ck * F + f) + 1]; }
    mid[2 * i_] = s1; mid[2 * i_ + 1] = s2;
}
__global__ void kc_colsum_fin(long ngroup, int F, const double* __restrict__ mid, float* __restrict__ out1, float* __restrict__ out2) {
    JT_IDX(F);
    double s1 = 0.0, s2 = 0.0;
    for (long gi = 0; gi < ngroup; ++gi) { s1 += mid[2 * (gi * F + i_)]; s2 += mid[2 * (gi * F + i_) + 1]; }
    out1[i_] = (float)s1; out2[i_] = (float)s2;
}
// per-molecule sums of the live rows: edge rows -> [B N, F] (over the columns c), then node rows -> [B, F]
__global__ void kc_sum_cols(Geo g, int F, const float* __restrict__ x, float* __restrict__ out) {
    JT_IDX((long)g.B * g.N * F);
    const long br = i_ / F; const int f = (int)(i_ % F);
    float s = 0.f;
    for (int c = 0; c < g.N; ++c)
        if (edge_live(g, br * g.N + c)) s += x[(br * g.N + c) * F + f];
    out[i_] = s;
}
__global__ void kc_sum_nodes(Geo g, int masked, int F, const float* __restrict__ x, float* __restrict__ out) {
    JT_IDX((long)g.B * F);
    const long b = i_ / F; const int f = (int)(i_ % F);
    float s = 0.f;
    for (int i = 0; i < g.N; ++i)
        if (!masked || i < g.nn[b]) s += x[(b * g.N + i) * F + f];
    out[i_] = s;
}

// ================================================================ edge-gated attention =========================================
// rows (b, j, i): j = source, i = target.  logit[b, j, i, h] = sum_ch q[b, i] k[b, j] g0[b, j, i] / sqrt(Ch)
__global__ void kc_attn_logit(Geo g, int D, int H, float isc, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ g0,
                              float* __restrict__ logit) {
    JT_IDX((long)g.B * g.N * g.N * H);
    const long er = i_ / H; const int hd = (int)(i_ % H), Ch = D / H;
    const long i = er % g.N, bj = er / g.N, b = bj / g.N;
    float s = 0.f;
    if (edge_live(g, er))
        for (int c = hd * Ch; c < (hd + 1) * Ch; ++c) s += q[(b * g.N + i) * D + c] * k[bj * D + c] * g0[er * D + c];
    logit[i_] = s * isc;
}
// per (target, head): softmax over the live sources (max, exp, sum + 1e-16), in place; 0 on the rows that are no real pair
__global__ void kc_attn_softmax(Geo g, int H, float* __restrict__ al) {
    JT_IDX((long)g.B * g.N * H);
    const long bi = i_ / H; const int hd = (int)(i_ % H);
    const long b = bi / g.N, i = bi % g.N;
    const int n = g.nn[b];
    const bool tgt = i < n;
    float mx = -INFINITY, sum = 0.f;
    for (int j = 0; j < n; ++j)
        if (tgt && j != i) mx = fmaxf(mx, al[((b * g.N + j) * g.N + i) * H + hd]);
    for (int j = 0; j < n; ++j)
        if (tgt && j != i) sum += expf(al[((b * g.N + j) * g.N + i) * H + hd] - mx);
    const float inv = 1.f / (sum + 1e-16f);
    for (int j = 0; j < g.N; ++j) {
        const long at = ((b * g.N + j) * g.N + i) * H + hd;
        al[at] = (tgt && j < n && j != i) ? expf(al[at] - mx) * inv : 0.f;
    }
}
// att[b, i, c] = sum_j v[b, j, c] g1[b, j, i, c] alpha[b, j, i, h(c)]
__global__ void kc_attn_msg(Geo g, int D, int H, const float* __restrict__ v, const float* __restrict__ g1, const float* __restrict__ al,
                            float* __restrict__ att) {
    JT_IDX((long)g.B * g.N * D);
    const long bi = i_ / D; const int c = (int)(i_ % D), hd = c / (D / H);
    const long b = bi / g.N, i = bi % g.N;
    const int n = g.nn[b];
    float s = 0.f;
    for (int j = 0; j < n; ++j) {
        const long er = (b * g.N + j) * g.N + i;
        s = fmaf(v[(b * g.N + j) * D + c] * g1[er * D + c], al[er * H + hd], s);
    }
    att[i_] = s;
}
// d v[b, j, c] = sum_i datt[b, i, c] g1[b, j, i, c] alpha      (one owner per source)
__global__ void kc_attn_bwd_v(Geo g, int D, int H, const float* __restrict__ datt, const float* __restrict__ g1, const float* __restrict__ al,
                              float* __restrict__ dv) {
    JT_IDX((long)g.B * g.N * D);
    const long bj = i_ / D; const int c = (int)(i_ % D), hd = c / (D / H);
    const long b = bj / g.N;
    const int n = g.nn[b];
    float s = 0.f;
    for (int i = 0; i < n; ++i) {
        const long er = bj * g.N + i;
        s = fmaf(datt[(b * g.N + i) * D + c] * g1[er * D + c], al[er * H + hd], s);
    }
    dv[i_] = s;
}
// d alpha[b, j, i, h] = sum_{c in h} datt[b, i, c] v[b, j, c] g1[b, j, i, c]
__global__ void kc_attn_bwd_alpha(Geo g, int D, int H, const float* __restrict__ datt, const float* __restrict__ v, const float* __restrict__ g1,
                                  float* __restrict__ dal) {
    JT_IDX((long)g.B * g.N * g.N * H);
    const long er = i_ / H; const int hd = (int)(i_ % H), Ch = D / H;
    const long i = er % g.N, bj = er / g.N, b = bj / g.N;
    float s = 0.f;
    if (edge_live(g, er))
        for (int c = hd * Ch; c < (hd + 1) * Ch; ++c) s += datt[(b * g.N + i) * D + c] * v[bj * D + c] * g1[er * D + c];
    dal[i_] = s;
}
// d logit = alpha (d alpha - sum_j alpha d alpha) per (target, head), in place on d alpha
__global__ void kc_attn_bwd_softmax(Geo g, int H, const float* __restrict__ al, float* __restrict__ dal) {
    JT_IDX((long)g.B * g.N * H);
    const long bi = i_ / H; const int hd = (int)(i_ % H);
    const long b = bi / g.N, i = bi % g.N;
    float dot = 0.f;
    for (int j = 0; j < g.N; ++j) { const long at = ((b * g.N + j) * g.N + i) * H + hd; dot = fmaf(al[at], dal[at], dot); }
    for (int j = 0; j < g.N; ++j) { const long at = ((b * g.N + j) * g.N + i) * H + hd; dal[at] = al[at] * (dal[at] - dot); }
}
// d (lin_edge1 he)[b, j, i, c] = datt[b, i, c] v[b, j, c] alpha (1 - g1^2); 0 on the rows that are no real pair (alpha = 0 there)
__global__ void kc_attn_bwd_t1(Geo g, int D, int H, const float* __restrict__ datt, const float* __restrict__ v, const float* __restrict__ g1,
                               const float* __restrict__ al, float* __restrict__ dt1) {
    JT_IDX((long)g.B * g.N * g.N * D);
    const long er = i_ / D; const int c = (int)(i_ % D), hd = c / (D / H);
    const long i = er % g.N, bj = er / g.N, b = bj / g.N;
    const float t = g1[i_];
    dt1[i_] = datt[(b * g.N + i) * D + c] * v[bj * D + c] * al[er * H + hd] * (1.f - t * t);
}
// d (lin_edge0 he)[b, j, i, c] = d logit[b, j, i, h] q[b, i, c] k[b, j, c] / sqrt(Ch) (1 - g0^2)
__global__ void kc_attn_bwd_t0(Geo g, int D, int H, float isc, const float* __restrict__ dlg, const float* __restrict__ q, const float* __restrict__ k,
                               const float* __restrict__ g0, float* __restrict__ dt0) {
    JT_IDX((long)g.B * g.N * g.N * D);
    const long er = i_ / D; const int c = (int)(i_ % D), hd = c / (D / H);
    const long i = er % g.N, bj = er / g.N, b = bj / g.N;
    const float t = g0[i_];
    dt0[i_] = dlg[er * H + hd] * isc * q[(b * g.N + i) * D + c] * k[bj * D + c] * (1.f - t * t);
}
// d q[b, i, c] = sum_j d logit k[b, j, c] g0[b, j, i, c] / sqrt(Ch)        (one owner per target)
__global__ void kc_attn_bwd_q(Geo g, int D, int H, float isc, const float* __restrict__ dlg, const float* __restrict__ k, const float* __restrict__ g0,
                              float* __restrict__ dq) {
    JT_IDX((long)g.B * g.N * D);
    const long bi = i_ / D; const int c = (int)(i_ % D), hd = c / (D / H);
    const long b = bi / g.N, i = bi % g.N;
    const int n = g.nn[b];
    float s = 0.f;
    for (int j = 0; j < n; ++j) {
        const long er = (b * g.N + j) * g.N + i;
        s = fmaf(dlg[er * H + hd], k[(b * g.N + j) * D + c] * g0[er * D + c], s);
    }
    dq[i_] = s * isc;
}
// d k[b, j, c] = sum_i d logit q[b, i, c] g0[b, j, i, c] / sqrt(Ch)        (one owner per source)
__global__ void kc_attn_bwd_k(Geo g, int D, int H, float isc, const float* __restrict__ dlg, const float* __restrict__ q, const float* __restrict__ g0,
                              float* __restrict__ dk) {
    JT_IDX((long)g.B * g.N * D);
    const long bj = i_ / D; const int c = (int)(i_ % D), hd = c / (D / H);
    const long b = bj / g.N;
    const int n = g.nn[b];
    float s = 0.f;
    for (int i = 0; i < n; ++i) {
        const long er = bj * g.N + i;
        s = fmaf(dlg[er * H + hd], q[(b * g.N + i) * D + c] * g0[er * D + c], s);
    }
    dk[i_] = s * isc;
}

// ================================================================ outputs ======================================================
__global__ void kc_out_nodes(Geo g, int ach, const float* __restrict__ a3, float* __restrict__ out) {
    JT_IDX((long)g.B * g.N * ach);
    out[i_] = node_live(g, i_ / ach) ? a3[i_] : 0.f;
}
// (s + s^T) / 2 on real pairs, both ways (forward: Ep -> out; backward: d out -> d Ep, the same map)
__global__ void kc_out_edges(Geo g, int ch, const float* __restrict__ src, float* __restrict__ dst) {
    JT_IDX((long)g.B * g.N * g.N * ch);
    const long er = i_ / ch; const int c = (int)(i_ % ch);
    const long j = er % g.N, bi = er / g.N, b = bi / g.N, i = bi % g.N;
    dst[i_] = edge_live(g, er) ? (src[i_] + src[((b * g.N + j) * g.N + i) * ch + c]) * 0.5f : 0.f;
}

// ================================================================ launch sequences ============================================
// The multi-launch sequences of the step on explicit pointers: forward() / backward() call them on the workspace, the test entry
// jodo_cdgs_train_debug_op (at the end) on the caller's arrays.
// floats of the double scratch: (sum, sum) per (tile row, group) of the edge GroupNorm; per (chunk, column) + per (group of chunks, column)
// of the column sums
size_t egn_part_floats(size_t M, size_t G) { return 2 * 2 * M * G; }
size_t colsum_part_floats(size_t rows, size_t F) { const size_t nchunk = (rows + 63) / 64; return 2 * 2 * (nchunk + nchunk / COLSUM_PER + 1) * F; }

// thresholded adjacency and random-walk features: adj, AD, cnt [B N^2], onehot [B N^2, K + 1], land [B N, K], deg [B N, ch]; pa, pb hold
// the powers in turn
void rw_prologue(hipStream_t s, const Geo& g, int K, int ch, const float* edge_x, float* adj, float* AD, float* pa, float* pb, float* cnt, float* onehot,
                 float* land, float* deg) {
    const long M = (long)g.B * g.N, R = M * g.N;
    JT_LAUNCH(kc_adj, R, s, g, ch, edge_x, adj);
    JT_LAUNCH(kc_adnorm, R, s, g, (const float*)adj, AD, pa, cnt);
    for (int m = 0; m < K; ++m)
        JT_LAUNCH(kc_rw_step, R, s, g, K, m, (const float*)((m & 1) ? pb : pa), (const float*)AD, (m & 1) ? pa : pb, cnt, land);
    JT_LAUNCH(kc_onehot, R * (K + 1), s, R, K + 1, (const float*)cnt, onehot);
    JT_LAUNCH(kc_deg, M * ch, s, g, ch, edge_x, deg);
}
void gine_backward(hipStream_t s, const Geo& g, int D, const float* eps, const float* hs, const float* he, const float* adj, const float* dagg, float* dhe,
                   float* dhs) {
    const long M = (long)g.B * g.N, R = M * g.N;
    JT_LAUNCH(kc_gine_bwd_e, R * D, s, g, D, hs, he, adj, dagg, dhe);
    JT_LAUNCH(kc_gine_bwd_n, M * D, s, g, D, eps, dagg, (const float*)dhe, dhs);
}
// norm2_edge over the padded tile: x -> xhat in place, e_out, rstd [B, D / 8]; part, gsum: double scratch
void egn_forward(hipStream_t s, const Geo& g, int D, float* x, const float* gamma, const float* beta, double* part, double* gsum, float* rstd, float* eout) {
    const int G = D / GW;
    const long M = (long)g.B * g.N, R = M * g.N;
    JT_LAUNCH(kc_egn_part, M * G, s, g, 0, D, (const float*)x, (const float*)nullptr, (const float*)nullptr, part);
    JT_LAUNCH(kc_egn_fin, (long)g.B * G, s, g, G, (const double*)part, gsum);
    JT_LAUNCH(kc_egn_apply, R * D, s, g, D, (const double*)gsum, x, gamma, beta, rstd, eout);
}
void egn_backward(hipStream_t s, const Geo& g, int D, const float* de, const float* xhat, const float* rstd, const float* gamma, double* part, double* gsum,
                  float* dpre) {
    const int G = D / GW;
    const long M = (long)g.B * g.N, R = M * g.N;
    JT_LAUNCH(kc_egn_part, M * G, s, g, 2, D, de, xhat, gamma, part);
    JT_LAUNCH(kc_egn_fin, (long)g.B * G, s, g, G, (const double*)part, gsum);
    JT_LAUNCH(kc_egn_bwd, R * D, s, g, D, (const double*)gsum, de, xhat, rstd, gamma, dpre);
}
// norm weights: dbeta = column sums of dy over the live rows, dgamma = of dy xhat.  Three levels, each in a fixed order: 64-row chunks,
// groups of COLSUM_PER chunks, then the groups (at QM9 batch 128: 1 458 chunks -> 46 groups, instead of one thread per column walking
// all 1 458)
void colsum_grads(hipStream_t s, const Geo& g, int mode, long rows, int F, const float* dy, const float* xhat, double* part, float* dbeta, float* dgamma) {
    const long nchunk = (rows + 63) / 64;
    const long ngroup = (nchunk + COLSUM_PER - 1) / COLSUM_PER;
    double* mid = part + 2 * nchunk * F;
    JT_LAUNCH(kc_colsum_part, nchunk * F, s, g, mode, rows, F, dy, xhat, part);
    JT_LAUNCH(kc_colsum_mid, ngroup * F, s, nchunk, COLSUM_PER, F, (const double*)part, mid);
    JT_LAUNCH(kc_colsum_fin, F, s, ngroup, F, (const double*)mid, dbeta, dgamma);
}
// per-molecule sums of an edge tensor: cols [B N, F] = over the real pairs of a tile row, out [B, F] = over the tile rows (masked: the
// molecule's own only)
void tile_sums(hipStream_t s, const Geo& g, int F, const float* x, float* cols, int masked, float* out) {
    JT_LAUNCH(kc_sum_cols, (long)g.B * g.N * F, s, g, F, x, cols);
    JT_LAUNCH(kc_sum_nodes, (long)g.B * F, s, g, masked, F, (const float*)cols, out);
}
// alpha [B N^2, H] (logits, then the softmax in place), att [B N, D]
void attn_forward(hipStream_t s, const Geo& g, int D, int H, float isc, const float* q, const float* k, const float* v, const float* g0, const float* g1,
                  float* alpha, float* att) {
    const long M = (long)g.B * g.N, R = M * g.N;
    JT_LAUNCH(kc_attn_logit, R * H, s, g, D, H, isc, q, k, g0, alpha);
    JT_LAUNCH(kc_attn_softmax, M * H, s, g, H, alpha);
    JT_LAUNCH(kc_attn_msg, M * D, s, g, D, H, v, g1, (const float*)alpha, att);
}
struct AttnBwd { const float *datt, *q, *k, *v, *g0, *g1, *alpha; float *dv, *dal, *dt1, *dt0, *dq, *dk; };
// the seven kernels in the step's order; dal: d alpha, turned into d logit in place.  `done(stage)` runs when dv (0), dt1 (1), dt0 (2),
// dq (3), dk (4) is complete: the step consumes each of them in its GEMMs right there, so dt1 / dt0 and dq / dk may share a buffer
template <class Fn>
void attn_backward(hipStream_t s, const Geo& g, int D, int H, float isc, const AttnBwd& a, Fn&& done) {
    const long M = (long)g.B * g.N, R = M * g.N;
    JT_LAUNCH(kc_attn_bwd_v, M * D, s, g, D, H, a.datt, a.g1, a.alpha, a.dv);
    done(0);
    JT_LAUNCH(kc_attn_bwd_alpha, R * H, s, g, D, H, a.datt, a.v, a.g1, a.dal);
    JT_LAUNCH(kc_attn_bwd_softmax, M * H, s, g, H, a.alpha, a.dal);
    JT_LAUNCH(kc_attn_bwd_t1, R * D, s, g, D, H, a.datt, a.v, a.g1, a.alpha, a.dt1);
    done(1);
    JT_LAUNCH(kc_attn_bwd_t0, R * D, s, g, D, H, isc, (const float*)a.dal, a.q, a.k, a.g0, a.dt0);
    done(2);
    JT_LAUNCH(kc_attn_bwd_q, M * D, s, g, D, H, isc, (const float*)a.dal, a.k, a.g0, a.dq);
    done(3);
    JT_LAUNCH(kc_attn_bwd_k, M * D, s, g, D, H, isc, (const float*)a.dal, a.q, a.g0, a.dk);
    done(4);
}

}  // namespace

struct jodo_cdgs_train {
    jodo_cdgs_cfg cfg;
    int B, N, D, F, L, H, K, ach, ch, cat, Kc, w_ec, w_es, w_nd, w_nc;      // widths: edge cate / exist (w_ec each), spd (w_es); node degree / rw (w_nd each), cate (w_nc)
    long M, R;
    std::vector<int> tables;          // n_nodes [B]
    int n_params;
    std::vector<size_t> numel;
    Lin time0, time1, ecate, eexist, espd, eemb, adeg, acate, arw, aemb, ah[3], bh[3], xh[3];
    std::vector<BlkIx> blk;
    size_t ws_bytes;
    int split = 0;                    // option 3: product forms in split-bf16 (1 forward, 2 data gradients, 4 weight gradients)
};

namespace {

void layout(const jodo_cdgs_train& t, Arena& a, Bufs& b) {
    const size_t B = t.B, M = t.M, R = t.R, D = t.D, F = t.F, L = t.L, H = t.H, G = D / GW;
    b.tin = a.f(B * D); b.t1p = a.f(B * 2 * D); b.t1a = a.f(B * 2 * D); b.temb = a.f(B * D); b.tact = a.f(B * D);
    b.adj = a.f(R); b.AD = a.f(R); b.pa = a.f(R); b.pb = a.f(R); b.cnt = a.f(R); b.onehot = a.f(R * (t.K + 1)); b.land = a.f(M * t.K);
    b.deg = a.f(M * t.ch); b.ein = a.f(R * D); b.nin = a.f(M * D); b.ahid = a.f(M * t.Kc); b.bhid = a.f(R * t.Kc); b.a3 = a.f(M * t.ach);
    b.Ep = a.f(R * t.ch);
    b.h.resize(L + 1); b.e.resize(L + 1);
    for (size_t l = 0; l <= L; ++l) { b.h[l] = a.f(M * D); b.e[l] = a.f(R * D); }
    b.blk.resize(L);
    for (size_t l = 0; l < L; ++l) {
        BlkBuf& k = b.blk[l];
        k.te = a.f(B * D); k.tn = a.f(B * D); k.hs = a.f(M * D); k.agg = a.f(M * D); k.g1 = a.f(M * D);
        k.xh1 = a.f(M * D); k.rs1 = a.f(M * G); k.xh2 = a.f(M * D); k.rs2 = a.f(M * G); k.xh3 = a.f(M * D); k.rs3 = a.f(M * G);
        k.q = a.f(M * D); k.k = a.f(M * D); k.v = a.f(M * D); k.t0 = a.f(R * D); k.t1 = a.f(R * D); k.alpha = a.f(R * H); k.hc = a.f(M * D);
        k.f1p = a.f(M * F); k.a1 = a.f(M * F); k.f3p = a.f(R * F); k.a3 = a.f(R * F); k.xhe = a.f(R * D); k.rse = a.f(B * G);
    }
    for (int s = 0; s < 3; ++s) {
        const size_t rows = s == 0 ? M : R;
        b.hd[s].p1 = a.f(rows * D); b.hd[s].a1 = a.f(rows * D); b.hd[s].p2 = a.f(rows * D / 2); b.hd[s].a2 = a.f(rows * D / 2);
    }
    for (int s = 0; s < 5; ++s) b.sE[s] = a.f(R * D);
    b.sE_F = a.f(R * F); b.sE_H = a.f(R * H);
    for (int s = 0; s < 6; ++s) b.sN[s] = a.f(M * D);
    b.sN_F = a.f(M * F);
    for (int s = 0; s < 2; ++s) b.sB[s] = a.f(B * 2 * D);
    b.dtact = a.f(B * D); b.dein = a.f(R * D); b.dnin = a.f(M * D); b.dah = a.f(M * t.Kc); b.dbh = a.f(R * t.Kc); b.dEp = a.f(R * t.ch);
    b.da3 = a.f(M * t.ach);
    b.part = a.f(std::max(egn_part_floats(M, G), colsum_part_floats(R, D)));          // doubles, shared by the edge GroupNorm and the column sums
    b.gsum = a.f(2 * 2 * B * G);
    b.splitk_floats = std::min<size_t>((size_t)32 << 20, ((R + 511) / 512 + 1) * (F * D + F));
    b.splitk = a.f(b.splitk_floats);
}

struct Ctx {
    const jodo_cdgs_train& t; Geo g; const float* const* P; float* const* G; Bufs& b; hipStream_t s; float p_drop; unsigned long long seed;
    int split = 0;                    // jodo_cdgs_train::split: which of the product forms below run as GemmEpi::split
    GemmEpi epi(int act, float* out2, Drop d, float* dbias, int form) const {
        GemmEpi e; e.act = act; e.out2 = out2; e.drop = d; e.dbias = dbias; e.split = (split & form) ? 1 : 0;
        return e;
    }
    const float* p(int i) const { return P[i]; }
    float* gr(int i) const { return G[i]; }
    Drop drop(int l, int site) const { Drop d; d.p = p_drop; d.seed = seed; d.site = (unsigned)(l * 8 + site); return d; }
    Drop nod() const { Drop d; d.p = 0.f; d.seed = 0; d.site = 0; return d; }
    // Y[rows, N] (ldy) (+)= X[rows, K] (ldx) W[N, K]^T (ldw) + bias
    void lin(const float* X, int ldx, long rows, int K, const float* W, int ldw, int N, const float* bias, float* Y, int ldy, int acc) const {
        const GemmEpi e = epi(0, nullptr, nod(), nullptr, 1);
        gemm(s, 0, 1, (int)rows, N, K, X, ldx, W, ldw, Y, ldy, bias, acc, b.splitk, b.splitk_floats, &e);
    }
    void lin_tanh(const float* X, long rows, int K, const float* W, int N, float* Y) const {
        const GemmEpi e = epi(1, nullptr, nod(), nullptr, 1);
        gemm(s, 0, 1, (int)rows, N, K, X, K, W, K, Y, N, nullptr, 0, b.splitk, b.splitk_floats, &e);
    }
    // pre = X W^T + bias (kept), act = SiLU(pre) * dropout(row N + col); both dense [rows, N]
    void lin_silu(const float* X, long rows, int K, const float* W, int N, const float* bias, float* pre, float* act, Drop d) const {
        const GemmEpi e = epi(2, act, d, nullptr, 1);
        gemm(s, 0, 1, (int)rows, N, K, X, K, W, K, pre, N, bias, 0, b.splitk, b.splitk_floats, &e);
    }
    // dX[rows, K] (ldx) (+)= dY[rows, N] (ldy) W[N, K] (ldw)
    void lin_dx(const float* dY, int ldy, long rows, int N, const float* W, int ldw, int K, float* dX, int ldx, int acc) const {
        const GemmEpi e = epi(0, nullptr, nod(), nullptr, 2);
        gemm(s, 0, 0, (int)rows, K, N, dY, ldy, W, ldw, dX, ldx, nullptr, acc, b.splitk, b.splitk_floats, &e);
    }
    // dW[N, K] (lddw) += dY[rows, N]^T X[rows, K]; db[N] += column sums of dY
    void lin_dw(const float* dY, int ldy, long rows, int N, const float* X, int ldx, int K, float* dW, int lddw, float* db = nullptr) const {
        const GemmEpi e = epi(0, nullptr, nod(), db, 4);
        gemm(s, 1, 0, N, K, (int)rows, dY, ldy, X, ldx, dW, lddw, nullptr, 1, b.splitk, b.splitk_floats, &e);
    }
    // a whole Linear on dense operands: forward, and its backward (weight and bias gradients, dX written or accumulated; dX may be null)
    void fwd(Lin l, const float* X, long rows, int K, int N, float* Y) const { lin(X, K, rows, K, p(l.w), K, N, p(l.b), Y, N, 0); }
    void bwd(Lin l, const float* dY, long rows, int N, const float* X, int K, float* dX, int acc) const {
        lin_dw(dY, N, rows, N, X, K, K, gr(l.w), K, gr(l.b));
        if (dX) lin_dx(dY, N, rows, N, p(l.w), K, K, dX, K, acc);
    }
    void scale(int mode, long rows, int F, const float* src, Drop d, float* dst, int acc) const {
        JT_LAUNCH(kc_scale, rows * F, s, g, mode, rows, F, src, d, dst, acc);
    }
    // norm weights: beta gradient = column sums of dy over the live rows, gamma gradient = of dy xhat
    void norm_grads(int mode, long rows, int F, const float* dy, const float* xhat, Lin n) const {
        colsum_grads(s, g, mode, rows, F, dy, xhat, reinterpret_cast<double*>(b.part), gr(n.b), gr(n.w));
    }
};

// MLP head on an input of two column ranges [Xa (Ka) | Xb (Kb)]: Linear SiLU Linear SiLU Linear.  The reference's masks between the
// layers act on whole rows whose outputs are masked again at the end, so they change no output and no gradient: left out.
void head_fwd(const Ctx& c, const Lin* l, const float* Xa, int lda, int Ka, const float* Xb, int ldb, int Kb, long rows, int NO, const HeadBuf& hb,
              float* out, int ldo) {
    const int D = c.t.D, K0 = Ka + Kb;
    c.lin(Xa, lda, rows, Ka, c.p(l[0].w), K0, D, c.p(l[0].b), hb.p1, D, 0);
    c.lin(Xb, ldb, rows, Kb, c.p(l[0].w) + Ka, K0, D, nullptr, hb.p1, D, 1);
    JT_LAUNCH(k_silu_fwd, rows * D, c.s, rows * D, (const float*)hb.p1, hb.a1, c.nod());
    c.lin_silu(hb.a1, rows, D, c.p(l[1].w), D / 2, c.p(l[1].b), hb.p2, hb.a2, c.nod());
    c.lin(hb.a2, D / 2, rows, D / 2, c.p(l[2].w), D / 2, NO, c.p(l[2].b), out, ldo, 0);
}
void head_bwd(const Ctx& c, const Lin* l, const float* Xa, int lda, int Ka, const float* Xb, int ldb, int Kb, long rows, int NO, const HeadBuf& hb,
              const float* dOut, int ldo, float* t1, float* t2, float* dXa, int ldda, float* dXb, int lddb, int accb) {
    const int D = c.t.D, K0 = Ka + Kb;
    c.lin_dw(dOut, ldo, rows, NO, hb.a2, D / 2, D / 2, c.gr(l[2].w), D / 2, c.gr(l[2].b));
    c.lin_dx(dOut, ldo, rows, NO, c.p(l[2].w), D / 2, D / 2, t2, D / 2, 0);
    JT_LAUNCH(k_silu_bwd, rows * (D / 2), c.s, rows * (D / 2), (const float*)hb.p2, (const float*)t2, t2, c.nod());
    c.lin_dw(t2, D / 2, rows, D / 2, hb.a1, D, D, c.gr(l[1].w), D, c.gr(l[1].b));
    c.lin_dx(t2, D / 2, rows, D / 2, c.p(l[1].w), D, D, t1, D, 0);
    JT_LAUNCH(k_silu_bwd, rows * D, c.s, rows * D, (const float*)hb.p1, (const float*)t1, t1, c.nod());
    c.lin_dw(t1, D, rows, D, Xa, lda, Ka, c.gr(l[0].w), K0, c.gr(l[0].b));
    c.lin_dw(t1, D, rows, D, Xb, ldb, Kb, c.gr(l[0].w) + Ka, K0);
    c.lin_dx(t1, D, rows, D, c.p(l[0].w), K0, Ka, dXa, ldda, 0);
    c.lin_dx(t1, D, rows, D, c.p(l[0].w) + Ka, K0, Kb, dXb, lddb, accb);
}

void forward(const Ctx& c, const float* tt, const float* freq, const float* x, const float* edge_x, float* out_x, float* out_e) {
    const jodo_cdgs_train& t = c.t; Bufs& b = c.b; const Geo& g = c.g; hipStream_t s = c.s;
    const int B = t.B, D = t.D, F = t.F, L = t.L, H = t.H, K = t.K, ch = t.ch, ach = t.ach, G = D / GW;
    const long M = t.M, R = t.R;
    const float isc = 1.f / sqrtf((float)(D / H));
    // time embedding: the blocks read it through SiLU only
    JT_LAUNCH(kc_time, (long)B * D, s, B, D, tt, freq, b.tin);
    c.lin_silu(b.tin, B, D, c.p(t.time0.w), 2 * D, c.p(t.time0.b), b.t1p, b.t1a, c.nod());
    c.lin_silu(b.t1a, B, 2 * D, c.p(t.time1.w), D, c.p(t.time1.b), b.temb, b.tact, c.nod());
    // thresholded adjacency and random-walk features (no gradient)
    rw_prologue(s, g, K, ch, edge_x, b.adj, b.AD, b.pa, b.pb, b.cnt, b.onehot, b.land, b.deg);
    // embeddings: ein = [cate | exist | spd] masked, e = lin(ein) masked; nin = [degree | cate | rw], h = lin(nin)
    c.lin(edge_x + 1, ch, R, ch - 1, c.p(t.ecate.w), ch - 1, t.w_ec, c.p(t.ecate.b), b.ein, D, 0);
    c.lin(edge_x, ch, R, 1, c.p(t.eexist.w), 1, t.w_ec, c.p(t.eexist.b), b.ein + t.w_ec, D, 0);
    c.lin(b.onehot, K + 1, R, K + 1, c.p(t.espd.w), K + 1, t.w_es, c.p(t.espd.b), b.ein + 2 * t.w_ec, D, 0);
    c.scale(2, R, D, b.ein, c.nod(), b.ein, 0);
    c.fwd(t.eemb, b.ein, R, D, D, b.e[0]);
    c.scale(2, R, D, b.e[0], c.nod(), b.e[0], 0);
    c.lin(b.deg, ch, M, ch, c.p(t.adeg.w), ch, t.w_nd, c.p(t.adeg.b), b.nin, D, 0);
    c.lin(x, ach, M, ach, c.p(t.acate.w), ach, t.w_nc, c.p(t.acate.b), b.nin + t.w_nd, D, 0);
    c.lin(b.land, K, M, K, c.p(t.arw.w), K, t.w_nd, c.p(t.arw.b), b.nin + t.w_nd + t.w_nc, D, 0);
    c.fwd(t.aemb, b.nin, M, D, D, b.h[0]);
    for (int l = 0; l < L; ++l) {
        const BlkIx& ix = t.blk[l]; BlkBuf& k = b.blk[l];
        float *he = b.sE[0], *tmpN = b.sN[0], *tmpE = b.sE[1];
        c.fwd(ix.t_edge, b.tact, B, D, D, k.te);
        c.fwd(ix.t_node, b.tact, B, D, D, k.tn);
        JT_LAUNCH(kc_addt, R * D, s, g, 2, R, D, (const float*)b.e[l], (const float*)k.te, he);
        JT_LAUNCH(kc_addt, M * D, s, g, 1, M, D, (const float*)b.h[l], (const float*)k.tn, k.hs);
        // local: GINE over the thresholded adjacency, its two Linears, residual with dropout site 1, norm1_local
        JT_LAUNCH(kc_gine, M * D, s, g, D, c.p(ix.eps), (const float*)k.hs, (const float*)he, (const float*)b.adj, k.agg);
        c.fwd(ix.gin0, k.agg, M, D, D, k.g1);
        JT_LAUNCH(kc_relu, M * D, s, M * D, (const float*)k.g1, k.g1);
        c.fwd(ix.gin2, k.g1, M, D, D, tmpN);
        JT_LAUNCH(kc_gn_fwd, M * G, s, g, M, D, (const float*)b.h[l], (const float*)tmpN, c.drop(l, 1), 1, c.p(ix.nl.w), c.p(ix.nl.b), k.xh1, k.rs1, k.hc, 0);
        // global: edge-gated attention over every real ordered pair, residual with dropout site 2, norm1_attn
        c.fwd(ix.query, k.hs, M, D, D, k.q);
        c.fwd(ix.key, k.hs, M, D, D, k.k);
        c.fwd(ix.value, k.hs, M, D, D, k.v);
        c.lin_tanh(he, R, D, c.p(ix.le0), D, k.t0);
        c.lin_tanh(he, R, D, c.p(ix.le1), D, k.t1);
        attn_forward(s, g, D, H, isc, k.q, k.k, k.v, k.t0, k.t1, k.alpha, tmpN);
        JT_LAUNCH(kc_gn_fwd, M * G, s, g, M, D, (const float*)b.h[l], (const float*)tmpN, c.drop(l, 2), 0, c.p(ix.na.w), c.p(ix.na.b), k.xh2, k.rs2, k.hc, 1);
        // node feed-forward (sites 3, 4), norm2_node
        c.lin_silu(k.hc, M, D, c.p(ix.ff1.w), F, c.p(ix.ff1.b), k.f1p, k.a1, c.drop(l, 3));
        c.fwd(ix.ff2, k.a1, M, F, D, tmpN);
        JT_LAUNCH(kc_gn_fwd, M * G, s, g, M, D, (const float*)k.hc, (const float*)tmpN, c.drop(l, 4), 0, c.p(ix.nn.w), c.p(ix.nn.b), k.xh3, k.rs3, b.h[l + 1], 0);
        // edge feed-forward over the whole padded tile (sites 5, 6), residual, norm2_edge over 8 channels x N x N positions
        JT_LAUNCH(kc_pair, R * D, s, g, D, (const float*)k.hc, tmpE);
        c.lin_silu(tmpE, R, D, c.p(ix.ff3.w), F, c.p(ix.ff3.b), k.f3p, k.a3, c.drop(l, 5));
        c.fwd(ix.ff4, k.a3, R, F, D, k.xhe);
        c.scale(0, R, D, k.xhe, c.drop(l, 6), k.xhe, 0);
        JT_LAUNCH(k_add, R * D, s, R * D, k.xhe, (const float*)b.e[l]);
        double *part = reinterpret_cast<double*>(b.part), *gsum = reinterpret_cast<double*>(b.gsum);
        egn_forward(s, g, D, k.xhe, c.p(ix.ne.w), c.p(ix.ne.b), part, gsum, k.rse, b.e[l + 1]);
        // readouts straight into the head inputs
        c.lin(b.h[l + 1], D, M, D, c.p(ix.ro_n.w), D, t.cat, c.p(ix.ro_n.b), b.ahid + l * t.cat, t.Kc, 0);
        c.lin(b.e[l + 1], D, R, D, c.p(ix.ro_e.w), D, t.cat, c.p(ix.ro_e.b), b.bhid + l * t.cat, t.Kc, 0);
    }
    head_fwd(c, t.ah, b.nin + t.w_nd, D, t.w_nc, b.ahid, t.Kc, t.Kc, M, ach, b.hd[0], b.a3, ach);
    head_fwd(c, t.bh, b.ein, D, t.w_ec, b.bhid, t.Kc, t.Kc, R, ch - 1, b.hd[1], b.Ep + 1, ch);
    head_fwd(c, t.xh, b.ein + t.w_ec, D, t.w_ec, b.bhid, t.Kc, t.Kc, R, 1, b.hd[2], b.Ep, ch);
    JT_LAUNCH(kc_out_nodes, M * ach, s, g, ach, (const float*)b.a3, out_x);
    JT_LAUNCH(kc_out_edges, R * ch, s, g, ch, (const float*)b.Ep, out_e);
}

void backward(const Ctx& c, const float* x, const float* edge_x, const float* d_out_x, const float* d_out_e) {
    const jodo_cdgs_train& t = c.t; Bufs& b = c.b; const Geo& g = c.g; hipStream_t s = c.s;
    const int B = t.B, D = t.D, F = t.F, L = t.L, H = t.H, K = t.K, ch = t.ch, ach = t.ach, G = D / GW;
    const long M = t.M, R = t.R;
    const float isc = 1.f / sqrtf((float)(D / H));
    // gradients are accumulated below: zero them first — adjacent buffers (and alignment gaps under 16 bytes between them) in one fill;
    // buffers have no slot (null)
    for (int i = 0; i < t.n_params;) {
        if (!c.gr(i)) { ++i; continue; }
        char* beg = reinterpret_cast<char*>(c.gr(i));
        size_t bytes = t.numel[i] * 4;
        int j = i + 1;
        while (j < t.n_params && c.gr(j) && reinterpret_cast<char*>(c.gr(j)) >= beg + bytes && reinterpret_cast<char*>(c.gr(j)) - (beg + bytes) < 16) {
            bytes = (size_t)(reinterpret_cast<char*>(c.gr(j)) - beg) + t.numel[j] * 4;
            ++j;
        }
        (void)hipMemsetAsync(beg, 0, bytes, s);
        i = j;
    }
    (void)hipMemsetAsync(b.dtact, 0, (size_t)B * D * 4, s);
    (void)hipMemsetAsync(b.dein, 0, (size_t)R * D * 4, s);
    (void)hipMemsetAsync(b.dnin, 0, (size_t)M * D * 4, s);
    // outputs and heads
    JT_LAUNCH(kc_out_nodes, M * ach, s, g, ach, d_out_x, b.da3);
    JT_LAUNCH(kc_out_edges, R * ch, s, g, ch, d_out_e, b.dEp);
    head_bwd(c, t.ah, b.nin + t.w_nd, D, t.w_nc, b.ahid, t.Kc, t.Kc, M, ach, b.hd[0], b.da3, ach, b.sN[0], b.sN[1], b.dnin + t.w_nd, D, b.dah, t.Kc, 0);
    head_bwd(c, t.bh, b.ein, D, t.w_ec, b.bhid, t.Kc, t.Kc, R, ch - 1, b.hd[1], b.dEp + 1, ch, b.sE[0], b.sE[1], b.dein, D, b.dbh, t.Kc, 0);
    head_bwd(c, t.xh, b.ein + t.w_ec, D, t.w_ec, b.bhid, t.Kc, t.Kc, R, 1, b.hd[2], b.dEp, ch, b.sE[0], b.sE[1], b.dein + t.w_ec, D, b.dbh, t.Kc, 1);
    float *dh = b.sN[4], *dh_prev = b.sN[5], *de = b.sE[3], *de_prev = b.sE[4];
    (void)hipMemsetAsync(dh, 0, (size_t)M * D * 4, s);
    (void)hipMemsetAsync(de, 0, (size_t)R * D * 4, s);
    double *part = reinterpret_cast<double*>(b.part), *gsum = reinterpret_cast<double*>(b.gsum);
    for (int l = L - 1; l >= 0; --l) {
        const BlkIx& ix = t.blk[l]; BlkBuf& k = b.blk[l];
        float *E0 = b.sE[0], *E1 = b.sE[1], *E2 = b.sE[2], *N0 = b.sN[0], *N1 = b.sN[1], *N2 = b.sN[2], *N3 = b.sN[3];
        // readouts
        c.lin_dw(b.dah + l * t.cat, t.Kc, M, t.cat, b.h[l + 1], D, D, c.gr(ix.ro_n.w), D, c.gr(ix.ro_n.b));
        c.lin_dx(b.dah + l * t.cat, t.Kc, M, t.cat, c.p(ix.ro_n.w), D, D, dh, D, 1);
        c.lin_dw(b.dbh + l * t.cat, t.Kc, R, t.cat, b.e[l + 1], D, D, c.gr(ix.ro_e.w), D, c.gr(ix.ro_e.b));
        c.lin_dx(b.dbh + l * t.cat, t.Kc, R, t.cat, c.p(ix.ro_e.w), D, D, de, D, 1);
        // ---- norm2_edge over the padded tile: d pre at every position -> de_prev (the residual's share of d e[l])
        c.norm_grads(2, R, D, de, k.xhe, ix.ne);
        egn_backward(s, g, D, de, k.xhe, k.rse, c.p(ix.ne.w), part, gsum, de_prev);
        // ---- edge feed-forward, every row of the tile
        c.scale(0, R, D, de_prev, c.drop(l, 6), E1, 0);                                           // d f4
        c.bwd(ix.ff4, E1, R, D, k.a3, F, b.sE_F, 0);
        JT_LAUNCH(k_silu_bwd, R * F, s, R * F, (const float*)k.f3p, (const float*)b.sE_F, b.sE_F, c.drop(l, 5));
        JT_LAUNCH(kc_pair, R * D, s, g, D, (const float*)k.hc, E1);
        c.bwd(ix.ff3, b.sE_F, R, F, E1, D, E0, 0);                                                // E0 = d (h_r + h_c)
        float* dhc = N0;
        JT_LAUNCH(kc_pair_bwd, M * D, s, g, D, (const float*)E0, dhc);
        // ---- norm2_node, node feed-forward
        c.norm_grads(1, M, D, dh, k.xh3, ix.nn);
        JT_LAUNCH(kc_gn_bwd, M * G, s, g, M, D, (const float*)dh, (const float*)k.xh3, (const float*)k.rs3, c.p(ix.nn.w), N1, 0);      // d (hc + drop(f2))
        JT_LAUNCH(k_add, M * D, s, M * D, dhc, (const float*)N1);
        c.scale(0, M, D, N1, c.drop(l, 4), N1, 0);                                                // d f2
        c.bwd(ix.ff2, N1, M, D, k.a1, F, b.sN_F, 0);
        JT_LAUNCH(k_silu_bwd, M * F, s, M * F, (const float*)k.f1p, (const float*)b.sN_F, b.sN_F, c.drop(l, 3));
        c.bwd(ix.ff1, b.sN_F, M, F, k.hc, D, dhc, 1);
        // ---- hc = (norm1_local(.) + norm1_attn(.)) * node mask
        c.norm_grads(1, M, D, dhc, k.xh2, ix.na);
        JT_LAUNCH(kc_gn_bwd, M * G, s, g, M, D, (const float*)dhc, (const float*)k.xh2, (const float*)k.rs2, c.p(ix.na.w), dh_prev, 0);
        float* datt = N1;
        c.scale(0, M, D, dh_prev, c.drop(l, 2), datt, 0);
        c.norm_grads(1, M, D, dhc, k.xh1, ix.nl);
        JT_LAUNCH(kc_gn_bwd, M * G, s, g, M, D, (const float*)dhc, (const float*)k.xh1, (const float*)k.rs1, c.p(ix.nl.w), N2, 0);
        JT_LAUNCH(k_add, M * D, s, M * D, dh_prev, (const float*)N2);
        c.scale(1, M, D, N2, c.drop(l, 1), N2, 0);                                                // d loc
        c.bwd(ix.gin2, N2, M, D, k.g1, D, N3, 0);
        JT_LAUNCH(kc_relu_bwd, M * D, s, M * D, (const float*)k.g1, N3);
        c.bwd(ix.gin0, N3, M, D, k.agg, D, N2, 0);                                                // N2 = d agg
        // ---- GINE: he recomputed; d he written into E2, d hs into dhs
        float *he = E0, *dhe = E2, *dhs = N3;
        JT_LAUNCH(kc_addt, R * D, s, g, 2, R, D, (const float*)b.e[l], (const float*)k.te, he);
        gine_backward(s, g, D, c.p(ix.eps), k.hs, he, b.adj, N2, dhe, dhs);
        // ---- attention
        // ---- attention: d t1 and d t0 share E1, d q and d k share N2; each is consumed by its GEMMs as soon as it is complete
        float *dv = N0, *dq = N2;
        const AttnBwd ab{datt, k.q, k.k, k.v, k.t0, k.t1, k.alpha, dv, b.sE_H, E1, E1, dq, dq};
        attn_backward(s, g, D, H, isc, ab, [&](int stage) {
            const Lin le{stage == 1 ? ix.le1 : ix.le0, -1};
            switch (stage) {
                case 0: c.bwd(ix.value, dv, M, D, k.hs, D, dhs, 1); break;
                case 1: case 2:
                    c.lin_dw(E1, D, R, D, he, D, D, c.gr(le.w), D);
                    c.lin_dx(E1, D, R, D, c.p(le.w), D, D, dhe, D, 1);
                    break;
                case 3: c.bwd(ix.query, dq, M, D, k.hs, D, dhs, 1); break;
                default: c.bwd(ix.key, dq, M, D, k.hs, D, dhs, 1); break;
            }
        });
        // ---- he = (e + t_edge) * edge mask, hs = (h + t_node) * node mask: per-molecule sums for the time shifts
        c.scale(2, R, D, dhe, c.nod(), de_prev, 1);
        tile_sums(s, g, D, dhe, N0, 0, b.sB[0]);
        c.bwd(ix.t_edge, b.sB[0], B, D, b.tact, D, b.dtact, 1);
        c.scale(1, M, D, dhs, c.nod(), dh_prev, 1);
        JT_LAUNCH(kc_sum_nodes, (long)B * D, s, g, 1, D, (const float*)dhs, b.sB[0]);
        c.bwd(ix.t_node, b.sB[0], B, D, b.tact, D, b.dtact, 1);
        std::swap(dh, dh_prev); std::swap(de, de_prev);
    }
    // embeddings
    c.bwd(t.aemb, dh, M, D, b.nin, D, b.dnin, 1);
    c.lin_dw(b.dnin, D, M, t.w_nd, b.deg, ch, ch, c.gr(t.adeg.w), ch, c.gr(t.adeg.b));
    c.lin_dw(b.dnin + t.w_nd, D, M, t.w_nc, x, ach, ach, c.gr(t.acate.w), ach, c.gr(t.acate.b));
    c.lin_dw(b.dnin + t.w_nd + t.w_nc, D, M, t.w_nd, b.land, K, K, c.gr(t.arw.w), K, c.gr(t.arw.b));
    c.scale(2, R, D, de, c.nod(), de, 0);
    c.bwd(t.eemb, de, R, D, b.ein, D, b.dein, 1);
    c.scale(2, R, D, b.dein, c.nod(), b.dein, 0);
    c.lin_dw(b.dein, D, R, t.w_ec, edge_x + 1, ch, ch - 1, c.gr(t.ecate.w), ch - 1, c.gr(t.ecate.b));
    c.lin_dw(b.dein + t.w_ec, D, R, t.w_ec, edge_x, ch, 1, c.gr(t.eexist.w), 1, c.gr(t.eexist.b));
    c.lin_dw(b.dein + 2 * t.w_ec, D, R, t.w_es, b.onehot, K + 1, K + 1, c.gr(t.espd.w), K + 1, c.gr(t.espd.b));
    // the time MLP behind every block's shifts
    JT_LAUNCH(k_silu_bwd, (long)B * D, s, (long)B * D, (const float*)b.temb, (const float*)b.dtact, b.dtact, c.nod());
    c.bwd(t.time1, b.dtact, B, D, b.t1a, 2 * D, b.sB[0], 0);
    JT_LAUNCH(k_silu_bwd, (long)B * 2 * D, s, (long)B * 2 * D, (const float*)b.t1p, (const float*)b.sB[0], b.sB[0], c.nod());
    c.bwd(t.time0, b.sB[0], B, 2 * D, b.tin, D, nullptr, 0);
}

}  // namespace

extern "C" {

int jodo_cdgs_train_create(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes, const jodo_tensor* params, int n_params, jodo_cdgs_train** out) {
    if (!cfg || !n_nodes || !params || !out || B <= 0 || N <= 0) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_create: null / non-positive argument");
    if (cfg->nf <= 0 || cfg->nf % 32 || cfg->nf / GW != std::min(cfg->nf / 4, 32) || cfg->n_heads <= 0 || cfg->nf % cfg->n_heads)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_cdgs_train_create: nf %d / n_heads %d (GroupNorm groups of %d channels)", cfg->nf, cfg->n_heads, GW);
    if (cfg->n_layers < 1 || cfg->n_layers > 16 || cfg->edge_ch < 2 || cfg->atom_ch < 1 || cfg->rw_depth < 1)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_cdgs_train_create: n_layers %d / edge_ch %d / atom_ch %d / rw_depth %d", cfg->n_layers, cfg->edge_ch,
                              cfg->atom_ch, cfg->rw_depth);
    for (int b = 0; b < B; ++b)
        if (n_nodes[b] < 1 || n_nodes[b] > N) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_create: n_nodes[%d] = %d outside 1..%d", b, n_nodes[b], N);
    // gemm takes its row count as int, and a [rows, 2 nf] array is indexed in long
    if ((long)B * N * N > (1L << 30)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_cdgs_train_create: %ld tile rows", (long)B * N * N);
    jodo_cdgs_train* t = new jodo_cdgs_train();
    t->cfg = *cfg; t->B = B; t->N = N; t->M = (long)B * N; t->R = (long)B * N * N;
    t->D = cfg->nf; t->F = 2 * cfg->nf; t->L = cfg->n_layers; t->H = cfg->n_heads; t->K = cfg->rw_depth; t->ach = cfg->atom_ch; t->ch = cfg->edge_ch;
    t->cat = 2 * t->D / t->L; t->Kc = t->cat * t->L;
    const jcdgs::Widths wd = jcdgs::widths(t->D);
    t->w_es = wd.edge_se; t->w_nd = wd.atom_se; t->w_ec = wd.edge_type; t->w_nc = wd.atom_type;
    t->tables.assign(n_nodes, n_nodes + B);
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
    auto mod = [&](int i) { return "all_modules." + std::to_string(i); };
    const size_t D = t->D, F = t->F, K = t->K, ch = t->ch, ach = t->ach;
    t->time0 = lin(mod(0), 2 * D, D); t->time1 = lin(mod(1), D, 2 * D);
    t->ecate = lin(mod(2), t->w_ec, ch - 1); t->eexist = lin(mod(3), t->w_ec, 1); t->espd = lin(mod(4), t->w_es, K + 1); t->eemb = lin(mod(5), D, D);
    t->adeg = lin(mod(6), t->w_nd, ch); t->acate = lin(mod(7), t->w_nc, ach); t->arw = lin(mod(8), t->w_nd, K); t->aemb = lin(mod(9), D, D);
    t->blk.resize(t->L);
    for (int l = 0; l < t->L; ++l) {
        const std::string p = mod(10 + 3 * l) + ".";
        BlkIx& k = t->blk[l];
        k.t_node = lin(p + "t_node", D, D); k.t_edge = lin(p + "t_edge", D, D);
        k.gin0 = lin(p + "local_model.nn.0", D, D); k.gin2 = lin(p + "local_model.nn.2", D, D); k.eps = find(p + "local_model.eps", 1);
        k.key = lin(p + "self_attn.lin_key", D, D); k.query = lin(p + "self_attn.lin_query", D, D); k.value = lin(p + "self_attn.lin_value", D, D);
        k.le0 = find(p + "self_attn.lin_edge0.weight", D * D); k.le1 = find(p + "self_attn.lin_edge1.weight", D * D);
        k.nl = lin(p + "norm1_local", D, 1); k.na = lin(p + "norm1_attn", D, 1); k.nn = lin(p + "norm2_node", D, 1); k.ne = lin(p + "norm2_edge", D, 1);
        k.ff1 = lin(p + "ff_linear1", F, D); k.ff2 = lin(p + "ff_linear2", D, F); k.ff3 = lin(p + "ff_linear3", F, D); k.ff4 = lin(p + "ff_linear4", D, F);
        k.ro_n = lin(mod(11 + 3 * l), t->cat, D); k.ro_e = lin(mod(12 + 3 * l), t->cat, D);
    }
    const int h0 = 10 + 3 * t->L;
    t->ah[0] = lin(mod(h0), D, t->Kc + t->w_nc); t->ah[1] = lin(mod(h0 + 1), D / 2, D); t->ah[2] = lin(mod(h0 + 2), ach, D / 2);
    t->bh[0] = lin(mod(h0 + 3), D, t->Kc + t->w_ec); t->bh[1] = lin(mod(h0 + 4), D / 2, D); t->bh[2] = lin(mod(h0 + 5), ch - 1, D / 2);
    t->xh[0] = lin(mod(h0 + 6), D, t->Kc + t->w_ec); t->xh[1] = lin(mod(h0 + 7), D / 2, D); t->xh[2] = lin(mod(h0 + 8), 1, D / 2);
    if (!missing.empty()) { delete t; return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_create: parameter '%s' missing or mis-sized", missing.c_str()); }
    if (2 * t->w_ec + t->w_es != t->D || 2 * t->w_nd + t->w_nc != t->D) { delete t; return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_cdgs_train_create: nf %d", t->D); }
    Arena a{nullptr, 0}; Bufs bufs;
    layout(*t, a, bufs);
    t->ws_bytes = a.off;
    *out = t;
    return JODO_OK;
}

void jodo_cdgs_train_destroy(jodo_cdgs_train* t) { delete t; }
size_t jodo_cdgs_train_desc_bytes(const jodo_cdgs_train* t) { return t ? t->tables.size() * sizeof(int) : 0; }
size_t jodo_cdgs_train_workspace_bytes(const jodo_cdgs_train* t) { return t ? t->ws_bytes : 0; }
// option 2 (accepted for parity with jodo_train2d_set_option; the forward keeps the same tensors either way) and option 3: the product
// forms that run in split-bf16 (train_gemm.h GemmEpi::split), a bit mask: 1 forward products, 2 data gradients, 4 weight gradients;
// read by the forward and by the backward when they run.  The host build of this file has no split form: it stays exact fp32 and refuses.
int jodo_cdgs_train_set_option(jodo_cdgs_train* t, int option, int value) {
    if (!t) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_set_option: null handle");
    if (option == 3) {
        if (value < 0 || value > 7) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_set_option: option 3 takes a mask 0..7, got %d", value);
        if (value != 0 && !gemm_split_built)
            return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_cdgs_train_set_option: the host build has no split-bf16 products (exact fp32 only)");
        t->split = value;
        return JODO_OK;
    }
    if (option != 2 || (value != 0 && value != 1)) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_set_option: option %d value %d", option, value);
    return JODO_OK;
}
int jodo_cdgs_train_get_option(const jodo_cdgs_train* t, int option, int* value) {
    if (!t || !value) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_get_option: null argument");
    if (option == 2) *value = 1;
    else if (option == 3) *value = t->split;
    else return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_get_option: option %d", option);
    return JODO_OK;
}
// tests: where a kept tensor lives in the workspace.  0 = h after `layer` blocks [B N, nf] (layer 0 .. n_layers), 1 = e after `layer`
// blocks [B N^2, nf], 2 = alpha of block `layer` [B N^2, n_heads], 3 = xhat of its norm2_edge [B N^2, nf]
int jodo_cdgs_train_debug_locate(const jodo_cdgs_train* t, int what, int layer, size_t* byte_offset, size_t* count) {
    if (!t || !byte_offset || !count) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_locate: null argument");
    if (layer < 0 || layer > t->L || (what >= 2 && layer == t->L)) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_locate: layer %d of %d", layer, t->L);
    Arena a{reinterpret_cast<char*>(256), 0};              // any non-null base: only the differences are used
    Bufs b;
    layout(*t, a, b);
    const float* ptr = nullptr;
    size_t n = 0;
    switch (what) {
        case 0: ptr = b.h[layer]; n = (size_t)t->M * t->D; break;
        case 1: ptr = b.e[layer]; n = (size_t)t->R * t->D; break;
        case 2: ptr = b.blk[layer].alpha; n = (size_t)t->R * t->H; break;
        case 3: ptr = b.blk[layer].xhe; n = (size_t)t->R * t->D; break;
        default: return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_locate: unknown selector %d", what);
    }
    *byte_offset = (size_t)(reinterpret_cast<const char*>(ptr) - reinterpret_cast<const char*>(256));
    *count = n;
    return JODO_OK;
}
// tests: out[rows, F] = the dropout multipliers of rows row0 .. of a [., F] tensor at `site` (any row0: flat indices beyond 2^34 included)
int jodo_cdgs_train_debug_drop(float dropout_p, uint64_t seed, int site, int64_t row0, int rows, int F, float* out, void* stream) {
    if (!out || rows <= 0 || F <= 0 || row0 < 0 || site < 0) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_drop: bad argument");
    Drop d; d.p = dropout_p; d.seed = seed; d.site = (unsigned)site;
    JT_LAUNCH(kc_drop_rows, (long)rows * F, static_cast<hipStream_t>(stream), (long)row0, (long)rows, F, d, out);
    return jodo_check_launch("jodo_cdgs_train_debug_drop");
}
const void* jodo_cdgs_train_desc_host(const jodo_cdgs_train* t) { return t ? t->tables.data() : nullptr; }
int jodo_cdgs_train_upload(jodo_cdgs_train* t, void* desc_dev, void* stream) {
    if (!t || !desc_dev) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_upload: null argument");
    (void)hipMemcpyAsync(desc_dev, t->tables.data(), t->tables.size() * sizeof(int), hipMemcpyHostToDevice, static_cast<hipStream_t>(stream));
    (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));          // the host table may be freed with the handle
    return jodo_check_launch("jodo_cdgs_train_upload");
}

int jodo_cdgs_train_forward(jodo_cdgs_train* t, const void* desc_dev, const float* const* params_dev, int n_params, const float* time_freq, const float* tt,
                            const float* x, const float* edge_x, float dropout_p, uint64_t seed, float* out_x, float* out_e, void* workspace, void* stream) {
    if (!t || !desc_dev || !params_dev || !time_freq || !tt || !x || !edge_x || !out_x || !out_e || !workspace)
        return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_forward: null argument");
    if (n_params != t->n_params) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_forward: %d tensors, handle was created with %d", n_params, t->n_params);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_forward: dropout %g", dropout_p);
    Arena a{static_cast<char*>(workspace), 0}; Bufs bufs;
    layout(*t, a, bufs);
    const Geo g{t->B, t->N, static_cast<const int*>(desc_dev)};
    Ctx c{*t, g, params_dev, nullptr, bufs, static_cast<hipStream_t>(stream), dropout_p, seed, t->split};
    forward(c, tt, time_freq, x, edge_x, out_x, out_e);
    return jodo_check_launch("jodo_cdgs_train_forward");
}

int jodo_cdgs_train_backward(jodo_cdgs_train* t, const void* desc_dev, const float* const* params_dev, float* const* grads_dev, int n_params, const float* x,
                             const float* edge_x, const float* d_out_x, const float* d_out_e, float dropout_p, uint64_t seed, void* workspace, void* stream) {
    if (!t || !desc_dev || !params_dev || !grads_dev || !x || !edge_x || !d_out_x || !d_out_e || !workspace)
        return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_backward: null argument");
    if (n_params != t->n_params) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_backward: %d tensors, handle was created with %d", n_params, t->n_params);
    for (int i = 0; i < n_params; ++i) {
        bool is_eps = false;
        for (const BlkIx& k : t->blk) is_eps |= k.eps == i;
        if (is_eps != (grads_dev[i] == nullptr)) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_backward: gradient slot %d (buffers take null, parameters a buffer)", i);
    }
    Arena a{static_cast<char*>(workspace), 0}; Bufs bufs;
    layout(*t, a, bufs);
    const Geo g{t->B, t->N, static_cast<const int*>(desc_dev)};
    Ctx c{*t, g, params_dev, grads_dev, bufs, static_cast<hipStream_t>(stream), dropout_p, seed, t->split};
    backward(c, x, edge_x, d_out_x, d_out_e);
    return jodo_check_launch("jodo_cdgs_train_backward");
}

// tests: one launch sequence of the step on caller-owned arrays (include/jodo_hip.h).  No kernel and no launch sequence lives here;
// the entry is the safety boundary of tests/test_cdgs_kernels_gpu.py: everything is checked on the host before anything is launched.
int jodo_cdgs_train_debug_op(const jodo_cdgs_op_test_args* args, void* stream) {
    static const char* const OP[JODO_CT_N_OPS] = {"RW", "ADDT", "SCALE", "RELU", "RELU_BWD", "PAIR", "PAIR_BWD", "OUT_NODES", "OUT_EDGES", "SUMS", "GINE",
                                                  "GINE_BWD", "GN_FWD", "GN_BWD", "EGN_FWD", "EGN_BWD", "NORM_GRADS", "ATTN_FWD", "ATTN_BWD"};
    static const char* const SLOT[JODO_CT_N_SLOTS] = {"edge_x", "adj", "ad", "pa", "pb", "cnt", "onehot", "land", "deg", "x", "tb", "y", "z", "eps", "hs", "he",
                                                      "agg", "dagg", "dhe", "dhs", "h", "a", "gamma", "beta", "xhat", "rstd", "dy", "dx", "part", "gsum",
                                                      "dbeta", "dgamma", "q", "k", "v", "g0", "g1", "alpha", "att", "datt", "dv", "dal", "dt1", "dt0", "dq", "dk"};
    if (!args) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op: args is a null pointer");
    const jodo_cdgs_op_test_args& a = *args;
    if (a.op < 0 || a.op >= JODO_CT_N_OPS) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op: unknown op %d", a.op);
    const char* op = OP[a.op];
    if (a.B < 1 || a.N < 1 || !a.n_nodes) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): B %d, N %d or a null n_nodes", op, a.B, a.N);
    if ((long)a.B * a.N * a.N > (1L << 30)) return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_cdgs_train_debug_op(%s): %ld tile rows", op, (long)a.B * a.N * a.N);
    for (int b = 0; b < a.B; ++b)
        if (a.n_nodes[b] < 1 || a.n_nodes[b] > a.N)
            return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): n_nodes[%d] = %d outside 1..%d", op, b, a.n_nodes[b], a.N);
    if (a.D < GW || a.D % GW || a.H < 1 || a.D % a.H || a.F < 1 || a.K < 1 || a.ch < 2)
        return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): D %d (a multiple of %d) / H %d (dividing D) / F %d / K %d / ch %d", op, a.D, GW, a.H, a.F,
                              a.K, a.ch);
    if (a.D > 4096 || a.F > 4096 || a.K > 256 || a.ch > 256)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_cdgs_train_debug_op(%s): D %d / F %d above 4096 or K %d / ch %d above 256", op, a.D, a.F, a.K, a.ch);
    if (!(a.drop_p >= 0.f && a.drop_p < 1.f) || a.drop_site < 0) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): dropout %g at site %d", op, a.drop_p, a.drop_site);
    if ((a.acc != 0 && a.acc != 1) || (a.amask != 0 && a.amask != 1)) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): acc %d / amask %d", op, a.acc, a.amask);
    const int o = a.op;
    const int mode_lo = (o == JODO_CT_OP_ADDT || o == JODO_CT_OP_NORM_GRADS) ? 1 : 0;
    const int mode_hi = (o == JODO_CT_OP_ADDT || o == JODO_CT_OP_NORM_GRADS || o == JODO_CT_OP_SCALE) ? 2 : o == JODO_CT_OP_SUMS ? 1 : 0;
    if (a.mode < mode_lo || a.mode > mode_hi) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): mode %d outside %d..%d", op, a.mode, mode_lo, mode_hi);
    const size_t B = (size_t)a.B, M = B * a.N, R = M * a.N, D = (size_t)a.D, G = D / GW, H = (size_t)a.H, F = (size_t)a.F, K = (size_t)a.K, ch = (size_t)a.ch;
    // rows of the flat ops: the whole tensor (M node rows in mode 1, R tile rows otherwise), or a leading part of it where the op allows
    const size_t full = a.mode == 1 && o != JODO_CT_OP_SUMS ? M : R;
    const bool partial = o == JODO_CT_OP_SCALE || o == JODO_CT_OP_RELU || o == JODO_CT_OP_RELU_BWD || o == JODO_CT_OP_NORM_GRADS;
    if (a.rows < 0 || (size_t)a.rows > full || (a.rows != 0 && !partial))
        return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): rows %ld (0, or 1..%zu where the op takes a leading part)", op, (long)a.rows, full);
    const size_t rows = a.rows ? (size_t)a.rows : full;
    // slot -> element count the op touches; kind 1 = array (exactly that many), 2 = scratch (at least that many)
    size_t need[JODO_CT_N_SLOTS];
    int kind[JODO_CT_N_SLOTS];
    for (int s = 0; s < JODO_CT_N_SLOTS; ++s) { need[s] = 0; kind[s] = 0; }
    auto use = [&](int s, size_t n) { need[s] = n; kind[s] = 1; };
    auto scratch = [&](int s, size_t n) { need[s] = n; kind[s] = 2; };
    switch (o) {
        case JODO_CT_OP_RW:
            use(JODO_CT_EDGE_X, R * ch); use(JODO_CT_ADJ, R); use(JODO_CT_AD, R); use(JODO_CT_CNT, R); use(JODO_CT_ONEHOT, R * (K + 1)); use(JODO_CT_LAND, M * K);
            use(JODO_CT_DEG, M * ch); scratch(JODO_CT_PA, R); scratch(JODO_CT_PB, R);
            break;
        case JODO_CT_OP_ADDT: use(JODO_CT_X, rows * F); use(JODO_CT_TB, B * F); use(JODO_CT_Y, rows * F); break;
        case JODO_CT_OP_SCALE: case JODO_CT_OP_RELU: case JODO_CT_OP_RELU_BWD: use(JODO_CT_X, rows * F); use(JODO_CT_Y, rows * F); break;
        case JODO_CT_OP_PAIR: use(JODO_CT_X, M * D); use(JODO_CT_Y, R * D); break;
        case JODO_CT_OP_PAIR_BWD: use(JODO_CT_X, R * D); use(JODO_CT_Y, M * D); break;
        case JODO_CT_OP_OUT_NODES: use(JODO_CT_X, M * F); use(JODO_CT_Y, M * F); break;
        case JODO_CT_OP_OUT_EDGES: use(JODO_CT_X, R * ch); use(JODO_CT_Y, R * ch); break;
        case JODO_CT_OP_SUMS: use(JODO_CT_X, R * F); use(JODO_CT_Y, M * F); use(JODO_CT_Z, B * F); break;
        case JODO_CT_OP_GINE: case JODO_CT_OP_GINE_BWD:
            use(JODO_CT_EPS, 1); use(JODO_CT_HS, M * D); use(JODO_CT_HE, R * D); use(JODO_CT_ADJ, R);
            if (o == JODO_CT_OP_GINE) use(JODO_CT_AGG, M * D);
            else { use(JODO_CT_DAGG, M * D); use(JODO_CT_DHE, R * D); use(JODO_CT_DHS, M * D); }
            break;
        case JODO_CT_OP_GN_FWD:
            use(JODO_CT_H, M * D); use(JODO_CT_A, M * D); use(JODO_CT_GAMMA, D); use(JODO_CT_BETA, D); use(JODO_CT_XHAT, M * D); use(JODO_CT_RSTD, M * G);
            use(JODO_CT_Y, M * D);
            break;
        case JODO_CT_OP_GN_BWD: use(JODO_CT_DY, M * D); use(JODO_CT_XHAT, M * D); use(JODO_CT_RSTD, M * G); use(JODO_CT_GAMMA, D); use(JODO_CT_DX, M * D); break;
        case JODO_CT_OP_EGN_FWD:
            use(JODO_CT_XHAT, R * D); use(JODO_CT_GAMMA, D); use(JODO_CT_BETA, D); use(JODO_CT_RSTD, B * G); use(JODO_CT_Y, R * D);
            scratch(JODO_CT_PART, egn_part_floats(M, G)); scratch(JODO_CT_GSUM, 2 * 2 * B * G);
            break;
        case JODO_CT_OP_EGN_BWD:
            use(JODO_CT_DY, R * D); use(JODO_CT_XHAT, R * D); use(JODO_CT_RSTD, B * G); use(JODO_CT_GAMMA, D); use(JODO_CT_DX, R * D);
            scratch(JODO_CT_PART, egn_part_floats(M, G)); scratch(JODO_CT_GSUM, 2 * 2 * B * G);
            break;
        case JODO_CT_OP_NORM_GRADS:
            use(JODO_CT_DY, rows * F); use(JODO_CT_XHAT, rows * F); use(JODO_CT_DBETA, F); use(JODO_CT_DGAMMA, F); scratch(JODO_CT_PART, colsum_part_floats(rows, F));
            break;
        case JODO_CT_OP_ATTN_FWD: case JODO_CT_OP_ATTN_BWD:
            use(JODO_CT_Q, M * D); use(JODO_CT_K, M * D); use(JODO_CT_V, M * D); use(JODO_CT_G0, R * D); use(JODO_CT_G1, R * D); use(JODO_CT_ALPHA, R * H);
            if (o == JODO_CT_OP_ATTN_FWD) use(JODO_CT_ATT, M * D);
            else {
                use(JODO_CT_DATT, M * D); use(JODO_CT_DV, M * D); use(JODO_CT_DAL, R * H); use(JODO_CT_DT1, R * D); use(JODO_CT_DT0, R * D); use(JODO_CT_DQ, M * D);
                use(JODO_CT_DK, M * D);
            }
            break;
    }
    for (int s = 0; s < JODO_CT_N_SLOTS; ++s) {
        if (!kind[s]) continue;
        if (kind[s] == 2 ? a.n[s] < need[s] : a.n[s] != need[s])
            return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): array %s has %zu elements, the op touches %zu", op, SLOT[s], a.n[s], need[s]);
        if (!a.a[s]) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): array %s is a null pointer", op, SLOT[s]);
        if (((uintptr_t)a.a[s] & 15) != 0) return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): array %s is not 16-byte aligned", op, SLOT[s]);
    }
    if (!a.nn_dev || a.nn_dev_count < B || ((uintptr_t)a.nn_dev & 15) != 0)
        return jodo_set_error(JODO_ERR_ARG, "jodo_cdgs_train_debug_op(%s): nn_dev is null, misaligned or holds %zu counts of %zu", op, a.nn_dev_count, B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(a.nn_dev, a.n_nodes, B * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return jodo_set_error(JODO_ERR_LAUNCH, "jodo_cdgs_train_debug_op(%s): upload of the counts failed", op);      // (the caller may free n_nodes: wait)
    const Geo g{a.B, a.N, a.nn_dev};
    Drop d; d.p = a.drop_p; d.seed = a.drop_seed; d.site = (unsigned)a.drop_site;
    auto A = [&](int slot) { return a.a[slot]; };
    auto C = [&](int slot) { return (const float*)a.a[slot]; };
    const long Ml = (long)M, Rl = (long)R, rl = (long)rows;
    switch (o) {
        case JODO_CT_OP_RW:
            rw_prologue(s, g, a.K, a.ch, C(JODO_CT_EDGE_X), A(JODO_CT_ADJ), A(JODO_CT_AD), A(JODO_CT_PA), A(JODO_CT_PB), A(JODO_CT_CNT), A(JODO_CT_ONEHOT),
                        A(JODO_CT_LAND), A(JODO_CT_DEG));
            break;
        case JODO_CT_OP_ADDT: JT_LAUNCH(kc_addt, rl * a.F, s, g, a.mode, rl, a.F, C(JODO_CT_X), C(JODO_CT_TB), A(JODO_CT_Y)); break;
        case JODO_CT_OP_SCALE: JT_LAUNCH(kc_scale, rl * a.F, s, g, a.mode, rl, a.F, C(JODO_CT_X), d, A(JODO_CT_Y), a.acc); break;
        case JODO_CT_OP_RELU: JT_LAUNCH(kc_relu, rl * a.F, s, rl * a.F, C(JODO_CT_X), A(JODO_CT_Y)); break;
        case JODO_CT_OP_RELU_BWD: JT_LAUNCH(kc_relu_bwd, rl * a.F, s, rl * a.F, C(JODO_CT_X), A(JODO_CT_Y)); break;
        case JODO_CT_OP_PAIR: JT_LAUNCH(kc_pair, Rl * a.D, s, g, a.D, C(JODO_CT_X), A(JODO_CT_Y)); break;
        case JODO_CT_OP_PAIR_BWD: JT_LAUNCH(kc_pair_bwd, Ml * a.D, s, g, a.D, C(JODO_CT_X), A(JODO_CT_Y)); break;
        case JODO_CT_OP_OUT_NODES: JT_LAUNCH(kc_out_nodes, Ml * a.F, s, g, a.F, C(JODO_CT_X), A(JODO_CT_Y)); break;
        case JODO_CT_OP_OUT_EDGES: JT_LAUNCH(kc_out_edges, Rl * a.ch, s, g, a.ch, C(JODO_CT_X), A(JODO_CT_Y)); break;
        case JODO_CT_OP_SUMS: tile_sums(s, g, a.F, C(JODO_CT_X), A(JODO_CT_Y), a.mode, A(JODO_CT_Z)); break;
        case JODO_CT_OP_GINE: JT_LAUNCH(kc_gine, Ml * a.D, s, g, a.D, C(JODO_CT_EPS), C(JODO_CT_HS), C(JODO_CT_HE), C(JODO_CT_ADJ), A(JODO_CT_AGG)); break;
        case JODO_CT_OP_GINE_BWD:
            gine_backward(s, g, a.D, C(JODO_CT_EPS), C(JODO_CT_HS), C(JODO_CT_HE), C(JODO_CT_ADJ), C(JODO_CT_DAGG), A(JODO_CT_DHE), A(JODO_CT_DHS));
            break;
        case JODO_CT_OP_GN_FWD:
            JT_LAUNCH(kc_gn_fwd, Ml * (long)G, s, g, Ml, a.D, C(JODO_CT_H), C(JODO_CT_A), d, a.amask, C(JODO_CT_GAMMA), C(JODO_CT_BETA), A(JODO_CT_XHAT),
                      A(JODO_CT_RSTD), A(JODO_CT_Y), a.acc);
            break;
        case JODO_CT_OP_GN_BWD:
            JT_LAUNCH(kc_gn_bwd, Ml * (long)G, s, g, Ml, a.D, C(JODO_CT_DY), C(JODO_CT_XHAT), C(JODO_CT_RSTD), C(JODO_CT_GAMMA), A(JODO_CT_DX), a.acc);
            break;
        case JODO_CT_OP_EGN_FWD:
            egn_forward(s, g, a.D, A(JODO_CT_XHAT), C(JODO_CT_GAMMA), C(JODO_CT_BETA), reinterpret_cast<double*>(A(JODO_CT_PART)),
                        reinterpret_cast<double*>(A(JODO_CT_GSUM)), A(JODO_CT_RSTD), A(JODO_CT_Y));
            break;
        case JODO_CT_OP_EGN_BWD:
            egn_backward(s, g, a.D, C(JODO_CT_DY), C(JODO_CT_XHAT), C(JODO_CT_RSTD), C(JODO_CT_GAMMA), reinterpret_cast<double*>(A(JODO_CT_PART)),
                         reinterpret_cast<double*>(A(JODO_CT_GSUM)), A(JODO_CT_DX));
            break;
        case JODO_CT_OP_NORM_GRADS:
            colsum_grads(s, g, a.mode, rl, a.F, C(JODO_CT_DY), C(JODO_CT_XHAT), reinterpret_cast<double*>(A(JODO_CT_PART)), A(JODO_CT_DBETA), A(JODO_CT_DGAMMA));
            break;
        case JODO_CT_OP_ATTN_FWD:
            attn_forward(s, g, a.D, a.H, a.isc, C(JODO_CT_Q), C(JODO_CT_K), C(JODO_CT_V), C(JODO_CT_G0), C(JODO_CT_G1), A(JODO_CT_ALPHA), A(JODO_CT_ATT));
            break;
        case JODO_CT_OP_ATTN_BWD: {
            const AttnBwd ab{C(JODO_CT_DATT), C(JODO_CT_Q), C(JODO_CT_K), C(JODO_CT_V), C(JODO_CT_G0), C(JODO_CT_G1), C(JODO_CT_ALPHA), A(JODO_CT_DV),
                             A(JODO_CT_DAL), A(JODO_CT_DT1), A(JODO_CT_DT0), A(JODO_CT_DQ), A(JODO_CT_DK)};
            attn_backward(s, g, a.D, a.H, a.isc, ab, [](int) {});
            break;
        }
    }
    return jodo_check_launch("jodo_cdgs_train_debug_op");
}

}  // extern "C"

// Training step of the 2-D score network (DGT_concat_2D) behind the C ABI: jodo_train2d_forward evaluates the network with every
// activation the backward needs kept in the caller's workspace (dropout active when p > 0, as under model.train()), and
// jodo_train2d_backward returns d loss / d parameter for all 235 tensors of the state_dict given d loss / d outputs — what
// loss.backward() computes through
//   DGT_concat_2D.forward                models/mol_gnn.py:868-946 of the reference
//   EquivariantMixBlock_2D.forward       models/mol_gnn.py:325-407
//   TransMixLayer (one adjacency head)   models/layers.py:131-186
// The design is the 3-D training path's (dgt_train.hip), not the 2-D inference path's: dense DIRECTED n x n tiles per molecule
// (the reference draws the edge FFN's dropout per directed edge, so under model.train() the edge state stops being symmetric after
// the first block and the once-per-pair layout of dgt2d_forward.hip cannot express it), parameters in their PyTorch layouts,
// jt::gemm for every projection and both of its gradient products, train_ops.h for everything else.  The block is the 3-D block
// without the Gaussian basis, the per-block edge_emb and the equivariant update; H = 16, XH = 1, SC = 17 (QK = 255).
// Dropout sites and element numbering are the 3-D path's (site = 8 l + {A1 1, F2 2, A3 3, F4 4}; edge element = row of the dense
// tile, diagonal carried), so oracle/philox_ref.dropout_masks restates the masks unchanged.
// Gradient buffers are fully written (zeroed, then accumulated in a fixed launch order: bit-deterministic, no atomics).
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
#define JT_OPS_NS jt2d        // this translation unit's own copy of the train_ops.h kernels (dgt_train.hip owns jt::k_*)
#include "train_ops.h"
#include "train_fused.h"

using namespace jt;
using namespace jt2d;

namespace {

struct Lin { int w = -1, b = -1; };
struct BlkIx {
    Lin n2e, key, query, value, ff1, ff2, ff3, ff4, node_time, edge_time, node_ro, edge_ro;
    int le0 = -1, le1 = -1;
};

struct Arena {
    char* base; size_t off;
    float* f(size_t n) { const size_t o = off; off += (n * 4 + 255) / 256 * 256; return base ? reinterpret_cast<float*>(base + o) : nullptr; }
    int* i(size_t n) { return reinterpret_cast<int*>(f(n)); }
};

struct BlkBuf {
    float *nmod, *emod, *xh_e1, *rs_e1, *et, *xh_h, *rs_h, *ht, *q, *k, *v, *qkv, *t0, *t1, *alpha, *hhat, *n2e;
    float *xh_hn, *rs_hn, *hn, *f1, *a1, *f2, *xh_en, *rs_en, *en, *f3, *a3, *f4;
};
struct Bufs {
    int* flags;
    float *feat, *t1pre, *t1a, *temb, *tau;
    float *nin, *ein, *adj2d, *ah, *eh;
    std::vector<float*> h, e;
    std::vector<BlkBuf> blk;
    float *nh1pre, *nh1, *nh2pre, *nh2, *atom, *x1pre[2], *x1[2], *x2pre[2], *x2[2], *Ep;
    // scratch shared by all phases
    float *tE_D, *tE_De[4], *tE_QK, *tE_rD, *tE_H, *tN_D[4], *tN_QK[2], *tN_rD, *tN_De, *tN_nd, *tE_ch, *tRow[2], *tcatn, *tcate;
    float *dtau, *dtemb, *tB_T[2], *part, *part2, *rowpart, *splitk;
    float *Wall, *ball, *mods_all, *dmods_all, *dWall, *dball;      // batched modulation projections (train_ops.h ModTable)
    float *Wqkv, *bqkv, *dqkv, *dWqkv, *dbqkv;                      // lin_query / lin_key / lin_value of a block as one product
    size_t splitk_floats;
    float* fpack;                     // packed MFMA operands of the fused chains (forward + transposed images), one slice per block
    size_t fpack_block;
    float* tE_De2[2];                 // scratch of the fused backward chain B': d f4 | d en
};

// ---- the element-wise kernels the 3-D set has no position-free form of -------------------------------------------------------
// nin[i, 0:nd] = xh, [nd:2 nd] = cond_x (0 on the first step)
__global__ void k2_pack_nodes(Topo t, int nd, const float* __restrict__ xh, const float* __restrict__ cond_x, float* __restrict__ nin) {
    JT_IDX((long)t.Nn * nd);
    const int node = (int)(i_ / nd), j = (int)(i_ % nd);
    const int b = t.node_mol[node], i = node - t.node_off[b];
    const long src = ((long)b * t.N + i) * nd + j;
    nin[(long)node * 2 * nd + j] = xh[src];
    nin[(long)node * 2 * nd + nd + j] = cond_x ? cond_x[src] : 0.f;
}
// ein[r, 0:ch] = edge_x, [ch:2 ch] = cond_edge_x (0 on the first step); adjacency head: cond_edge_x[..., 0] >= edge_th, or 1 without
// a conditioning input (mol_gnn.py:893-899)
__global__ void k2_pack_edges(Topo t, int ch, float edge_th, const float* __restrict__ edge_x, const float* __restrict__ cond_edge_x,
                              float* __restrict__ ein, float* __restrict__ adj2d) {
    JT_IDX(t.R);
    const int b = t.edge_mol[i_], n = t.nn[b];
    const int loc = (int)(i_ - t.edge_off[b]), a = loc / n, c = loc % n;
    const long src = (((long)b * t.N + a) * t.N + c) * ch;
    for (int k = 0; k < ch; ++k) { ein[i_ * 2 * ch + k] = edge_x[src + k]; ein[i_ * 2 * ch + ch + k] = cond_edge_x ? cond_edge_x[src + k] : 0.f; }
    adj2d[i_] = cond_edge_x ? (cond_edge_x[src] >= edge_th ? 1.f : 0.f) : 1.f;
}
// out_xh[b, i, :] = atom inside the molecule, 0 on padding
__global__ void k2_node_out(Topo t, int nd, const float* __restrict__ atom, float* __restrict__ out) {
    JT_IDX((long)t.B * t.N * nd);
    const int j = (int)(i_ % nd);
    const long x = i_ / nd;
    const int i = (int)(x % t.N), b = (int)(x / t.N);
    out[i_] = i < t.nn[b] ? atom[((long)t.node_off[b] + i) * nd + j] : 0.f;
}
__global__ void k2_node_out_bwd(Topo t, int nd, const float* __restrict__ dout, float* __restrict__ datom) {
    JT_IDX((long)t.Nn * nd);
    const long r = i_ / nd; const int j = (int)(i_ % nd);
    const int b = t.node_mol[r], i = (int)r - t.node_off[b];
    datom[i_] = dout[((long)b * t.N + i) * nd + j];
}

}  // namespace

struct jodo_train2d {
    jodo_cfg2d cfg;
    int B, N, Nn, R;
    int D, De, T, L, H, XH, SC, QK, C, r, nd, ch, cn, ce, catn, cate, half;
    std::vector<int> tables;          // node_off | edge_off | nn | node_mol | edge_mol | edge_a | edge_c | ec_off | ec_mol_off
    size_t o_node_off, o_edge_off, o_nn, o_node_mol, o_edge_mol, o_edge_a, o_edge_c, o_ec_off, o_ec_mol_off;
    int NC;
    int n_params;
    std::vector<size_t> numel;
    Lin node_emb, edge_emb, np0, np2, np4, et0, et2, et4, ee0, ee2, ee4, time1, time3;
    int time_w;
    std::vector<BlkIx> blk;
    size_t ws_bytes;
    int fused;                        // option 0: 1 = chain A, chain B and the node LayerNorms of a block run as fused kernels (train_fused.hip)
    int fused_bwd;                    // option 1: their input-gradient sides too (the weight-gradient products stay GEMMs)
    int save_activations;             // option 2: 0 = the following forwards are not followed by a backward: the fused chains skip backward-only stores
    int Mtot;                         // modulation floats per molecule: L (6 D + 6 De)
};

namespace {

void layout(const jodo_train2d& t, Arena& a, Bufs& b) {
    const size_t B = t.B, Nn = t.Nn, R = t.R, D = t.D, De = t.De, T = t.T, L = t.L, QK = t.QK, H = t.H, r = t.r, nd = t.nd, ch = t.ch;
    b.flags = a.i(8);
    b.feat = a.f(B * (2 * t.half + 1)); b.t1pre = a.f(B * T); b.t1a = a.f(B * T); b.temb = a.f(B * T); b.tau = a.f(B * T);
    b.nin = a.f(Nn * 2 * nd); b.ein = a.f(R * 2 * ch); b.adj2d = a.f(R);
    b.ah = a.f(Nn * t.catn); b.eh = a.f(R * t.cate);
    b.h.resize(L + 1); b.e.resize(L + 1);
    for (size_t l = 0; l <= L; ++l) { b.h[l] = a.f(Nn * D); b.e[l] = a.f(R * De); }
    b.blk.resize(L);
    for (size_t l = 0; l < L; ++l) {
        BlkBuf& k = b.blk[l];
        k.nmod = a.f(B * 6 * D); k.emod = a.f(B * 6 * De);
        k.xh_e1 = a.f(R * De); k.rs_e1 = a.f(R); k.et = a.f(R * De);
        k.xh_h = a.f(Nn * D); k.rs_h = a.f(Nn); k.ht = a.f(Nn * D); k.q = a.f(Nn * QK); k.k = a.f(Nn * QK); k.v = a.f(Nn * D);
        k.qkv = a.f(Nn * (2 * QK + D));
        k.t0 = a.f(R * QK); k.t1 = a.f(R * D); k.alpha = a.f(R * H); k.hhat = a.f(Nn * D); k.n2e = a.f(Nn * De);
        k.xh_hn = a.f(Nn * D); k.rs_hn = a.f(Nn); k.hn = a.f(Nn * D); k.f1 = a.f(Nn * r * D); k.a1 = a.f(Nn * r * D); k.f2 = a.f(Nn * D);
        k.xh_en = a.f(R * De); k.rs_en = a.f(R); k.en = a.f(R * De); k.f3 = a.f(R * r * De); k.a3 = a.f(R * r * De); k.f4 = a.f(R * De);
    }
    b.nh1pre = a.f(Nn * D); b.nh1 = a.f(Nn * D); b.nh2pre = a.f(Nn * D / 2); b.nh2 = a.f(Nn * D / 2); b.atom = a.f(Nn * nd);
    for (int s = 0; s < 2; ++s) { b.x1pre[s] = a.f(R * De); b.x1[s] = a.f(R * De); b.x2pre[s] = a.f(R * De / 2); b.x2[s] = a.f(R * De / 2); }
    b.Ep = a.f(R * ch);
    b.tE_D = a.f(R * D);
    for (int s = 0; s < 4; ++s) b.tE_De[s] = a.f(R * De);
    b.tE_QK = a.f(R * QK); b.tE_rD = a.f(R * r * De); b.tE_H = a.f(R * H);
    for (int s = 0; s < 4; ++s) b.tN_D[s] = a.f(Nn * D);
    for (int s = 0; s < 2; ++s) b.tN_QK[s] = a.f(Nn * QK);
    b.tN_rD = a.f(Nn * r * D); b.tN_De = a.f(Nn * De); b.tN_nd = a.f(Nn * nd); b.tE_ch = a.f(R * ch);
    const size_t rows = R > Nn ? R : Nn;
    for (int s = 0; s < 2; ++s) b.tRow[s] = a.f(rows);
    b.tcatn = a.f(Nn * t.catn); b.tcate = a.f(R * t.cate);
    b.dtau = a.f(B * T); b.dtemb = a.f(B * T);
    for (int s = 0; s < 2; ++s) b.tB_T[s] = a.f(B * T);
    const size_t maxF = std::max<size_t>({(size_t)6 * D, T, r * D});
    const size_t part_floats = ((rows + 31) / 32 + B + 1) * maxF;        // first-level partial sums: 32-row chunks x the widest reduced array
    b.part = a.f(part_floats);
    b.part2 = a.f((part_floats / maxF / 32 + 2) * maxF);
    b.rowpart = a.f(rows * 16);                               // eight (sum, sum of squares) pairs per row
    b.splitk_floats = (size_t)32 << 20;                       // 128 MiB of split-K partial tiles at most
    const size_t need = ((rows + 1023) / 1024 + 1) * (size_t)D * (2 * D + 2 * De);
    if (b.splitk_floats > need) b.splitk_floats = need;
    b.splitk = a.f(b.splitk_floats);
    const size_t Mt = (size_t)t.Mtot;
    b.Wall = a.f(Mt * T); b.ball = a.f(Mt); b.mods_all = a.f(B * Mt); b.dmods_all = a.f(B * Mt); b.dWall = a.f(Mt * T); b.dball = a.f(Mt);
    const size_t F3 = 2 * QK + D;
    b.Wqkv = a.f(L * F3 * D); b.bqkv = a.f(L * F3); b.dqkv = a.f(Nn * F3); b.dWqkv = a.f(L * F3 * D); b.dbqkv = a.f(L * F3);
    const FusedDims fd{t.D, t.De, t.r, t.QK, t.ce, t.L};
    b.fpack_block = fused_pack_layout(fd).total_bwd;
    b.fpack = a.f(b.fpack_block * L);
    for (int s = 0; s < 2; ++s) b.tE_De2[s] = a.f(R * De);
}

// The launch helpers of dgt_train.hip's Ctx in their immediate form (the op-by-op sequence queues nothing)
struct Ctx {
    const jodo_train2d& t; Topo tp; const float* const* P; float* const* G; Bufs& b; hipStream_t s;
    const float* p(int i) const { return P[i]; }
    float* g(int i) const { return G[i]; }
    Drop drop(float p, unsigned long long seed, int l, int site) const { Drop d; d.p = p; d.seed = seed; d.site = (unsigned)(l * 8 + site); return d; }
    // Y[rows, N] (ldy) (+)= X[rows, K] (ldx) W[N, K]^T (ldw) + bias
    void lin(const float* X, int ldx, int rows, int K, const float* W, int ldw, int N, const float* bias, float* Y, int ldy, int acc) const {
        gemm(s, 0, 1, rows, N, K, X, ldx, W, ldw, Y, ldy, bias, acc, b.splitk, b.splitk_floats);
    }
    void lin_tanh(const float* X, int ldx, int rows, int K, const float* W, int ldw, int N, const float* bias, float* Y) const {
        GemmEpi e; e.act = 1; e.out2 = nullptr; e.drop = drop(0.f, 0, 0, 0); e.dbias = nullptr;
        gemm(s, 0, 1, rows, N, K, X, ldx, W, ldw, Y, N, bias, 0, b.splitk, b.splitk_floats, &e);
    }
    // pre = X W^T + bias (kept for the backward), act = SiLU(pre) * dropout; both dense [rows, N]
    void lin_silu(const float* X, int ldx, int rows, int K, const float* W, int ldw, int N, const float* bias, float* pre, float* act, Drop d) const {
        GemmEpi e; e.act = 2; e.out2 = act; e.drop = d; e.dbias = nullptr;
        gemm(s, 0, 1, rows, N, K, X, ldx, W, ldw, pre, N, bias, 0, b.splitk, b.splitk_floats, &e);
    }
    // dX[rows, K] (ldx) (+)= dY[rows, N] (ldy) W[N, K] (ldw)
    void lin_dx(const float* dY, int ldy, int rows, int N, const float* W, int ldw, int K, float* dX, int ldx, int acc) const {
        gemm(s, 0, 0, rows, K, N, dY, ldy, W, ldw, dX, ldx, nullptr, acc, b.splitk, b.splitk_floats);
    }
    // dW[N, K] (lddw) += dY[rows, N]^T X[rows, K]; db[N] += column sums of dY
    void lin_dw(const float* dY, int ldy, int rows, int N, const float* X, int ldx, int K, float* dW, int lddw, float* db = nullptr) const {
        GemmEpi e; e.act = 0; e.out2 = nullptr; e.drop = drop(0.f, 0, 0, 0); e.dbias = db;
        gemm(s, 1, 0, N, K, rows, dY, ldy, X, ldx, dW, lddw, nullptr, 1, b.splitk, b.splitk_floats, &e);
    }
    void seg_edge(int F, const float* a, const float* bb, float* out, int ldo, int ocol) const {
        JT_LAUNCH(k_seg_part, (long)tp.NC * F, s, tp.NC, F, tp.ec_off, a, bb, b.part);
        JT_LAUNCH(k_seg_fin, (long)t.B * F, s, t.B, F, tp.ec_mol_off, (const float*)b.part, out, ldo, ocol, 0);
    }
    void seg_edge_ehat(int F, const float* a, const float* p, const float* bias, float* out, int ldo, int ocol) const {
        JT_LAUNCH(k_seg_part_ehat, (long)tp.NC * F, s, tp, F, a, p, bias, b.part);
        JT_LAUNCH(k_seg_fin, (long)t.B * F, s, t.B, F, tp.ec_mol_off, (const float*)b.part, out, ldo, ocol, 0);
    }
    void seg2_edge(int F, const float* a, const float* bb, float* out, int ldo, int c1, int c2) const {
        JT_LAUNCH(k_seg_part2, (long)tp.NC * F, s, tp.NC, F, tp.ec_off, a, bb, b.part);
        JT_LAUNCH(k_seg_fin2, (long)t.B * 2 * F, s, t.B, F, tp.ec_mol_off, (const float*)b.part, out, ldo, c1, c2);
    }
    void seg(int F, const int* off, const float* a, const float* bb, float* out, int ldo, int ocol) const {
        if (off == tp.edge_off) seg_edge(F, a, bb, out, ldo, ocol);
        else JT_LAUNCH(k_seg_colsum, (long)t.B * F, s, t.B, F, off, a, bb, out, ldo, ocol, 0, drop(0.f, 0, 0, 0));
    }
    void seg_node_drop(int F, const float* a, const float* bb, Drop db, float* out, int ldo, int ocol) const {
        JT_LAUNCH(k_seg_colsum, (long)t.B * F, s, t.B, F, tp.node_off, a, bb, out, ldo, ocol, 0, db);
    }
    void silu(long n, const float* x, float* y, Drop d) const { JT_LAUNCH(k_silu_fwd, n, s, n, x, y, d); }
    void silu_bwd(long n, const float* x, const float* dy, float* dx, Drop d) const { JT_LAUNCH(k_silu_bwd, n, s, n, x, dy, dx, d); }
    void stats(long rows, int F, const float* x, float* mean, float* rstd) const {
        JT_LAUNCH(k_row_part, rows * 8, s, rows, F, x, b.rowpart);
        JT_LAUNCH(k_row_stats, rows, s, rows, F, x, (const float*)b.rowpart, mean, rstd);
    }
    void ln_mod(long rows, int F, const float* x, const float* mean, const float* rstd, const int* row_mol, const float* mods, int ldm, int sh, int sc,
                float* xhat, float* y) const {
        JT_LAUNCH(k_ln_mod_fwd, rows * F, s, rows, F, x, mean, rstd, row_mol, mods, ldm, sh, sc, xhat, y);
    }
    // LayerNorm + modulate backward: modulation gradients into dmods[:, sh], [:, sc] (written), dx (acc)
    void ln_mod_bwd(long rows, int F, const float* dy, const float* xhat, const float* rstd, const int* row_mol, const int* seg_off, const float* mods,
                    int ldm, int sh, int sc, float* dmods, int ldd, float* dx, int acc) const {
        if (seg_off == tp.edge_off) seg2_edge(F, dy, xhat, dmods, ldd, sh, sc);
        else JT_LAUNCH(k_seg_colsum2, (long)t.B * F, s, t.B, F, seg_off, dy, xhat, dmods, ldd, sh, sc);
        if (t.fused_bwd && seg_off != tp.edge_off) {             // node rows: the two row means and the result in one launch, a wave per row
            fused_node_ln_mod_bwd(s, rows, F, dy, xhat, rstd, row_mol, mods, ldm, sc, dx, acc);
            return;
        }
        JT_LAUNCH(k_ln_bwd_part, rows * 8, s, rows, F, dy, xhat, row_mol, mods, ldm, sc, b.rowpart);
        JT_LAUNCH(k_ln_bwd_stats, rows, s, rows, F, (const float*)b.rowpart, b.tRow[0], b.tRow[1]);
        JT_LAUNCH(k_ln_bwd_apply, rows * F, s, rows, F, dy, xhat, rstd, (const float*)b.tRow[0], (const float*)b.tRow[1], row_mol, mods,
                           ldm, sc, dx, acc);
    }
    void copy2d(long rows, int F, const float* src, int lds, int scol, float* dst, int ldd, int dcol, int acc) const {
        JT_LAUNCH(k_copy2d, rows * F, s, rows, F, src, lds, scol, dst, ldd, dcol, acc);
    }
};

enum { SITE_ALPHA = 0, SITE_A1, SITE_F2, SITE_A3, SITE_F4 };       // dgt_train.hip's numbering (SITE_ALPHA is an identity there and here)

// MLP head: Linear SiLU Linear SiLU Linear; saves the two pre-activations and activations
void head_fwd(const Ctx& c, const float* X, int ldx, long rows, int K, Lin l0, Lin l2, Lin l4, int H1, int H2, int NO, float* p1, float* a1, float* p2, float* a2,
              float* out, int ldo) {
    const Drop nod = c.drop(0.f, 0, 0, 0);
    c.lin_silu(X, ldx, rows, K, c.p(l0.w), K, H1, c.p(l0.b), p1, a1, nod);
    c.lin_silu(a1, H1, rows, H1, c.p(l2.w), H1, H2, c.p(l2.b), p2, a2, nod);
    c.lin(a2, H2, rows, H2, c.p(l4.w), H2, NO, c.p(l4.b), out, ldo, 0);
}
void head_bwd(const Ctx& c, const float* X, int ldx, long rows, int K, Lin l0, Lin l2, Lin l4, int H1, int H2, int NO, const float* p1, const float* a1,
              const float* p2, const float* a2, const float* dOut, int ldo, float* t1, float* t2, float* dX, int lddx, int acc) {
    const Drop nod = c.drop(0.f, 0, 0, 0);
    c.lin_dw(dOut, ldo, rows, NO, a2, H2, H2, c.g(l4.w), H2, c.g(l4.b));
    c.lin_dx(dOut, ldo, rows, NO, c.p(l4.w), H2, H2, t2, H2, 0);
    c.silu_bwd(rows * H2, p2, t2, t2, nod);
    c.lin_dw(t2, H2, rows, H2, a1, H1, H1, c.g(l2.w), H1, c.g(l2.b));
    c.lin_dx(t2, H2, rows, H2, c.p(l2.w), H1, H1, t1, H1, 0);
    c.silu_bwd(rows * H1, p1, t1, t1, nod);
    c.lin_dw(t1, H1, rows, H1, X, ldx, K, c.g(l0.w), K, c.g(l0.b));
    c.lin_dx(t1, H1, rows, H1, c.p(l0.w), K, K, dX, lddx, acc);
}

// the 2 L modulation projections in the order of their columns in [., Mtot]: per block node | edge
int mod_entries(const jodo_train2d& t, Lin* lin, int* F, int* col) {
    int n = 0, at = 0;
    for (int l = 0; l < t.L; ++l) {
        lin[n] = t.blk[l].node_time; F[n] = 6 * t.D; col[n] = at; at += F[n]; ++n;
        lin[n] = t.blk[l].edge_time; F[n] = 6 * t.De; col[n] = at; at += F[n]; ++n;
    }
    return n;
}

void forward(const Ctx& c, const float* xh, const float* edge_x, const float* cond_x, const float* cond_edge_x, const float* nl,
             float p_drop, unsigned long long seed, float* out_xh, float* out_edge) {
    const jodo_train2d& t = c.t; Bufs& b = c.b; const Topo& tp = c.tp; hipStream_t s = c.s;
    const int B = t.B, Nn = t.Nn, R = t.R, D = t.D, De = t.De, T = t.T, L = t.L, QK = t.QK, H = t.H, r = t.r, nd = t.nd, ch = t.ch;
    const int F17 = 2 * t.half + 1;
    const Drop nod = c.drop(0.f, 0, 0, 0);
    (void)hipMemsetAsync(b.flags, 0, 8 * sizeof(int), s);
    JT_LAUNCH(k2_pack_nodes, (long)Nn * nd, s, tp, nd, xh, cond_x, b.nin);
    JT_LAUNCH(k2_pack_edges, R, s, tp, ch, t.cfg.edge_quan_th, edge_x, cond_edge_x, b.ein, b.adj2d);
    // time embedding (mol_gnn.py:880-886)
    JT_LAUNCH(k_time_feat, (long)B * F17, s, B, t.half, nl, c.p(t.time_w), b.feat);
    c.lin(b.feat, F17, B, F17, c.p(t.time1.w), F17, T, c.p(t.time1.b), b.t1pre, T, 0);
    JT_LAUNCH(k_gelu_fwd, (long)B * T, s, (long)B * T, (const float*)b.t1pre, b.t1a);
    c.lin(b.t1a, T, B, T, c.p(t.time3.w), T, T, c.p(t.time3.b), b.temb, T, 0);
    c.silu((long)B * T, b.temb, b.tau, nod);
    {   // every modulation row of every block in ONE product (train_ops.h ModTable): gather the weights, project, hand the rows out
        ModTable M;
        Lin lin[MOD_MAX]; int F[MOD_MAX], col[MOD_MAX];
        M.n = mod_entries(t, lin, F, col);
        int fmax = 0;
        for (int i = 0; i < M.n; ++i) {
            M.w[i] = c.p(lin[i].w); M.bias[i] = c.p(lin[i].b); M.F[i] = F[i]; M.col[i] = col[i];
            M.out[i] = (i & 1) ? b.blk[i / 2].emod : b.blk[i / 2].nmod;
            fmax = F[i] > fmax ? F[i] : fmax;
        }
        hipLaunchKernelGGL(k_mod_gather, dim3((unsigned)(((long)fmax * T + 255) / 256), (unsigned)M.n), dim3(256), 0, s, M, T, b.Wall, b.ball);
        c.lin(b.tau, T, B, T, b.Wall, T, t.Mtot, b.ball, b.mods_all, t.Mtot, 0);
        hipLaunchKernelGGL(k_mod_scatter, dim3((unsigned)(((long)B * fmax + 255) / 256), (unsigned)M.n), dim3(256), 0, s, M, B, t.Mtot, (const float*)b.mods_all);
    }
    const int F3 = 2 * QK + D;
    {   // lin_query | lin_key | lin_value of every block gathered into [L][2 QK + D, D]: one product per block (and two in its backward)
        ModTable M;
        M.n = 3 * L;
        for (int l = 0; l < L; ++l) {
            const BlkIx& ix = t.blk[l];
            const Lin ls[3] = {ix.query, ix.key, ix.value};
            for (int j = 0; j < 3; ++j) {
                const int i = 3 * l + j;
                M.w[i] = c.p(ls[j].w); M.bias[i] = c.p(ls[j].b); M.out[i] = nullptr; M.F[i] = j < 2 ? QK : D; M.col[i] = l * F3 + j * QK;
            }
        }
        hipLaunchKernelGGL(k_mod_gather, dim3((unsigned)(((long)D * D + 255) / 256), (unsigned)M.n), dim3(256), 0, s, M, D, b.Wqkv, b.bqkv);
    }
    // embeddings of [x ; cond] (:888-891)
    c.lin(b.ein, 2 * ch, R, 2 * ch, c.p(t.edge_emb.w), 2 * ch, De, c.p(t.edge_emb.b), b.e[0], De, 0);
    c.lin(b.nin, 2 * nd, Nn, 2 * nd, c.p(t.node_emb.w), 2 * nd, D, c.p(t.node_emb.b), b.h[0], D, 0);
    c.copy2d(Nn, D, b.h[0], D, 0, b.ah, t.catn, 0, 0);
    c.copy2d(R, De, b.e[0], De, 0, b.eh, t.cate, 0, 0);
    for (int l = 0; l < L; ++l) {
        const BlkIx& ix = t.blk[l]; BlkBuf& k = b.blk[l];
        const FusedDims fd{D, De, r, QK, t.ce, L};
        FusedBlockParams fp{};
        const FusedTopo ft{R, tp.edge_a, tp.edge_c, tp.edge_mol, t.save_activations};
        float* fpk = b.fpack + (size_t)l * b.fpack_block;
        // the two modulated LayerNorms at the top of the block
        if (t.fused) {
            fp.le0 = c.p(ix.le0); fp.le1 = c.p(ix.le1); fp.ff3_w = c.p(ix.ff3.w); fp.ff3_b = c.p(ix.ff3.b); fp.ff4_w = c.p(ix.ff4.w); fp.ff4_b = c.p(ix.ff4.b);
            fp.ero_w = c.p(ix.edge_ro.w); fp.ero_b = c.p(ix.edge_ro.b); fp.n2e_b = c.p(ix.n2e.b);
            fused2d_pack_block(s, fd, fp, fpk);
            // chain A: LayerNorm1 -> modulate -> tanh(lin_edge0 .), tanh(lin_edge1 .), one kernel (train_fused.hip k2d_chain_a)
            fused2d_chain_a(s, fd, ft, fpk, b.e[l], k.emod, k.xh_e1, k.rs_e1, k.et, k.t0, k.t1);
            fused_node_ln_mod(s, Nn, D, b.h[l], nullptr, tp.node_mol, k.nmod, 6 * D, 0, 0, D, k.xh_h, k.rs_h, k.ht);
        } else {
            c.stats(R, De, b.e[l], b.tRow[0], k.rs_e1);
            c.ln_mod(R, De, b.e[l], b.tRow[0], k.rs_e1, tp.edge_mol, k.emod, 6 * De, 0, De, k.xh_e1, k.et);
            c.stats(Nn, D, b.h[l], b.tRow[0], k.rs_h);
            c.ln_mod(Nn, D, b.h[l], b.tRow[0], k.rs_h, tp.node_mol, k.nmod, 6 * D, 0, D, k.xh_h, k.ht);
        }
        // attention (layers.py:131-186): q | k | v in one product, then handed out to the compact arrays the attention kernels read
        c.lin(k.ht, D, Nn, D, b.Wqkv + (size_t)l * F3 * D, D, F3, b.bqkv + (size_t)l * F3, k.qkv, F3, 0);
        {
            ModTable M;
            M.n = 3;
            float* outs[3] = {k.q, k.k, k.v};
            for (int j = 0; j < 3; ++j) { M.w[j] = nullptr; M.bias[j] = nullptr; M.out[j] = outs[j]; M.F[j] = j < 2 ? QK : D; M.col[j] = j * QK; }
            hipLaunchKernelGGL(k_mod_scatter, dim3((unsigned)(((long)Nn * D + 255) / 256), 3u), dim3(256), 0, s, M, Nn, F3, (const float*)k.qkv);
        }
        if (!t.fused) {
            c.lin_tanh(k.et, De, R, De, c.p(ix.le0), De, QK, nullptr, k.t0);
            c.lin_tanh(k.et, De, R, De, c.p(ix.le1), De, D, nullptr, k.t1);
        }
        // (one adjacency head: the spatial head's array is never read at XH = 1)
        JT_LAUNCH(k_attn_scores, (long)R * H, s, tp, H, t.XH, t.SC, 1.f / sqrtf((float)t.C), (const float*)k.q, (const float*)k.k,
                           (const float*)k.t0, (const float*)b.adj2d, (const float*)b.adj2d, k.alpha);
        JT_LAUNCH(k_attn_softmax, (long)Nn * H, s, tp, H, k.alpha);
        JT_LAUNCH(k_attn_msg, (long)Nn * D, s, tp, D, H, (const float*)k.v, (const float*)k.t1, (const float*)k.alpha,
                           c.drop(0.f, seed, l, SITE_ALPHA), k.hhat);
        c.lin(k.hhat, D, Nn, D, c.p(ix.n2e.w), D, De, nullptr, k.n2e, De, 0);
        // edges: gated residual of node2edge_lin(hn_r + hn_c), LayerNorm2 + modulate, FFN with sites A3 / F4
        if (t.fused) {
            // chain B: residual -> LN2 -> modulate -> ff_linear3 -> SiLU, dropout -> ff_linear4 -> dropout -> gate -> readout, one kernel
            fused_chain_b(s, fd, ft, fp, fpk, b.e[l], k.n2e, k.emod, c.drop(p_drop, seed, l, SITE_A3), c.drop(p_drop, seed, l, SITE_F4), k.xh_en, k.rs_en,
                          k.en, k.f3, k.a3, k.f4, b.e[l + 1], b.eh, t.cate, De + l * t.ce);
        } else {
            float* x1e = b.tE_De[0];
            JT_LAUNCH(k_edge_bcast, (long)R * De, s, tp, De, (const float*)b.e[l], (const float*)k.n2e, (const float*)k.n2e, c.p(ix.n2e.b),
                               (const float*)k.emod, 6 * De, 2 * De, x1e);
            c.stats(R, De, x1e, b.tRow[0], k.rs_en);
            c.ln_mod(R, De, x1e, b.tRow[0], k.rs_en, tp.edge_mol, k.emod, 6 * De, 3 * De, 4 * De, k.xh_en, k.en);
            c.lin_silu(k.en, De, R, De, c.p(ix.ff3.w), De, r * De, c.p(ix.ff3.b), k.f3, k.a3, c.drop(p_drop, seed, l, SITE_A3));
            c.lin(k.a3, r * De, R, r * De, c.p(ix.ff4.w), r * De, De, c.p(ix.ff4.b), k.f4, De, 0);
            JT_LAUNCH(k_drop, (long)R * De, s, (long)R * De, (const float*)k.f4, b.tE_De[1], c.drop(p_drop, seed, l, SITE_F4));
            JT_LAUNCH(k_gate_add, (long)R * De, s, (long)R, De, (const float*)k.en, (const float*)b.tE_De[1], tp.edge_mol, (const float*)k.emod,
                               6 * De, 5 * De, b.e[l + 1]);
        }
        // nodes: gated residual, LayerNorm2 + modulate, FFN with sites A1 / F2
        if (t.fused) {
            fused_node_ln_mod(s, Nn, D, b.h[l], k.hhat, tp.node_mol, k.nmod, 6 * D, 2 * D, 3 * D, 4 * D, k.xh_hn, k.rs_hn, k.hn);
        } else {
            float* x1n = b.tN_D[0];
            JT_LAUNCH(k_gate_add, (long)Nn * D, s, (long)Nn, D, (const float*)b.h[l], (const float*)k.hhat, tp.node_mol, (const float*)k.nmod,
                               6 * D, 2 * D, x1n);
            c.stats(Nn, D, x1n, b.tRow[0], k.rs_hn);
            c.ln_mod(Nn, D, x1n, b.tRow[0], k.rs_hn, tp.node_mol, k.nmod, 6 * D, 3 * D, 4 * D, k.xh_hn, k.hn);
        }
        c.lin_silu(k.hn, D, Nn, D, c.p(ix.ff1.w), D, r * D, c.p(ix.ff1.b), k.f1, k.a1, c.drop(p_drop, seed, l, SITE_A1));
        c.lin(k.a1, r * D, Nn, r * D, c.p(ix.ff2.w), r * D, D, c.p(ix.ff2.b), k.f2, D, 0);
        JT_LAUNCH(k_drop_gate_add, (long)Nn * D, s, (long)Nn, D, (const float*)k.hn, (const float*)k.f2, c.drop(p_drop, seed, l, SITE_F2), tp.node_mol,
                           (const float*)k.nmod, 6 * D, 5 * D, b.h[l + 1]);
        // readouts written into the head inputs in place
        c.lin(b.h[l + 1], D, Nn, D, c.p(ix.node_ro.w), D, t.cn, c.p(ix.node_ro.b), b.ah + D + l * t.cn, t.catn, 0);
        if (!t.fused) c.lin(b.e[l + 1], De, R, De, c.p(ix.edge_ro.w), De, t.ce, c.p(ix.edge_ro.b), b.eh + De + l * t.ce, t.cate, 0);
    }
    // heads and outputs: the symmetrised, masked edge output
    head_fwd(c, b.ah, t.catn, Nn, t.catn, t.np0, t.np2, t.np4, D, D / 2, nd, b.nh1pre, b.nh1, b.nh2pre, b.nh2, b.atom, nd);
    head_fwd(c, b.eh, t.cate, R, t.cate, t.ee0, t.ee2, t.ee4, De, De / 2, 1, b.x1pre[0], b.x1[0], b.x2pre[0], b.x2[0], b.Ep, ch);
    head_fwd(c, b.eh, t.cate, R, t.cate, t.et0, t.et2, t.et4, De, De / 2, ch - 1, b.x1pre[1], b.x1[1], b.x2pre[1], b.x2[1], b.Ep + 1, ch);
    JT_LAUNCH(k_edge_out, (long)B * t.N * t.N * ch, s, tp, ch, (const float*)b.Ep, out_edge);
    JT_LAUNCH(k2_node_out, (long)B * t.N * nd, s, tp, nd, (const float*)b.atom, out_xh);
}

void backward(const Ctx& c, const float* nl, const float* d_out_xh, const float* d_out_edge, float p_drop, unsigned long long seed) {
    const jodo_train2d& t = c.t; Bufs& b = c.b; const Topo& tp = c.tp; hipStream_t s = c.s;
    const int B = t.B, Nn = t.Nn, R = t.R, D = t.D, De = t.De, T = t.T, L = t.L, QK = t.QK, H = t.H, r = t.r, nd = t.nd, ch = t.ch;
    const int F17 = 2 * t.half + 1, F3 = 2 * QK + D, Mt = t.Mtot;
    const Drop nod = c.drop(0.f, 0, 0, 0);
    // gradients are accumulated below: zero them first — adjacent buffers (and alignment gaps under 16 bytes between them, the contract
    // of jodo_train_backward) in one fill
    for (int i = 0; i < t.n_params;) {
        char* beg = reinterpret_cast<char*>(c.g(i));
        size_t bytes = t.numel[i] * 4;
        int j = i + 1;
        while (j < t.n_params && reinterpret_cast<char*>(c.g(j)) >= beg + bytes && reinterpret_cast<char*>(c.g(j)) - (beg + bytes) < 16) {
            bytes = (size_t)(reinterpret_cast<char*>(c.g(j)) - beg) + t.numel[j] * 4;
            ++j;
        }
        (void)hipMemsetAsync(beg, 0, bytes, s);
        i = j;
    }
    (void)hipMemsetAsync(b.dtau, 0, (size_t)B * T * 4, s);
    (void)hipMemsetAsync(b.dWqkv, 0, (size_t)L * F3 * D * 4, s);
    (void)hipMemsetAsync(b.dbqkv, 0, (size_t)L * F3 * 4, s);
    // outputs -> packed gradients, heads
    float *datom = b.tN_nd, *dEp = b.tE_ch;
    JT_LAUNCH(k2_node_out_bwd, (long)Nn * nd, s, tp, nd, d_out_xh, datom);
    JT_LAUNCH(k_edge_out_bwd, (long)R * ch, s, tp, ch, d_out_edge, dEp);
    float *dah = b.tcatn, *deh = b.tcate;
    head_bwd(c, b.ah, t.catn, Nn, t.catn, t.np0, t.np2, t.np4, D, D / 2, nd, b.nh1pre, b.nh1, b.nh2pre, b.nh2, datom, nd, b.tN_D[0], b.tN_D[1], dah, t.catn, 0);
    head_bwd(c, b.eh, t.cate, R, t.cate, t.ee0, t.ee2, t.ee4, De, De / 2, 1, b.x1pre[0], b.x1[0], b.x2pre[0], b.x2[0], dEp, ch, b.tE_De[0], b.tE_De[1], deh, t.cate, 0);
    head_bwd(c, b.eh, t.cate, R, t.cate, t.et0, t.et2, t.et4, De, De / 2, ch - 1, b.x1pre[1], b.x1[1], b.x2pre[1], b.x2[1], dEp + 1, ch, b.tE_De[0], b.tE_De[1], deh,
             t.cate, 1);
    float *dh = b.tN_D[2], *dh_prev = b.tN_D[3], *de = b.tE_De[2], *de_prev = b.tE_De[3];
    (void)hipMemsetAsync(dh, 0, (size_t)Nn * D * 4, s);           // the head inputs hold h / e after the EMBEDDINGS in their first columns,
    (void)hipMemsetAsync(de, 0, (size_t)R * De * 4, s);           // so that part of dah / deh joins d h[0] / d e[0] after the loop
    for (int l = L - 1; l >= 0; --l) {
        const BlkIx& ix = t.blk[l]; BlkBuf& k = b.blk[l];
        float *dnmod = b.dmods_all + (size_t)l * (6 * D + 6 * De), *demod = dnmod + 6 * D;           // row stride Mt
        // readouts
        c.lin_dw(dah + D + l * t.cn, t.catn, Nn, t.cn, b.h[l + 1], D, D, c.g(ix.node_ro.w), D, c.g(ix.node_ro.b));
        c.lin_dx(dah + D + l * t.cn, t.catn, Nn, t.cn, c.p(ix.node_ro.w), D, D, dh, D, 1);
        c.lin_dw(deh + De + l * t.ce, t.cate, R, t.ce, b.e[l + 1], De, De, c.g(ix.edge_ro.w), De, c.g(ix.edge_ro.b));
        c.lin_dx(deh + De + l * t.ce, t.cate, R, t.ce, c.p(ix.edge_ro.w), De, De, de, De, 1);
        // ---- edge FFN, LayerNorm2 + modulate, gated residual
        float *dten = b.tE_De[1], *tE = b.tE_rD;
        const FusedDims fd{D, De, r, QK, t.ce, L};
        FusedBlockParams fp{};
        const FusedTopo ft{R, tp.edge_a, tp.edge_c, tp.edge_mol};
        float* fpk = b.fpack + (size_t)l * b.fpack_block;
        if (t.fused_bwd) {
            fp.le0 = c.p(ix.le0); fp.le1 = c.p(ix.le1); fp.ff3_w = c.p(ix.ff3.w); fp.ff4_w = c.p(ix.ff4.w);
            fused2d_pack_block_bwd(s, fd, fp, fpk);
            // chain B': dropout / gate backward, ff_linear4^T, SiLU' x dropout, ff_linear3^T, LayerNorm2 + modulate backward — one kernel; it leaves
            // dropout(f4) in dten (d g2 sums), d f4 and d hidden for the weight-gradient products, d en for the modulation sums, and writes de_prev
            float *df4 = b.tE_De2[0], *den = b.tE_De2[1];
            fused_bwd_b(s, fd, ft, fp, fpk, de, k.f4, k.f3, k.xh_en, k.rs_en, k.emod, c.drop(p_drop, seed, l, SITE_A3), c.drop(p_drop, seed, l, SITE_F4),
                        dten, df4, tE, den, de_prev);
            c.seg(De, tp.edge_off, de, dten, demod, Mt, 5 * De);                                     // d eg2
            c.lin_dw(df4, De, R, De, k.a3, r * De, r * De, c.g(ix.ff4.w), r * De, c.g(ix.ff4.b));
            c.lin_dw(tE, r * De, R, r * De, k.en, De, De, c.g(ix.ff3.w), De, c.g(ix.ff3.b));
            c.seg2_edge(De, den, k.xh_en, demod, Mt, 3 * De, 4 * De);
        } else {
            JT_LAUNCH(k_drop, (long)R * De, s, (long)R * De, (const float*)k.f4, dten, c.drop(p_drop, seed, l, SITE_F4));
            c.seg(De, tp.edge_off, de, dten, demod, Mt, 5 * De);                                         // d eg2
            JT_LAUNCH(k_gate_bwd, (long)R * De, s, (long)R, De, (const float*)de, tp.edge_mol, (const float*)k.emod, 6 * De, 5 * De, dten, 0);
            JT_LAUNCH(k_drop, (long)R * De, s, (long)R * De, (const float*)dten, dten, c.drop(p_drop, seed, l, SITE_F4));
            c.lin_dw(dten, De, R, De, k.a3, r * De, r * De, c.g(ix.ff4.w), r * De, c.g(ix.ff4.b));
            c.lin_dx(dten, De, R, De, c.p(ix.ff4.w), r * De, r * De, tE, r * De, 0);
            c.silu_bwd((long)R * r * De, k.f3, tE, tE, c.drop(p_drop, seed, l, SITE_A3));
            c.lin_dw(tE, r * De, R, r * De, k.en, De, De, c.g(ix.ff3.w), De, c.g(ix.ff3.b));
            c.lin_dx(tE, r * De, R, r * De, c.p(ix.ff3.w), De, De, de, De, 1);                          // de is now d en
            c.ln_mod_bwd(R, De, de, k.xh_en, k.rs_en, tp.edge_mol, tp.edge_off, k.emod, 6 * De, 3 * De, 4 * De, demod, Mt, de_prev, 0);   // de_prev = d x1e = d e[l] (residual)
        }
        // d eg1 = sum over the molecule of d x1e * ehat, ehat = node2edge_lin(hn_a) + node2edge_lin(hn_c) + bias formed on the fly
        c.seg_edge_ehat(De, de_prev, k.n2e, c.p(ix.n2e.b), demod, Mt, 2 * De);
        // d n2e[i] = g1 (sum_c d x1e[(i, c)] + sum_a d x1e[(a, i)]); the bias saw every edge once, the node sums see it twice: its
        // gradient rides on the weight-gradient product and is halved (exactly) for all blocks at the end
        float* dn2e = b.tN_De;
        JT_LAUNCH(k_edge_to_node, (long)Nn * De, s, tp, De, (const float*)de_prev, dn2e, dn2e, 0, (const float*)k.emod, 6 * De, 2 * De);
        c.lin_dw(dn2e, De, Nn, De, k.hhat, D, D, c.g(ix.n2e.w), D, c.g(ix.n2e.b));
        float* dhhat = b.tN_D[0];
        c.lin_dx(dn2e, De, Nn, De, c.p(ix.n2e.w), D, D, dhhat, D, 0);
        // ---- node FFN, LayerNorm2 + modulate, gated residual
        float *dtn = b.tN_D[1], *tNr = b.tN_rD;
        c.seg_node_drop(D, dh, k.f2, c.drop(p_drop, seed, l, SITE_F2), dnmod, Mt, 5 * D);             // d ng2 = sum dh dropout(f2)
        JT_LAUNCH(k_gate_drop_bwd, (long)Nn * D, s, (long)Nn, D, (const float*)dh, tp.node_mol, (const float*)k.nmod, 6 * D, 5 * D, dtn,
                           c.drop(p_drop, seed, l, SITE_F2));                                        // d f2 = (g2 dh) mask
        c.lin_dw(dtn, D, Nn, D, k.a1, r * D, r * D, c.g(ix.ff2.w), r * D, c.g(ix.ff2.b));
        c.lin_dx(dtn, D, Nn, D, c.p(ix.ff2.w), r * D, r * D, tNr, r * D, 0);
        c.silu_bwd((long)Nn * r * D, k.f1, tNr, tNr, c.drop(p_drop, seed, l, SITE_A1));
        c.lin_dw(tNr, r * D, Nn, r * D, k.hn, D, D, c.g(ix.ff1.w), D, c.g(ix.ff1.b));
        c.lin_dx(tNr, r * D, Nn, r * D, c.p(ix.ff1.w), D, D, dh, D, 1);                              // dh is now d hn
        c.ln_mod_bwd(Nn, D, dh, k.xh_hn, k.rs_hn, tp.node_mol, tp.node_off, k.nmod, 6 * D, 3 * D, 4 * D, dnmod, Mt, dh_prev, 0);      // dh_prev = d x1n = d h[l] (residual)
        c.seg(D, tp.node_off, dh_prev, k.hhat, dnmod, Mt, 2 * D);                                    // d ng1
        JT_LAUNCH(k_gate_bwd, (long)Nn * D, s, (long)Nn, D, (const float*)dh_prev, tp.node_mol, (const float*)k.nmod, 6 * D, 2 * D, dhhat, 1);
        // ---- attention backwards
        const float isc = 1.f / sqrtf((float)t.C);
        const Drop da = c.drop(0.f, seed, l, SITE_ALPHA);
        float *dv = b.tN_D[1], *dt1 = b.tE_D, *dS = b.tE_H, *dq = b.tN_QK[0], *dk = b.tN_QK[1], *dt0 = b.tE_QK;
        JT_LAUNCH(k_attn_bwd_v, (long)Nn * D, s, tp, D, H, (const float*)dhhat, (const float*)k.t1, (const float*)k.alpha, da, dv);
        JT_LAUNCH(k_attn_bwd_t1, (long)R * D, s, tp, D, H, (const float*)dhhat, (const float*)k.v, (const float*)k.t1, (const float*)k.alpha, da, dt1);
        JT_LAUNCH(k_attn_bwd_alpha, (long)R * H, s, tp, D, H, (const float*)dhhat, (const float*)k.v, (const float*)k.t1, da, dS);
        JT_LAUNCH(k_attn_bwd_softmax, (long)Nn * H, s, tp, H, (const float*)k.alpha, dS);
        JT_LAUNCH(k_attn_bwd_qk, (long)Nn * QK, s, tp, H, t.XH, t.SC, isc, (const float*)dS, (const float*)k.q, (const float*)k.k, (const float*)k.t0, dq, dk);
        JT_LAUNCH(k_attn_bwd_t0, (long)R * QK, s, tp, H, t.XH, t.SC, isc, (const float*)dS, (const float*)k.q, (const float*)k.k, (const float*)k.t0, dt0);
        // det = lin_edge1^T dt1 + lin_edge0^T dt0 -> LayerNorm1 + modulate backward -> accumulated into de_prev (no edge_emb term here)
        float* det = b.tE_De[1];
        c.lin_dw(dt1, D, R, D, k.et, De, De, c.g(ix.le1), De);
        c.lin_dw(dt0, QK, R, QK, k.et, De, De, c.g(ix.le0), De);
        if (t.fused_bwd) {
            // chain A': lin_edge1^T, lin_edge0^T, LayerNorm1 + modulate backward — one kernel (train_fused.hip k2d_bwd_a); it leaves det for
            // the modulation sums and adds into de_prev
            fused2d_bwd_a(s, fd, ft, fpk, dt1, dt0, k.xh_e1, k.rs_e1, k.emod, det, de_prev);
            c.seg2_edge(De, det, k.xh_e1, demod, Mt, 0, De);
        } else {
            c.lin_dx(dt1, D, R, D, c.p(ix.le1), De, De, det, De, 0);
            c.lin_dx(dt0, QK, R, QK, c.p(ix.le0), De, De, det, De, 1);
            c.ln_mod_bwd(R, De, det, k.xh_e1, k.rs_e1, tp.edge_mol, tp.edge_off, k.emod, 6 * De, 0, De, demod, Mt, de_prev, 1);
        }
        float* dht = b.tN_D[0];
        {   // d q | d k | d v side by side: one weight-gradient and one input-gradient product on the gathered weights of the forward
            ModTable M;
            M.n = 3;
            float* srcs[3] = {dq, dk, dv};
            for (int j = 0; j < 3; ++j) { M.w[j] = nullptr; M.bias[j] = nullptr; M.out[j] = srcs[j]; M.F[j] = j < 2 ? QK : D; M.col[j] = j * QK; }
            hipLaunchKernelGGL(k_mod_gather_cols, dim3((unsigned)(((long)Nn * D + 255) / 256), 3u), dim3(256), 0, s, M, Nn, F3, b.dqkv);
            c.lin_dw(b.dqkv, F3, Nn, F3, k.ht, D, D, b.dWqkv + (size_t)l * F3 * D, D, b.dbqkv + (size_t)l * F3);
            c.lin_dx(b.dqkv, F3, Nn, F3, b.Wqkv + (size_t)l * F3 * D, D, D, dht, D, 0);
        }
        c.ln_mod_bwd(Nn, D, dht, k.xh_h, k.rs_h, tp.node_mol, tp.node_off, k.nmod, 6 * D, 0, D, dnmod, Mt, dh_prev, 1);
        std::swap(dh, dh_prev); std::swap(de, de_prev);
    }
    // embeddings
    c.copy2d(Nn, D, dah, t.catn, 0, dh, D, 0, 1);
    c.copy2d(R, De, deh, t.cate, 0, de, De, 0, 1);
    c.lin_dw(dh, D, Nn, D, b.nin, 2 * nd, 2 * nd, c.g(t.node_emb.w), 2 * nd, c.g(t.node_emb.b));
    c.lin_dw(de, De, R, De, b.ein, 2 * ch, 2 * ch, c.g(t.edge_emb.w), 2 * ch, c.g(t.edge_emb.b));
    {   // the gathered q | k | v weight gradients of every block back to their tensors
        ModGradTable M;
        M.n = 3 * L;
        for (int l = 0; l < L; ++l) {
            const BlkIx& ix = t.blk[l];
            const Lin ls[3] = {ix.query, ix.key, ix.value};
            for (int j = 0; j < 3; ++j) { const int i = 3 * l + j; M.gw[i] = c.g(ls[j].w); M.gb[i] = c.g(ls[j].b); M.F[i] = j < 2 ? QK : D; M.col[i] = l * F3 + j * QK; }
        }
        hipLaunchKernelGGL(k_mod_scatter_grads, dim3((unsigned)(((long)D * D + 255) / 256), (unsigned)M.n), dim3(256), 0, s, M, D, (const float*)b.dWqkv, (const float*)b.dbqkv);
    }
    {   // every modulation projection at once: dW += dmod^T tau, db += column sums, dtau += dmod W; rows back to their tensors
        (void)hipMemsetAsync(b.dWall, 0, (size_t)Mt * T * 4, s);
        (void)hipMemsetAsync(b.dball, 0, (size_t)Mt * 4, s);
        c.lin_dw(b.dmods_all, Mt, B, Mt, b.tau, T, T, b.dWall, T, b.dball);
        c.lin_dx(b.dmods_all, Mt, B, Mt, b.Wall, T, T, b.dtau, T, 1);
        ModGradTable M;
        Lin lin[MOD_MAX]; int F[MOD_MAX], col[MOD_MAX];
        M.n = mod_entries(t, lin, F, col);
        int fmax = 0;
        for (int i = 0; i < M.n; ++i) { M.gw[i] = c.g(lin[i].w); M.gb[i] = c.g(lin[i].b); M.F[i] = F[i]; M.col[i] = col[i]; fmax = F[i] > fmax ? F[i] : fmax; }
        hipLaunchKernelGGL(k_mod_scatter_grads, dim3((unsigned)(((long)fmax * T + 255) / 256), (unsigned)M.n), dim3(256), 0, s, M, T, (const float*)b.dWall, (const float*)b.dball);
    }
    // the time embedding
    c.silu_bwd((long)B * T, b.temb, b.dtau, b.dtemb, nod);
    c.lin_dw(b.dtemb, T, B, T, b.t1a, T, T, c.g(t.time3.w), T, c.g(t.time3.b));
    c.lin_dx(b.dtemb, T, B, T, c.p(t.time3.w), T, T, b.tB_T[0], T, 0);
    JT_LAUNCH(k_gelu_bwd, (long)B * T, s, (long)B * T, (const float*)b.t1pre, (const float*)b.tB_T[0], b.tB_T[0]);
    c.lin_dw(b.tB_T[0], T, B, T, b.feat, F17, F17, c.g(t.time1.w), F17, c.g(t.time1.b));
    c.lin_dx(b.tB_T[0], T, B, T, c.p(t.time1.w), F17, F17, b.tB_T[1], F17, 0);
    JT_LAUNCH(k_time_feat_bwd, t.half, s, B, t.half, nl, c.p(t.time_w), (const float*)b.tB_T[1], c.g(t.time_w));
    for (int l0 = 0; l0 < L; l0 += 16) {                     // node2edge bias gradients: the node sums counted every edge twice (see the block loop)
        ScaleTable S;
        S.n_arrays = L - l0 < 16 ? L - l0 : 16;
        for (int i = 0; i < S.n_arrays; ++i) S.x[i] = c.g(t.blk[l0 + i].n2e.b);
        JT_LAUNCH(k_scale_arrays, (long)S.n_arrays * De, s, S, De, 0.5f);
    }
}

Topo make_topo(const jodo_train2d& t, const void* desc_dev) {
    const int* d = static_cast<const int*>(desc_dev);
    Topo tp;
    tp.B = t.B; tp.Nn = t.Nn; tp.R = t.R; tp.N = t.N;
    tp.node_off = d + t.o_node_off; tp.edge_off = d + t.o_edge_off; tp.nn = d + t.o_nn; tp.node_mol = d + t.o_node_mol;
    tp.edge_mol = d + t.o_edge_mol; tp.edge_a = d + t.o_edge_a; tp.edge_c = d + t.o_edge_c;
    tp.NC = t.NC; tp.ec_off = d + t.o_ec_off; tp.ec_mol_off = d + t.o_ec_mol_off;
    return tp;
}

}  // namespace

extern "C" {

int jodo_train2d_create(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes, const jodo_tensor* params, int n_params, jodo_train2d** out) {
    if (!cfg || !n_nodes || !params || !out || B <= 0 || N <= 0) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_create: null / non-positive argument");
    if (cfg->nf <= 0 || cfg->n_heads <= 0 || cfg->nf % cfg->n_heads || cfg->n_extra != 1 || cfg->n_heads <= cfg->n_extra)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_train2d_create: nf %d / n_heads %d / n_extra_heads %d", cfg->nf, cfg->n_heads, cfg->n_extra);
    if (cfg->n_layers < 1 || cfg->n_layers > 16)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_train2d_create: n_layers %d (1 .. 16: the batched modulation tables)", cfg->n_layers);
    if (cfg->nf % 32)       // LayerNorm rows of nf / 4 features are reduced in eight equal parts (train_ops.h k_row_part)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_train2d_create: nf %d is not a multiple of 32", cfg->nf);
    if (cfg->in_node_dim < 1 || cfg->edge_ch < 2 || cfg->mlp_ratio < 1)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_train2d_create: in_node_dim %d / edge_ch %d / mlp_ratio %d", cfg->in_node_dim, cfg->edge_ch, cfg->mlp_ratio);
    jodo_train2d* t = new jodo_train2d();
    t->cfg = *cfg; t->B = B; t->N = N;
    t->D = cfg->nf; t->De = cfg->nf / 4; t->T = cfg->nf * 4; t->L = cfg->n_layers; t->H = cfg->n_heads; t->XH = cfg->n_extra;
    t->C = t->D / t->H; t->SC = (t->H * t->C) / (t->H - t->XH); t->QK = (t->H - t->XH) * t->SC; t->r = cfg->mlp_ratio; t->nd = cfg->in_node_dim;
    t->ch = cfg->edge_ch; t->cn = (2 * t->D) / t->L; t->ce = (2 * t->De) / t->L; t->catn = t->D + t->L * t->cn;
    t->cate = t->De + t->L * t->ce;
    long Nn = 0, R = 0;
    for (int b = 0; b < B; ++b) {
        if (n_nodes[b] < 1 || n_nodes[b] > N) { delete t; return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_create: n_nodes[%d] = %d outside 1..%d", b, n_nodes[b], N); }
        Nn += n_nodes[b]; R += (long)n_nodes[b] * n_nodes[b];
    }
    // every index below stays under 2^31: the widest per-row array has r * nf / 4 .. nf floats, indexed in long
    if (R > (1L << 30)) { delete t; return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_train2d_create: %ld edge rows", R); }
    t->Nn = (int)Nn; t->R = (int)R;
    std::vector<int>& tb = t->tables;
    t->o_node_off = 0; t->o_edge_off = t->o_node_off + B + 1; t->o_nn = t->o_edge_off + B + 1; t->o_node_mol = t->o_nn + B;
    t->o_edge_mol = t->o_node_mol + Nn; t->o_edge_a = t->o_edge_mol + R; t->o_edge_c = t->o_edge_a + R;
    // chunks of a molecule's edge rows: at most 64 per molecule, at least 32 rows each (two-level per-molecule sums)
    std::vector<int> ec_off, ec_mol_off;
    {
        int eo2 = 0;
        for (int b = 0; b < B; ++b) {
            const int n2 = n_nodes[b] * n_nodes[b];
            const int chk = std::max(32, (n2 + 63) / 64);
            ec_mol_off.push_back((int)ec_off.size());
            for (int r0 = 0; r0 < n2; r0 += chk) ec_off.push_back(eo2 + r0);
            eo2 += n2;
        }
        ec_mol_off.push_back((int)ec_off.size());
        ec_off.push_back(eo2);
    }
    t->NC = (int)ec_off.size() - 1;
    t->o_ec_off = t->o_edge_c + R; t->o_ec_mol_off = t->o_ec_off + ec_off.size();
    tb.assign(t->o_ec_mol_off + ec_mol_off.size(), 0);
    std::copy(ec_off.begin(), ec_off.end(), tb.begin() + t->o_ec_off);
    std::copy(ec_mol_off.begin(), ec_mol_off.end(), tb.begin() + t->o_ec_mol_off);
    int no = 0, eo = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_nodes[b];
        tb[t->o_node_off + b] = no; tb[t->o_edge_off + b] = eo; tb[t->o_nn + b] = n;
        for (int i = 0; i < n; ++i) tb[t->o_node_mol + no + i] = b;
        for (int a = 0; a < n; ++a)
            for (int c = 0; c < n; ++c) {
                tb[t->o_edge_mol + eo + a * n + c] = b; tb[t->o_edge_a + eo + a * n + c] = no + a; tb[t->o_edge_c + eo + a * n + c] = no + c;
            }
        no += n; eo += n * n;
    }
    tb[t->o_node_off + B] = no; tb[t->o_edge_off + B] = eo;
    // parameters by name
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
    const size_t D = t->D, De = t->De, T = t->T, QK = t->QK, r = t->r, nd = t->nd, ch = t->ch;
    t->node_emb = lin("node_emb", D, 2 * nd); t->edge_emb = lin("edge_emb", De, 2 * ch);
    t->np0 = lin("node_pred_mlp.0", D, t->catn); t->np2 = lin("node_pred_mlp.2", D / 2, D); t->np4 = lin("node_pred_mlp.4", nd, D / 2);
    t->et0 = lin("edge_type_mlp.0", De, t->cate); t->et2 = lin("edge_type_mlp.2", De / 2, De); t->et4 = lin("edge_type_mlp.4", ch - 1, De / 2);
    t->ee0 = lin("edge_exist_mlp.0", De, t->cate); t->ee2 = lin("edge_exist_mlp.2", De / 2, De); t->ee4 = lin("edge_exist_mlp.4", 1, De / 2);
    {
        auto it = ix.find("time_mlp.0.weights");
        if (it == ix.end() || t->numel[it->second] < 1) { if (missing.empty()) missing = "time_mlp.0.weights"; t->time_w = -1; t->half = 8; }
        else { t->time_w = it->second; t->half = (int)t->numel[it->second]; }
    }
    t->time1 = lin("time_mlp.1", T, 2 * t->half + 1); t->time3 = lin("time_mlp.3", T, T);
    t->blk.resize(t->L);
    for (int l = 0; l < t->L; ++l) {
        const std::string p = "e_block_" + std::to_string(l) + ".";
        BlkIx& k = t->blk[l];
        k.n2e = lin(p + "node2edge_lin", De, D);
        k.key = lin(p + "attn_mpnn.lin_key", QK, D); k.query = lin(p + "attn_mpnn.lin_query", QK, D); k.value = lin(p + "attn_mpnn.lin_value", D, D);
        k.le0 = find(p + "attn_mpnn.lin_edge0.weight", QK * De); k.le1 = find(p + "attn_mpnn.lin_edge1.weight", D * De);
        k.ff1 = lin(p + "ff_linear1", r * D, D); k.ff2 = lin(p + "ff_linear2", D, r * D); k.ff3 = lin(p + "ff_linear3", r * De, De); k.ff4 = lin(p + "ff_linear4", De, r * De);
        k.node_time = lin(p + "node_time_mlp.1", 6 * D, T); k.edge_time = lin(p + "edge_time_mlp.1", 6 * De, T);
        k.node_ro = lin("node_" + std::to_string(l), t->cn, D); k.edge_ro = lin("edge_" + std::to_string(l), t->ce, De);
    }
    if (!missing.empty()) { delete t; return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_create: parameter '%s' missing or mis-sized", missing.c_str()); }
    t->fused = 0;                     // the op-by-op form is the default until the fused one is measured faster: options 0 / 1
    t->fused_bwd = 0;
    t->save_activations = 1;
    t->Mtot = t->L * (6 * t->D + 6 * t->De);
    Arena a{nullptr, 0}; Bufs bufs;
    layout(*t, a, bufs);
    t->ws_bytes = a.off;
    *out = t;
    return JODO_OK;
}

void jodo_train2d_destroy(jodo_train2d* t) { delete t; }
size_t jodo_train2d_desc_bytes(const jodo_train2d* t) { return t ? t->tables.size() * sizeof(int) : 0; }
size_t jodo_train2d_workspace_bytes(const jodo_train2d* t) { return t ? t->ws_bytes : 0; }
// option 0: the fused forward chains of a block (train_fused.hip: k2d_chain_a, k_chain_b, the node LayerNorms): 1 (where the width is
//           supported) / 0 (default: op-by-op, the reference form, which the host-emulation build runs)
// option 1: the same for the input-gradient side of the backward (k2d_bwd_a, k_bwd_b, the node LayerNorm backward)
// option 2: 1 (default) every forward keeps what a backward needs; 0: the following forwards will not be differentiated (the no-grad
//           self-conditioning forward of a training step): the fused chains skip the stores only a backward reads
int jodo_train2d_set_option(jodo_train2d* t, int option, int value) {
    if (!t) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_set_option: null handle");
    if (option < 0 || option > 2 || (value != 0 && value != 1)) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_set_option: option %d value %d", option, value);
    if (option == 2) { t->save_activations = value; return JODO_OK; }
    if (value && !fused2d_available(FusedDims{t->D, t->De, t->r, t->QK, t->ce, t->L}))
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_train2d_set_option: fused chains are not built for this shape");
    if (option == 0) t->fused = value; else t->fused_bwd = value;
    return JODO_OK;
}
// tests: where a kept activation of block `layer` lives in the workspace.  Selectors 0 .. 7 as jodo_train_debug_locate (hhat, alpha,
// f1, a1, f2, f3, a3, f4); 8 = xhat of LayerNorm1 on edges [R, De], 9 = its rstd [R], 10 = et [R, De], 11 = t0 [R, QK], 12 = t1 [R, D]
int jodo_train2d_debug_locate(const jodo_train2d* t, int what, int layer, size_t* byte_offset, size_t* count) {
    if (!t || !byte_offset || !count) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_debug_locate: null argument");
    if (layer < 0 || layer >= t->L) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_debug_locate: layer %d of %d", layer, t->L);
    Arena a{reinterpret_cast<char*>(256), 0};              // any non-null base: only the differences are used
    Bufs b;
    layout(*t, a, b);
    const BlkBuf& k = b.blk[layer];
    const size_t Nn = t->Nn, R = t->R, D = t->D, De = t->De, r = t->r;
    const float* ptr = nullptr;
    size_t n = 0;
    switch (what) {
        case 0: ptr = k.hhat; n = Nn * D; break;
        case 1: ptr = k.alpha; n = R * t->H; break;
        case 2: ptr = k.f1; n = Nn * r * D; break;
        case 3: ptr = k.a1; n = Nn * r * D; break;
        case 4: ptr = k.f2; n = Nn * D; break;
        case 5: ptr = k.f3; n = R * r * De; break;
        case 6: ptr = k.a3; n = R * r * De; break;
        case 7: ptr = k.f4; n = R * De; break;
        case 8: ptr = k.xh_e1; n = R * De; break;
        case 9: ptr = k.rs_e1; n = R; break;
        case 10: ptr = k.et; n = R * De; break;
        case 11: ptr = k.t0; n = R * t->QK; break;
        case 12: ptr = k.t1; n = R * D; break;
        default: return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_debug_locate: unknown selector %d", what);
    }
    *byte_offset = (size_t)(reinterpret_cast<const char*>(ptr) - reinterpret_cast<const char*>(256));
    *count = n;
    return JODO_OK;
}
const void* jodo_train2d_desc_host(const jodo_train2d* t) { return t ? t->tables.data() : nullptr; }
int jodo_train2d_upload(jodo_train2d* t, void* desc_dev, void* stream) {
    if (!t || !desc_dev) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_upload: null argument");
    (void)hipMemcpyAsync(desc_dev, t->tables.data(), t->tables.size() * sizeof(int), hipMemcpyHostToDevice, static_cast<hipStream_t>(stream));
    (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));          // the host table may be freed with the handle
    return jodo_check_launch("jodo_train2d_upload");
}

int jodo_train2d_forward(jodo_train2d* t, const void* desc_dev, const float* const* params_dev, int n_params, const float* xh, const float* edge_x,
                         const float* cond_x, const float* cond_edge_x, const float* noise_level, const float* context, float dropout_p, uint64_t seed,
                         float* out_xh, float* out_edge, int32_t* flags_out, void* workspace, void* stream) {
    if (!t || !desc_dev || !params_dev || !xh || !edge_x || !noise_level || !out_xh || !out_edge || !workspace)
        return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_forward: null argument");
    if (n_params != t->n_params) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_forward: %d parameters, handle was created with %d", n_params, t->n_params);
    if ((cond_x == nullptr) != (cond_edge_x == nullptr)) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_forward: cond_x and cond_edge_x go together");
    if (context) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_forward: the 2-D model takes no context");
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_forward: dropout %g", dropout_p);
    Arena a{static_cast<char*>(workspace), 0}; Bufs bufs;
    layout(*t, a, bufs);
    Ctx c{*t, make_topo(*t, desc_dev), params_dev, nullptr, bufs, static_cast<hipStream_t>(stream)};
    forward(c, xh, edge_x, cond_x, cond_edge_x, noise_level, dropout_p, seed, out_xh, out_edge);
    if (flags_out) (void)hipMemcpyAsync(flags_out, bufs.flags, 8 * sizeof(int), hipMemcpyDeviceToDevice, c.s);
    return jodo_check_launch("jodo_train2d_forward");
}

int jodo_train2d_backward(jodo_train2d* t, const void* desc_dev, const float* const* params_dev, float* const* grads_dev, int n_params,
                          const float* noise_level, const float* d_out_xh, const float* d_out_edge, float dropout_p, uint64_t seed, void* workspace,
                          void* stream) {
    if (!t || !desc_dev || !params_dev || !grads_dev || !noise_level || !d_out_xh || !d_out_edge || !workspace)
        return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_backward: null argument");
    if (n_params != t->n_params) return jodo_set_error(JODO_ERR_ARG, "jodo_train2d_backward: %d parameters, handle was created with %d", n_params, t->n_params);
    Arena a{static_cast<char*>(workspace), 0}; Bufs bufs;
    layout(*t, a, bufs);
    Ctx c{*t, make_topo(*t, desc_dev), params_dev, grads_dev, bufs, static_cast<hipStream_t>(stream)};
    backward(c, noise_level, d_out_xh, d_out_edge, dropout_p, seed);
    return jodo_check_launch("jodo_train2d_backward");
}

}  // extern "C"

// Evaluation kernels: atom and molecule stability of decoded molecules, on the device.
//
//   jodo_stability_3d     the distance rule (evaluation/stability.py:17-73 of the reference: check_stability): a bond order per real
//                         pair from the ordered threshold matrix, integer valences, one allowed-valence mask per atom type
//   jodo_stability_bonds  the bond rule without aromatic bonds (evaluation/stability.py:76-161: check_2D_stability): valences from the
//                         upper triangle of the decoded bond orders, one allowed-valence mask per (atom type, formal charge)
//
// Both run one workgroup per molecule (one wave for N <= 64, four above) and share the tail: connected components over the bonds by
// min-label propagation on per-atom adjacency bit rows in LDS, per-molecule counts into per_mol_out, and one integer atomic per total.
// The rule tables are DATA handed in by the caller (jodo_amd/evaluation/rules.py); no table lives in this file.  Everything an atom
// index >= n_nodes[b] holds (position, type, charge, bond row) is never read into a decision.  Plain C++, vector stores, integer
// atomics only; no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"

namespace {
constexpr int EVAL_MAX_N = 256;                               // atoms per molecule: 8 adjacency words per atom
constexpr int EVAL_MAX_T = 255;                               // atom types (atom_type is a byte)

// dynamic LDS of one molecule: N-sized arrays carved from one allocation
struct EvalLds {
    float* px; float* py; float* pz;                          // 3-D rule only
    uint32_t* adj;                                            // [N][W] adjacency bit rows
    int* label;                                               // [N]
    int* val;                                                 // [N] valences (bond rule: summed with LDS atomics)
    uint8_t* type;                                            // [N]
    int* cnt;                                                 // [4] stable atoms, fragments, needs_kekulize, pass-changed flag
};

__host__ __device__ inline size_t eval_lds_bytes(int N, int W, bool with_pos) {
    return (size_t)N * ((with_pos ? 12 : 0) + 4 * W + 4 + 4) + 16 + (size_t)((N + 3) & ~3);
}

__device__ __forceinline__ EvalLds eval_carve(unsigned char* base, int N, int W, bool with_pos) {
    EvalLds L;
    float* f = (float*)base;
    L.px = f; L.py = f + (with_pos ? N : 0); L.pz = f + (with_pos ? 2 * N : 0);
    uint32_t* u = (uint32_t*)(f + (with_pos ? 3 * N : 0));
    L.adj = u;
    L.label = (int*)(u + (size_t)N * W);
    L.val = L.label + N;
    L.cnt = L.val + N;
    L.type = (uint8_t*)(L.cnt + 4);
    return L;
}

// bond order of the pair (ta, tb) at distance d (Angstrom) from thr [T][T][3] (integer picometres, margins included, 0 = no such bond):
// the cascade 100 d < t1, then < t2, then < t3; a missing t2 ends at single, a missing t3 at double
__device__ __forceinline__ int bond_order(const int32_t* __restrict__ thr, int T, int ta, int tb, float d) {
    const int32_t* t = thr + ((size_t)ta * T + tb) * 3;
    const float pm = 100.f * d;
    if (t[0] <= 0 || !(pm < (float)t[0])) return 0;
    if (t[1] <= 0 || !(pm < (float)t[1])) return 1;
    if (t[2] <= 0 || !(pm < (float)t[2])) return 2;
    return 3;
}

// order of the real pair (a, b), a < b by atom index, of the molecule held in LDS; pair_order 0: the lookup is (type[a], type[b]),
// 1: the pair sorted by type index
__device__ __forceinline__ int pair_order_3d(const EvalLds& L, const int32_t* __restrict__ thr, int T, int pair_order, int a, int b) {
    int ta = L.type[a], tb = L.type[b];
    if (ta >= T || tb >= T) return 0;                         // a type outside the table bonds to nothing (and is unstable)
    if (pair_order && ta > tb) { const int s = ta; ta = tb; tb = s; }
    const float dx = L.px[a] - L.px[b], dy = L.py[a] - L.py[b], dz = L.pz[a] - L.pz[b];
    return bond_order(thr, T, ta, tb, sqrtf(dx * dx + dy * dy + dz * dz));
}

// Connected components over the adjacency rows (min-label propagation with one pointer jump per pass, until a pass changes nothing),
// then the molecule's row of per_mol_out and its share of the totals.  Labels only ever decrease and always name an atom of the same
// component, so the unordered reads of a pass are harmless.  Called by every thread of the block, after a barrier that follows the
// last write to adj / val / cnt[0] / cnt[2].
__device__ void eval_finish(const EvalLds& L, int n, int W, int b, int32_t* __restrict__ per_mol, unsigned long long* __restrict__ totals) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < n; i += nt) L.label[i] = i;
    for (;;) {
        __syncthreads();
        if (tid == 0) L.cnt[3] = 0;
        __syncthreads();
        bool changed = false;
        for (int i = tid; i < n; i += nt) {
            int m = L.label[i];
            const int before = m;
            for (int w = 0; w < W; ++w) {
                uint32_t bits = L.adj[(size_t)i * W + w];
                while (bits) {
                    const int j = 32 * w + __ffs((int)bits) - 1;
                    bits &= bits - 1;
                    m = min(m, L.label[j]);
                }
            }
            m = min(m, L.label[m]);
            if (m != before) { L.label[i] = m; changed = true; }
        }
        if (changed) L.cnt[3] = 1;
        __syncthreads();
        if (!L.cnt[3]) break;
    }
    int roots = 0;
    for (int i = tid; i < n; i += nt) roots += L.label[i] == i;
    if (roots) atomicAdd(&L.cnt[1], roots);
    __syncthreads();
    if (tid == 0) {
        const int stable = L.cnt[0], frags = L.cnt[1];
        int32_t* row = per_mol + 4 * (size_t)b;
        row[0] = stable; row[1] = n; row[2] = frags; row[3] = L.cnt[2];
        if (n > 0) {                                          // a molecule without atoms (padding of a gathered batch) counts nowhere
            if (stable == n) atomicAdd(&totals[0], 1ull);
            if (stable) atomicAdd(&totals[1], (unsigned long long)stable);
            atomicAdd(&totals[2], (unsigned long long)n);
            if (frags == 1) atomicAdd(&totals[3], 1ull);
        }
    }
}

__global__ void k_stability_3d(int B, int N, int T, int W, int pair_order, const int32_t* __restrict__ thr, const uint32_t* __restrict__ allowed,
                               const int32_t* __restrict__ n_nodes, const float* __restrict__ pos, const uint8_t* __restrict__ atom_type,
                               int32_t* __restrict__ per_mol, uint8_t* __restrict__ order_out, unsigned long long* __restrict__ totals) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const EvalLds L = eval_carve(lds_raw, N, W, true);
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = min(max(n_nodes[b], 0), N);
    for (int i = tid; i < n; i += nt) {
        const float* p = pos + ((size_t)b * N + i) * 3;
        L.px[i] = p[0]; L.py[i] = p[1]; L.pz[i] = p[2];
        L.type[i] = atom_type[(size_t)b * N + i];
    }
    if (tid < 4) L.cnt[tid] = 0;
    __syncthreads();
    int stable = 0;
    for (int i = tid; i < n; i += nt) {                       // atom i walks every other real atom; both ends of a pair compute the
        int v = 0;                                            // same expression on (min, max), so the two valences agree
        for (int w = 0; w < W; ++w) {
            uint32_t bits = 0;
            const int j1 = min(32 * w + 32, n);
            for (int j = 32 * w; j < j1; ++j) {
                if (j == i) continue;
                const int o = pair_order_3d(L, thr, T, pair_order, min(i, j), max(i, j));
                v += o;
                if (o) bits |= 1u << (j & 31);
            }
            L.adj[(size_t)i * W + w] = bits;
        }
        const int t = L.type[i];
        stable += (t < T && v < 32) ? (int)((allowed[t] >> v) & 1u) : 0;
    }
    if (stable) atomicAdd(&L.cnt[0], stable);
    if (order_out) {                                          // every cell of the molecule's [N, N] block, coalesced; zero off the molecule
        uint8_t* o = order_out + (size_t)b * N * N;
        for (int c = tid; c < N * N; c += nt) {
            const int r = c / N, q = c - r * N;
            o[c] = (r < n && q < n && r != q) ? (uint8_t)pair_order_3d(L, thr, T, pair_order, min(r, q), max(r, q)) : (uint8_t)0;
        }
    }
    __syncthreads();
    eval_finish(L, n, W, b, per_mol, totals);
}

__global__ void k_stability_bonds(int B, int N, int T, int W, int fc_lo, int fc_hi, const uint32_t* __restrict__ allowed_fc,
                                  const int32_t* __restrict__ n_nodes, const uint8_t* __restrict__ atom_type, const int8_t* __restrict__ fc,
                                  const uint8_t* __restrict__ edge_type, int32_t* __restrict__ per_mol,
                                  unsigned long long* __restrict__ totals) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const EvalLds L = eval_carve(lds_raw, N, W, false);
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = min(max(n_nodes[b], 0), N);
    for (int i = tid; i < n; i += nt) {
        L.val[i] = 0;
        for (int w = 0; w < W; ++w) L.adj[(size_t)i * W + w] = 0;
    }
    if (tid < 4) L.cnt[tid] = 0;
    __syncthreads();
    // the strict upper triangle of the real block, rows read along their length (coalesced); bonds are sparse, so the LDS integer
    // atomics of a cell with an order are few
    const uint8_t* e = edge_type + (size_t)b * N * N;
    int aromatic = 0;
    for (int c = tid; c < n * n; c += nt) {
        const int r = c / n, q = c - r * n;
        if (q <= r) continue;
        const int o = e[(size_t)r * N + q];
        if (!o) continue;
        if (o <= 3) { atomicAdd(&L.val[r], o); atomicAdd(&L.val[q], o); }
        else ++aromatic;                                      // aromatic (4) or unknown: counted, never folded into a valence
        atomicOr(&L.adj[(size_t)r * W + (q >> 5)], 1u << (q & 31));
        atomicOr(&L.adj[(size_t)q * W + (r >> 5)], 1u << (r & 31));
    }
    if (aromatic) atomicAdd(&L.cnt[2], aromatic);
    __syncthreads();
    const int nfc = fc_hi - fc_lo + 1;
    int stable = 0;
    for (int i = tid; i < n; i += nt) {
        const int t = atom_type[(size_t)b * N + i], v = L.val[i];
        int q = fc[(size_t)b * N + i];
        if (q < fc_lo || q > fc_hi) q = 0;                    // a charge no element lists: every element's entry for 0
        stable += (t < T && v < 32) ? (int)((allowed_fc[(size_t)t * nfc + (q - fc_lo)] >> v) & 1u) : 0;
    }
    if (stable) atomicAdd(&L.cnt[0], stable);
    __syncthreads();
    eval_finish(L, n, W, b, per_mol, totals);
}

int eval_check_shape(const char* what, int B, int N, int T) {
    if (B <= 0 || N <= 0 || T < 1) return jodo_set_error(JODO_ERR_ARG, "%s: bad shape", what);
    if (N > EVAL_MAX_N || T > EVAL_MAX_T)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "%s: at most %d atoms per molecule and %d atom types", what, EVAL_MAX_N, EVAL_MAX_T);
    return JODO_OK;
}
}  // namespace

extern "C" int jodo_stability_3d(int B, int N, int T, int pair_order, const int32_t* thr_dev, const uint32_t* allowed_dev,
                                 const int32_t* n_nodes_dev, const float* pos, const uint8_t* atom_type, int32_t* per_mol_out,
                                 uint8_t* order_out, int64_t* totals_out, void* stream) {
    int rc = eval_check_shape("stability_3d", B, N, T);
    if (rc != JODO_OK) return rc;
    if (pair_order != JODO_PAIR_BY_INDEX && pair_order != JODO_PAIR_BY_TYPE) return jodo_set_error(JODO_ERR_ARG, "stability_3d: pair_order is 0 or 1");
    if (!thr_dev || !allowed_dev || !n_nodes_dev || !pos || !atom_type || !per_mol_out || !totals_out)
        return jodo_set_error(JODO_ERR_ARG, "stability_3d: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(totals_out, 0, 4 * sizeof(int64_t), st) != hipSuccess) return jodo_set_error(JODO_ERR_LAUNCH, "stability_3d: memset failed");
    const int W = (N + 31) / 32;
    hipLaunchKernelGGL(k_stability_3d, dim3(B), dim3(N <= 64 ? 64 : 256), eval_lds_bytes(N, W, true), st, B, N, T, W, pair_order, thr_dev,
                       allowed_dev, n_nodes_dev, pos, atom_type, per_mol_out, order_out, (unsigned long long*)totals_out);
    return jodo_check_launch("k_stability_3d");
}

extern "C" int jodo_stability_bonds(int B, int N, int T, int fc_lo, int fc_hi, const uint32_t* allowed_fc_dev, const int32_t* n_nodes_dev,
                                    const uint8_t* atom_type, const int8_t* fc, const uint8_t* edge_type, int32_t* per_mol_out,
                                    int64_t* totals_out, void* stream) {
    int rc = eval_check_shape("stability_bonds", B, N, T);
    if (rc != JODO_OK) return rc;
    if (fc_lo > 0 || fc_hi < 0 || fc_lo < -128 || fc_hi > 127) return jodo_set_error(JODO_ERR_ARG, "stability_bonds: the charge range must hold 0 and fit a byte");
    if (!allowed_fc_dev || !n_nodes_dev || !atom_type || !fc || !edge_type || !per_mol_out || !totals_out)
        return jodo_set_error(JODO_ERR_ARG, "stability_bonds: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(totals_out, 0, 4 * sizeof(int64_t), st) != hipSuccess) return jodo_set_error(JODO_ERR_LAUNCH, "stability_bonds: memset failed");
    const int W = (N + 31) / 32;
    hipLaunchKernelGGL(k_stability_bonds, dim3(B), dim3(N <= 64 ? 64 : 256), eval_lds_bytes(N, W, false), st, B, N, T, W, fc_lo, fc_hi,
                       allowed_fc_dev, n_nodes_dev, atom_type, fc, edge_type, per_mol_out, (unsigned long long*)totals_out);
    return jodo_check_launch("k_stability_bonds");
}

// TEST INFRASTRUCTURE ONLY: plain-loop stand-in for jt::gemm (jodo_amd/csrc/train_gemm.hip) in the host emulation build
// (tests/emul/hip/hip_runtime.h explains the build).  Same signature, same semantics; accumulates in double.
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>
#include "train_gemm.h"
thread_local emu_idx threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;
namespace jt {
// Rows [m0, m1) of the product.  Every output element keeps ITS OWN chain of operations exactly as the one-element-at-a-time loop had
// it (two fp32 fused-multiply-add chains per slice taken in turn by the k-pairs, slices into eight interleaved sums, those in order):
// only the loop nest is turned inside out (k outside, the N independent chains of a row inside), so that a batch of 10^5 edge rows
// finishes in seconds instead of minutes.  Compiled twice: with the FMA instruction where the CPU has it (fmaf is then one instruction,
// same result as libm's correctly rounded fmaf), without otherwise.
#define JT_GEMM_ROWS(NAME, ATTR) \
ATTR static void NAME(int m0, int m1, int tA, int tB, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc, \
                      const float* bias, int acc, int nsplit, int kchunk, const GemmEpi* epi) { \
    std::vector<float> c0(N), c1(N), sg((size_t)8 * N); \
    for (int m = m0; m < m1; ++m) { \
        std::fill(sg.begin(), sg.end(), 0.f); \
        for (int z = 0; z < nsplit; ++z) { \
            std::fill(c0.begin(), c0.end(), 0.f); std::fill(c1.begin(), c1.end(), 0.f); \
            const int k1 = K < (z + 1) * kchunk ? K : (z + 1) * kchunk; \
            for (int k = z * kchunk; k < k1; ++k) { \
                const float a = tA ? A[(long)k * lda + m] : A[(long)m * lda + k]; \
                float* c = (((k - z * kchunk) >> 1) & 1) ? c1.data() : c0.data(); \
                if (tB) { const float* b = B + k; for (int n = 0; n < N; ++n) c[n] = fmaf(a, b[(long)n * ldb], c[n]); } \
                else { const float* b = B + (long)k * ldb; for (int n = 0; n < N; ++n) c[n] = fmaf(a, b[n], c[n]); } \
            } \
            if (nsplit > 1) { float* g = sg.data() + (size_t)(z & 7) * N; for (int n = 0; n < N; ++n) g[n] += c0[n] + c1[n]; } \
        } \
        for (int n = 0; n < N; ++n) { \
            float total; \
            if (nsplit > 1) { total = sg[n]; for (int g = 1; g < 8; ++g) total += sg[(size_t)g * N + n]; } \
            else total = c0[n] + c1[n]; \
            if (bias) total += bias[n]; \
            if (epi && epi->act) { gemm_epilogue(*epi, total, C, (long)m * ldc + n, (long)m * N + n); continue; } \
            float* o = C + (long)m * ldc + n; \
            *o = acc ? *o + total : total; \
        } \
    } \
}
JT_GEMM_ROWS(gemm_rows_plain, )
#if defined(__x86_64__)
JT_GEMM_ROWS(gemm_rows_fma, __attribute__((target("fma"))))
#else
#define gemm_rows_fma gemm_rows_plain
#endif

// Mirrors the ROUNDING STRUCTURE of the device kernel so that the CPU suite predicts its accuracy: fp32 fused multiply-adds, two
// accumulator chains taken in turn by the k-pairs, the split-K slices of train_gemm.h gemm_plan() added the way k_splitk_sum adds them:
// eight interleaved partial sums (slices z = g mod 8, ascending), then those in the order g = 0 .. 7.
void gemm(hipStream_t, int tA, int tB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
          const float* bias, int acc, float* ws, size_t ws_floats, const GemmEpi* epi) {
    // debugging aid: products summed in double; value = bit mask of the products it applies to (1 forward, 2 input gradient, 4 weight gradient)
    static const int exact_mask = getenv("JODO_EMUL_GEMM_DOUBLE") ? atoi(getenv("JODO_EMUL_GEMM_DOUBLE")) : 0;
    const int kind = tA ? 4 : (tB ? 1 : 2);
    static const int only_n = getenv("JODO_EMUL_ONLY_N") ? atoi(getenv("JODO_EMUL_ONLY_N")) : 0, only_k = getenv("JODO_EMUL_ONLY_K") ? atoi(getenv("JODO_EMUL_ONLY_K")) : 0;
    if ((exact_mask & kind) && (!only_n || N == only_n) && (!only_k || K == only_k)) {
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) {
                double t = 0.0;
                for (int k = 0; k < K; ++k) t += (double)(tA ? A[(long)k * lda + m] : A[(long)m * lda + k]) * (double)(tB ? B[(long)n * ldb + k] : B[(long)k * ldb + n]);
                if (epi && epi->dbias && tA && n == 0) { double bsum = 0.0; for (int k = 0; k < K; ++k) bsum += (double)A[(long)k * lda + m]; epi->dbias[m] += (float)bsum; }
                if (bias) t += bias[n];
                if (epi && epi->act) { gemm_epilogue(*epi, (float)t, C, (long)m * ldc + n, (long)m * N + n); continue; }
                float* o = C + (long)m * ldc + n;
                *o = acc ? (float)(*o + t) : (float)t;
            }
        return;
    }
    const GemmPlan pl = gemm_plan(tA, M, N, K, ws != nullptr, ws_floats);
    const int nsplit = pl.nsplit, kchunk = pl.kchunk;
    if (epi && epi->dbias && tA) {                              // bias gradient: per slice a double sum, slices added in order
        for (int m = 0; m < M; ++m) {
            float sg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bs = 0.f;
            for (int z = 0; z < nsplit; ++z) {
                double t = 0.0;
                const int k1 = K < (z + 1) * kchunk ? K : (z + 1) * kchunk;
                for (int k = z * kchunk; k < k1; ++k) t += (double)A[(long)k * lda + m];
                if (nsplit > 1) sg[z & 7] += (float)t; else bs = (float)t;
            }
            if (nsplit > 1) { bs = sg[0]; for (int g = 1; g < 8; ++g) bs += sg[g]; }
            epi->dbias[m] += bs;
        }
    }
    static const bool have_fma = __builtin_cpu_supports("fma");
    // rows m0 .. m1 - 1 of the product; threads share nothing but the read-only operands (every output element has one owner)
    auto run = [&](int m0, int m1) {
        (have_fma ? gemm_rows_fma : gemm_rows_plain)(m0, m1, tA, tB, N, K, A, lda, B, ldb, C, ldc, bias, acc, nsplit, kchunk, epi);
    };
    const unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw < 1 ? 1 : hw > 16 ? 16 : hw);
    if ((double)M * N * K < 4e6) nt = 1;
    if (nt > M) nt = M;
    if (nt <= 1) { run(0, M); return; }
    std::vector<std::thread> th;
    for (int i = 0; i < nt; ++i) th.emplace_back(run, (int)((long)M * i / nt), (int)((long)M * (i + 1) / nt));
    for (auto& t : th) t.join();
}
}

// the plan itself, for the CPU suite to hold restatements of it against (tests/test_train_gemm_plan.py)
extern "C" void emul_gemm_plan(int tA, int M, int N, int K, int have_ws, size_t ws_floats, int* nsplit, int* kchunk) {
    const jt::GemmPlan p = jt::gemm_plan(tA, M, N, K, have_ws != 0, ws_floats);
    *nsplit = p.nsplit;
    *kchunk = p.kchunk;
}

// The fused forward chains (jodo_amd/csrc/train_fused.hip) are matrix-instruction kernels: not available to the host emulation, which
// runs — and thereby checks — the op-by-op sequence they replace.
#include "train_fused.h"
namespace jt {
FusedPackLayout fused_pack_layout(const FusedDims&) { return FusedPackLayout{}; }
// the grouped weight-gradient launch: job by job (the device form runs the same plans in one launch, bit-identical to its own
// job-by-job form)
void gemm_dw_group(hipStream_t s, const GemmJob* jobs, int n, float* ws, size_t, size_t plan_floats) {
    for (int i = 0; i < n; ++i) {
        const GemmJob& q = jobs[i];
        GemmEpi e; e.act = 0; e.out2 = nullptr; e.drop.p = 0.f; e.drop.seed = 0; e.drop.site = 0; e.dbias = q.dbias;
        gemm(s, 1, 0, q.M, q.N, q.K, q.A, q.lda, q.B, q.ldb, q.C, q.ldc, nullptr, 1, ws, plan_floats, &e);
    }
}
bool fused_available(const FusedDims&) { return false; }
void fused_pack_block(hipStream_t, const FusedDims&, const FusedBlockParams&, float*) {}
void fused_chain_a(hipStream_t, const FusedDims&, const FusedTopo&, const FusedBlockParams&, const float*, const float*, const float*, const float*,
                   const float*, float*, float*, float*, float*, float*, float*, float*) {}
void fused_chain_b(hipStream_t, const FusedDims&, const FusedTopo&, const FusedBlockParams&, const float*, const float*, const float*, const float*, Drop,
                   Drop, float*, float*, float*, float*, float*, float*, float*, float*, int, int) {}
void fused_chain_c(hipStream_t, const FusedDims&, const FusedTopo&, const FusedBlockParams&, const float*, const float*, const float*, const float*,
                   const float*, const float*, float*, float*, float*, float*, float*, float*) {}
}
namespace jt {
void fused_pack_block_bwd(hipStream_t, const FusedDims&, const FusedBlockParams&, float*) {}
void fused_bwd_c(hipStream_t, const FusedDims&, const FusedTopo&, const FusedBlockParams&, const float*, const float*, float*, const float*, const float*,
                 const float*, const float*, float*, float*, float*, float*, float*) {}
void fused_bwd_b(hipStream_t, const FusedDims&, const FusedTopo&, const FusedBlockParams&, const float*, const float*, const float*, const float*, const float*,
                 const float*, const float*, Drop, Drop, float*, float*, float*, float*, float*) {}
void fused_bwd_a(hipStream_t, const FusedDims&, const FusedTopo&, const FusedBlockParams&, const float*, const float*, const float*, const float*, const float*,
                 const float*, float*, float*, float*, float*) {}
void fused_node_ln_mod(hipStream_t, long, int, const float*, const float*, const int*, const float*, int, int, int, int, float*, float*, float*) {}
void fused_node_ln_mod_bwd(hipStream_t, long, int, const float*, const float*, const float*, const int*, const float*, int, int, float*, int) {}
bool fused_attention_available(int, int, int) { return false; }
void fused_attn_fwd(hipStream_t, const AttnTopo&, int, int, int, int, float, const float*, const float*, const float*, const float*, const float*, const float*,
                    const float*, float*, float*) {}
void fused_attn_bwd(hipStream_t, const AttnTopo&, int, int, int, int, float, const float*, const float*, const float*, const float*, const float*, const float*,
                    const float*, float*, float*, float*, float*, float*, float*) {}
void fused_gbf_bwd(hipStream_t, long, int, const float*, const int*, const float*, const float*, const float*, const float*, int, int, float*, float*, int,
                   float*, float*) {}
}

// TEST INFRASTRUCTURE ONLY: the 2-D fused chains (jodo_amd/csrc/train_fused.hip) are matrix-instruction kernels, not available to the
// host emulation, which runs — and thereby checks — the op-by-op sequence they replace (../emul/emul_gemm.cpp does the same for the 3-D ones).
#include "train_fused.h"
namespace jt {
bool fused_chain_b_available(const FusedDims&) { return false; }
bool fused2d_available(const FusedDims&) { return false; }
void fused2d_pack_block(hipStream_t, const FusedDims&, const FusedBlockParams&, float*) {}
void fused2d_pack_block_bwd(hipStream_t, const FusedDims&, const FusedBlockParams&, float*) {}
void fused2d_chain_a(hipStream_t, const FusedDims&, const FusedTopo&, const float*, const float*, const float*, float*, float*, float*, float*, float*) {}
void fused2d_bwd_a(hipStream_t, const FusedDims&, const FusedTopo&, const float*, const float*, const float*, const float*, const float*, const float*, float*,
                   float*) {}
}

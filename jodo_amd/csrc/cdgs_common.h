// Shared by the CDGS inference kernels (cdgs_forward.hip), the training engine (cdgs_train.hip) and the packer (cdgs_pack.cpp): the
// few pieces both sides must agree on — the widths of the embedding parts, the sinusoid of the time embedding and the adjacency
// threshold.  (The walks themselves share nothing: inference is LDS / barrier kernels on compact rows, training is cooperation-free
// kernels on the reference's dense padded tile.)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace jcdgs {

// widths of the parts of the 256-wide embedding inputs, as the reference derives them from nf (models/cdgs.py): edges
// [cate | exist | spd] = [edge_type | edge_type | edge_se], atoms [degree | cate | rw] = [atom_se | atom_type | atom_se]
struct Widths { int edge_se, edge_type, atom_se, atom_type; };
inline Widths widths(int nf) {
    Widths w;
    w.edge_se = (int)(nf * 0.4); w.atom_se = (int)(nf * 0.2);
    w.edge_type = (int)(0.5 * (nf - w.edge_se)); w.atom_type = nf - 2 * w.atom_se;
    return w;
}

// channel c of the sinusoid of t * 999: [sin (half) | cos (half)], freq = the caller-made table [half]
__host__ __device__ __forceinline__ float sinusoid(float t, const float* freq, int c, int half) {
    const float arg = (t * 999.f) * freq[c < half ? c : c - half];
    return c < half ? sinf(arg) : cosf(arg);
}

// an ordered pair (r, c) of real atoms is adjacent when the first edge channel is not negative
__host__ __device__ __forceinline__ bool adjacent(bool real_pair, float edge_ch0) { return real_pair && edge_ch0 >= 0.f; }

}  // namespace jcdgs

// OPT-IN split-bf16 form of the UN-FOLDED pair update: the conditional model (cond_DGT_concat, nf 256) under JODO_OPT_SPLIT_BF16.
//
// Same work item, same formulas, same stores as wide::k_edge_update_sym<256, R, FOLD = false, ROT = false> (dgt_kernels_wide.h; the
// reference: MultiCondEquiUpdate models/mol_gnn.py:51-94, edge FFN + readout :313-317).  Every molecule has its own modulation row (its
// context enters the time embedding), so neither the folded coord_mlp.0 matrix nor the rotated statistics exist here:
//     S = W_in [e ; G]                 8 output blocks, K = 2 De = 8 K16 steps each; plain LayerNorm statistics around m0 (A.rmean)
//     Z = W0 (S (1 + sc))              8 output blocks, K = D = 16 steps each; sc = the molecule's own scale row
//     y = [Z + A_a + B_c - mean wg] rstd + bs,  SiLU, coord_mlp.2          per direction, wg / bs = the molecule's rows
// The machinery is the folded split kernel's (dgt_kernels_split.h): a workgroup of four waves, one pair item each, ONE weight stream
// through a three-slot LDS ring (here the node kernel's eight-step chunks), the split operands of dgt_split.h.  All weights are static, so a block is one tape (dgt_pack.cpp
// pack_split_cond_tape) and nothing comes from the workspace:
//     [edge FFN: per hidden chunk ff_linear3 blocks 2c, 2c + 1 | ff_linear4 steps 4c .. 4c + 3 of every block] [readout]
//     [input_lin's [e ; G] columns, blocks 0 .. 7] [coord_mlp.0, blocks 0 .. 7]          32 r / 2 + 4 + 64 + 128 steps = 228 (r = 2), 260 (r = 4)
// What the un-folded form has to keep is S (1 + sc): 128 values per lane from the S section into every block of the Z section.  It is
// kept as its split image (16 Split8 = 192 registers, converted once per pair offset), which does not fit beside a second workgroup:
// ONE workgroup per CU, one wave per SIMD, the 512-register budget (256 + 213 registers, no scratch).  Measured on MI355X, conditional
// B = 1250, pair update per block (profiles/split_cond_ab.txt): exact fp32 525 us; this kernel with the four-step ring and the per-node
// rows requested a block ahead 442, rows requested at their block's start 425, eight-step ring 407 (what is built).
#pragma once
#include "dgt_kernels_split.h"

namespace jd {
namespace split {

template <int V> using ic = std::integral_constant<int, V>;

// NS steps of the eight-step ring (Tape2: the node kernel's, dgt_kernels_split.h) starting H steps into chunk g, any alignment: a block may
// start in the middle of a chunk and cross its boundary (the readout is four steps long, so every S and Z block does).  Fragments are read
// one step ahead as in tape2_block; the read behind the tape's last step lands in a ring slot and is never used.
template <int NS, int H>
__device__ __forceinline__ f32x16 tape2_block_any(Tape2& T, int& g, const Split8* act, f32x16 acc) {
    static_assert(H >= 0 && H < N_CHS, "offset inside a chunk");
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int w = (H + s) % N_CHS, gi = g + (H + s) / N_CHS;
        if (w == 0) tape2_boundary(T, gi);
        const bf16x8 wh = as_bf16x8(T.cur[0]), wm = as_bf16x8(T.cur[1]), wl = as_bf16x8(T.cur[2]);
        const int wn = (H + s + 1) % N_CHS, gn = g + (H + s + 1) / N_CHS;
        const char* nx = T.ring + (gn % N_SLOTS) * N_CH_BYTES + wn * 3072 + T.rd_off;
        T.cur[0] = *reinterpret_cast<const u32x4*>(nx);
        T.cur[1] = *reinterpret_cast<const u32x4*>(nx + 1024);
        T.cur[2] = *reinterpret_cast<const u32x4*>(nx + 2048);
        pipeline_fence();
        acc = mfma_step_s(wh, wm, wl, act[s], acc);
    }
    g += (H + NS) / N_CHS;
    return acc;
}

template <int D, int R>
__global__ __launch_bounds__(SPLIT_WAVES * 64, 1) void k_edge_update_sym_split_cond(KArgs A) {
    static_assert(D == 256, "the un-folded split-bf16 pair update is built for nf = 256");
    if (A.flags[FLAG_ASYM]) return;                  // (per-molecule modulation rows are the point: no FLAG_UNIFORM_T condition; a violated
                                                     // symmetric pin is reported by k_finalize_nodes like for every pinned launch)
    using X = wide::Dim<D>;
    constexpr int NCH = R * X::De / 64;              // hidden chunks of the edge FFN
    constexpr int NSE = X::De / 16;                  // K16 steps of a K = De projection (4)
    constexpr int NSZ = 2 * NSE;                     // steps of a K = 2 De projection (8)
    constexpr int NSD = D / 16;                      // steps of a K = D projection (16)
    constexpr int CHUNK_STEPS_FFN = 2 * NSE + X::NE * 4;
    constexpr int STEPS = NCH * CHUNK_STEPS_FFN + NSE + X::ND * NSZ + X::ND * NSD;
    static_assert(NSD % N_CHS == 0, "Z blocks keep their offset inside an eight-step chunk");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, jl = lane & 31, half = lane >> 5;
    // items: as the folded split kernel — workgroup w lives on XCD w % 8 and takes four of that XCD's items (xcd_order)
    int it = ((int)blockIdx.x >> 3) * 32 + ((int)blockIdx.x & 7) + 8 * wave;
    const bool live = it < A.pd.n_pitems;            // an idle wave walks item 0 without stores: the ring needs all four waves
    if (!live) it = 0;
    const int strip = A.pd.pitem_strip[it], t = A.pd.pitem_t0[it];
    const LaneNode L = lane_node(A, strip, jl);
    const float* mrow = mod_row(A, L.b) + A.mod_base;
    const float* eg1 = mrow + X::M_EDGE + 2 * X::De;
    const float gscale = mrow[X::M_GBF + 0], gshift = mrow[X::M_GBF + 1];
    const float4 pv = reinterpret_cast<const float4*>(A.pos_out)[L.v];
    const float cscale = A.W[A.wb[JB_CSCALE]];

    __shared__ u32x4 ring[N_SLOTS * N_CH_BYTES / 16];
    __shared__ float4 w2s[3 * D / 4];
    {
        const float4* src = reinterpret_cast<const float4*>(A.W + A.wb[JB_C2_W]);
        for (int i = threadIdx.x; i < 3 * D / 4; i += SPLIT_WAVES * 64) w2s[i] = src[i];
    }
    // The eight-step ring of the node kernel (Tape2, 3 x 24 KiB: one workgroup per CU has the LDS to itself).  The descriptor covers exactly
    // this block's tape: the last chunk is half a chunk (228 = 28 * 8 + 4 steps), its upper half reads as zero instead of reaching behind
    // the tape.
    Tape2 T;
    T.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(A.wsplit), 0, STEPS * 3072, 0x00020000);
    T.ntot = (STEPS + N_CHS - 1) / N_CHS;
    T.ld_off = (unsigned)wave * (unsigned)(N_CH_BYTES / SPLIT_WAVES) + (unsigned)lane * 16u;
    T.rd_off = (unsigned)lane * 16u;
    T.ring = reinterpret_cast<char*>(ring);
    tape2_start(T, 0);                                // (its barrier also publishes w2s)
    int g = 0;                                        // tape chunk being consumed
    // NS steps that start OFF steps into the tape (every section's position is known at compile time)
    auto blk = [&](auto ns, auto off, const Split8* act, f32x16 acc) -> f32x16 {
        return tape2_block_any<decltype(ns)::value, decltype(off)::value % N_CHS>(T, g, act, acc);
    };
    constexpr int OFF_RO = NCH * CHUNK_STEPS_FFN, OFF_S = OFF_RO + NSE, OFF_Z = OFF_S + X::ND * NSZ;

    const PairLane P = pair_of(L, t + 1);
    const bool okw = P.ok && live;
    const float* eg1_ = launder(eg1);
    const float* es2_ = eg1_ + X::De, *ec2_ = es2_ + X::De, *eg2_ = ec2_ + X::De;
    const float* qsc_ = launder(mrow + X::M_EQUI) + D;
    const float* cst = launder(A.W);
    const float* n2bias_ = cst + A.wb[JB_N2E_B], *b3_ = cst + A.wb[JB_FF3_B], *b4_ = cst + A.wb[JB_FF4_B];
    const float* tab_ = cst + A.wb[JB_GBF], *bro_ = cst + A.wb[JB_ERO_B];
    const BRow wrow_i = brow(A.wrow, X::ND, L.v, half), wcol_i = brow(A.wcol, X::ND, L.v, half);
    const BRow wrow_j = brow(A.wrow, X::ND, P.u, half), wcol_j = brow(A.wcol, X::ND, P.u, half);
    const BRow ua_i = brow(A.ua, X::ND, L.v, half), ub_i = brow(A.ub, X::ND, L.v, half);
    const BRow ua_j = brow(A.ua, X::ND, P.u, half), ub_j = brow(A.ub, X::ND, P.u, half);
    const float4 pu = reinterpret_cast<const float4*>(A.pos_out)[P.u];
    const float dx = pv.x - pu.x, dy = pv.y - pu.y, dz = pv.z - pu.z;
    const float d2 = dx * dx + dy * dy + dz * dz;
    // ---- edge residual + LN2 + modulate (symmetric) ----
    float en[X::HE];
    {
        const TRow ra = trow(A.n2e, X::NE, L.v, half), rc = trow(A.n2e, X::NE, P.u, half);
#pragma unroll
        for (int b = 0; b < X::NE; ++b) {
            float e[16], ta[16], tc2[16], g[16], bb[16];
            load16(A.e + P.rij * X::De + b * 32 + half * 16, e);
            load16T(ra, b, ta);
            load16T(rc, b, tc2);
            load16(eg1_ + b * 32 + half * 16, g);
            load16(n2bias_ + b * 32 + half * 16, bb);
#pragma unroll
            for (int s = 0; s < 16; ++s) en[b * 16 + s] = fmaf(g[s], ta[s] + tc2[s] + bb[s], e[s]);
        }
    }
    layer_norm<X::HE>(en);
    modulate<X::NE>(en, es2_, ec2_, half);
    Split8 zs[NSZ];                                   // [en ; G] as split operands: steps 0 .. NSE - 1 = en, NSE .. = G (filled behind the FFN)
    split_regs<X::HE>(en, zs);
    // ---- edge FFN ----
    {
        f32x16 o[X::NE];
#pragma unroll
        for (int b = 0; b < X::NE; ++b) o[b] = zero16();
        static_for<NCH>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            float hid[32];
            static_for<2>([&](auto bc) {
                constexpr int b2 = decltype(bc)::value;
                float bb[16];
                load16(b3_ + (c * 2 + b2) * 32 + half * 16, bb);
                const f32x16 acc = blk(ic<NSE>{}, ic<c * CHUNK_STEPS_FFN + b2 * NSE>{}, zs, zero16());
                silu_bias16(acc, bb, hid + b2 * 16);
            });
            Split8 hs[4];
            split_regs<32>(hid, hs);
            static_for<X::NE>([&](auto oc) {
                constexpr int ob = decltype(oc)::value;
                o[ob] = blk(ic<4>{}, ic<c * CHUNK_STEPS_FFN + 2 * NSE + ob * 4>{}, hs, o[ob]);
            });
        });
#pragma unroll
        for (int b = 0; b < X::NE; ++b) {
            float ob4[16], og2[16];
            load16(b4_ + b * 32 + half * 16, ob4);
            load16(eg2_ + b * 32 + half * 16, og2);
#pragma unroll
            for (int s = 0; s < 16; ++s) en[b * 16 + s] = fmaf(og2[s], o[b][s] + ob4[s], en[b * 16 + s]);
        }
    }
    if (okw) {
        store_nat<X::NE>(A.e_out + P.rij * X::De, half, en);
        if (!A.half_rows || L.n > PAIR_GROUP_LANES) store_nat<X::NE>(A.e_out + P.rji * X::De, half, en);
    }
    split_regs<X::HE>(en, zs);                        // the block's output edge state feeds the readout and S
    {
        float G[X::HE];
        gbf_n<X::NE>(d2, gscale, gshift, tab_, half, G);
        split_regs<X::HE>(G, zs + NSE);
    }
    const float m00 = A.rmean[(size_t)L.v * 2] + A.rmean[(size_t)P.u * 2 + 1];          // direction 0: a = i, c = j
    const float m01 = A.rmean[(size_t)P.u * 2] + A.rmean[(size_t)L.v * 2 + 1];          // direction 1: a = j, c = i
    // ---- readout ----
    {
        float bb[16];
        load16(bro_ + half * 16, bb);
        const f32x16 acc = blk(ic<NSE>{}, ic<OFF_RO>{}, zs, zero16());
        float rr[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) rr[s] = acc[s] + bb[s];
        if (okw && (half == 0 || A.d.cep == 32)) {
            store16(A.ehid + P.rij * A.d.KEH + X::De + A.layer * A.d.cep + half * 16, rr);
            if (!A.half_rows || L.n > PAIR_GROUP_LANES) store16(A.ehid + P.rji * A.d.KEH + X::De + A.layer * A.d.cep + half * 16, rr);
        }
    }
    // ---- S = W_in [e ; G] block by block: LayerNorm statistics of both directions (variance around m0 = mean(R_a) + mean(C_c), corrected
    // by meanS^2: dgt_kernels_wide.h), and S (1 + sc) straight into its split image ----
    Split8 sgs[NSD];
    f32x2 q02 = {0.f, 0.f}, q12 = {0.f, 0.f}, ssum2 = {0.f, 0.f};
    static_for<X::ND>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        // the block's per-node rows are requested at its start and consumed behind its MFMAs (1.5 k matrix cycles of cover; a request one
        // block ahead, as the exact kernel does it, costs 32 more live registers and spills)
        float sc[16], n0[16], n1[16], n2[16], n3[16];
        bload16(wrow_i, b, n0); bload16(wcol_j, b, n1); bload16(wrow_j, b, n2); bload16(wcol_i, b, n3);
        load16(qsc_ + b * 32 + half * 16, sc);
        pipeline_fence();
        const f32x16 acc = blk(ic<NSZ>{}, ic<OFF_S + b * NSZ>{}, zs, zero16());
        float m[16];
#pragma unroll
        for (int s = 0; s < 16; s += 2) {
            const f32x2 sv = pk2(acc[s], acc[s + 1]);
            ssum2 = ssum2 + sv;
            const f32x2 mm = sv * (pk2(sc[s], sc[s + 1]) + 1.f);
            m[s] = mm.x; m[s + 1] = mm.y;
            const f32x2 t0 = (pk2(n0[s], n0[s + 1]) + pk2(n1[s], n1[s + 1])) - m00, t1 = (pk2(n2[s], n2[s + 1]) + pk2(n3[s], n3[s + 1])) - m01;
            const f32x2 d0 = sv + t0, d1 = sv + t1;
            q02 = __builtin_elementwise_fma(d0, d0, q02);
            q12 = __builtin_elementwise_fma(d1, d1, q12);
        }
        sgs[2 * b] = split8(m);
        sgs[2 * b + 1] = split8(m + 8);
    });
    const float meanS = pair_sum(ssum2.x + ssum2.y) * (1.f / D);
    const float rstd0 = __builtin_amdgcn_rsqf(fmaxf(pair_sum(q02.x + q02.y) * (1.f / D) - meanS * meanS, 0.f) + 1e-6f);
    const float rstd1 = __builtin_amdgcn_rsqf(fmaxf(pair_sum(q12.x + q12.y) * (1.f / D) - meanS * meanS, 0.f) + 1e-6f);
    const float mr0 = (meanS + m00) * rstd0, mr1 = (meanS + m01) * rstd1;
    // ---- Z = W0 (S (1 + sc)) block by block, SiLU / coord_mlp.2 tails of both directions ----
    const float* wg_v = launder(mrow + X::M_WG);
    const float* bs_v = wg_v + D;
    f32x2 c00 = {0.f, 0.f}, c01 = c00, c02 = c00, c10 = c00, c11 = c00, c12 = c00;
#pragma unroll 1
    for (int b = 0; b < X::ND; ++b) {
        // rows of this block: requested here, consumed by the tails behind the block's 3 k matrix cycles
        float n0[16], n1[16], n2[16], n3[16], wgb[16], bsb[16];
        bload16(ua_i, b, n0); bload16(ub_j, b, n1); bload16(ua_j, b, n2); bload16(ub_i, b, n3);
        load16(wg_v + b * 32 + half * 16, wgb);
        load16(bs_v + b * 32 + half * 16, bsb);
        pipeline_fence();
        const f32x16 z = blk(ic<NSD>{}, ic<OFF_Z>{}, sgs, zero16());      // (NSD is a whole number of chunks: every Z block starts at the same offset)
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
            float k0[8], k1[8], k2[8], ca[8];
            auto ld8 = [&](const float* p8, float (&r)[8]) {
                const float4 a = reinterpret_cast<const float4*>(p8)[0], c = reinterpret_cast<const float4*>(p8)[1];
                r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = c.x; r[5] = c.y; r[6] = c.z; r[7] = c.w;
            };
            const int fo = b * 32 + half * 16 + hq * 8;
            const float* w2l = reinterpret_cast<const float*>(w2s);
            ld8(w2l + fo, k0); ld8(w2l + D + fo, k1); ld8(w2l + 2 * D + fo, k2);
#pragma unroll
            for (int s = 0; s < 8; s += 2) {
                const f32x2 c = __builtin_elementwise_fma((f32x2)(-mr0), pk2(wgb[hq * 8 + s], wgb[hq * 8 + s + 1]), pk2(bsb[hq * 8 + s], bsb[hq * 8 + s + 1]));
                ca[s] = c.x; ca[s + 1] = c.y;
            }
            pipeline_fence();
#pragma unroll
            for (int s = 0; s < 8; s += 2) {
                const f32x2 pre = pk2(z[hq * 8 + s], z[hq * 8 + s + 1]) + (pk2(n0[hq * 8 + s], n0[hq * 8 + s + 1]) + pk2(n1[hq * 8 + s], n1[hq * 8 + s + 1]));
                const f32x2 ys0 = silu_f2(__builtin_elementwise_fma(pre, (f32x2)(rstd0), pk2(ca[s], ca[s + 1])));
                c00 = __builtin_elementwise_fma(ys0, pk2(k0[s], k0[s + 1]), c00);
                c01 = __builtin_elementwise_fma(ys0, pk2(k1[s], k1[s + 1]), c01);
                c02 = __builtin_elementwise_fma(ys0, pk2(k2[s], k2[s + 1]), c02);
            }
            pipeline_fence();
#pragma unroll
            for (int s = 0; s < 8; s += 2) {
                const f32x2 c = __builtin_elementwise_fma((f32x2)(-mr1), pk2(wgb[hq * 8 + s], wgb[hq * 8 + s + 1]), pk2(bsb[hq * 8 + s], bsb[hq * 8 + s + 1]));
                ca[s] = c.x; ca[s + 1] = c.y;
            }
#pragma unroll
            for (int s = 0; s < 8; s += 2) {
                const f32x2 pre = pk2(z[hq * 8 + s], z[hq * 8 + s + 1]) + (pk2(n2[hq * 8 + s], n2[hq * 8 + s + 1]) + pk2(n3[hq * 8 + s], n3[hq * 8 + s + 1]));
                const f32x2 ys1 = silu_f2(__builtin_elementwise_fma(pre, (f32x2)(rstd1), pk2(ca[s], ca[s + 1])));
                c10 = __builtin_elementwise_fma(ys1, pk2(k0[s], k0[s + 1]), c10);
                c11 = __builtin_elementwise_fma(ys1, pk2(k1[s], k1[s + 1]), c11);
                c12 = __builtin_elementwise_fma(ys1, pk2(k2[s], k2[s + 1]), c12);
            }
            pipeline_fence();
        }
    }
    const float nrm = fmaxf(sqrtf(d2), 1e-8f);
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const float c0 = tanh_f(pair_sum(dir == 0 ? c00.x + c00.y : c10.x + c10.y));
        const float c1 = tanh_f(pair_sum(dir == 0 ? c01.x + c01.y : c11.x + c11.y));
        const float c2 = tanh_f(pair_sum(dir == 0 ? c02.x + c02.y : c12.x + c12.y));
        const size_t rr = dir == 0 ? P.rij : P.rji;
        const int fl = A.eflag[rr];
        const float iota = (c0 + ((fl & 1) ? c1 : 0.f) + ((fl & 2) ? c2 : 0.f)) * (1.f / 3.f);
        const float f = cscale * iota / nrm;
        const float sgn = dir == 0 ? 1.f : -1.f;
        if (okw && half == 0)
            reinterpret_cast<float4*>(A.dposE)[rr] = make_float4(sgn * dx * f, sgn * dy * f, sgn * dz * f, 0.f);
    }
}

}  // namespace split
}  // namespace jd

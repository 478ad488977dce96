// Test entry into the fused training kernels (train_fused.h): jodo_train_debug_fused runs ONE of their public host functions on
// caller-owned device arrays, so that tests/test_fused_kernels_gpu.py can compare every array a kernel stores with a float64
// restatement.  No kernel lives here.  The entry is the safety boundary of those tests: the availability predicates, every topology
// index, every array length and alignment are checked on the host before anything is launched (include/jodo_hip.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"
#include "train_fused.h"

namespace {

const char* const OP_NAME[JODO_FT_N_OPS] = {
    "fused_pack_block", "fused_pack_block_bwd", "fused2d_pack_block", "fused2d_pack_block_bwd", "fused_chain_a", "fused_chain_b", "fused_chain_c",
    "fused_bwd_a", "fused_bwd_b", "fused_bwd_c", "fused2d_chain_a", "fused2d_bwd_a", "fused_node_ln_mod", "fused_node_ln_mod_bwd",
    "fused_attn_fwd", "fused_attn_bwd", "fused_gbf_bwd"};
const char* const SLOT_NAME[JODO_FT_N_SLOTS] = {
    "edge_emb_w", "edge_emb_b", "le0", "le1", "ff3_w", "ff3_b", "ff4_w", "ff4_b", "ero_w", "ero_b", "in_w", "in_b", "c0_w", "c0_b", "c2_w", "n2e_b",
    "gbf_means", "gbf_stds", "packed", "pos", "gm", "e_in", "emod", "d2", "G", "xh", "rs", "et", "t0", "t1", "n2e", "en", "f3", "a3", "f4", "e_out",
    "eh", "hr", "hc", "qmod", "u", "c0pre", "c0a", "inv", "dinv", "dc0", "du", "dpre", "de", "dG", "de_out", "f4d", "df4", "dhid", "den", "de_prev",
    "dt1", "dt0", "det", "de1", "mods", "q", "k", "v", "adj2d", "adjsp", "alpha", "hhat", "dhhat", "dS", "dq", "dk", "dv", "dxp", "dd2", "part_m",
    "part_s"};

// the checks of one call: the first failure records its message and every later check is skipped
struct Check {
    const jodo_fused_test_args& a;
    const char* op;
    int rc = JODO_OK;
    int32_t* dev;          // next free int of topo_dev
    size_t dev_left;
    hipStream_t s;

    bool fail(const char* what) { if (rc == JODO_OK) rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): %s", op, what); return false; }
    // a device float array of at least `need` elements; align: 16 bytes where the kernel moves float4s, 4 where it reads single floats
    float* arr(int slot, size_t need, unsigned align = 16) {
        if (rc != JODO_OK) return nullptr;
        float* p = a.a[slot];
        if (!p) { rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): array %s is a null pointer", op, SLOT_NAME[slot]); return nullptr; }
        if (((uintptr_t)p & (align - 1)) != 0) { rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): array %s is not %u-byte aligned", op, SLOT_NAME[slot], align); return nullptr; }
        if (a.n[slot] < need) {
            rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): array %s has %zu floats, the op touches %zu", op, SLOT_NAME[slot], a.n[slot], need);
            return nullptr;
        }
        return p;
    }
    float* arr_opt(int slot, size_t need) { return a.a[slot] ? arr(slot, need) : nullptr; }
    // rows of `width` floats at stride ld
    float* strided(int slot, long rows, int ld, int width) {
        if (rc != JODO_OK) return nullptr;
        if (ld < width || width < 1) {
            rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): row stride %d of %s does not hold its %d columns", op, ld, SLOT_NAME[slot], width);
            return nullptr;
        }
        return arr(slot, (size_t)(rows - 1) * ld + width, 4);
    }
    // a host index array of `count` entries in [0, bound): checked, then uploaded
    const int* idx(const int32_t* host, const char* name, long count, long bound) {
        if (rc != JODO_OK) return nullptr;
        if (!host) { rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): topology array %s is a null pointer", op, name); return nullptr; }
        for (long i = 0; i < count; ++i)
            if (host[i] < 0 || host[i] >= bound) {
                rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): %s[%ld] = %d is out of range [0, %ld)", op, name, i, host[i], bound);
                return nullptr;
            }
        return upload(host, name, count);
    }
    const int* upload(const int32_t* host, const char* name, long count) {
        if (rc != JODO_OK) return nullptr;
        if (!a.topo_dev || ((uintptr_t)a.topo_dev & 3) != 0) { fail("topo_dev is a null or misaligned pointer"); return nullptr; }
        if (dev_left < (size_t)count) {
            rc = jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): topo_dev has %zu ints, the op uploads more (at %s)", op, a.topo_dev_count, name);
            return nullptr;
        }
        if (hipMemcpyAsync(dev, host, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess) {
            rc = jodo_set_error(JODO_ERR_LAUNCH, "jodo_train_debug_fused(%s): upload of %s failed", op, name);
            return nullptr;
        }
        const int* p = dev;
        dev += count; dev_left -= (size_t)count;
        return p;
    }
};

int unsupported(const char* op, const char* pred, const jodo_fused_test_args& a) {
    return jodo_set_error(JODO_ERR_UNSUPPORTED, "jodo_train_debug_fused(%s): %s is false for D %d, De %d, r %d, QK %d, ce %d, nco %d, H %d, N %d", op, pred,
                          a.D, a.De, a.r, a.QK, a.ce, a.nco, a.H, a.N);
}

}  // namespace

extern "C" int jodo_train_debug_fused(const jodo_fused_test_args* args, void* stream) {
    using namespace jt;
    if (!args) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused: args is a null pointer");
    const jodo_fused_test_args& a = *args;
    if (a.op < 0 || a.op >= JODO_FT_N_OPS) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused: unknown op %d", a.op);
    const char* op = OP_NAME[a.op];
    hipStream_t s = (hipStream_t)stream;
    Check c{a, op, JODO_OK, a.topo_dev, a.topo_dev_count, s};
    const bool pack = a.op <= JODO_FT_PACK_2D_BWD, node = a.op == JODO_FT_NODE_LN_MOD || a.op == JODO_FT_NODE_LN_MOD_BWD;
    const bool attn = a.op == JODO_FT_ATTN_FWD || a.op == JODO_FT_ATTN_BWD, gbf = a.op == JODO_FT_GBF_BWD, chain = !pack && !node && !attn && !gbf;
    if ((chain || attn || gbf) && (a.R <= 0 || a.B <= 0)) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): non-positive count (R %d, B %d)", op, a.R, a.B);
    if ((node || attn || a.op == JODO_FT_CHAIN_A || a.op == JODO_FT_CHAIN_B || a.op == JODO_FT_CHAIN_C) && (a.Nn <= 0 || a.B <= 0))
        return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): non-positive count (Nn %d, B %d)", op, a.Nn, a.B);

    // ---- availability: the predicate of the op on its dims, before anything else is looked at
    FusedDims d{a.D, a.De, a.r, a.QK, a.ce, 1, a.nco};
    if (pack || chain) {
        if (a.D <= 0 || a.De <= 0 || a.r <= 0 || a.QK <= 0 || a.ce <= 0)
            return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): non-positive dim (D %d, De %d, r %d, QK %d, ce %d)", op, a.D, a.De, a.r, a.QK, a.ce);
        const bool two_d = a.op == JODO_FT_PACK_2D || a.op == JODO_FT_PACK_2D_BWD || a.op == JODO_FT_CHAIN_A_2D || a.op == JODO_FT_BWD_A_2D;
        const bool only_b = a.op == JODO_FT_CHAIN_B || a.op == JODO_FT_BWD_B;
        if (two_d) { if (!fused2d_available(d)) return unsupported(op, "fused2d_available", a); }
        else if (only_b) { if (!fused_chain_b_available(d)) return unsupported(op, "fused_chain_b_available", a); }
        else if (!fused_available(d)) return unsupported(op, "fused_available", a);
    }
    if (node && !(a.D == 128 || a.D == 256 || a.D == 384)) return unsupported(op, "F in {128, 256, 384}", a);
    if (attn) {
        if (a.H <= 0 || a.N <= 0 || a.D <= 0) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): non-positive dim (D %d, H %d, N %d)", op, a.D, a.H, a.N);
        if (!fused_attention_available(a.D, a.H, a.N)) return unsupported(op, "fused_attention_available", a);
    }
    if (gbf && (a.De < 2 || a.De > 129)) return unsupported(op, "2 <= De <= 129", a);

    const size_t D = (size_t)a.D, De = (size_t)a.De, HID = (size_t)a.r * De, QK = (size_t)a.QK, R = (size_t)a.R, Nn = (size_t)a.Nn, B = (size_t)a.B;
    FusedBlockParams p{};
    float* packed = nullptr;
    if (pack || chain) packed = c.arr(JODO_FT_PACKED, fused_pack_layout(d).total_bwd);
    FusedTopo t{a.R, nullptr, nullptr, nullptr, a.save ? 1 : 0};
    const Drop d3{a.drop_p, a.seed, (unsigned)a.site_a3}, d4{a.drop_p, a.seed, (unsigned)a.site_f4};
    if ((a.op == JODO_FT_CHAIN_B || a.op == JODO_FT_BWD_B) && !(a.drop_p >= 0.f && a.drop_p < 1.f)) c.fail("dropout probability outside [0, 1)");
#define ARR(slot, need) c.arr(JODO_FT_##slot, (size_t)(need))
#define RUN(call) do { if (c.rc != JODO_OK) return c.rc; call; return jodo_check_launch(op); } while (0)

    switch (a.op) {
    case JODO_FT_PACK: {          // in: the eight weight matrices, gbf_means, gbf_stds;  out: packed (forward images and the Gaussian table)
        p.edge_emb_w = ARR(EDGE_EMB_W, De * 2 * De); p.le0 = ARR(LE0, QK * De); p.le1 = ARR(LE1, D * De); p.ff3_w = ARR(FF3_W, HID * De);
        p.ff4_w = ARR(FF4_W, De * HID); p.ero_w = ARR(ERO_W, a.ce * De); p.in_w = ARR(IN_W, D * (2 * D + 2 * De)); p.c0_w = ARR(C0_W, D * D);
        p.gbf_means = ARR(GBF_MEANS, De - 1); p.gbf_stds = ARR(GBF_STDS, De - 1);
        RUN(fused_pack_block(s, d, p, packed));
    }
    case JODO_FT_PACK_BWD: {      // in: c0_w, in_w, ff4_w, ff3_w, le1, le0, edge_emb_w;  out: packed (transposed images)
        p.c0_w = ARR(C0_W, D * D); p.in_w = ARR(IN_W, D * (2 * D + 2 * De)); p.ff4_w = ARR(FF4_W, De * HID); p.ff3_w = ARR(FF3_W, HID * De);
        p.le1 = ARR(LE1, D * De); p.le0 = ARR(LE0, QK * De); p.edge_emb_w = ARR(EDGE_EMB_W, De * 2 * De);
        RUN(fused_pack_block_bwd(s, d, p, packed));
    }
    case JODO_FT_PACK_2D: {       // in: le0, le1, ff3_w, ff4_w, ero_w;  out: packed
        p.le0 = ARR(LE0, QK * De); p.le1 = ARR(LE1, D * De); p.ff3_w = ARR(FF3_W, HID * De); p.ff4_w = ARR(FF4_W, De * HID); p.ero_w = ARR(ERO_W, a.ce * De);
        RUN(fused2d_pack_block(s, d, p, packed));
    }
    case JODO_FT_PACK_2D_BWD: {   // in: ff4_w, ff3_w, le1, le0;  out: packed
        p.ff4_w = ARR(FF4_W, De * HID); p.ff3_w = ARR(FF3_W, HID * De); p.le1 = ARR(LE1, D * De); p.le0 = ARR(LE0, QK * De);
        RUN(fused2d_pack_block_bwd(s, d, p, packed));
    }
    case JODO_FT_CHAIN_A: {       // in: packed, edge_emb_b, pos, gm, e_in, emod;  out: d2, G, xh, rs, et, t0, t1
        t.edge_a = c.idx(a.edge_a, "edge_a", a.R, a.Nn); t.edge_c = c.idx(a.edge_c, "edge_c", a.R, a.Nn); t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        p.edge_emb_b = ARR(EDGE_EMB_B, De);
        const float *pos = ARR(POS, Nn * 3), *gm = ARR(GM, B * 2), *e_in = ARR(E_IN, R * De), *emod = ARR(EMOD, B * 6 * De);
        float *d2 = ARR(D2, R), *G = ARR(G, R * De), *xh = ARR(XH, R * De), *rs = ARR(RS, R), *et = ARR(ET, R * De), *t0 = ARR(T0, R * QK), *t1 = ARR(T1, R * D);
        RUN(fused_chain_a(s, d, t, p, packed, pos, gm, e_in, emod, d2, G, xh, rs, et, t0, t1));
    }
    case JODO_FT_CHAIN_B: {       // in: packed, n2e_b, ff3_b, ff4_b, ero_b, e_in, n2e, emod;  out: xh, rs, en, f3, a3, f4, e_out, eh (ld_eh, eh_col)
        t.edge_a = c.idx(a.edge_a, "edge_a", a.R, a.Nn); t.edge_c = c.idx(a.edge_c, "edge_c", a.R, a.Nn); t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        p.n2e_b = ARR(N2E_B, De); p.ff3_b = ARR(FF3_B, HID); p.ff4_b = ARR(FF4_B, De); p.ero_b = ARR(ERO_B, a.ce);
        const float *e_in = ARR(E_IN, R * De), *n2e = ARR(N2E, Nn * De), *emod = ARR(EMOD, B * 6 * De);
        float *xh = ARR(XH, R * De), *rs = ARR(RS, R), *en = ARR(EN, R * De), *f3 = ARR(F3, R * HID), *a3 = ARR(A3, R * HID), *f4 = ARR(F4, R * De), *e_out = ARR(E_OUT, R * De);
        if (a.eh_col < 0 || a.ld_eh < a.eh_col + a.ce) c.fail("ld_eh does not hold columns eh_col .. eh_col + ce - 1");
        float* eh = c.rc == JODO_OK ? c.arr(JODO_FT_EH, (R - 1) * (size_t)a.ld_eh + (size_t)(a.eh_col + a.ce)) : nullptr;
        RUN(fused_chain_b(s, d, t, p, packed, e_in, n2e, emod, d3, d4, xh, rs, en, f3, a3, f4, e_out, eh, a.ld_eh, a.eh_col));
    }
    case JODO_FT_CHAIN_C: {       // in: packed, in_b, c0_b, c2_w, e_in, G, hr, hc, qmod;  out: xh [R, D], rs, u, c0pre, c0a, inv [R, nco]
        t.edge_a = c.idx(a.edge_a, "edge_a", a.R, a.Nn); t.edge_c = c.idx(a.edge_c, "edge_c", a.R, a.Nn); t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        p.in_b = ARR(IN_B, D); p.c0_b = ARR(C0_B, D); p.c2_w = ARR(C2_W, a.nco * D);
        const float *e_in = ARR(E_IN, R * De), *G = ARR(G, R * De), *hr = ARR(HR, Nn * D), *hc = ARR(HC, Nn * D), *qmod = ARR(QMOD, B * 2 * D);
        float *xh = ARR(XH, R * D), *rs = ARR(RS, R), *u = ARR(U, R * D), *c0pre = ARR(C0PRE, R * D), *c0a = ARR(C0A, R * D), *inv = ARR(INV, R * a.nco);
        RUN(fused_chain_c(s, d, t, p, packed, e_in, G, hr, hc, qmod, xh, rs, u, c0pre, c0a, inv));
    }
    case JODO_FT_BWD_C: {         // in: packed, c2_w, inv, c0pre, xh [R, D], rs, qmod;  in/out: dinv, de (+=);  out: dc0, du, dpre, dG
        t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        p.c2_w = ARR(C2_W, a.nco * D);
        const float *inv = ARR(INV, R * a.nco), *c0pre = ARR(C0PRE, R * D), *xh = ARR(XH, R * D), *rs = ARR(RS, R), *qmod = ARR(QMOD, B * 2 * D);
        float *dinv = ARR(DINV, R * a.nco), *dc0 = ARR(DC0, R * D), *du = ARR(DU, R * D), *dpre = ARR(DPRE, R * D), *de = ARR(DE, R * De), *dG = ARR(DG, R * De);
        RUN(fused_bwd_c(s, d, t, p, packed, inv, dinv, c0pre, xh, rs, qmod, dc0, du, dpre, de, dG));
    }
    case JODO_FT_BWD_B: {         // in: packed, de_out, f4, f3, xh, rs, emod;  out: f4d, df4, dhid, den, de_prev
        t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        const float *de_out = ARR(DE_OUT, R * De), *f4 = ARR(F4, R * De), *f3 = ARR(F3, R * HID), *xh = ARR(XH, R * De), *rs = ARR(RS, R), *emod = ARR(EMOD, B * 6 * De);
        float *f4d = ARR(F4D, R * De), *df4 = ARR(DF4, R * De), *dhid = ARR(DHID, R * HID), *den = ARR(DEN, R * De), *de_prev = ARR(DE_PREV, R * De);
        RUN(fused_bwd_b(s, d, t, p, packed, de_out, f4, f3, xh, rs, emod, d3, d4, f4d, df4, dhid, den, de_prev));
    }
    case JODO_FT_BWD_A: {         // in: packed, dt1, dt0, xh, rs, emod;  out: det, de1;  in/out: dG (+=), de_prev (+=)
        t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        const float *dt1 = ARR(DT1, R * D), *dt0 = ARR(DT0, R * QK), *xh = ARR(XH, R * De), *rs = ARR(RS, R), *emod = ARR(EMOD, B * 6 * De);
        float *det = ARR(DET, R * De), *de1 = ARR(DE1, R * De), *dG = ARR(DG, R * De), *de_prev = ARR(DE_PREV, R * De);
        RUN(fused_bwd_a(s, d, t, p, packed, dt1, dt0, xh, rs, emod, det, de1, dG, de_prev));
    }
    case JODO_FT_CHAIN_A_2D: {    // in: packed, e_in, emod;  out: xh, rs, et, t0, t1
        t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        const float *e_in = ARR(E_IN, R * De), *emod = ARR(EMOD, B * 6 * De);
        float *xh = ARR(XH, R * De), *rs = ARR(RS, R), *et = ARR(ET, R * De), *t0 = ARR(T0, R * QK), *t1 = ARR(T1, R * D);
        RUN(fused2d_chain_a(s, d, t, packed, e_in, emod, xh, rs, et, t0, t1));
    }
    case JODO_FT_BWD_A_2D: {      // in: packed, dt1, dt0, xh, rs, emod;  out: det;  in/out: de_prev (+=)
        t.edge_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        const float *dt1 = ARR(DT1, R * D), *dt0 = ARR(DT0, R * QK), *xh = ARR(XH, R * De), *rs = ARR(RS, R), *emod = ARR(EMOD, B * 6 * De);
        float *det = ARR(DET, R * De), *de_prev = ARR(DE_PREV, R * De);
        RUN(fused2d_bwd_a(s, d, t, packed, dt1, dt0, xh, rs, emod, det, de_prev));
    }
    case JODO_FT_NODE_LN_MOD: {   // in: e_in = a [Nn, F], n2e = res_b [Nn, F] or NULL, mods [B, ldm];  out: xh, rs, e_out = y
        const int* row_mol = c.idx(a.row_mol, "row_mol", a.Nn, a.B);
        const float *x = ARR(E_IN, Nn * D), *res = c.arr_opt(JODO_FT_N2E, Nn * D);
        const int lo = res ? (a.g_off < a.sh_off ? a.g_off : a.sh_off) : a.sh_off, lo2 = lo < a.sc_off ? lo : a.sc_off;
        const int hi = res && a.g_off > a.sh_off ? a.g_off : a.sh_off, hi2 = hi > a.sc_off ? hi : a.sc_off;
        if (lo2 < 0 || (size_t)hi2 + D > (size_t)(a.ldm > 0 ? a.ldm : 0)) c.fail("a column offset of mods lies outside its row (ldm)");
        const float* mods = ARR(MODS, B * (size_t)(a.ldm > 0 ? a.ldm : 0));
        float *xh = ARR(XH, Nn * D), *rs = ARR(RS, Nn), *y = ARR(E_OUT, Nn * D);
        RUN(fused_node_ln_mod(s, a.Nn, a.D, x, res, row_mol, mods, a.ldm, a.g_off, a.sh_off, a.sc_off, xh, rs, y));
    }
    case JODO_FT_NODE_LN_MOD_BWD: {   // in: de_out = dy [Nn, F], xh, rs, mods;  out or in/out (acc): de_prev = dx
        const int* row_mol = c.idx(a.row_mol, "row_mol", a.Nn, a.B);
        if (a.sc_off < 0 || (size_t)a.sc_off + D > (size_t)(a.ldm > 0 ? a.ldm : 0)) c.fail("a column offset of mods lies outside its row (ldm)");
        const float *dy = ARR(DE_OUT, Nn * D), *xh = ARR(XH, Nn * D), *rs = ARR(RS, Nn), *mods = ARR(MODS, B * (size_t)(a.ldm > 0 ? a.ldm : 0));
        float* dx = ARR(DE_PREV, Nn * D);
        RUN(fused_node_ln_mod_bwd(s, a.Nn, a.D, dy, xh, rs, row_mol, mods, a.ldm, a.sc_off, dx, a.acc ? 1 : 0));
    }
    case JODO_FT_ATTN_FWD:        // in: q, k (ldqk), v (ldv), t0 [R, QK], t1 [R, D], adj2d / adjsp [R] (XH >= 1 / 2);  out: alpha [R, H], hhat [Nn, D]
    case JODO_FT_ATTN_BWD: {      // in: dhhat, q, k, v, t0, t1, alpha;  out: dS [R, H], dt1, dt0, dq, dk (ldd_qk), dv (ldd_v)
        if (a.XH < 0 || a.XH > 2 || a.XH >= a.H || a.SC <= 0 || a.D % a.H != 0 || (long)(a.H - a.XH) * a.SC > a.D)
            return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): heads do not fit (H %d, XH %d, SC %d, D %d)", op, a.H, a.XH, a.SC, a.D);
        const int qk = (a.H - a.XH) * a.SC;
        if (!a.nn || !a.node_off || !a.edge_off || !a.node_mol) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): a topology array is a null pointer", op);
        if (a.node_off[0] != 0 || a.edge_off[0] != 0) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): node_off[0] / edge_off[0] is not 0", op);
        for (int b = 0; b < a.B; ++b) {
            const long n = a.nn[b];
            if (n < 1 || n > a.N) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): nn[%d] = %ld is out of range [1, N = %d]", op, b, n, a.N);
            if (a.node_off[b + 1] != a.node_off[b] + n || a.edge_off[b + 1] != a.edge_off[b] + n * n || a.node_off[b + 1] > a.Nn || a.edge_off[b + 1] > a.R)
                return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): node_off / edge_off of molecule %d are not consistent with nn (n %ld)", op, b, n);
            for (long i = a.node_off[b]; i < a.node_off[b + 1]; ++i)
                if (a.node_mol[i] != b) return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): node_mol[%ld] = %d is out of range: the row belongs to molecule %d", op, i, a.node_mol[i], b);
        }
        if (a.node_off[a.B] != a.Nn || a.edge_off[a.B] != a.R)
            return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused(%s): the offsets end at %d nodes / %d edge rows, the counts are Nn %d / R %d", op, a.node_off[a.B], a.edge_off[a.B], a.Nn, a.R);
        AttnTopo at{a.Nn, a.N, nullptr, nullptr, nullptr, nullptr, a.one_wave ? 1 : 0, a.ldqk, a.ldv, a.ldd_qk, a.ldd_v};
        at.node_mol = c.upload(a.node_mol, "node_mol", a.Nn); at.nn = c.upload(a.nn, "nn", a.B);
        at.node_off = c.upload(a.node_off, "node_off", a.B + 1); at.edge_off = c.upload(a.edge_off, "edge_off", a.B + 1);
        const float *q = c.strided(JODO_FT_Q, a.Nn, a.ldqk, qk), *k = c.strided(JODO_FT_K, a.Nn, a.ldqk, qk), *v = c.strided(JODO_FT_V, a.Nn, a.ldv, a.D);
        const float *t0 = ARR(T0, R * (size_t)qk), *t1 = ARR(T1, R * D);
        if (a.op == JODO_FT_ATTN_FWD) {
            const float *adj2d = a.XH >= 1 ? ARR(ADJ2D, R) : nullptr, *adjsp = a.XH >= 2 ? ARR(ADJSP, R) : nullptr;
            float *alpha = ARR(ALPHA, R * (size_t)a.H), *hhat = ARR(HHAT, Nn * D);
            RUN(fused_attn_fwd(s, at, a.D, a.H, a.XH, a.SC, a.inv_sqrt_c, q, k, t0, adj2d, adjsp, v, t1, alpha, hhat));
        }
        const float *dhhat = ARR(DHHAT, Nn * D), *alpha = ARR(ALPHA, R * (size_t)a.H);
        float *dS = ARR(DS, R * (size_t)a.H), *dt1 = ARR(DT1, R * D), *dt0 = ARR(DT0, R * (size_t)qk);
        float *dq = c.strided(JODO_FT_DQ, a.Nn, a.ldd_qk, qk), *dk = c.strided(JODO_FT_DK, a.Nn, a.ldd_qk, qk), *dv = c.strided(JODO_FT_DV, a.Nn, a.ldd_v, a.D);
        RUN(fused_attn_bwd(s, at, a.D, a.H, a.XH, a.SC, a.inv_sqrt_c, dhhat, q, k, v, t0, t1, alpha, dS, dt1, dt0, dq, dk, dv));
    }
    case JODO_FT_GBF_BWD: {       // in: d2 [R], gm [B, 2], gbf_means, gbf_stds [De - 1], dG (ldg, gcol);  out: dxp [R], dd2 [R] (optional; += with acc), part_m, part_s
        const int* row_mol = c.idx(a.edge_mol, "edge_mol", a.R, a.B);
        const float *d2 = ARR(D2, R), *gm = ARR(GM, B * 2), *means = ARR(GBF_MEANS, De - 1), *stds = ARR(GBF_STDS, De - 1);
        if (a.gcol < 0) c.fail("gcol is negative");
        const float* dG = c.strided(JODO_FT_DG, a.R, a.ldg, a.gcol + a.De);
        const size_t nch = (R + 31) / 32;
        float *dxp = ARR(DXP, R), *dd2 = c.arr_opt(JODO_FT_DD2, R), *pm = ARR(PART_M, nch * (De - 1)), *ps = ARR(PART_S, nch * (De - 1));
        RUN(fused_gbf_bwd(s, a.R, a.De, d2, row_mol, gm, means, stds, dG, a.ldg, a.gcol, dxp, dd2, a.acc ? 1 : 0, pm, ps));
    }
    }
#undef ARR
#undef RUN
    return jodo_set_error(JODO_ERR_ARG, "jodo_train_debug_fused: unknown op %d", a.op);
}

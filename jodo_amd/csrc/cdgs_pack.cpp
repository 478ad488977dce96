// jodo_cdgs_pack_weights_host: the state_dict of CDGS (334 tensors at 8 blocks, 260 at 6; names `all_modules.<i>...`) plus the caller's
// "time_freq" -> one fp32 blob + offset table (enum jodo_cdgs_wslot_global / jodo_cdgs_wslot_block, include/jodo_hip.h).  Host-only code.
//
// "Tiled" projections use the layout of csrc/dgt2d_pack.cpp: a matrix with `nb` output blocks of 32 logical rows and `nk` K chunks of 64
// columns is float [nb][nk][8 quads][64 lanes][4]; element (quad q, lane l, i) feeds k-step a = 4 q + i of the chunk: column = chunk * 64
// + (a / 16) * 32 + (l / 32) * 16 + a % 16, and MFMA row m = l % 32 is logical output position block * 32 + 16 ((m / 4) % 2) + 4 (m / 8)
// + m % 4.  Every tiled matrix here is given as a function (logical row, logical column) -> value, which is how the odd widths (77, 102,
// 51, 154, 85) are zero-padded and how the head inputs' columns are permuted to the kernels' row layout.
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"
#include "split_tape.h"

namespace {

struct Mat { const float* p; int64_t rows, cols; };

struct Packer {
    std::unordered_map<std::string, const jodo_tensor*> by_name;
    float* blob = nullptr;                     // NULL: size pass
    size_t pos = 0;
    int rc = JODO_OK;

    // a vector (cols < 0) or a matrix whose trailing dimensions beyond the second are 1 (conv 1x1 weights)
    Mat get(const std::string& name, int64_t rows, int64_t cols) {
        Mat s{nullptr, rows, cols < 0 ? 1 : cols};
        if (!blob) return s;
        auto it = by_name.find(name);
        if (it == by_name.end()) { if (!rc) rc = jodo_set_error(JODO_ERR_ARG, "pack_cdgs: missing tensor %s", name.c_str()); return s; }
        const jodo_tensor* t = it->second;
        bool ok = t->data != nullptr && t->ndim >= 1 && t->shape[0] == rows;
        if (cols < 0) ok = ok && t->ndim == 1;
        else ok = ok && t->ndim >= 2 && t->shape[1] == cols;
        for (int i = 2; ok && i < t->ndim; ++i) ok = t->shape[i] == 1;
        if (!ok) {
            if (!rc) rc = jodo_set_error(JODO_ERR_ARG, "pack_cdgs: tensor %s has %d dims (first %lld), expected [%lld%s%lld]", name.c_str(), t->ndim,
                                         (long long)(t->ndim ? t->shape[0] : 0), (long long)rows, cols < 0 ? "" : ", ", (long long)(cols < 0 ? 0 : cols));
            return s;
        }
        s.p = t->data;
        return s;
    }
    size_t begin() { pos = (pos + 63) / 64 * 64; return pos; }      // every slot 256-byte aligned
    void put(float v) { if (blob) blob[pos] = v; ++pos; }

    size_t plain(const Mat& s) {
        const size_t at = begin();
        for (int64_t i = 0; i < s.rows * s.cols; ++i) put(s.p ? s.p[i] : 0.f);
        return at;
    }
    size_t tiled(int rows, int K, const std::function<float(int, int)>& f) {
        const size_t at = begin();
        const int nb = (rows + 31) / 32, nk = (K + 63) / 64;
        if (!blob) { pos += (size_t)nb * nk * 2048; return at; }
        for (int b = 0; b < nb; ++b)
            for (int kc = 0; kc < nk; ++kc)
                for (int q = 0; q < 8; ++q)
                    for (int l = 0; l < 64; ++l)
                        for (int i = 0; i < 4; ++i) {
                            const int a = 4 * q + i, m = l % 32;
                            const int col = kc * 64 + (a / 16) * 32 + (l / 32) * 16 + a % 16;
                            const int row = b * 32 + 16 * ((m / 4) % 2) + 4 * (m / 8) + m % 4;
                            put(row < rows && col < K ? f(row, col) : 0.f);
                        }
        return at;
    }
    size_t vec(int rows, const std::function<float(int)>& f) {     // padded to a multiple of 32
        const size_t at = begin();
        const int n = (rows + 31) / 32 * 32;
        for (int i = 0; i < n; ++i) put(blob && i < rows ? f(i) : 0.f);
        return at;
    }
};

float at(const Mat& m, int64_t r, int64_t c) { return m.p && r < m.rows && c < m.cols ? m.p[r * m.cols + c] : 0.f; }

int run(const jodo_cdgs_cfg* c, Packer& P, int64_t* woff) {
    const int D = c->nf, L = c->n_layers, ach = c->atom_ch, ch = c->edge_ch, K = c->rw_depth;
    const int bse = (int)(D * 0.4), bt = (int)(0.5 * (D - bse)), ase = (int)(D * 0.2), att = D - 2 * ase;
    const int cat = 2 * D / L, catp = (cat + 31) / 32 * 32;
    const int KA = (L * catp + att + 63) / 64 * 64, KE = (L * catp + 192 + 63) / 64 * 64;
    auto nm = [](int i) { return "all_modules." + std::to_string(i); };
    auto W = [&](int i, int64_t r, int64_t k) { return P.get(nm(i) + ".weight", r, k); };
    auto Bv = [&](int i, int64_t r) { return P.get(nm(i) + ".bias", r, -1); };
    auto lin = [&](Mat w, int rows, int Kc) { return P.tiled(rows, Kc, [w](int r, int cc) { return at(w, r, cc); }); };
    auto bias = [&](Mat b, int rows) { return P.vec(rows, [b](int r) { return at(b, r, 0); }); };

    woff[JCG_FREQ] = (int64_t)P.plain(P.get("time_freq", D / 2, -1));
    woff[JCG_T1_W] = (int64_t)lin(W(0, 2 * D, D), 2 * D, D);
    woff[JCG_T1_B] = (int64_t)bias(Bv(0, 2 * D), 2 * D);
    woff[JCG_T2_W] = (int64_t)lin(W(1, D, 2 * D), D, 2 * D);
    woff[JCG_T2_B] = (int64_t)bias(Bv(1, D), D);
    {   // the time shifts of all blocks: per block [t_node (D) | t_edge (D)]
        std::vector<Mat> ws, bs;
        for (int l = 0; l < L; ++l) {
            const std::string pre = nm(10 + 3 * l) + ".";
            ws.push_back(P.get(pre + "t_node.weight", D, D)); ws.push_back(P.get(pre + "t_edge.weight", D, D));
            bs.push_back(P.get(pre + "t_node.bias", D, -1)); bs.push_back(P.get(pre + "t_edge.bias", D, -1));
        }
        woff[JCG_TMOD_W] = (int64_t)P.tiled(2 * L * D, D, [&ws, D](int r, int cc) { return at(ws[(size_t)(r / D)], r % D, cc); });
        woff[JCG_TMOD_B] = (int64_t)P.vec(2 * L * D, [&bs, D](int r) { return at(bs[(size_t)(r / D)], r % D, 0); });
    }
    woff[JCG_EC_W] = (int64_t)P.plain(W(2, bt, ch - 1));
    woff[JCG_EC_B] = (int64_t)P.plain(Bv(2, bt));
    woff[JCG_EX_W] = (int64_t)P.plain(W(3, bt, 1));
    woff[JCG_EX_B] = (int64_t)P.plain(Bv(3, bt));
    woff[JCG_SPD_W] = (int64_t)P.plain(W(4, bse, K + 1));
    woff[JCG_SPD_B] = (int64_t)P.plain(Bv(4, bse));
    woff[JCG_EEMB_W] = (int64_t)lin(W(5, D, D), D, D);
    woff[JCG_EEMB_B] = (int64_t)bias(Bv(5, D), D);
    woff[JCG_AD_W] = (int64_t)P.plain(W(6, ase, ch));
    woff[JCG_AD_B] = (int64_t)P.plain(Bv(6, ase));
    woff[JCG_AC_W] = (int64_t)P.plain(W(7, att, ach));
    woff[JCG_AC_B] = (int64_t)P.plain(Bv(7, att));
    woff[JCG_AR_W] = (int64_t)P.plain(W(8, ase, K));
    woff[JCG_AR_B] = (int64_t)P.plain(Bv(8, ase));
    woff[JCG_NEMB_W] = (int64_t)lin(W(9, D, D), D, D);
    woff[JCG_NEMB_B] = (int64_t)bias(Bv(9, D), D);

    const int h0 = 10 + 3 * L;
    {   // atom head: the reference's input is [atom_cate (att) | hids (L cat)]; the kernels' row is [hids (L catp) | atom_cate]
        Mat w1 = W(h0, D, att + L * cat);
        woff[JCG_AH1_W] = (int64_t)P.tiled(D, KA, [=](int r, int cc) {
            if (cc < L * catp) { const int l = cc / catp, k = cc % catp; return k < cat ? at(w1, r, att + l * cat + k) : 0.f; }
            const int k = cc - L * catp;
            return k < att ? at(w1, r, k) : 0.f;
        });
        woff[JCG_AH1_B] = (int64_t)bias(Bv(h0, D), D);
        woff[JCG_AH2_W] = (int64_t)lin(W(h0 + 1, D / 2, D), D / 2, D);
        woff[JCG_AH2_B] = (int64_t)bias(Bv(h0 + 1, D / 2), D / 2);
        woff[JCG_AH3_W] = (int64_t)lin(W(h0 + 2, ach, D / 2), 32, D / 2);
        woff[JCG_AH3_B] = (int64_t)bias(Bv(h0 + 2, ach), 32);
    }
    {   // edge heads stacked [exist ; type]: inputs [dense_exist | hids] and [dense_cate | hids]; the kernels' row is
        // [hids (L catp) | dense_cate (bt, at +0) | dense_exist (bt, at +96)]
        Mat wt1 = W(h0 + 3, D, bt + L * cat), we1 = W(h0 + 6, D, bt + L * cat);
        woff[JCG_EH1_W] = (int64_t)P.tiled(2 * D, KE, [=](int r, int cc) {
            const bool ex = r < D;
            const Mat& w = ex ? we1 : wt1;
            const int rr = ex ? r : r - D;
            if (cc < L * catp) { const int l = cc / catp, k = cc % catp; return k < cat ? at(w, rr, bt + l * cat + k) : 0.f; }
            const int k = cc - L * catp - (ex ? 96 : 0);
            return k >= 0 && k < bt ? at(w, rr, k) : 0.f;
        });
        Mat bt1 = Bv(h0 + 3, D), be1 = Bv(h0 + 6, D);
        woff[JCG_EH1_B] = (int64_t)P.vec(2 * D, [=](int r) { return r < D ? at(be1, r, 0) : at(bt1, r - D, 0); });
        Mat wt2 = W(h0 + 4, D / 2, D), we2 = W(h0 + 7, D / 2, D);
        woff[JCG_EH2_W] = (int64_t)P.tiled(D, 2 * D, [=](int r, int cc) {
            if (r < D / 2) return cc < D ? at(we2, r, cc) : 0.f;
            return cc >= D ? at(wt2, r - D / 2, cc - D) : 0.f;
        });
        Mat bt2 = Bv(h0 + 4, D / 2), be2 = Bv(h0 + 7, D / 2);
        woff[JCG_EH2_B] = (int64_t)P.vec(D, [=](int r) { return r < D / 2 ? at(be2, r, 0) : at(bt2, r - D / 2, 0); });
        Mat wt3 = W(h0 + 5, ch - 1, D / 2), we3 = W(h0 + 8, 1, D / 2);
        woff[JCG_EH3_W] = (int64_t)P.tiled(32, D, [=](int r, int cc) {
            if (r == 0) return cc < D / 2 ? at(we3, 0, cc) : 0.f;
            return r < ch && cc >= D / 2 ? at(wt3, r - 1, cc - D / 2) : 0.f;
        });
        Mat bt3 = Bv(h0 + 5, ch - 1), be3 = Bv(h0 + 8, 1);
        woff[JCG_EH3_B] = (int64_t)P.vec(32, [=](int r) { return r == 0 ? at(be3, 0, 0) : (r < ch ? at(bt3, r - 1, 0) : 0.f); });
    }
    for (int l = 0; l < L; ++l) {
        int64_t* wb = woff + JCG_GLOBAL_COUNT + (size_t)l * JCB_BLOCK_COUNT;
        const std::string pre = nm(10 + 3 * l) + ".", sa = pre + "self_attn.";
        auto Wn = [&](const std::string& n, int64_t r, int64_t k) { return P.get(pre + n + ".weight", r, k); };
        auto Bn = [&](const std::string& n, int64_t r) { return P.get(pre + n + ".bias", r, -1); };
        wb[JCB_EPS] = (int64_t)P.plain(P.get(pre + "local_model.eps", 1, -1));
        wb[JCB_GIN1_W] = (int64_t)lin(Wn("local_model.nn.0", D, D), D, D);
        wb[JCB_GIN1_B] = (int64_t)bias(Bn("local_model.nn.0", D), D);
        wb[JCB_GIN2_W] = (int64_t)lin(Wn("local_model.nn.2", D, D), D, D);
        wb[JCB_GIN2_B] = (int64_t)bias(Bn("local_model.nn.2", D), D);
        {
            Mat q = P.get(sa + "lin_query.weight", D, D), k = P.get(sa + "lin_key.weight", D, D), v = P.get(sa + "lin_value.weight", D, D);
            Mat qb = P.get(sa + "lin_query.bias", D, -1), kb = P.get(sa + "lin_key.bias", D, -1), vb = P.get(sa + "lin_value.bias", D, -1);
            wb[JCB_QKV_W] = (int64_t)P.tiled(3 * D, D, [=](int r, int cc) { return r < D ? at(q, r, cc) : (r < 2 * D ? at(k, r - D, cc) : at(v, r - 2 * D, cc)); });
            wb[JCB_QKV_B] = (int64_t)P.vec(3 * D, [=](int r) { return r < D ? at(qb, r, 0) : (r < 2 * D ? at(kb, r - D, 0) : at(vb, r - 2 * D, 0)); });
            Mat e0 = P.get(sa + "lin_edge0.weight", D, D), e1 = P.get(sa + "lin_edge1.weight", D, D);
            wb[JCB_E01_W] = (int64_t)P.tiled(2 * D, D, [=](int r, int cc) { return r < D ? at(e0, r, cc) : at(e1, r - D, cc); });
        }
        wb[JCB_NL_G] = (int64_t)P.plain(Wn("norm1_local", D, -1));
        wb[JCB_NL_B] = (int64_t)P.plain(Bn("norm1_local", D));
        wb[JCB_NA_G] = (int64_t)P.plain(Wn("norm1_attn", D, -1));
        wb[JCB_NA_B] = (int64_t)P.plain(Bn("norm1_attn", D));
        wb[JCB_FF1_W] = (int64_t)lin(Wn("ff_linear1", 2 * D, D), 2 * D, D);
        wb[JCB_FF1_B] = (int64_t)bias(Bn("ff_linear1", 2 * D), 2 * D);
        wb[JCB_FF2_W] = (int64_t)lin(Wn("ff_linear2", D, 2 * D), D, 2 * D);
        wb[JCB_FF2_B] = (int64_t)bias(Bn("ff_linear2", D), D);
        wb[JCB_NN_G] = (int64_t)P.plain(Wn("norm2_node", D, -1));
        wb[JCB_NN_B] = (int64_t)P.plain(Bn("norm2_node", D));
        wb[JCB_FF3_W] = (int64_t)lin(Wn("ff_linear3", 2 * D, D), 2 * D, D);
        wb[JCB_FF3_B] = (int64_t)bias(Bn("ff_linear3", 2 * D), 2 * D);
        wb[JCB_FF4_W] = (int64_t)lin(Wn("ff_linear4", D, 2 * D), D, 2 * D);
        wb[JCB_FF4_B] = (int64_t)bias(Bn("ff_linear4", D), D);
        wb[JCB_NE_G] = (int64_t)P.plain(Wn("norm2_edge", D, -1));
        wb[JCB_NE_B] = (int64_t)P.plain(Bn("norm2_edge", D));
        wb[JCB_RN_W] = (int64_t)lin(W(11 + 3 * l, cat, D), catp, D);
        wb[JCB_RN_B] = (int64_t)bias(Bv(11 + 3 * l, cat), catp);
        wb[JCB_RE_W] = (int64_t)lin(W(12 + 3 * l, cat, D), catp, D);
        wb[JCB_RE_B] = (int64_t)bias(Bv(12 + 3 * l, cat), catp);
    }
    P.begin();
    return P.rc;
}

}  // namespace

extern "C" int jodo_cdgs_check_cfg(const jodo_cdgs_cfg* c) {
    if (!c) return jodo_set_error(JODO_ERR_ARG, "cdgs: null configuration");
    if (c->nf != 256) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: nf=%d, the kernels are built for nf=256", c->nf);
    if (c->n_heads != 16) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: n_heads=%d, the kernels are built for 16", c->n_heads);
    if (c->n_layers < 1 || c->n_layers > 16) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: n_layers=%d outside [1, 16]", c->n_layers);
    if (c->atom_ch < 1 || c->atom_ch > 16) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: atom_types=%d outside [1, 16]", c->atom_ch);
    if (c->edge_ch < 2 || c->edge_ch > 3) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: edge_ch=%d, supported 2 and 3", c->edge_ch);
    if (c->rw_depth < 1 || c->rw_depth > 16) return jodo_set_error(JODO_ERR_UNSUPPORTED, "cdgs: rw_depth=%d outside [1, 16]", c->rw_depth);
    return JODO_OK;
}

extern "C" int jodo_cdgs_packed_size(const jodo_cdgs_cfg* cfg, size_t* n_floats, int* n_woff) {
    if (!n_floats || !n_woff) return jodo_set_error(JODO_ERR_ARG, "cdgs_packed_size: null argument");
    if (int rc = jodo_cdgs_check_cfg(cfg)) return rc;
    Packer P;
    std::vector<int64_t> woff((size_t)JCG_GLOBAL_COUNT + (size_t)cfg->n_layers * JCB_BLOCK_COUNT);
    run(cfg, P, woff.data());
    *n_floats = P.pos;
    *n_woff = (int)woff.size();
    return JODO_OK;
}

extern "C" int jodo_cdgs_pack_weights_host(const jodo_cdgs_cfg* cfg, const jodo_tensor* tensors, int n_tensors, float* packed_host,
                                           size_t capacity_floats, int64_t* woff, int n_woff) {
    if (!tensors || !packed_host || !woff) return jodo_set_error(JODO_ERR_ARG, "cdgs_pack_weights: null argument");
    size_t need = 0;
    int n_need = 0;
    if (int rc = jodo_cdgs_packed_size(cfg, &need, &n_need)) return rc;
    if (capacity_floats < need || n_woff != n_need)
        return jodo_set_error(JODO_ERR_ARG, "cdgs_pack_weights: buffer of %zu floats / %d slots, need %zu / %d", capacity_floats, n_woff, need, n_need);
    Packer P;
    for (int i = 0; i < n_tensors; ++i) {
        std::string name = tensors[i].name ? tensors[i].name : "";
        if (name.rfind("module.", 0) == 0) name = name.substr(7);
        P.by_name[name] = &tensors[i];
    }
    std::memset(packed_host, 0, need * sizeof(float));
    P.blob = packed_host;
    return run(cfg, P, woff);
}

// ---- split-bf16 ("bf16x3") weight tape of the row GEMMs over node rows and edge rows (opt-in form, csrc/cdgs_forward.hip kc_gemm_s) ----
// A function of the packed blob, exactly as the 2-D model's tape (csrc/dgt2d_pack.cpp): every covered tiled matrix float
// [nb][nk][8 quads][64 lanes][4] is re-read as bf16 [nb][nk * 4 K16 steps][3 terms: hi, mid, lo][64 lanes][8] by jd_tape::split_tiles
// (csrc/split_tape.h).  The three GEMMs over the B time-embedding rows (T1, T2, TMOD) stay exact fp32 and have no slot.
namespace {

struct SplitSlot { int slot, nb, nk; };                   // slot: index into the woff table

std::vector<SplitSlot> split_slots(const jodo_cdgs_cfg* c) {
    const int D = c->nf, L = c->n_layers, catp = (2 * D / L + 31) / 32 * 32;
    const int KA = (L * catp + (D - 2 * (int)(D * 0.2)) + 63) / 64 * 64, KE = (L * catp + 192 + 63) / 64 * 64;
    std::vector<SplitSlot> s;
    for (int l = 0; l < L; ++l) {
        const int at = JCG_GLOBAL_COUNT + l * JCB_BLOCK_COUNT;
        s.push_back({at + JCB_GIN1_W, D / 32, D / 64});
        s.push_back({at + JCB_GIN2_W, D / 32, D / 64});
        s.push_back({at + JCB_QKV_W, 3 * D / 32, D / 64});
        s.push_back({at + JCB_E01_W, 2 * D / 32, D / 64});
        s.push_back({at + JCB_FF1_W, 2 * D / 32, D / 64});
        s.push_back({at + JCB_FF2_W, D / 32, 2 * D / 64});
        s.push_back({at + JCB_FF3_W, 2 * D / 32, D / 64});
        s.push_back({at + JCB_FF4_W, D / 32, 2 * D / 64});
        s.push_back({at + JCB_RN_W, catp / 32, D / 64});
        s.push_back({at + JCB_RE_W, catp / 32, D / 64});
    }
    s.push_back({JCG_NEMB_W, D / 32, D / 64});
    s.push_back({JCG_EEMB_W, D / 32, D / 64});
    s.push_back({JCG_AH1_W, D / 32, KA / 64});
    s.push_back({JCG_AH2_W, D / 2 / 32, D / 64});
    s.push_back({JCG_AH3_W, 1, D / 2 / 64});
    s.push_back({JCG_EH1_W, 2 * D / 32, KE / 64});
    s.push_back({JCG_EH2_W, D / 32, 2 * D / 64});
    s.push_back({JCG_EH3_W, 1, D / 64});
    return s;
}

}  // namespace

extern "C" int jodo_cdgs_split_size(const jodo_cdgs_cfg* cfg, size_t* tape_bytes, int64_t* toff_out, int n_woff) {
    if (!tape_bytes || !toff_out) return jodo_set_error(JODO_ERR_ARG, "cdgs_split_size: null argument");
    if (int rc = jodo_cdgs_check_cfg(cfg)) return rc;
    const int want = JCG_GLOBAL_COUNT + cfg->n_layers * JCB_BLOCK_COUNT;
    if (n_woff != want) return jodo_set_error(JODO_ERR_ARG, "cdgs_split_size: offset table of %d slots, expected %d", n_woff, want);
    for (int i = 0; i < n_woff; ++i) toff_out[i] = -1;
    size_t at = 0;
    for (const SplitSlot& s : split_slots(cfg)) {
        toff_out[s.slot] = (int64_t)at;
        at += (size_t)s.nb * s.nk * jd_tape::TILE_BYTES;  // a multiple of 16 bytes: every slot stays 16-byte aligned
    }
    *tape_bytes = at;
    return JODO_OK;
}

extern "C" int jodo_cdgs_pack_split_host(const jodo_cdgs_cfg* cfg, const float* packed_host, const int64_t* woff, int n_woff, void* tape_host,
                                         size_t cap_bytes) {
    if (!packed_host || !woff || !tape_host) return jodo_set_error(JODO_ERR_ARG, "cdgs_pack_split: null argument");
    if (int rc = jodo_cdgs_check_cfg(cfg)) return rc;
    const int want = JCG_GLOBAL_COUNT + cfg->n_layers * JCB_BLOCK_COUNT;
    if (n_woff != want) return jodo_set_error(JODO_ERR_ARG, "cdgs_pack_split: offset table of %d slots, expected %d", n_woff, want);
    std::vector<int64_t> toff((size_t)n_woff);
    size_t need = 0;
    if (int rc = jodo_cdgs_split_size(cfg, &need, toff.data(), n_woff)) return rc;
    if (cap_bytes < need) return jodo_set_error(JODO_ERR_ARG, "cdgs_pack_split: buffer of %zu bytes, need %zu", cap_bytes, need);
    size_t blob_floats = 0;
    int nw = 0;
    if (int rc = jodo_cdgs_packed_size(cfg, &blob_floats, &nw)) return rc;
    for (const SplitSlot& s : split_slots(cfg)) {
        const size_t tiles = (size_t)s.nb * s.nk;
        if (woff[s.slot] < 0 || (size_t)woff[s.slot] + tiles * jd_tape::TILE_FLOATS > blob_floats)
            return jodo_set_error(JODO_ERR_ARG, "cdgs_pack_split: weight offset of slot %d outside the packed blob", s.slot);
        jd_tape::split_tiles(packed_host + woff[s.slot], tiles, reinterpret_cast<uint16_t*>(static_cast<char*>(tape_host) + toff[(size_t)s.slot]));
    }
    return JODO_OK;
}

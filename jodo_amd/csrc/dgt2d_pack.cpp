// jodo_dgt2d_pack_weights_host: the state_dict of DGT_concat_2D (235 tensors at L = 8) -> one fp32 blob + offset table
// (enum jodo2d_wslot_global / jodo2d_wslot_block, include/jodo_hip.h).  Host-only code.
//
// "Tiled" projections (everything that runs on v_mfma_f32_32x32x2_f32, transposed orientation D[out, item] += W[out, k] X[k, item],
// weights as A operand): a matrix with `nb` output blocks of 32 logical rows and `nk` K chunks of 64 columns is
//     float [nb][nk][8 quads][64 lanes][4]
// where element (quad q, lane l, i) feeds k-step a = 4 q + i of the chunk: column = chunk * 64 + (a / 16) * 32 + (l / 32) * 16 + a % 16
// (the "natural-half" register order of csrc/dgt_device.h), and MFMA row m = l % 32 is the accumulator register s = 4 (m / 8) + m % 4
// of half-lane h = (m / 4) % 2, i.e. logical output position block * 32 + 16 h + s.  A row map then says which row of the source
// matrix a logical position holds (-1 = zero).  Biases are plain vectors in logical position order.
//
// Row maps of the attention projections (15 learned heads of 17 channels + 1 adjacency head):
//   q / k / lin_edge0 "slot" order: a lane half owns 128 slots; slots 17 g .. 17 g + 16 (g = 0..6) are the 17 channels of learned head
//   g (half 0) or 8 + g (half 1); slots 119..127 are channels 0..8 (half 0) / 9..16 (half 1, slot 127 is padding) of learned head 7.
//   Both halves therefore share one compile-time segment structure, and only head 7 needs a cross-half sum.
//   q and k live in memory as [half][128]; lin_edge0's block b holds slots 16 b .. 16 b + 15 of both halves.
//   lin_edge1: block b, half h = the 16 value channels of attention head 8 h + b (0 = the adjacency head).
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"
#include "split_tape.h"

namespace {

struct Src { const float* p; int64_t rows, cols; };

int slot_feature(int half, int t) {            // learned-head feature (0..254) of slot t of a lane half, -1 = padding
    if (t < 119) return (half ? 136 : 0) + t;
    if (half == 0) return t;                   // 119..127: head 7 channels 0..8
    return t < 127 ? 128 + (t - 119) : -1;     // head 7 channels 9..16
}

struct Packer {
    std::unordered_map<std::string, const jodo_tensor*> by_name;
    std::vector<float>* blob;                  // NULL: size pass
    size_t pos = 0;
    int rc = JODO_OK;

    Src get(const std::string& name, int64_t rows, int64_t cols) {
        Src s{nullptr, rows, cols};
        if (!blob) return s;
        auto it = by_name.find(name);
        if (it == by_name.end()) { if (!rc) rc = jodo_set_error(JODO_ERR_ARG, "pack2d: missing tensor %s", name.c_str()); return s; }
        const jodo_tensor* t = it->second;
        int64_t n = 1;
        for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
        const bool ok = cols < 0 ? (t->ndim == 1 && t->shape[0] == rows) : (t->ndim == 2 && t->shape[0] == rows && t->shape[1] == cols);
        if (!ok || !t->data) {
            if (!rc) rc = jodo_set_error(JODO_ERR_ARG, "pack2d: tensor %s has %lld elements in %d dims, expected [%lld%s%lld]", name.c_str(),
                                         (long long)n, t->ndim, (long long)rows, cols < 0 ? "" : ", ", (long long)(cols < 0 ? 0 : cols));
            return s;
        }
        s.p = t->data;
        return s;
    }
    size_t begin() { pos = (pos + 63) / 64 * 64; return pos; }      // every slot 256-byte aligned
    void put(float v) { if (blob) (*blob)[pos] = v; ++pos; }

    // plain copy of a vector / row-major matrix
    size_t plain(const std::string& name, int64_t rows, int64_t cols) {
        const size_t at = begin();
        Src s = get(name, rows, cols);
        const int64_t n = rows * (cols < 0 ? 1 : cols);
        for (int64_t i = 0; i < n; ++i) put(s.p ? s.p[i] : 0.f);
        return at;
    }
    // rows of several stacked sources seen as one matrix [sum rows, K]; rowmap[logical position] = stacked row or -1
    size_t tiled(const std::vector<Src>& srcs, int K, const std::vector<int>& rowmap) {
        const size_t at = begin();
        const int nb = (int)rowmap.size() / 32, nk = (K + 63) / 64;
        if (!blob) { pos += (size_t)nb * nk * 2048; return at; }      // size pass
        for (int b = 0; b < nb; ++b)
            for (int kc = 0; kc < nk; ++kc)
                for (int q = 0; q < 8; ++q)
                    for (int l = 0; l < 64; ++l)
                        for (int i = 0; i < 4; ++i) {
                            const int a = 4 * q + i, m = l % 32;
                            const int col = kc * 64 + (a / 16) * 32 + (l / 32) * 16 + a % 16;
                            const int row = rowmap[(size_t)b * 32 + 16 * ((m / 4) % 2) + 4 * (m / 8) + m % 4];
                            float v = 0.f;
                            if (row >= 0 && col < K) {
                                int64_t r = row;
                                for (const Src& s : srcs) {
                                    if (r < s.rows) { if (s.p) v = s.p[r * s.cols + col]; break; }
                                    r -= s.rows;
                                }
                            }
                            put(v);
                        }
        return at;
    }
    size_t bias(const std::vector<Src>& srcs, const std::vector<int>& rowmap) {
        const size_t at = begin();
        for (int row : rowmap) {
            float v = 0.f;
            int64_t r = row;
            if (row >= 0)
                for (const Src& s : srcs) {
                    if (r < s.rows) { if (s.p) v = s.p[r]; break; }
                    r -= s.rows;
                }
            put(v);
        }
        return at;
    }
};

std::vector<int> ident(int n, int valid = -1) {
    std::vector<int> m((size_t)(n + 31) / 32 * 32, -1);
    for (int i = 0; i < (valid < 0 ? n : valid); ++i) m[(size_t)i] = i;
    return m;
}

int check_cfg(const jodo_cfg2d* c) {
    if (!c) return jodo_set_error(JODO_ERR_ARG, "dgt2d: null configuration");
    if (c->nf != 256) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: nf=%d, the 2-D kernels are built for nf=256", c->nf);
    if (c->n_heads != 16 || c->n_extra != 1)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: n_heads=%d n_extra_heads=%d, the 2-D kernels are built for 16/1", c->n_heads, c->n_extra);
    if (c->mlp_ratio != 2) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: mlp_ratio=%d, supported 2", c->mlp_ratio);
    if (c->n_layers != 8) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: n_layers=%d, supported 8", c->n_layers);
    if (c->in_node_dim < 1 || c->in_node_dim > 16) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: in_node_dim=%d outside [1, 16]", c->in_node_dim);
    if (c->edge_ch < 2 || c->edge_ch > 3) return jodo_set_error(JODO_ERR_UNSUPPORTED, "dgt2d: edge_ch=%d, supported 2 and 3", c->edge_ch);
    return JODO_OK;
}

int run(const jodo_cfg2d* c, Packer& P, int64_t* woff) {
    const int D = c->nf, De = D / 4, T = 4 * D, L = c->n_layers, nd = c->in_node_dim, ch = c->edge_ch;
    const int cn = 2 * D / L, ce = 2 * De / L;
    auto W = [&](const std::string& n, int64_t r, int64_t k) { return P.get(n + ".weight", r, k); };
    auto Bv = [&](const std::string& n, int64_t r) { return P.get(n + ".bias", r, -1); };
    woff[J2_TIME_FREQ] = (int64_t)P.plain("time_mlp.0.weights", 8, -1);
    woff[J2_TIME_W1] = (int64_t)P.plain("time_mlp.1.weight", T, 17);
    woff[J2_TIME_B1] = (int64_t)P.plain("time_mlp.1.bias", T, -1);
    woff[J2_TIME_W3] = (int64_t)P.tiled({W("time_mlp.3", T, T)}, T, ident(T));
    woff[J2_TIME_B3] = (int64_t)P.bias({Bv("time_mlp.3", T)}, ident(T));
    {   // modulation rows of all blocks: per block [node_time_mlp.1 (6 D) | edge_time_mlp.1 (6 De)]
        std::vector<Src> ws, bs;
        for (int l = 0; l < L; ++l) {
            const std::string pre = "e_block_" + std::to_string(l) + ".";
            ws.push_back(W(pre + "node_time_mlp.1", 6 * D, T)); ws.push_back(W(pre + "edge_time_mlp.1", 6 * De, T));
            bs.push_back(Bv(pre + "node_time_mlp.1", 6 * D)); bs.push_back(Bv(pre + "edge_time_mlp.1", 6 * De));
        }
        woff[J2_MOD_W] = (int64_t)P.tiled(ws, T, ident(L * 6 * (D + De)));
        woff[J2_MOD_B] = (int64_t)P.bias(bs, ident(L * 6 * (D + De)));
    }
    woff[J2_NODE_EMB_W] = (int64_t)P.plain("node_emb.weight", D, 2 * nd);
    woff[J2_NODE_EMB_B] = (int64_t)P.plain("node_emb.bias", D, -1);
    woff[J2_EDGE_EMB_W] = (int64_t)P.plain("edge_emb.weight", De, 2 * ch);
    woff[J2_EDGE_EMB_B] = (int64_t)P.plain("edge_emb.bias", De, -1);
    const int KN = D + L * cn, KE = De + L * ce;
    woff[J2_NH1_W] = (int64_t)P.tiled({W("node_pred_mlp.0", D, KN)}, KN, ident(D));
    woff[J2_NH1_B] = (int64_t)P.bias({Bv("node_pred_mlp.0", D)}, ident(D));
    woff[J2_NH2_W] = (int64_t)P.tiled({W("node_pred_mlp.2", D / 2, D)}, D, ident(D / 2));
    woff[J2_NH2_B] = (int64_t)P.bias({Bv("node_pred_mlp.2", D / 2)}, ident(D / 2));
    woff[J2_NH3_W] = (int64_t)P.tiled({W("node_pred_mlp.4", nd, D / 2)}, D / 2, ident(32, nd));
    woff[J2_NH3_B] = (int64_t)P.bias({Bv("node_pred_mlp.4", nd)}, ident(32, nd));
    // edge heads: first layers stacked [exist ; type] (2 De rows), second layers as two De / 2-row blocks, last layers plain
    woff[J2_EH1_W] = (int64_t)P.tiled({W("edge_exist_mlp.0", De, KE), W("edge_type_mlp.0", De, KE)}, KE, ident(2 * De));
    woff[J2_EH1_B] = (int64_t)P.bias({Bv("edge_exist_mlp.0", De), Bv("edge_type_mlp.0", De)}, ident(2 * De));
    woff[J2_EH2_W] = (int64_t)P.tiled({W("edge_exist_mlp.2", De / 2, De)}, De, ident(De / 2));
    P.tiled({W("edge_type_mlp.2", De / 2, De)}, De, ident(De / 2));
    woff[J2_EH2_B] = (int64_t)P.bias({Bv("edge_exist_mlp.2", De / 2), Bv("edge_type_mlp.2", De / 2)}, ident(De));
    woff[J2_EH3_W] = (int64_t)P.plain("edge_exist_mlp.4.weight", 1, De / 2);
    {   // directly behind: the type rows, then the biases [exist, type...] (kept unaligned on purpose: one contiguous group)
        Src s = W("edge_type_mlp.4", ch - 1, De / 2);
        for (int i = 0; i < (ch - 1) * (De / 2); ++i) P.put(s.p ? s.p[i] : 0.f);
    }
    woff[J2_EH3_B] = (int64_t)P.plain("edge_exist_mlp.4.bias", 1, -1);
    {
        Src s = Bv("edge_type_mlp.4", ch - 1);
        for (int i = 0; i < ch - 1; ++i) P.put(s.p ? s.p[i] : 0.f);
    }
    // slot-order row maps
    std::vector<int> qkv((size_t)3 * D, -1), le((size_t)2 * D, -1);
    for (int half = 0; half < 2; ++half)
        for (int t = 0; t < 128; ++t) {
            const int f = slot_feature(half, t);
            qkv[(size_t)half * 128 + t] = f;                               // lin_query rows (stack offset 0)
            qkv[(size_t)D + half * 128 + t] = f < 0 ? -1 : 255 + f;        // lin_key rows (stacked behind the 255 query rows)
            le[(size_t)(t / 16) * 32 + half * 16 + t % 16] = f;            // lin_edge0: block t / 16, half, register t % 16
        }
    for (int i = 0; i < D; ++i) qkv[(size_t)2 * D + i] = 510 + i;          // lin_value in natural order
    for (int b = 0; b < 8; ++b)
        for (int h = 0; h < 2; ++h)
            for (int s = 0; s < 16; ++s) le[(size_t)D + b * 32 + h * 16 + s] = 255 + (8 * h + b) * 16 + s;    // lin_edge1 behind lin_edge0
    for (int l = 0; l < L; ++l) {
        int64_t* wb = woff + J2_GLOBAL_COUNT + (size_t)l * J2B_BLOCK_COUNT;
        const std::string pre = "e_block_" + std::to_string(l) + ".", at = pre + "attn_mpnn.";
        wb[J2B_QKV_W] = (int64_t)P.tiled({W(at + "lin_query", 255, D), W(at + "lin_key", 255, D), W(at + "lin_value", D, D)}, D, qkv);
        wb[J2B_QKV_B] = (int64_t)P.bias({Bv(at + "lin_query", 255), Bv(at + "lin_key", 255), Bv(at + "lin_value", D)}, qkv);
        wb[J2B_LE_W] = (int64_t)P.tiled({W(at + "lin_edge0", 255, De), W(at + "lin_edge1", D, De)}, De, le);
        wb[J2B_N2E_W] = (int64_t)P.tiled({W(pre + "node2edge_lin", De, D)}, D, ident(De));
        wb[J2B_N2E_B] = (int64_t)P.bias({Bv(pre + "node2edge_lin", De)}, ident(De));
        wb[J2B_FF1_W] = (int64_t)P.tiled({W(pre + "ff_linear1", 2 * D, D)}, D, ident(2 * D));
        wb[J2B_FF1_B] = (int64_t)P.bias({Bv(pre + "ff_linear1", 2 * D)}, ident(2 * D));
        wb[J2B_FF2_W] = (int64_t)P.tiled({W(pre + "ff_linear2", D, 2 * D)}, 2 * D, ident(D));
        wb[J2B_FF2_B] = (int64_t)P.bias({Bv(pre + "ff_linear2", D)}, ident(D));
        wb[J2B_FF3_W] = (int64_t)P.tiled({W(pre + "ff_linear3", 2 * De, De)}, De, ident(2 * De));
        wb[J2B_FF3_B] = (int64_t)P.bias({Bv(pre + "ff_linear3", 2 * De)}, ident(2 * De));
        wb[J2B_FF4_W] = (int64_t)P.tiled({W(pre + "ff_linear4", De, 2 * De)}, 2 * De, ident(De));
        wb[J2B_FF4_B] = (int64_t)P.bias({Bv(pre + "ff_linear4", De)}, ident(De));
        wb[J2B_NRO_W] = (int64_t)P.tiled({W("node_" + std::to_string(l), cn, D)}, D, ident(cn));
        wb[J2B_NRO_B] = (int64_t)P.bias({Bv("node_" + std::to_string(l), cn)}, ident(cn));
        wb[J2B_ERO_W] = (int64_t)P.tiled({W("edge_" + std::to_string(l), ce, De)}, De, ident(32, ce));
        wb[J2B_ERO_B] = (int64_t)P.bias({Bv("edge_" + std::to_string(l), ce)}, ident(32, ce));
    }
    P.begin();
    return P.rc;
}

}  // namespace

extern "C" int jodo_dgt2d_check_cfg(const jodo_cfg2d* cfg) { return check_cfg(cfg); }

extern "C" int jodo_dgt2d_packed_size(const jodo_cfg2d* cfg, size_t* n_floats, int* n_woff) {
    if (!n_floats || !n_woff) return jodo_set_error(JODO_ERR_ARG, "dgt2d_packed_size: null argument");
    if (int rc = check_cfg(cfg)) return rc;
    Packer P;
    P.blob = nullptr;
    std::vector<int64_t> woff((size_t)J2_GLOBAL_COUNT + (size_t)cfg->n_layers * J2B_BLOCK_COUNT);
    if (int rc = run(cfg, P, woff.data())) return rc;
    *n_floats = P.pos;
    *n_woff = (int)woff.size();
    return JODO_OK;
}

extern "C" int jodo_dgt2d_pack_weights_host(const jodo_cfg2d* cfg, const jodo_tensor* tensors, int n_tensors, float* packed_host,
                                            size_t cap_floats, int64_t* woff_out, int n_woff) {
    if (!tensors || !packed_host || !woff_out) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pack_weights: null argument");
    size_t need = 0;
    int nw = 0;
    if (int rc = jodo_dgt2d_packed_size(cfg, &need, &nw)) return rc;
    if (cap_floats < need || n_woff != nw)
        return jodo_set_error(JODO_ERR_ARG, "dgt2d_pack_weights: buffer of %zu floats / %d slots, need %zu / %d", cap_floats, n_woff, need, nw);
    Packer P;
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pack_weights: tensor %d has no name", i);
        std::string n(tensors[i].name);
        if (n.rfind("module.", 0) == 0) n = n.substr(7);
        P.by_name[n] = &tensors[i];
    }
    std::vector<float> blob(need, 0.f);
    P.blob = &blob;
    if (int rc = run(cfg, P, woff_out)) return rc;
    std::memcpy(packed_host, blob.data(), need * sizeof(float));
    return JODO_OK;
}

// ---- split-bf16 ("bf16x3") weight tape of the node GEMMs and the pair update (opt-in form, csrc/dgt2d_forward.hip) --------------------------------------
// A function of the packed blob: every covered tiled matrix float [nb][nk][8 quads][64 lanes][4] is re-read as
//     bf16 [nb][nk * 4 K16 steps][3 terms: hi, mid, lo][64 lanes][8]
// by jd_tape::split_tiles (csrc/split_tape.h, shared with the CDGS tape), so row maps and slot order have no second implementation.
namespace {

struct SplitSlot { int slot, nb, nk; };                   // slot: index into the woff table

std::vector<SplitSlot> split_slots(const jodo_cfg2d* c) {
    const int D = c->nf, De = D / 4, L = c->n_layers, cn = 2 * D / L, KN = D + L * cn;
    std::vector<SplitSlot> s;
    for (int l = 0; l < L; ++l) {
        const int at = J2_GLOBAL_COUNT + l * J2B_BLOCK_COUNT;
        s.push_back({at + J2B_QKV_W, 3 * D / 32, D / 64});
        s.push_back({at + J2B_N2E_W, De / 32, D / 64});
        s.push_back({at + J2B_FF1_W, 2 * D / 32, D / 64});
        s.push_back({at + J2B_FF2_W, D / 32, 2 * D / 64});
        s.push_back({at + J2B_NRO_W, (cn + 31) / 32, D / 64});
        s.push_back({at + J2B_FF3_W, 2 * De / 32, De / 64});
        s.push_back({at + J2B_FF4_W, De / 32, 2 * De / 64});
        s.push_back({at + J2B_ERO_W, 1, De / 64});
    }
    s.push_back({J2_NH1_W, D / 32, (KN + 63) / 64});
    s.push_back({J2_NH2_W, D / 2 / 32, D / 64});
    s.push_back({J2_NH3_W, 1, D / 2 / 64});
    return s;
}

}  // namespace

extern "C" int jodo_dgt2d_split_size(const jodo_cfg2d* cfg, size_t* tape_bytes, int64_t* toff_out, int n_woff) {
    if (!tape_bytes || !toff_out) return jodo_set_error(JODO_ERR_ARG, "dgt2d_split_size: null argument");
    if (int rc = check_cfg(cfg)) return rc;
    const int want = J2_GLOBAL_COUNT + cfg->n_layers * J2B_BLOCK_COUNT;
    if (n_woff != want) return jodo_set_error(JODO_ERR_ARG, "dgt2d_split_size: offset table of %d slots, expected %d", n_woff, want);
    for (int i = 0; i < n_woff; ++i) toff_out[i] = -1;
    size_t at = 0;
    for (const SplitSlot& s : split_slots(cfg)) {
        toff_out[s.slot] = (int64_t)at;
        at += (size_t)s.nb * s.nk * 4 * 3072;             // a multiple of 16 bytes: every slot stays 16-byte aligned
    }
    *tape_bytes = at;
    return JODO_OK;
}

extern "C" int jodo_dgt2d_pack_split_host(const jodo_cfg2d* cfg, const float* packed_host, const int64_t* woff, int n_woff, void* tape_host,
                                          size_t cap_bytes) {
    if (!packed_host || !woff || !tape_host) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pack_split: null argument");
    if (int rc = check_cfg(cfg)) return rc;
    const int want = J2_GLOBAL_COUNT + cfg->n_layers * J2B_BLOCK_COUNT;
    if (n_woff != want) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pack_split: offset table of %d slots, expected %d", n_woff, want);
    std::vector<int64_t> toff((size_t)n_woff);
    size_t need = 0;
    if (int rc = jodo_dgt2d_split_size(cfg, &need, toff.data(), n_woff)) return rc;
    if (cap_bytes < need) return jodo_set_error(JODO_ERR_ARG, "dgt2d_pack_split: buffer of %zu bytes, need %zu", cap_bytes, need);
    size_t blob_floats = 0;
    int nw = 0;
    if (int rc = jodo_dgt2d_packed_size(cfg, &blob_floats, &nw)) return rc;
    for (const SplitSlot& s : split_slots(cfg)) {
        const size_t tiles = (size_t)s.nb * s.nk;
        if (woff[s.slot] < 0 || (size_t)woff[s.slot] + tiles * 2048 > blob_floats)
            return jodo_set_error(JODO_ERR_ARG, "dgt2d_pack_split: weight offset of slot %d outside the packed blob", s.slot);
        jd_tape::split_tiles(packed_host + woff[s.slot], tiles, reinterpret_cast<uint16_t*>(static_cast<char*>(tape_host) + toff[(size_t)s.slot]));
    }
    return JODO_OK;
}

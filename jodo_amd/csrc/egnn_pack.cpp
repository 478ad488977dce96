// jodo_egnn_pack_weights_host: the state_dict of the property classifier (EGNN of cond_gen/model.py, 80 tensors at 7 layers with
// attention) -> one fp32 blob + offset table (enum jodo_egnn_wslot_global / jodo_egnn_wslot_layer, include/jodo_hip.h).  Host-only code.
//
// "Tiled" projections are laid out as in csrc/dgt2d_pack.cpp: a matrix with `nb` output blocks of 32 rows and `nk` K chunks of 64
// columns is float [nb][nk][8 quads][64 lanes][4]; element (quad q, lane l, i) feeds k-step a = 4 q + i of the chunk: column =
// chunk * 64 + (a / 16) * 32 + (l / 32) * 16 + a % 16, and MFMA row m = l % 32 is output position block * 32 + 16 ((m / 4) % 2) +
// 4 (m / 8) + m % 4.  All row maps are the identity here; a source is a column window of a stored matrix (edge_mlp.0 = [W_src | W_tgt |
// w_r], node_mlp.0 = [W_h | W_agg | W_attr]).  Biases and the two row vectors (radial column, attention row) are plain vectors.
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/jodo_hip.h"
#include "jodo_hip_internal.h"

namespace {

struct Src { const float* p; int64_t rows, ld, col0, cols; };      // rows x cols window starting at column col0 of a [rows, ld] matrix

struct Packer {
    std::unordered_map<std::string, const jodo_tensor*> by_name;
    std::vector<float>* blob;                  // NULL: size pass
    size_t pos = 0;
    int rc = JODO_OK;

    // the whole tensor `name`, expected [rows, cols] (cols < 0: a vector of `rows`)
    const float* get(const std::string& name, int64_t rows, int64_t cols) {
        if (!blob) return nullptr;
        auto it = by_name.find(name);
        if (it == by_name.end()) { if (!rc) rc = jodo_set_error(JODO_ERR_ARG, "egnn_pack: missing tensor %s", name.c_str()); return nullptr; }
        const jodo_tensor* t = it->second;
        const bool ok = cols < 0 ? (t->ndim == 1 && t->shape[0] == rows) : (t->ndim == 2 && t->shape[0] == rows && t->shape[1] == cols);
        if (!ok || !t->data) {
            if (!rc) rc = jodo_set_error(JODO_ERR_ARG, "egnn_pack: tensor %s has %d dims (first %lld), expected [%lld%s%lld]", name.c_str(), t->ndim,
                                         (long long)(t->ndim > 0 ? t->shape[0] : 0), (long long)rows, cols < 0 ? "" : ", ", (long long)(cols < 0 ? 0 : cols));
            return nullptr;
        }
        return t->data;
    }
    size_t begin() { pos = (pos + 63) / 64 * 64; return pos; }      // every slot 256-byte aligned
    void put(float v) { if (blob) (*blob)[pos] = v; ++pos; }

    // sources stacked by rows, all with K columns; output rows padded to blocks of 32, K to chunks of 64, both with zeros
    size_t tiled(const std::vector<Src>& srcs, int K) {
        const size_t at = begin();
        int64_t rows = 0;
        for (const Src& s : srcs) rows += s.rows;
        const int nb = (int)((rows + 31) / 32), nk = (K + 63) / 64;
        if (!blob) { pos += (size_t)nb * nk * 2048; return at; }
        for (int b = 0; b < nb; ++b)
            for (int kc = 0; kc < nk; ++kc)
                for (int q = 0; q < 8; ++q)
                    for (int l = 0; l < 64; ++l)
                        for (int i = 0; i < 4; ++i) {
                            const int a = 4 * q + i, m = l % 32;
                            const int col = kc * 64 + (a / 16) * 32 + (l / 32) * 16 + a % 16;
                            int64_t r = (int64_t)b * 32 + 16 * ((m / 4) % 2) + 4 * (m / 8) + m % 4;
                            float v = 0.f;
                            if (r < rows && col < K)
                                for (const Src& s : srcs) {
                                    if (r < s.rows) { if (s.p) v = s.p[r * s.ld + s.col0 + col]; break; }
                                    r -= s.rows;
                                }
                            put(v);
                        }
        return at;
    }
    // n values: the first `len` from p (stride `stride`), zeros behind
    size_t vec(const float* p, int64_t len, int64_t stride, int64_t n) {
        const size_t at = begin();
        for (int64_t i = 0; i < n; ++i) put(p && i < len ? p[i * stride] : 0.f);
        return at;
    }
};

int check_cfg(const jodo_egnn_cfg* c) {
    if (!c) return jodo_set_error(JODO_ERR_ARG, "egnn: null configuration");
    if (c->hidden_nf < 64 || c->hidden_nf > 256 || c->hidden_nf % 64)
        return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: hidden_nf=%d, supported: multiples of 64 in [64, 256]", c->hidden_nf);
    if (c->n_layers < 1 || c->n_layers > 16) return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: n_layers=%d outside [1, 16]", c->n_layers);
    if (c->in_node_nf < 1 || c->in_node_nf > 16) return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: in_node_nf=%d outside [1, 16]", c->in_node_nf);
    if (c->attention != 0 && c->attention != 1) return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: attention=%d, supported 0 and 1", c->attention);
    if (c->node_attr != 0 && c->node_attr != 1) return jodo_set_error(JODO_ERR_UNSUPPORTED, "egnn: node_attr=%d, supported 0 and 1", c->node_attr);
    return JODO_OK;
}

int run(const jodo_egnn_cfg* c, Packer& P, int64_t* woff) {
    const int nf = c->hidden_nf, in = c->in_node_nf, L = c->n_layers;
    auto full = [&](const std::string& n, int64_t r, int64_t k) { return Src{P.get(n + ".weight", r, k), r, k, 0, k}; };
    auto bias = [&](const std::string& n, int64_t r) { return P.vec(P.get(n + ".bias", r, -1), r, 1, (r + 31) / 32 * 32); };
    woff[JE_EMB_W] = (int64_t)P.tiled({full("embedding", nf, in)}, in);
    woff[JE_EMB_B] = (int64_t)bias("embedding", nf);
    woff[JE_ND0_W] = (int64_t)P.tiled({full("node_dec.0", nf, nf)}, nf);
    woff[JE_ND0_B] = (int64_t)bias("node_dec.0", nf);
    woff[JE_ND2_W] = (int64_t)P.tiled({full("node_dec.2", nf, nf)}, nf);
    woff[JE_ND2_B] = (int64_t)bias("node_dec.2", nf);
    woff[JE_GD0_W] = (int64_t)P.tiled({full("graph_dec.0", nf, nf)}, nf);
    woff[JE_GD0_B] = (int64_t)bias("graph_dec.0", nf);
    woff[JE_GD2_W] = (int64_t)P.vec(P.get("graph_dec.2.weight", 1, nf), nf, 1, nf);
    woff[JE_GD2_B] = (int64_t)P.vec(P.get("graph_dec.2.bias", 1, -1), 1, 1, 1);
    for (int l = 0; l < L; ++l) {
        int64_t* wl = woff + JE_GLOBAL_COUNT + (size_t)l * JEL_LAYER_COUNT;
        const std::string pre = "gcl_" + std::to_string(l) + ".";
        const float* w1 = P.get(pre + "edge_mlp.0.weight", nf, 2 * nf + 1);
        wl[JEL_P_W] = (int64_t)P.tiled({Src{w1, nf, 2 * nf + 1, 0, nf}, Src{w1, nf, 2 * nf + 1, nf, nf}}, nf);
        wl[JEL_P_B] = (int64_t)P.vec(P.get(pre + "edge_mlp.0.bias", nf, -1), nf, 1, 2 * nf);
        wl[JEL_WR] = (int64_t)P.vec(w1 ? w1 + 2 * nf : nullptr, nf, 2 * nf + 1, nf);
        wl[JEL_W2] = (int64_t)P.tiled({full(pre + "edge_mlp.2", nf, nf)}, nf);
        wl[JEL_B2] = (int64_t)bias(pre + "edge_mlp.2", nf);
        if (c->attention) {
            wl[JEL_ATT_W] = (int64_t)P.vec(P.get(pre + "att_mlp.0.weight", 1, nf), nf, 1, nf);
            wl[JEL_ATT_B] = (int64_t)P.vec(P.get(pre + "att_mlp.0.bias", 1, -1), 1, 1, 1);
        } else {
            wl[JEL_ATT_W] = wl[JEL_ATT_B] = -1;
        }
        const int KN = 2 * nf + (c->node_attr ? in : 0);
        wl[JEL_N0_W] = (int64_t)P.tiled({full(pre + "node_mlp.0", nf, KN)}, KN);
        wl[JEL_N0_B] = (int64_t)bias(pre + "node_mlp.0", nf);
        wl[JEL_N2_W] = (int64_t)P.tiled({full(pre + "node_mlp.2", nf, nf)}, nf);
        wl[JEL_N2_B] = (int64_t)bias(pre + "node_mlp.2", nf);
    }
    P.begin();
    return P.rc;
}

}  // namespace

extern "C" int jodo_egnn_check_cfg(const jodo_egnn_cfg* cfg) { return check_cfg(cfg); }

extern "C" int jodo_egnn_packed_size(const jodo_egnn_cfg* cfg, size_t* n_floats, int* n_woff) {
    if (!n_floats || !n_woff) return jodo_set_error(JODO_ERR_ARG, "egnn_packed_size: null argument");
    if (int rc = check_cfg(cfg)) return rc;
    Packer P;
    P.blob = nullptr;
    std::vector<int64_t> woff((size_t)JE_GLOBAL_COUNT + (size_t)cfg->n_layers * JEL_LAYER_COUNT);
    if (int rc = run(cfg, P, woff.data())) return rc;
    *n_floats = P.pos;
    *n_woff = (int)woff.size();
    return JODO_OK;
}

// the slot table alone (the training path rebuilds the blob on the device from the live parameters: egnn_train.hip)
extern "C" int jodo_egnn_packed_layout(const jodo_egnn_cfg* cfg, int64_t* woff_out, int n_woff, size_t* n_floats) {
    if (!woff_out || !n_floats) return jodo_set_error(JODO_ERR_ARG, "egnn_packed_layout: null argument");
    if (int rc = check_cfg(cfg)) return rc;
    if (n_woff != JE_GLOBAL_COUNT + cfg->n_layers * JEL_LAYER_COUNT)
        return jodo_set_error(JODO_ERR_ARG, "egnn_packed_layout: table of %d slots, expected %d", n_woff, JE_GLOBAL_COUNT + cfg->n_layers * JEL_LAYER_COUNT);
    Packer P;
    P.blob = nullptr;
    if (int rc = run(cfg, P, woff_out)) return rc;
    *n_floats = P.pos;
    return JODO_OK;
}

extern "C" int jodo_egnn_pack_weights_host(const jodo_egnn_cfg* cfg, const jodo_tensor* tensors, int n_tensors, float* packed_host,
                                           size_t cap_floats, int64_t* woff_out, int n_woff) {
    if (!tensors || !packed_host || !woff_out) return jodo_set_error(JODO_ERR_ARG, "egnn_pack_weights: null argument");
    size_t need = 0;
    int nw = 0;
    if (int rc = jodo_egnn_packed_size(cfg, &need, &nw)) return rc;
    if (cap_floats < need || n_woff != nw)
        return jodo_set_error(JODO_ERR_ARG, "egnn_pack_weights: buffer of %zu floats / %d slots, need %zu / %d", cap_floats, n_woff, need, nw);
    Packer P;
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name) return jodo_set_error(JODO_ERR_ARG, "egnn_pack_weights: tensor %d has no name", i);
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

// TEST INFRASTRUCTURE ONLY: one forward + backward of the CDGS training engine's host build (QM9 shapes, atoms [1, 2, 5, 17, 29, 9],
// N = 29, dropout 0.1) as a stand-alone program, so that the address and undefined-behaviour sanitizers check every index of the
// kernels and of the product calls on exactly sized heap buffers: `make cdgs_train_san && ./cdgs_train_san`.
#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/jodo_hip.h"

struct Named { std::string name; std::vector<int64_t> shape; std::vector<float> data, grad; };

static unsigned long long rng = 88172645463325252ull;
static float unif() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (float)((rng >> 11) * (1.0 / 9007199254740992.0)) * 2.f - 1.f; }

int main() {
    const jodo_cdgs_cfg cfg{256, 8, 16, 5, 2, 8};
    const int D = cfg.nf, L = cfg.n_layers, K = cfg.rw_depth, ch = cfg.edge_ch, ach = cfg.atom_ch, cat = 2 * D / L;
    std::vector<Named> ts;
    auto add = [&](const std::string& n, std::vector<int64_t> shape, float gain) {
        Named t; t.name = n; t.shape = shape;
        size_t ne = 1; for (int64_t s : shape) ne *= (size_t)s;
        t.data.resize(ne); t.grad.assign(ne, 0.f);
        for (float& v : t.data) v = gain * unif();
        ts.push_back(t);
    };
    auto lin = [&](const std::string& n, int out_f, int in_f, bool conv = false) {
        add(n + ".weight", conv ? std::vector<int64_t>{out_f, in_f, 1, 1} : std::vector<int64_t>{out_f, in_f}, 1.7f / std::max(1.f, sqrtf((float)in_f)));
        add(n + ".bias", {out_f}, 0.1f);
    };
    auto mod = [&](int i) { return "all_modules." + std::to_string(i); };
    lin(mod(0), 2 * D, D); lin(mod(1), D, 2 * D);
    lin(mod(2), 77, ch - 1, true); lin(mod(3), 77, 1, true); lin(mod(4), 102, K + 1, true); lin(mod(5), D, D);
    lin(mod(6), 51, ch); lin(mod(7), 154, ach); lin(mod(8), 51, K); lin(mod(9), D, D);
    for (int l = 0; l < L; ++l) {
        const std::string p = mod(10 + 3 * l) + ".";
        lin(p + "t_node", D, D); lin(p + "t_edge", D, D);
        lin(p + "local_model.nn.0", D, D); lin(p + "local_model.nn.2", D, D); add(p + "local_model.eps", {1}, 0.f);
        lin(p + "self_attn.lin_key", D, D); lin(p + "self_attn.lin_query", D, D); lin(p + "self_attn.lin_value", D, D);
        add(p + "self_attn.lin_edge0.weight", {D, D}, 0.1f); add(p + "self_attn.lin_edge1.weight", {D, D}, 0.1f);
        for (const char* n : {"norm1_local", "norm1_attn"}) { add(p + n + ".weight", {D}, 1.f); add(p + n + ".bias", {D}, 0.1f); }
        lin(p + "ff_linear1", 2 * D, D); lin(p + "ff_linear2", D, 2 * D);
        add(p + "norm2_node.weight", {D}, 1.f); add(p + "norm2_node.bias", {D}, 0.1f);
        lin(p + "ff_linear3", 2 * D, D); lin(p + "ff_linear4", D, 2 * D);
        add(p + "norm2_edge.weight", {D}, 1.f); add(p + "norm2_edge.bias", {D}, 0.1f);
        lin(mod(11 + 3 * l), cat, D); lin(mod(12 + 3 * l), cat, D);
    }
    const int h0 = 10 + 3 * L;
    lin(mod(h0), D, cat * L + 154); lin(mod(h0 + 1), D / 2, D); lin(mod(h0 + 2), ach, D / 2);
    lin(mod(h0 + 3), D, cat * L + 77, true); lin(mod(h0 + 4), D / 2, D, true); lin(mod(h0 + 5), ch - 1, D / 2, true);
    lin(mod(h0 + 6), D, cat * L + 77, true); lin(mod(h0 + 7), D / 2, D, true); lin(mod(h0 + 8), 1, D / 2, true);
    const int n_t = (int)ts.size();
    std::vector<jodo_tensor> named(n_t);
    std::vector<const float*> P(n_t);
    std::vector<float*> G(n_t);
    for (int i = 0; i < n_t; ++i) {
        named[i].name = ts[i].name.c_str(); named[i].data = nullptr; named[i].shape = ts[i].shape.data(); named[i].ndim = (int)ts[i].shape.size();
        P[i] = ts[i].data.data();
        G[i] = ts[i].name.find("local_model.eps") != std::string::npos ? nullptr : ts[i].grad.data();
    }
    const std::vector<int32_t> n_nodes{1, 2, 5, 17, 29, 9};
    const int B = (int)n_nodes.size(), N = 29;
    jodo_cdgs_train* t = nullptr;
    if (jodo_cdgs_train_create(&cfg, B, N, n_nodes.data(), named.data(), n_t, &t)) { fprintf(stderr, "create: %s\n", jodo_last_error()); return 1; }
    std::vector<char> desc(jodo_cdgs_train_desc_bytes(t)), ws(jodo_cdgs_train_workspace_bytes(t));
    if (jodo_cdgs_train_upload(t, desc.data(), nullptr)) return 1;
    std::vector<float> freq(D / 2), tt(B), x((size_t)B * N * ach), ex((size_t)B * N * N * ch), ox(x.size()), oe(ex.size()), dx(x.size()), de(ex.size());
    for (int i = 0; i < D / 2; ++i) freq[i] = expf(-(float)i * logf(10000.f) / (D / 2 - 1));
    for (float& v : tt) v = 0.5f + 0.4f * unif();
    for (float& v : x) v = unif();
    for (float& v : dx) v = unif();
    for (float& v : de) v = unif();
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < n_nodes[b]; ++r)
            for (int c = r + 1; c < n_nodes[b]; ++c)
                for (int k = 0; k < ch; ++k) ex[(((size_t)b * N + r) * N + c) * ch + k] = ex[(((size_t)b * N + c) * N + r) * ch + k] = unif();
    if (jodo_cdgs_train_forward(t, desc.data(), P.data(), n_t, freq.data(), tt.data(), x.data(), ex.data(), 0.1f, 0x100000007ull, ox.data(), oe.data(),
                                ws.data(), nullptr)) { fprintf(stderr, "forward: %s\n", jodo_last_error()); return 1; }
    if (jodo_cdgs_train_backward(t, desc.data(), P.data(), G.data(), n_t, x.data(), ex.data(), dx.data(), de.data(), 0.1f, 0x100000007ull, ws.data(),
                                 nullptr)) { fprintf(stderr, "backward: %s\n", jodo_last_error()); return 1; }
    double so = 0.0, sg = 0.0;
    for (float v : ox) so += v;
    for (float v : oe) so += v;
    int dead = 0;
    for (int i = 0; i < n_t; ++i) {
        if (!G[i]) continue;
        double m = 0.0;
        for (float v : ts[i].grad) { sg += v; m = std::max(m, (double)fabsf(v)); }
        if (!(m > 0.0) || m != m) ++dead;
    }
    jodo_cdgs_train_destroy(t);
    printf("%d tensors, output sum %.6g, gradient sum %.6g, %d gradients dead or not finite\n", n_t, so, sg, dead);
    return (so == so && sg == sg && dead == 0) ? 0 : 2;
}

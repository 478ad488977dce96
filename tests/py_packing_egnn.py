"""Independent numpy restatement of csrc/egnn_pack.cpp (the property classifier's packed blob and slot table), written from the layout
description in include/jodo_hip.h: tests/test_egnn_host.py compares the C packer with it element by element."""
import numpy as np

GLOBAL_SLOTS, LAYER_SLOTS = 10, 11


def tile(W):
    """[rows, K] -> float [nb][nk][8 quads][64 lanes][4] in MFMA A-operand order, rows / K zero-padded to 32 / 64."""
    rows, K = W.shape
    nb, nk = (rows + 31) // 32, (K + 63) // 64
    Wp = np.zeros((nb * 32, nk * 64), dtype=np.float32)
    Wp[:rows, :K] = W
    q, l, i = np.meshgrid(np.arange(8), np.arange(64), np.arange(4), indexing='ij')
    a, m = 4 * q + i, l % 32
    col = (a // 16) * 32 + (l // 32) * 16 + a % 16
    row = 16 * ((m // 4) % 2) + 4 * (m // 8) + m % 4
    out = np.empty((nb, nk, 8, 64, 4), dtype=np.float32)
    for b in range(nb):
        for kc in range(nk):
            out[b, kc] = Wp[b * 32 + row, kc * 64 + col]
    return out.reshape(-1)


def pack(sd, nf, n_layers, in_nf, attention, node_attr):
    """state dict of numpy arrays -> (blob, slot offsets; -1 for the attention slots of a model without attention)."""
    parts, woff, pos = [], [], 0

    def put(v):
        nonlocal pos
        pad = (-pos) % 64
        parts.append(np.zeros(pad, dtype=np.float32))
        pos += pad
        woff.append(pos)
        parts.append(np.asarray(v, dtype=np.float32).reshape(-1))
        pos += parts[-1].size

    def linear(name):
        put(tile(sd[name + '.weight']))
        put(sd[name + '.bias'])

    for name in ('embedding', 'node_dec.0', 'node_dec.2', 'graph_dec.0'):
        linear(name)
    put(sd['graph_dec.2.weight'])
    put(sd['graph_dec.2.bias'])
    for l in range(n_layers):
        pre = 'gcl_%d.' % l
        w1 = sd[pre + 'edge_mlp.0.weight']
        put(tile(np.concatenate([w1[:, :nf], w1[:, nf:2 * nf]], 0)))
        put(np.concatenate([sd[pre + 'edge_mlp.0.bias'], np.zeros(nf, dtype=np.float32)]))
        put(w1[:, 2 * nf])
        linear(pre + 'edge_mlp.2')
        if attention:
            put(sd[pre + 'att_mlp.0.weight'])
            put(sd[pre + 'att_mlp.0.bias'])
        else:
            woff += [-1, -1]
        linear(pre + 'node_mlp.0')
        linear(pre + 'node_mlp.2')
    parts.append(np.zeros((-pos) % 64, dtype=np.float32))
    return np.concatenate(parts), woff

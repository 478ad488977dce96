"""Independent Python packer of the 2-D model's weight blob (test infrastructure): numpy restatement of the layout documented in
include/jodo_hip.h / csrc/dgt2d_pack.cpp, kept in lock-step with the C packer blob for blob (tests/test_dgt2d_host.py)."""
import numpy as np

GLOBAL_SLOTS = ['TIME_FREQ', 'TIME_W1', 'TIME_B1', 'TIME_W3', 'TIME_B3', 'MOD_W', 'MOD_B', 'NODE_EMB_W', 'NODE_EMB_B', 'EDGE_EMB_W',
                'EDGE_EMB_B', 'NH1_W', 'NH1_B', 'NH2_W', 'NH2_B', 'NH3_W', 'NH3_B', 'EH1_W', 'EH1_B', 'EH2_W', 'EH2_B', 'EH3_W', 'EH3_B']
BLOCK_SLOTS = ['QKV_W', 'QKV_B', 'LE_W', 'N2E_W', 'N2E_B', 'FF1_W', 'FF1_B', 'FF2_W', 'FF2_B', 'FF3_W', 'FF3_B', 'FF4_W', 'FF4_B',
               'NRO_W', 'NRO_B', 'ERO_W', 'ERO_B']


def slot_feature(half, t):
    """q / k / lin_edge0 slot t (0..127) of lane half `half` -> learned-head feature 0..254, -1 = padding."""
    if t < 119:
        return (136 if half else 0) + t
    if half == 0:
        return t
    return 128 + (t - 119) if t < 127 else -1


def ident(n, valid=None):
    m = -np.ones((n + 31) // 32 * 32, dtype=np.int64)
    k = n if valid is None else valid
    m[:k] = np.arange(k)
    return m


def tile(W, rowmap):
    """W [R, K] (already stacked) -> float32 [nb, nk, 8, 64, 4] flattened."""
    R, K = W.shape
    nb, nk = len(rowmap) // 32, (K + 63) // 64
    Wp = np.zeros((R + 1, nk * 64), dtype=np.float32)
    Wp[:R, :K] = W
    m = np.arange(32)
    lp = 16 * ((m // 4) % 2) + 4 * (m // 8) + m % 4                       # MFMA row -> logical position inside the block
    rows = np.asarray(rowmap).reshape(nb, 32)[:, lp]                     # [nb, m]
    rows = np.where(rows < 0, R, rows)
    q, l, i = np.meshgrid(np.arange(8), np.arange(64), np.arange(4), indexing='ij')
    a = 4 * q + i
    col = (a // 16) * 32 + (l // 32) * 16 + a % 16                       # [8, 64, 4]
    out = np.empty((nb, nk, 8, 64, 4), dtype=np.float32)
    for kc in range(nk):
        out[:, kc] = Wp[rows[:, l % 32], kc * 64 + col]
    return out.reshape(-1)


def bias(b, rowmap):
    bp = np.concatenate([np.asarray(b, dtype=np.float32), np.zeros(1, np.float32)])
    return bp[np.where(np.asarray(rowmap) < 0, len(bp) - 1, rowmap)]


def pack(sd, nf, n_layers, nd, ch):
    """sd: name -> numpy float32 array.  Returns (blob float32, woff int64 list)."""
    D, De, T, L = nf, nf // 4, 4 * nf, n_layers
    parts, woff, pos = [], [], [0]

    def put(arr, aligned=True):
        if aligned:
            pad = (-pos[0]) % 64
            if pad:
                parts.append(np.zeros(pad, np.float32))
                pos[0] += pad
        at = pos[0]
        arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        parts.append(arr)
        pos[0] += arr.size
        return at

    w = lambda n: sd[n + '.weight']
    b = lambda n: sd[n + '.bias']
    woff.append(put(sd['time_mlp.0.weights']))
    woff.append(put(w('time_mlp.1')))
    woff.append(put(b('time_mlp.1')))
    woff.append(put(tile(w('time_mlp.3'), ident(T))))
    woff.append(put(bias(b('time_mlp.3'), ident(T))))
    mw = np.concatenate([np.concatenate([w('e_block_%d.node_time_mlp.1' % l), w('e_block_%d.edge_time_mlp.1' % l)]) for l in range(L)])
    mb = np.concatenate([np.concatenate([b('e_block_%d.node_time_mlp.1' % l), b('e_block_%d.edge_time_mlp.1' % l)]) for l in range(L)])
    woff.append(put(tile(mw, ident(len(mb)))))
    woff.append(put(bias(mb, ident(len(mb)))))
    for n in ('node_emb', 'edge_emb'):
        woff.append(put(w(n)))
        woff.append(put(b(n)))
    woff.append(put(tile(w('node_pred_mlp.0'), ident(D)))); woff.append(put(bias(b('node_pred_mlp.0'), ident(D))))
    woff.append(put(tile(w('node_pred_mlp.2'), ident(D // 2)))); woff.append(put(bias(b('node_pred_mlp.2'), ident(D // 2))))
    woff.append(put(tile(w('node_pred_mlp.4'), ident(32, nd)))); woff.append(put(bias(b('node_pred_mlp.4'), ident(32, nd))))
    woff.append(put(tile(np.concatenate([w('edge_exist_mlp.0'), w('edge_type_mlp.0')]), ident(2 * De))))
    woff.append(put(bias(np.concatenate([b('edge_exist_mlp.0'), b('edge_type_mlp.0')]), ident(2 * De))))
    woff.append(put(tile(w('edge_exist_mlp.2'), ident(De // 2))))
    put(tile(w('edge_type_mlp.2'), ident(De // 2)))
    woff.append(put(bias(np.concatenate([b('edge_exist_mlp.2'), b('edge_type_mlp.2')]), ident(De))))
    woff.append(put(w('edge_exist_mlp.4')))
    put(w('edge_type_mlp.4'), aligned=False)
    woff.append(put(b('edge_exist_mlp.4')))
    put(b('edge_type_mlp.4'), aligned=False)
    # attention row maps
    qkv = -np.ones(3 * D, dtype=np.int64)
    le = -np.ones(2 * D, dtype=np.int64)
    for half in range(2):
        for t in range(128):
            f = slot_feature(half, t)
            qkv[half * 128 + t] = f
            qkv[D + half * 128 + t] = -1 if f < 0 else 255 + f
            le[(t // 16) * 32 + half * 16 + t % 16] = f
    qkv[2 * D:] = 510 + np.arange(D)
    for blk in range(8):
        for h in range(2):
            le[D + blk * 32 + h * 16 + np.arange(16)] = 255 + (8 * h + blk) * 16 + np.arange(16)
    for l in range(L):
        pre, at = 'e_block_%d.' % l, 'e_block_%d.attn_mpnn.' % l
        woff.append(put(tile(np.concatenate([w(at + 'lin_query'), w(at + 'lin_key'), w(at + 'lin_value')]), qkv)))
        woff.append(put(bias(np.concatenate([b(at + 'lin_query'), b(at + 'lin_key'), b(at + 'lin_value')]), qkv)))
        woff.append(put(tile(np.concatenate([w(at + 'lin_edge0'), w(at + 'lin_edge1')]), le)))
        for name, rows, valid in ((pre + 'node2edge_lin', De, None), (pre + 'ff_linear1', 2 * D, None), (pre + 'ff_linear2', D, None),
                                  (pre + 'ff_linear3', 2 * De, None), (pre + 'ff_linear4', De, None), ('node_%d' % l, 2 * D // L, None),
                                  ('edge_%d' % l, 32, 2 * De // L)):
            woff.append(put(tile(w(name), ident(rows, valid))))
            woff.append(put(bias(b(name), ident(rows, valid))))
    pad = (-pos[0]) % 64
    if pad:
        parts.append(np.zeros(pad, np.float32))
    return np.concatenate(parts), woff

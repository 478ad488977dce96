"""Independent Python packer of the CDGS weights: the blob layout documented in include/jodo_hip.h (section "CDGS") and
csrc/cdgs_pack.cpp, rebuilt with numpy from the state_dict.  tests/test_cdgs_host.py compares it with the C packer bit for bit."""
import numpy as np

GLOBAL = ['FREQ', 'T1_W', 'T1_B', 'T2_W', 'T2_B', 'TMOD_W', 'TMOD_B', 'EC_W', 'EC_B', 'EX_W', 'EX_B', 'SPD_W', 'SPD_B', 'EEMB_W', 'EEMB_B',
          'AD_W', 'AD_B', 'AC_W', 'AC_B', 'AR_W', 'AR_B', 'NEMB_W', 'NEMB_B', 'AH1_W', 'AH1_B', 'AH2_W', 'AH2_B', 'AH3_W', 'AH3_B',
          'EH1_W', 'EH1_B', 'EH2_W', 'EH2_B', 'EH3_W', 'EH3_B']
BLOCK = ['EPS', 'GIN1_W', 'GIN1_B', 'GIN2_W', 'GIN2_B', 'QKV_W', 'QKV_B', 'E01_W', 'NL_G', 'NL_B', 'NA_G', 'NA_B', 'FF1_W', 'FF1_B',
         'FF2_W', 'FF2_B', 'NN_G', 'NN_B', 'FF3_W', 'FF3_B', 'FF4_W', 'FF4_B', 'NE_G', 'NE_B', 'RN_W', 'RN_B', 'RE_W', 'RE_B']


def _tile_index(nb, nk):
    """(logical row, logical column) of every element of a tiled matrix [nb][nk][8][64][4]."""
    b, kc, q, l, i = np.meshgrid(np.arange(nb), np.arange(nk), np.arange(8), np.arange(64), np.arange(4), indexing='ij')
    a, m = 4 * q + i, l % 32
    col = kc * 64 + (a // 16) * 32 + (l // 32) * 16 + a % 16
    row = b * 32 + 16 * ((m // 4) % 2) + 4 * (m // 8) + m % 4
    return row.reshape(-1), col.reshape(-1)


def tiled(mat):
    """mat: the LOGICAL matrix [rows, K] (already permuted / stacked); zero-padded to 32 x 64 multiples and tiled."""
    rows, K = mat.shape
    nb, nk = (rows + 31) // 32, (K + 63) // 64
    full = np.zeros((nb * 32, nk * 64), np.float32)
    full[:rows, :K] = mat
    r, c = _tile_index(nb, nk)
    return full[r, c]


def vec(v):
    out = np.zeros((len(v) + 31) // 32 * 32, np.float32)
    out[:len(v)] = v
    return out


def pack(sd, nf, n_layers, atom_ch, edge_ch, rw_depth, time_freq):
    """state_dict of numpy arrays -> (blob float32, {slot name: offset}, [per block {slot name: offset}])."""
    D, L, K, ch = nf, n_layers, rw_depth, edge_ch
    bse, ase = int(D * 0.4), int(D * 0.2)
    bt, att = int(0.5 * (D - bse)), D - 2 * ase
    cat = 2 * D // L
    catp = (cat + 31) // 32 * 32
    KA, KE = (L * catp + att + 63) // 64 * 64, (L * catp + 192 + 63) // 64 * 64
    g = lambda k: np.asarray(sd[k], np.float32)
    W = lambda i: g('all_modules.%d.weight' % i).reshape(g('all_modules.%d.weight' % i).shape[0], -1)
    B = lambda i: g('all_modules.%d.bias' % i)
    parts, pos = [], [0]

    def put(a):
        pad = (-pos[0]) % 64
        parts.append(np.zeros(pad, np.float32))
        at = pos[0] + pad
        a = np.asarray(a, np.float32).reshape(-1)
        parts.append(a)
        pos[0] = at + a.size
        return at

    def hids_cols(w, lead, extra_at):
        """first head layer [out, lead + L cat] -> the kernels' columns [hids (L catp) | ... lead columns at extra_at ...]"""
        out = np.zeros((w.shape[0], max(KA, KE)), np.float32)
        for l in range(L):
            out[:, l * catp:l * catp + cat] = w[:, lead + l * cat:lead + (l + 1) * cat]
        out[:, extra_at:extra_at + lead] = w[:, :lead]
        return out

    G = {}
    G['FREQ'] = put(time_freq)
    G['T1_W'] = put(tiled(W(0))); G['T1_B'] = put(vec(B(0)))
    G['T2_W'] = put(tiled(W(1))); G['T2_B'] = put(vec(B(1)))
    blk = lambda l, n: g('all_modules.%d.%s' % (10 + 3 * l, n))
    G['TMOD_W'] = put(tiled(np.concatenate([np.concatenate([blk(l, 't_node.weight'), blk(l, 't_edge.weight')]) for l in range(L)])))
    G['TMOD_B'] = put(vec(np.concatenate([np.concatenate([blk(l, 't_node.bias'), blk(l, 't_edge.bias')]) for l in range(L)])))
    for name, i in (('EC', 2), ('EX', 3), ('SPD', 4)):
        G[name + '_W'] = put(W(i)); G[name + '_B'] = put(B(i))
    G['EEMB_W'] = put(tiled(W(5))); G['EEMB_B'] = put(vec(B(5)))
    for name, i in (('AD', 6), ('AC', 7), ('AR', 8)):
        G[name + '_W'] = put(W(i)); G[name + '_B'] = put(B(i))
    G['NEMB_W'] = put(tiled(W(9))); G['NEMB_B'] = put(vec(B(9)))
    h0 = 10 + 3 * L
    G['AH1_W'] = put(tiled(hids_cols(W(h0), att, L * catp)[:, :KA])); G['AH1_B'] = put(vec(B(h0)))
    G['AH2_W'] = put(tiled(W(h0 + 1))); G['AH2_B'] = put(vec(B(h0 + 1)))
    a3 = np.zeros((32, D // 2), np.float32); a3[:atom_ch] = W(h0 + 2)
    G['AH3_W'] = put(tiled(a3)); G['AH3_B'] = put(vec(B(h0 + 2)))
    e1 = np.concatenate([hids_cols(W(h0 + 6), bt, L * catp + 96)[:, :KE], hids_cols(W(h0 + 3), bt, L * catp)[:, :KE]])
    G['EH1_W'] = put(tiled(e1)); G['EH1_B'] = put(vec(np.concatenate([B(h0 + 6), B(h0 + 3)])))
    e2 = np.zeros((D, 2 * D), np.float32)
    e2[:D // 2, :D] = W(h0 + 7); e2[D // 2:, D:] = W(h0 + 4)
    G['EH2_W'] = put(tiled(e2)); G['EH2_B'] = put(vec(np.concatenate([B(h0 + 7), B(h0 + 4)])))
    e3 = np.zeros((32, D), np.float32)
    e3[0, :D // 2] = W(h0 + 8)[0]; e3[1:ch, D // 2:] = W(h0 + 5)
    G['EH3_W'] = put(tiled(e3)); G['EH3_B'] = put(vec(np.concatenate([B(h0 + 8), B(h0 + 5)])))
    blocks = []
    for l in range(L):
        b = {}
        w = lambda n: blk(l, n + '.weight')
        bi = lambda n: blk(l, n + '.bias')
        b['EPS'] = put(blk(l, 'local_model.eps'))
        b['GIN1_W'] = put(tiled(w('local_model.nn.0'))); b['GIN1_B'] = put(vec(bi('local_model.nn.0')))
        b['GIN2_W'] = put(tiled(w('local_model.nn.2'))); b['GIN2_B'] = put(vec(bi('local_model.nn.2')))
        b['QKV_W'] = put(tiled(np.concatenate([w('self_attn.lin_query'), w('self_attn.lin_key'), w('self_attn.lin_value')])))
        b['QKV_B'] = put(vec(np.concatenate([bi('self_attn.lin_query'), bi('self_attn.lin_key'), bi('self_attn.lin_value')])))
        b['E01_W'] = put(tiled(np.concatenate([w('self_attn.lin_edge0'), w('self_attn.lin_edge1')])))
        b['NL_G'] = put(w('norm1_local')); b['NL_B'] = put(bi('norm1_local'))
        b['NA_G'] = put(w('norm1_attn')); b['NA_B'] = put(bi('norm1_attn'))
        b['FF1_W'] = put(tiled(w('ff_linear1'))); b['FF1_B'] = put(vec(bi('ff_linear1')))
        b['FF2_W'] = put(tiled(w('ff_linear2'))); b['FF2_B'] = put(vec(bi('ff_linear2')))
        b['NN_G'] = put(w('norm2_node')); b['NN_B'] = put(bi('norm2_node'))
        b['FF3_W'] = put(tiled(w('ff_linear3'))); b['FF3_B'] = put(vec(bi('ff_linear3')))
        b['FF4_W'] = put(tiled(w('ff_linear4'))); b['FF4_B'] = put(vec(bi('ff_linear4')))
        b['NE_G'] = put(w('norm2_edge')); b['NE_B'] = put(bi('norm2_edge'))
        for name, i in (('RN', 11 + 3 * l), ('RE', 12 + 3 * l)):
            r = np.zeros((catp, D), np.float32); r[:cat] = W(i)
            rb = np.zeros(catp, np.float32); rb[:cat] = B(i)
            b[name + '_W'] = put(tiled(r)); b[name + '_B'] = put(rb)
        blocks.append(b)
    put(np.zeros(0, np.float32))
    return np.concatenate(parts), G, blocks

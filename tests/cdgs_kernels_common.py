"""Shared by tests/test_cdgs_kernels_host.py (host emulation build) and tests/test_cdgs_kernels_gpu.py (device): the launch sequences of
the CDGS training step (csrc/cdgs_train.hip) one by one through the test entry jodo_cdgs_train_debug_op.

  * restate(op, d, dtype): every op in dense torch on the reference's padded [B, N, ...] tensors, in float64 (the yardstick) or float32
    (the measure of what float32 arithmetic reaches), written from the reference's semantics (masked GroupNorms, the softmax over the
    real sources with + 1e-16, GINE over the thresholded adjacency), not from the kernels' loops;
  * inputs(op, n_nodes, N, seed, hard, ...): the benign and the hard value sets, and the conditions under which a comparison is decided
    (checked by the host test on the float64 restatement alone);
  * Harness: the call itself on any device (host pointers for the emulation build): outputs poisoned with NaN, every array between two
    guard bands of 512 floats, inputs unchanged afterwards (but for the documented in-place arrays), the call repeated bit for bit;
  * compare(): every element of every stored array under the project's two rules, unchanged: helpers.close64 for activation-type
    arrays, train2d_common.compare_grads for gradient-type arrays, bit equality for what is exactly representable.
"""
import ctypes
import math

import numpy as np
import torch

from helpers import FWD_ATOL, FWD_RTOL, K64, close64
from oracle import philox_ref as PR
from train2d_common import GRAD_REL, K32, compare_grads

D, H, F = 256, 16, 512                  # the widths of both CDGS configs (nf, n_heads, feed-forward)
GW = 8                                  # channels per GroupNorm group
ISC = 1.0 / math.sqrt(D // H)
GUARD, PATTERN = 512, 0x5A5AC3C3
RELU_MARGIN = 5e-6                      # the rule of cdgs_train_common
SEED_HI = (0x1234 << 32) | 0x9E3779B9   # a dropout seed above 2^32

# tile widths: (n_nodes, N); the first four for every tiled op, the last three for ATTN_*, GINE*, EGN_*, PAIR*, SUMS and RW
SMALL = [([1], 1), ([2, 1], 2), ([9, 4, 7, 2], 12), ([12, 1, 5], 12)]
WIDE = [([64, 1], 64), ([65, 2], 65), ([181, 2], 181)]
COLSUM_ROWS = [1, 63, 64, 65, 2047, 2048, 2049, 2113]      # 32 / 33 chunks and a ragged tail; 6209 below: 3 groups + a ragged one
COLSUM_GROUPS = 6209                                        # 98 chunks = 3 groups of 32 + a group of 2, the last chunk of 1 row


def rw_dims(N):
    """(K, ch): the GEOM config's at N = 181, the QM9 config's elsewhere"""
    return (16, 3) if N == 181 else (8, 2)


# slot roles per op: ins (read only), outs with their rule, inout (documented in-place arrays: compared as outputs), scratch
OPS = {
    'RW': dict(ins=('EDGE_X',), outs=dict(ADJ='exact', AD='fwd', CNT='exact', ONEHOT='exact', LAND='fwd', DEG='fwd'), scratch=('PA', 'PB')),
    'ADDT': dict(ins=('X', 'TB'), outs=dict(Y='fwd')),
    'SCALE': dict(ins=('X',), outs=dict(Y='fwd')),
    'RELU': dict(ins=('X',), outs=dict(Y='exact')),
    'RELU_BWD': dict(ins=('X',), outs=dict(Y='exact')),
    'PAIR': dict(ins=('X',), outs=dict(Y='fwd')),
    'PAIR_BWD': dict(ins=('X',), outs=dict(Y='bwd')),
    'OUT_NODES': dict(ins=('X',), outs=dict(Y='exact')),
    'OUT_EDGES': dict(ins=('X',), outs=dict(Y='fwd')),
    'SUMS': dict(ins=('X',), outs=dict(Y='bwd', Z='bwd')),
    'GINE': dict(ins=('EPS', 'HS', 'HE', 'ADJ'), outs=dict(AGG='fwd')),
    'GINE_BWD': dict(ins=('EPS', 'HS', 'HE', 'ADJ', 'DAGG'), outs=dict(DHE='bwd', DHS='bwd')),
    'GN_FWD': dict(ins=('H', 'A', 'GAMMA', 'BETA'), outs=dict(XHAT='fwd', RSTD='fwd', Y='fwd')),
    'GN_BWD': dict(ins=('DY', 'XHAT', 'RSTD', 'GAMMA'), outs=dict(DX='bwd')),
    'EGN_FWD': dict(ins=('GAMMA', 'BETA'), outs=dict(XHAT='fwd', RSTD='fwd', Y='fwd'), inout=('XHAT',), scratch=('PART', 'GSUM')),
    'EGN_BWD': dict(ins=('DY', 'XHAT', 'RSTD', 'GAMMA'), outs=dict(DX='bwd'), scratch=('PART', 'GSUM')),
    'NORM_GRADS': dict(ins=('DY', 'XHAT'), outs=dict(DBETA='bwd', DGAMMA='bwd'), scratch=('PART',)),
    'ATTN_FWD': dict(ins=('Q', 'K', 'V', 'G0', 'G1'), outs=dict(ALPHA='fwd', ATT='fwd')),
    'ATTN_BWD': dict(ins=('DATT', 'Q', 'K', 'V', 'G0', 'G1', 'ALPHA'), outs=dict(DV='bwd', DAL='bwd', DT1='bwd', DT0='bwd', DQ='bwd', DK='bwd')),
}
SCALARS = ('F', 'ch', 'mode', 'acc', 'amask', 'drop_site', 'isc', 'drop_p', 'drop_seed', 'rows')


def masks(n_nodes, N, dtype=torch.float64):
    """node mask [B, N], mask of the real ordered pairs [B, N, N] (r != c, both inside the molecule)"""
    n = torch.as_tensor(list(n_nodes)).reshape(-1, 1)
    nm = (torch.arange(N).reshape(1, N) < n)
    em = nm[:, :, None] & nm[:, None, :] & ~torch.eye(N, dtype=torch.bool)[None]
    return nm.to(dtype), em.to(dtype)


def live_rows(d, rows, dtype):
    nm, em = masks(d['n_nodes'], d['N'], dtype)
    mode = d.get('mode', 0)
    return torch.ones(rows, dtype=dtype) if mode == 0 else (nm if mode == 1 else em).reshape(-1)[:rows]


def multipliers(d, shape, dtype):
    """the dropout multipliers of a dense tensor at the op's site: philox_ref's, element = flat index"""
    p = d.get('drop_p', 0.0)
    if p <= 0:
        return torch.ones(shape, dtype=dtype)
    count = int(np.prod(shape))
    return torch.from_numpy(PR.drop_mul(d.get('drop_seed', 0), d.get('drop_site', 0), p, count).reshape(shape)).to(dtype)


def group_norm_rows(x, eps=1e-6):
    """per row and group of 8 channels: (xhat, rstd [.., C / 8])"""
    g = x.reshape(x.shape[:-1] + (x.shape[-1] // GW, GW))
    mean = g.mean(-1, keepdim=True)
    var = ((g - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return ((g - mean) * rstd).reshape(x.shape), rstd.squeeze(-1)


def group_norm_tile(x, eps=1e-6):
    """per molecule and group of 8 channels over ALL N x N positions of the padded tile: (xhat, rstd [B, C / 8])"""
    B, N, _, C = x.shape
    g = x.reshape(B, N * N, C // GW, GW)
    mean = g.mean((1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return ((g - mean) * rstd).reshape(x.shape), rstd.reshape(B, C // GW)


def rw_restate(edge_x, n_nodes, N, K, dtype, keep=None):
    _, em = masks(n_nodes, N, dtype)
    ex = edge_x.to(dtype)
    adj = (ex[..., 0] >= 0).to(dtype) * em
    AD = adj / (adj.sum(-1, keepdim=True) + 1e-8)
    p, land = AD, []
    cnt = torch.zeros_like(adj)
    for _ in range(K):
        p = torch.bmm(p, AD)
        land.append(torch.diagonal(p, dim1=1, dim2=2))
        cnt = cnt + (p <= 0).to(dtype)
        if keep is not None:
            keep.append(p)
    onehot = torch.nn.functional.one_hot(cnt.long(), K + 1).to(dtype)
    return dict(ADJ=adj, AD=AD, CNT=cnt, ONEHOT=onehot, LAND=torch.stack(land, -1), DEG=ex.sum(2))


def attn_alpha(q, k, g0, em, isc, offset=None):
    """alpha [B, N(source j), N(target i), H]: softmax over the real sources of every target, exp / (sum + 1e-16); 0 where no real pair"""
    B, N, C = q.shape
    logit = (q[:, None] * k[:, :, None] * g0).reshape(B, N, N, H, -1).sum(-1) * isc
    if offset is not None:
        logit = logit + offset
    live = em[..., None] > 0
    logit = logit.masked_fill(~live, float('-inf'))
    mx = logit.max(dim=1, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    ex = torch.exp(logit - mx)
    return ex / (ex.sum(1, keepdim=True) + 1e-16), logit


def attn_msg(v, g1, alpha):
    B, N, C = v.shape
    return (v[:, :, None] * g1 * alpha.repeat_interleave(C // alpha.shape[-1], -1)).sum(1)


def restate(op, d, dtype=torch.float64):
    """slot -> what the op stores, in `dtype`, in the shapes of the arrays"""
    n_nodes, N = d['n_nodes'], d['N']
    nm, em = masks(n_nodes, N, dtype)
    t = lambda k: d[k].to(dtype)
    if op == 'RW':
        return rw_restate(d['EDGE_X'], n_nodes, N, d['depth'], dtype)
    if op in ('ADDT', 'SCALE', 'RELU', 'RELU_BWD'):
        x = t('X')
        rows = x.shape[0]
        live = live_rows(d, rows, dtype)[:, None]
        if op == 'ADDT':
            per = N if d['mode'] == 1 else N * N
            return dict(Y=(x + t('TB').repeat_interleave(per, 0)[:rows]) * live)
        if op == 'SCALE':
            y = x * multipliers(d, x.shape, dtype) * live
            return dict(Y=t('Y') + y if d.get('acc') else y)
        if op == 'RELU':
            return dict(Y=torch.relu(x))
        return dict(Y=t('Y') * (x > 0).to(dtype))
    if op == 'PAIR':
        x = t('X')
        return dict(Y=x[:, :, None, :] + x[:, None, :, :])
    if op == 'PAIR_BWD':
        x = t('X')
        return dict(Y=x.sum(2) + x.sum(1))
    if op == 'OUT_NODES':
        return dict(Y=t('X') * nm[..., None])
    if op == 'OUT_EDGES':
        x = t('X')
        return dict(Y=(x + x.transpose(1, 2)) / 2 * em[..., None])
    if op == 'SUMS':
        cols = (t('X') * em[..., None]).sum(2)
        return dict(Y=cols, Z=(cols * nm[..., None] if d['mode'] else cols).sum(1))
    if op in ('GINE', 'GINE_BWD'):
        hs, he, adj, eps = t('HS'), t('HE'), t('ADJ'), t('EPS')
        pre = hs[:, :, None, :] + he                                  # [b, source j, target i, c]
        if op == 'GINE':
            return dict(AGG=(1 + eps) * hs + (torch.relu(pre) * adj[..., None]).sum(1))
        dagg = t('DAGG')
        dhe = (pre > 0).to(dtype) * adj[..., None] * dagg[:, None, :, :]
        return dict(DHE=dhe, DHS=(1 + eps) * dagg + dhe.sum(2))
    if op == 'GN_FWD':
        a = t('A') * multipliers(d, d['A'].shape, dtype)
        xhat, rstd = group_norm_rows(t('H') + (a * nm[..., None] if d.get('amask') else a))
        y = (xhat * t('GAMMA') + t('BETA')) * nm[..., None]
        return dict(XHAT=xhat, RSTD=rstd, Y=t('Y') + y if d.get('acc') else y)
    if op == 'GN_BWD':
        xhat, rstd = t('XHAT'), t('RSTD')
        gd = (t('GAMMA') * t('DY') * nm[..., None])
        sh = gd.shape[:-1] + (gd.shape[-1] // GW, GW)
        g, xh = gd.reshape(sh), xhat.reshape(sh)
        dx = (rstd[..., None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))).reshape(gd.shape)
        return dict(DX=t('DX') + dx if d.get('acc') else dx)
    if op == 'EGN_FWD':
        xhat, rstd = group_norm_tile(t('XHAT'))
        return dict(XHAT=xhat, RSTD=rstd, Y=(xhat * t('GAMMA') + t('BETA')) * em[..., None])
    if op == 'EGN_BWD':
        xhat, rstd = t('XHAT'), t('RSTD')
        B = xhat.shape[0]
        gd = torch.where(em[..., None] > 0, t('GAMMA') * t('DY'), torch.zeros((), dtype=dtype))      # the padded rows of DY hold garbage
        g, xh = gd.reshape(B, N * N, -1, GW), xhat.reshape(B, N * N, -1, GW)
        m1, m2 = g.mean((1, 3), keepdim=True), (g * xh).mean((1, 3), keepdim=True)
        return dict(DX=(rstd.reshape(B, 1, -1, 1) * (g - m1 - xh * m2)).reshape(xhat.shape))
    if op == 'NORM_GRADS':
        dy, xhat = t('DY'), t('XHAT')
        live = live_rows(d, dy.shape[0], dtype)[:, None] > 0
        dy = torch.where(live, dy, torch.zeros((), dtype=dtype))
        return dict(DBETA=dy.sum(0), DGAMMA=(dy * torch.where(live, xhat, torch.zeros((), dtype=dtype))).sum(0))
    if op == 'ATTN_FWD':
        alpha, _ = attn_alpha(t('Q'), t('K'), t('G0'), em, d['isc'], d.get('LOGIT_OFFSET'))
        return dict(ALPHA=alpha, ATT=attn_msg(t('V'), t('G1'), alpha))
    if op == 'ATTN_BWD':
        q, k, v, g0, g1, al, datt = (t(x) for x in ('Q', 'K', 'V', 'G0', 'G1', 'ALPHA', 'DATT'))
        Ch = q.shape[-1] // al.shape[-1]
        heads = lambda x: x.reshape(x.shape[:-1] + (al.shape[-1], Ch))
        wide = lambda x: x.repeat_interleave(Ch, -1)
        isc = d['isc']
        dmsg = datt[:, None, :, :] * v[:, :, None, :]                  # [b, j, i, c]: d att_i / d (g1 alpha)
        dv = (datt[:, None, :, :] * g1 * wide(al)).sum(2)
        dal = heads(dmsg * g1).sum(-1) * em[..., None]
        dlg = al * (dal - (al * dal).sum(1, keepdim=True))
        dt1 = dmsg * wide(al) * (1 - g1 * g1)
        qk = q[:, None, :, :] * k[:, :, None, :]
        dt0 = wide(dlg) * isc * qk * (1 - g0 * g0)
        dq = (wide(dlg) * k[:, :, None, :] * g0).sum(1) * isc
        dk = (wide(dlg) * q[:, None, :, :] * g0).sum(2) * isc
        return dict(DV=dv, DAL=dlg, DT1=dt1, DT0=dt0, DQ=dq, DK=dk)
    raise KeyError(op)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def graph_edge_x(kind, n_nodes, N, ch, g):
    """edge_x [B, N, N, ch] whose first channel encodes a graph on every molecule (>= 0: adjacent), garbage on the padded positions (the
    degree feature sums them, the adjacency must not see them)"""
    B = len(n_nodes)
    ex = torch.randn(B, N, N, ch, generator=g)
    ex = ex + ex.transpose(1, 2)
    r, c = torch.arange(N)[:, None], torch.arange(N)[None, :]
    for b, n in enumerate(n_nodes):
        if kind == 'random':
            continue
        a = {'path': (r - c).abs() == 1, 'star': ((r == 0) | (c == 0)) & (r != c), 'complete': r != c, 'empty': r < 0,
             'isolated': (r != c) & (r != n - 1) & (c != n - 1)}[kind]          # isolated: complete but for the last atom
        ex[b, :, :, 0] = torch.where(a, torch.full((), 0.5), torch.full((), -0.5))
        ex[b, n:, :, 0] = 1.0                                                       # padded: would be adjacent if the mask were ignored
        ex[b, :, n:, 0] = 1.0
    return ex


def _tile_values(B, N, C, g, hard, n_nodes):
    x = torch.randn(B, N, N, C, generator=g)
    if hard == 'constant':
        x[0] = 0.75                                                                 # variance clamps to 0: xhat exactly 0, rstd 1000
    elif hard == 'mean':
        x[0] = 1e3 + 1e-2 * torch.randn(N, N, C, generator=g)
    return x


def inputs(op, n_nodes, N, seed, hard=None, **kw):
    """the arrays (float32, dense shapes) and scalars of one call.  kw: mode, acc, amask, drop_p, drop_seed, drop_site, rows, K, ch, Fw."""
    g = torch.Generator().manual_seed(seed)
    B, M = len(n_nodes), len(n_nodes) * N
    rn = lambda *s: torch.randn(*s, generator=g)
    nm, em = masks(n_nodes, N, torch.float32)
    K, ch = kw.get('K', rw_dims(N)[0]), kw.get('ch', rw_dims(N)[1])
    Fw = kw.get('Fw', D)
    d = dict(n_nodes=list(n_nodes), N=N, width=D, heads=H, F=Fw, depth=K, ch=ch, isc=ISC, mode=kw.get('mode', 0), acc=kw.get('acc', 0), amask=kw.get('amask', 0),
             drop_p=kw.get('drop_p', 0.0), drop_seed=kw.get('drop_seed', 0), drop_site=kw.get('drop_site', 0), rows=kw.get('rows', 0))
    if op == 'RW':
        d['EDGE_X'] = graph_edge_x(hard or 'random', n_nodes, N, ch, g)
    elif op in ('ADDT', 'SCALE', 'RELU', 'RELU_BWD', 'NORM_GRADS'):
        full = B * N if d['mode'] == 1 else B * N * N
        rows = d['rows'] or full
        d['X'] = rn(rows, Fw)
        if op == 'ADDT':
            d['TB'] = rn(B, Fw)
        if op == 'SCALE' and hard == 'ones':
            d['X'] = torch.ones(rows, Fw)
        if op in ('SCALE', 'RELU_BWD'):
            d['Y'] = rn(rows, Fw)                                                   # read when acc = 1 (RELU_BWD: the gradient, in place)
        if op == 'RELU':
            d['X'][0, :4] = torch.tensor([0.0, -0.0, 1e-38, -1e-38])
        if op == 'NORM_GRADS':
            d['DY'], d['XHAT'] = d.pop('X'), rn(rows, Fw)
            if kw.get('one_row') is not None:                                       # dy non-zero on ONE live row only
                keep = torch.zeros(rows, 1)
                keep[kw['one_row']] = 1.0
                d['DY'] = d['DY'] * keep
    elif op in ('PAIR', 'OUT_NODES'):
        d['X'] = rn(B, N, D if op == 'PAIR' else Fw)
    elif op == 'PAIR_BWD':
        d['X'] = rn(B, N, N, D)
    elif op == 'OUT_EDGES':
        d['X'] = rn(B, N, N, ch)
    elif op == 'SUMS':
        d['X'] = rn(B, N, N, Fw)
    elif op in ('GINE', 'GINE_BWD'):
        d['EPS'] = torch.tensor([0.1])
        d['HS'], d['HE'] = rn(B, N, D) * nm[..., None], rn(B, N, N, D) * em[..., None]
        d['ADJ'] = (rn(B, N, N) >= 0).float() * em
        pre = d['HS'][:, :, None, :] + d['HE']                                      # ReLU arguments within 1e-3 of the kink are moved off it
        d['HE'] = torch.where((pre.abs() < 1e-3) & (em[..., None] > 0), d['HE'] + torch.where(pre >= 0, 2e-3, -2e-3), d['HE'])
        if op == 'GINE_BWD':
            d['DAGG'] = rn(B, N, D)
    elif op == 'GN_FWD':
        d['H'], d['A'], d['GAMMA'], d['BETA'] = rn(B, N, D), rn(B, N, D), 1 + 0.5 * rn(D), rn(D)
        d['Y'] = rn(B, N, D)                                                        # read when acc = 1
        if hard:
            d['H'][:, :, 0:8] = 0.375                                               # a group of eight equal channels: xhat exactly 0
            d['A'][:, :, 0:8] = 0.0
            d['H'][:, :, 8:16] = 1e3 + 1e-2 * rn(B, N, 8)                           # a group with mean 1e3 and spread 1e-2
            d['A'][:, :, 8:16] = 1e-3 * rn(B, N, 8)
    elif op == 'GN_BWD':
        x = rn(B, N, D)
        if hard:
            x[:, :, 0:8] = 0.375
            x[:, :, 8:16] = 1e3 + 1e-2 * rn(B, N, 8)
        xhat, rstd = group_norm_rows(x.double())                                    # the float64 statistics of that x, rounded: what the forward keeps
        d['XHAT'], d['RSTD'], d['GAMMA'], d['DY'], d['DX'] = xhat.float(), rstd.float(), 1 + 0.5 * rn(D), rn(B, N, D), rn(B, N, D)
    elif op == 'EGN_FWD':
        d['XHAT'], d['GAMMA'], d['BETA'] = _tile_values(B, N, D, g, hard, n_nodes), 1 + 0.5 * rn(D), rn(D)
    elif op == 'EGN_BWD':
        xhat, rstd = group_norm_tile(_tile_values(B, N, D, g, hard, n_nodes).double())
        d['XHAT'], d['RSTD'], d['GAMMA'] = xhat.float(), rstd.float(), 1 + 0.5 * rn(D)
        d['DY'] = torch.where(em[..., None] > 0, rn(B, N, N, D), 1e4 * rn(B, N, N, D))      # garbage on the padded rows: ignored
    elif op in ('ATTN_FWD', 'ATTN_BWD'):
        d['Q'], d['K'], d['V'] = rn(B, N, D), rn(B, N, D), rn(B, N, D)
        d['G0'], d['G1'] = torch.tanh(rn(B, N, N, D)), torch.tanh(rn(B, N, N, D))
        if hard:                                                                    # |logit| up to about 60; head 0: all logits equal
            d['Q'], d['K'] = d['Q'] * 5.0, d['K'] * 5.0
            d['G0'] = torch.tanh(2.0 * rn(B, N, N, D))
            d['Q'][:, :, :D // H] = 0.0
        if op == 'ATTN_BWD':
            al = restate('ATTN_FWD', d, torch.float64)['ALPHA']
            d['ALPHA'], d['DATT'] = al.float(), rn(B, N, D)
    else:
        raise KeyError(op)
    return d


def relu_margin(d):
    """GINE_BWD: the smallest |hs_j + he_ji| over the adjacent pairs in float64"""
    pre = (d['HS'].double()[:, :, None, :] + d['HE'].double()).abs()
    live = d['ADJ'] > 0
    return float(pre[live].min()) if bool(live.any()) else float('inf')


def conditioned(op, n_nodes, N, seed0, hard=None, **kw):
    """inputs() at the first seed >= seed0 at which the comparison is decided: the ReLU margin of GINE_BWD, the walk decisions of RW, the
    sharpness of the hard softmax sets.  The yardstick alone decides (see the host test for the same conditions asserted)."""
    for seed in range(seed0, seed0 + 64):
        d = inputs(op, n_nodes, N, seed, hard, **kw)
        if condition_holds(op, d, hard):
            d['seed'] = seed
            return d
    raise AssertionError("no seed in %d .. %d conditions %s" % (seed0, seed0 + 63, op))


def rw_decided(d):
    p64, p32 = [], []
    rw_restate(d['EDGE_X'], d['n_nodes'], d['N'], d['depth'], torch.float64, p64)
    rw_restate(d['EDGE_X'], d['n_nodes'], d['N'], d['depth'], torch.float32, p32)
    for a, b in zip(p64, p32):
        if bool(((a <= 0) != (b <= 0)).any()) or (bool((a > 0).any()) and float(a[a > 0].min()) <= 1e-30):
            return False
    return True


def sharp_heads(d):
    """per head 1 .. H - 1 (head 0 has equal logits): the float64 alpha has an entry above 0.999 and a real pair below 1e-20"""
    _, em = masks(d['n_nodes'], d['N'])
    al = restate('ATTN_FWD', d, torch.float64)['ALPHA']
    live = em[..., None] > 0
    hi = (al > 0.999).flatten(0, 2).any(0)
    lo = ((al < 1e-20) & live).flatten(0, 2).any(0)
    return bool(hi[1:].all()) and bool(lo[1:].all())


def condition_holds(op, d, hard):
    if op == 'GINE_BWD':
        return relu_margin(d) > RELU_MARGIN
    if op == 'RW':
        return rw_decided(d)
    if op in ('ATTN_FWD', 'ATTN_BWD') and hard and max(d['n_nodes']) >= 9:
        return sharp_heads(d)
    return True


def norm_grads_geometry(rows, mode):
    """(n_nodes, N) of a real tile with at least `rows` rows of the mode's kind: molecules of 5, 12, 9, 7 atoms in turn at N = 12"""
    per = 12 if mode == 1 else 144
    B = (rows + per - 1) // per
    return [(5, 12, 9, 7)[b % 4] for b in range(B)], 12


def single_rows(rows, mode, n_nodes, N):
    """the rows on which the one-row cases put their only non-zero dy: the last live row, the first live row of the second group of 32
    chunks, a live row of the ragged last chunk (where they exist)"""
    live = torch.nonzero(live_rows(dict(n_nodes=n_nodes, N=N, mode=mode), rows, torch.float64) > 0).reshape(-1).tolist()
    if not live:
        return []
    out = {live[-1]}
    second = [r for r in live if r >= 2048]
    if second:
        out.add(second[0])
    tail = [r for r in live if r >= (rows - 1) // 64 * 64]
    if tail:
        out.add(tail[0])
    return sorted(out)


# ---- the call ---------------------------------------------------------------------------------------------------------------------------
class Buf:
    """A float32 array between two guard bands on `device`.  init: a tensor (the contents before every call) or a shape (NaN)."""

    def __init__(self, init, device):
        self.init = init.detach().to(torch.float32).contiguous() if isinstance(init, torch.Tensor) else torch.full(tuple(init), float('nan'))
        n = self.init.numel()
        self.full = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=device)
        self.view = self.full[GUARD:GUARD + n].view(torch.float32).view(self.init.shape)
        self.reset()

    def reset(self):
        self.view.copy_(self.init)

    def guards_ok(self):
        n = self.init.numel()
        return bool((self.full[:GUARD] == PATTERN).all()) and bool((self.full[GUARD + n:] == PATTERN).all())

    def bits(self):
        return self.view.detach().cpu().contiguous().view(torch.int32).clone()


def out_shapes(op, d):
    B, N, K, ch, Fw = len(d['n_nodes']), d['N'], d['depth'], d['ch'], d['F']
    G = D // GW
    node, tile = (B, N, D), (B, N, N, D)
    return {
        'RW': dict(ADJ=(B, N, N), AD=(B, N, N), CNT=(B, N, N), ONEHOT=(B, N, N, K + 1), LAND=(B, N, K), DEG=(B, N, ch), PA=(B, N, N), PB=(B, N, N)),
        'PAIR': dict(Y=tile), 'PAIR_BWD': dict(Y=node), 'SUMS': dict(Y=(B, N, Fw), Z=(B, Fw)),
        'GINE': dict(AGG=node), 'GINE_BWD': dict(DHE=tile, DHS=node),
        'GN_FWD': dict(XHAT=node, RSTD=(B, N, G)), 'NORM_GRADS': dict(DBETA=(Fw,), DGAMMA=(Fw,)),
        'EGN_FWD': dict(RSTD=(B, G), Y=tile, PART=(4 * B * N * G,), GSUM=(4 * B * G,)),
        'EGN_BWD': dict(DX=tile, PART=(4 * B * N * G,), GSUM=(4 * B * G,)),
        'ATTN_FWD': dict(ALPHA=(B, N, N, H), ATT=node),
        'ATTN_BWD': dict(DV=node, DAL=(B, N, N, H), DT1=tile, DT0=tile, DQ=node, DK=node),
    }.get(op, {})


class Harness:
    """library: a ctypes handle with jodo_cdgs_train_debug_op (None: libjodo_hip.so through jodo_amd.capi); device: where the arrays live"""

    def __init__(self, device, library=None):
        self.device, self.library = device, library
        self.ratios = {}

    def sync(self):
        if self.device != 'cpu':
            torch.cuda.synchronize()

    def case(self, op, d):
        return Case(self, op, d)


class Case:
    def __init__(self, hs, op, d):
        self.hs, self.op, self.d = hs, op, d
        spec = OPS[op]
        dev = hs.device
        shapes = out_shapes(op, d)
        self.ins = {k: Buf(d[k], dev) for k in spec['ins']}
        self.outs = {}
        for k in spec['outs']:
            # an output the op also reads (accumulation, in place) starts from the case's values, the others from NaN
            read = k in spec.get('inout', ()) or op == 'RELU_BWD' or (d['acc'] and k in ('Y', 'DX') and op in ('SCALE', 'GN_FWD', 'GN_BWD'))
            shape = shapes[k] if k in shapes else tuple(d[k].shape) if k in d else tuple(d['X'].shape)
            self.outs[k] = Buf(d[k] if read else shape, dev)
        self.scratch = {}
        for k in spec.get('scratch', ()):
            n = shapes[k] if k in shapes else None
            if op == 'NORM_GRADS':
                rows = d['DY'].shape[0]
                nchunk = (rows + 63) // 64
                n = (4 * (nchunk + nchunk // 32 + 1) * d['F'],)
            self.scratch[k] = Buf(n, dev)
        self.nn = torch.full((len(d['n_nodes']) + 2 * 4,), -1, dtype=torch.int32, device=dev)
        self.bufs = list(self.ins.values()) + list(self.outs.values()) + list(self.scratch.values())

    def call(self, op_index=None, n_nodes=None, override=None, **scalars):
        """-> (return code, error text).  override: slot -> (tensor view or None for NULL, element count or None for the array's own)"""
        from jodo_amd import capi as c
        a = c.CdgsOpTestArgs()
        d = dict(self.d)
        d.update(scalars)
        n = np.ascontiguousarray(d['n_nodes'] if n_nodes is None else n_nodes, dtype=np.int32)
        a.op = c.CT_OPS.index('OP_' + self.op) if op_index is None else op_index
        a.B, a.N, a.n_nodes = len(n), d['N'], n.ctypes.data
        for k in SCALARS:
            setattr(a, k, d[k])
        a.D, a.H, a.K = d['width'], d['heads'], d['depth']               # (D, H and K name arrays in `d`)
        a.nn_dev, a.nn_dev_count = self.nn[4:].data_ptr(), self.nn.numel() - 8
        slots = dict(self.ins)
        slots.update(self.scratch)
        slots.update(self.outs)
        for name, b in slots.items():
            i = c.CT_SLOTS.index(name)
            a.a[i], a.n[i] = b.view.data_ptr(), b.view.numel()
        for name, (view, cnt) in (override or {}).items():
            i = c.CT_SLOTS.index(name)
            if view is None and cnt is None:
                a.a[i] = None
            else:
                a.a[i] = slots[name].view.data_ptr() if view is None else view.data_ptr()
                a.n[i] = slots[name].view.numel() if cnt is None else cnt
        stream = ctypes.c_void_p(0) if self.hs.device == 'cpu' else ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = c.cdgs_debug_op(a, stream, self.hs.library)
        self.hs.sync()
        L = c.lib() if self.hs.library is None else self.hs.library
        L.jodo_last_error.restype = ctypes.c_char_p
        msg = L.jodo_last_error()
        return rc, (msg.decode() if msg else '')

    def intact(self, what):
        assert all(b.guards_ok() for b in self.bufs), "%s: a guard band was written" % what
        assert bool((self.nn[:4] == -1).all()) and bool((self.nn[4 + len(self.d['n_nodes']):] == -1).all()), "%s: the counts overran their scratch" % what
        for k, b in self.ins.items():
            assert torch.equal(b.bits(), b.init.view(torch.int32)), "%s: the input %s was modified" % (what, k)

    def run(self, what=''):
        """the op, twice: -> slot -> stored array (CPU, dense shape)"""
        what = what or self.op
        for b in list(self.outs.values()) + list(self.scratch.values()):
            b.reset()
        rc, msg = self.call()
        assert rc == 0, "%s: %s" % (what, msg)
        got = {k: b.view.detach().cpu().clone() for k, b in self.outs.items()}
        first = {k: b.bits() for k, b in self.outs.items()}
        self.intact(what)
        for k, v in got.items():
            assert not bool(torch.isnan(v).any()), "%s: %s has elements the kernel never wrote (or NaN)" % (what, k)
        for b in list(self.outs.values()) + list(self.scratch.values()):
            b.reset()
        rc, msg = self.call()
        assert rc == 0, "%s (second run): %s" % (what, msg)
        for k, b in self.outs.items():
            assert torch.equal(b.bits(), first[k]), "%s: %s differs between two runs" % (what, k)
        self.intact(what + ' (second run)')
        return got


def is_zero(t):
    return bool(((t.contiguous().view(torch.int32) & 0x7FFFFFFF) == 0).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def compare(hs, label, op, got, r32, r64):
    """every element of every stored array; -> the worst err / bound of the call (also kept per op in hs.ratios)"""
    worst = 0.0
    for k, rule in OPS[op]['outs'].items():
        g, a, b = got[k], r32[k], r64[k]
        assert tuple(g.shape) == tuple(b.shape), (label, k, g.shape, b.shape)
        if rule == 'exact':
            assert torch.equal(g.double(), b), "%s: %s is not exactly the restatement" % (label, k)
            continue
        err, e32 = (g.double() - b).abs(), float((a.double() - b).abs().max()) if b.numel() else 0.0
        if rule == 'fwd':
            stated = FWD_ATOL + FWD_RTOL * b.abs()
            ratio = float((err / torch.clamp(stated, min=K64 * e32)).max()) if b.numel() else 0.0
            widened = bool((err > stated).any())
            print("  %-28s %-7s fwd  err %.2e  float32 restatement %.2e  err / bound %.3f%s" % (label, k, float(err.max()), e32, ratio,
                                                                                                   '  (widened bound active)' if widened else ''))
            close64(g, a, b, what='%s %s' % (label, k))
        else:
            base = GRAD_REL * max(float(b.abs().max()), 1e-12)
            ratio = float(err.max()) / max(base, K32 * e32)
            widened = float(err.max()) > base
            print("  %-28s %-7s bwd  err %.2e  float32 restatement %.2e  err / bound %.3f%s" % (label, k, float(err.max()), e32, ratio,
                                                                                                   '  (widened bound active)' if widened else ''))
            compare_grads([(k, g)], {k: b}, want32={k: a}, what='%s %s' % (label, k))
        worst = max(worst, ratio)
        hs.ratios[op] = max(hs.ratios.get(op, 0.0), ratio)
        if widened:
            hs.ratios[op + ' widened'] = max(hs.ratios.get(op + ' widened', 0.0), ratio)
    return worst


def check_exact_parts(op, d, got):
    """what is exactly representable: masked zeros, padded rows, the diagonal"""
    n_nodes, N = d['n_nodes'], d['N']
    nm, em = masks(n_nodes, N, torch.float32)
    dead_n, dead_e = nm[..., None] == 0, em[..., None] == 0
    z = lambda t, m: is_zero(t[m.expand_as(t)])
    if op == 'ADDT' or (op == 'SCALE' and d['mode'] and not d['acc']):
        live = live_rows(d, got['Y'].shape[0], torch.float32)
        assert is_zero(got['Y'][live == 0]), op + ': a masked row is not exactly zero'
    if op == 'OUT_EDGES':
        assert z(got['Y'], dead_e) and same_bits(got['Y'], got['Y'].transpose(1, 2).contiguous())
    if op == 'GN_FWD' and not d['acc']:
        assert z(got['Y'], dead_n), 'GN_FWD: a padded row of y is not exactly zero'
    if op == 'EGN_FWD':
        assert z(got['Y'], dead_e), 'EGN_FWD: e_out off the real pairs is not exactly zero'
    if op == 'ATTN_FWD':
        assert z(got['ALPHA'], dead_e), 'ATTN_FWD: alpha off the real pairs is not exactly zero'
    if op == 'ATTN_BWD':
        assert z(got['DAL'], dead_e) and z(got['DT1'], dead_e) and z(got['DT0'], dead_e), 'ATTN_BWD: a gradient off the real pairs is not exactly zero'
    if op == 'GINE_BWD':
        assert z(got['DHE'], (d['ADJ'] == 0)[..., None]), 'GINE_BWD: d he off the adjacency is not exactly zero'


def run_and_compare(hs, op, d, label=None, r=None):
    """one case: the call (twice, guarded), every stored element against the restatement, the exact parts -> (case, got, r64)"""
    label = label or '%s N%d' % (op, d['N'])
    case = hs.case(op, d)
    got = case.run(label)
    r32, r64 = r if r is not None else (restate(op, d, torch.float32), restate(op, d, torch.float64))
    compare(hs, label, op, got, r32, r64)
    check_exact_parts(op, d, got)
    return case, got, r64


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
DROP_A = dict(drop_p=0.1, drop_seed=12345, drop_site=9)
DROP_B = dict(drop_p=0.5, drop_seed=SEED_HI, drop_site=14)
VARIANTS = {                                 # op -> [(tag, hard, options)]
    'RW': [(k, k, {}) for k in ('random', 'path', 'star', 'complete', 'empty', 'isolated')],
    'ADDT': [('nodes', None, dict(mode=1)), ('pairs', None, dict(mode=2, Fw=40))],
    'SCALE': [('all rows', None, dict(mode=0, Fw=24)), ('nodes acc drop .1', None, dict(mode=1, acc=1, **DROP_A)), ('pairs drop .5', None, dict(mode=2, **DROP_B))],
    'RELU': [('', None, {})], 'RELU_BWD': [('', None, {})], 'PAIR': [('', None, {})], 'PAIR_BWD': [('', None, {})],
    'OUT_NODES': [('', None, dict(Fw=5))], 'OUT_EDGES': [('', None, {})],
    'SUMS': [('all rows', None, dict(mode=0)), ('masked', None, dict(mode=1, Fw=40))],
    'GINE': [('', None, {})], 'GINE_BWD': [('', None, {})],
    'GN_FWD': [('benign', None, {}), ('amask acc drop .1', None, dict(amask=1, acc=1, **DROP_A)), ('hard amask drop .5', True, dict(amask=1, **DROP_B)),
               ('hard', True, {})],
    'GN_BWD': [('benign', None, {}), ('hard acc', True, dict(acc=1))],
    'EGN_FWD': [('benign', None, {}), ('constant', 'constant', {}), ('mean 1e3', 'mean', {})],
    'EGN_BWD': [('benign', None, {}), ('constant', 'constant', {}), ('mean 1e3', 'mean', {})],
    'ATTN_FWD': [('benign', None, {}), ('hard', True, {})],
    'ATTN_BWD': [('benign', None, {}), ('hard', True, {})],
}
TILED = [op for op in OPS if op != 'NORM_GRADS']
WIDE_OPS = ('ATTN_FWD', 'ATTN_BWD', 'GINE', 'GINE_BWD', 'EGN_FWD', 'EGN_BWD', 'PAIR', 'PAIR_BWD', 'SUMS', 'RW')


def case_seed(op, N, i):
    return 1000 * (list(OPS).index(op) + 1) + 10 * N + i


def run_variants(hs, op, n_nodes, N, variants=None):
    """every variant of `op` at one tile width -> [(tag, d, got, r64)]"""
    out = []
    for i, (tag, hard, kw) in enumerate(VARIANTS[op] if variants is None else variants):
        d = conditioned(op, n_nodes, N, case_seed(op, N, i), hard, **kw)
        _, got, r64 = run_and_compare(hs, op, d, '%s %s N%d' % (op, tag, N))
        if op == 'SCALE' and d['drop_p'] > 0 and not d['acc']:
            mult = multipliers(d, d['X'].shape, torch.float32) * live_rows(d, d['X'].shape[0], torch.float32)[:, None]
            ones = dict(d, X=torch.ones_like(d['X']))
            got1 = hs.case(op, ones).run('SCALE multipliers')['Y']
            assert same_bits(got1, mult), 'SCALE: the dropout multipliers are not philox_ref.drop_mul bit for bit'
        out.append((tag, d, got, r64))
    return out


def norm_grads_cases():
    """(rows, mode, one_row or None): dense dy, then dy non-zero on one live row only"""
    out = []
    for rows in COLSUM_ROWS + [COLSUM_GROUPS]:
        for mode in (1, 2):
            n_nodes, N = norm_grads_geometry(rows, mode)
            out.append((rows, mode, None))
            out.extend((rows, mode, r) for r in single_rows(rows, mode, n_nodes, N))
    return out


def run_norm_grads(hs, rows, mode, one_row):
    n_nodes, N = norm_grads_geometry(rows, mode)
    Fw = 256 if rows <= 2113 else 64
    d = inputs('NORM_GRADS', n_nodes, N, 77 + rows + mode, None, mode=mode, rows=rows, Fw=Fw, one_row=one_row)
    r32, r64 = restate('NORM_GRADS', d, torch.float32), restate('NORM_GRADS', d, torch.float64)
    if one_row is not None:                                  # the yardstick: that row alone carries the whole sum, at full size
        assert float(live_rows(d, rows, torch.float64)[one_row]) == 1.0
        assert torch.equal(r64['DBETA'], d['DY'][one_row].double()) and float(r64['DBETA'].abs().max()) > 1.0
    return run_and_compare(hs, 'NORM_GRADS', d, 'NORM_GRADS rows %d mode %d%s' % (rows, mode, '' if one_row is None else ' row %d' % one_row), (r32, r64))


def molecule_alone(hs, op, n_nodes, N, seed):
    """every molecule alone gives the bits of its rows in the batch"""
    d = conditioned(op, n_nodes, N, seed)
    base = hs.case(op, d).run(op + ' batch')
    for b, n in enumerate(n_nodes):
        one = {k: (v[b:b + 1].contiguous() if isinstance(v, torch.Tensor) and v.dim() >= 2 and v.shape[0] == len(n_nodes) and k not in ('GAMMA', 'BETA') else v)
               for k, v in d.items()}
        one['n_nodes'] = [n]
        got = hs.case(op, one).run('%s molecule %d alone' % (op, b))
        for k, v in got.items():
            assert same_bits(v, base[k][b:b + 1]), "%s: %s of molecule %d (n = %d) alone differs from the batch" % (op, k, b, n)


ARG, UNSUPPORTED = -1, -3


def refusals(hs):
    """No kernel runs: every call comes back with an error code and every poisoned output keeps its NaN."""
    d = inputs('ATTN_BWD', [3, 4], 4, 3)
    case = hs.case('ATTN_BWD', d)
    before = {k: b.bits() for k, b in case.outs.items()}
    R, M = 2 * 16, 2 * 4
    rc, msg = case.call(op_index=len(OPS))
    assert rc == ARG and 'unknown op' in msg, msg
    rc, msg = case.call(op_index=-1)
    assert rc == ARG and 'unknown op' in msg, msg
    rc, msg = case.call(n_nodes=[3, 0])
    assert rc == ARG and 'n_nodes[1] = 0' in msg, msg
    rc, msg = case.call(n_nodes=[5, 4])
    assert rc == ARG and 'n_nodes[0] = 5' in msg, msg
    rc, msg = case.call(n_nodes=[3, 4, 1])                   # other counts than the arrays were made for
    assert rc == ARG and 'elements, the op touches' in msg, msg
    rc, msg = case.call(override=dict(DT0=(None, R * D - 1)))
    assert rc == ARG and 'array dt0 has %d elements, the op touches %d' % (R * D - 1, R * D) in msg, msg
    rc, msg = case.call(override=dict(Q=(None, M * D + 1)))
    assert rc == ARG and 'array q has' in msg, msg
    rc, msg = case.call(override=dict(DATT=(case.ins['DATT'].view.view(-1)[1:], M * D)))
    assert rc == ARG and 'array datt is not 16-byte aligned' in msg, msg
    rc, msg = case.call(override=dict(DV=(None, None)))
    assert rc == ARG and 'array dv is a null pointer' in msg, msg
    rc, msg = case.call(width=260)
    assert rc == ARG and 'D 260' in msg, msg
    rc, msg = case.call(heads=7)
    assert rc == ARG and 'H 7' in msg, msg
    rc, msg = case.call(depth=0)
    assert rc == ARG, msg
    rc, msg = case.call(ch=1)
    assert rc == ARG, msg
    rc, msg = case.call(mode=1)
    assert rc == ARG and 'mode 1' in msg, msg
    rc, msg = case.call(rows=3)
    assert rc == ARG and 'rows 3' in msg, msg
    rc, msg = case.call(drop_p=1.0)
    assert rc == ARG and 'dropout' in msg, msg
    hs.sync()
    for k, b in case.outs.items():
        assert torch.equal(b.bits(), before[k]) and bool(torch.isnan(b.view).all()), k
    case.intact('refusals')
    # the double scratch of the sums, by the engine's sizing rule: one float short is refused
    n_nodes, N = norm_grads_geometry(2049, 2)
    d = inputs('NORM_GRADS', n_nodes, N, 5, None, mode=2, rows=2049, Fw=8)
    case = hs.case('NORM_GRADS', d)
    need = 4 * (33 + 1 + 1) * 8
    assert case.scratch['PART'].view.numel() == need
    rc, msg = case.call(override=dict(PART=(None, need - 1)))
    assert rc == ARG and 'array part has %d elements, the op touches %d' % (need - 1, need) in msg, msg
    rc, msg = case.call(rows=15 * 144 + 1)
    assert rc == ARG and 'rows' in msg, msg
    assert all(bool(torch.isnan(b.view).all()) for b in case.outs.values())
    d = inputs('EGN_FWD', [3, 4], 4, 3)
    case = hs.case('EGN_FWD', d)
    rc, msg = case.call(override=dict(GSUM=(None, 4 * 2 * 32 - 1)))
    assert rc == ARG and 'array gsum' in msg, msg
    assert bool(torch.isnan(case.outs['Y'].view).all()) and same_bits(case.outs['XHAT'].view.cpu(), d['XHAT'])

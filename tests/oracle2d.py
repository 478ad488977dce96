"""Dense CPU evaluation of the 2-D score network (DGT_concat_2D) on a flat state_dict.

Written from the block formulas (DESIGN.md, section "2-D model"), not from the sparse message-passing code: every
per-edge quantity lives in a dense [B, N, N, .] tensor indexed [b, r, c] like the edge input, and the attention of
target node c runs over the sources r of column c:

    score[b, r, c, 0]     = adjacency head: 1 where cond_edge_x[b, r, c, 0] >= edge_quan_th (all ones on the first step), else -1e10
    score[b, r, c, 1 + s] = sum_u q[b, c, s, u] k[b, r, s, u] tanh(W_e0 e~[b, r, c])[s, u] / sqrt(16)        (15 heads of 17 channels)
    hn[b, c, h, :]        = sum_r softmax_r(score)[b, r, c, h] * v[b, r, h, :] * tanh(W_e1 e~[b, r, c])[h, :]   (16 heads of 16 channels)

Works in float32 or float64 (the dtype of the tensors handed in).  Imports nothing outside torch.
"""
import math

import torch
from torch.nn import functional as F


class Hyper2D:
    def __init__(self, nf, n_layers, n_heads, n_extra, mlp_ratio, in_node_dim, edge_ch, edge_th):
        self.D, self.L, self.H, self.XH, self.r = nf, n_layers, n_heads, n_extra, mlp_ratio
        self.De = nf // 4
        self.nd, self.ch, self.edge_th = in_node_dim, edge_ch, float(edge_th)
        self.C = nf // n_heads
        self.SH = n_heads - n_extra
        self.SC = (n_heads * self.C) // self.SH

    @classmethod
    def from_config(cls, cfg):
        m = cfg.model
        return cls(m.nf, m.n_layers, m.n_heads, m.n_extra_heads, m.mlp_ratio, cfg.data.atom_types + int(m.include_fc_charge),
                   m.edge_ch, m.edge_quan_th)


def _lin(p, name, x):
    b = p.get(name + '.bias')
    return F.linear(x, p[name + '.weight'], b)


def _ln(x):
    return F.layer_norm(x, x.shape[-1:], eps=1e-6)


def _mod(x, shift, scale):
    return x * (1 + scale) + shift


def _mlp3(p, name, x):
    return _lin(p, name + '.4', F.silu(_lin(p, name + '.2', F.silu(_lin(p, name + '.0', x)))))


def forward_dense(sd, hp, xh, node_mask, edge_mask, edge_x, cond_x=None, cond_edge_x=None, noise_level=None, return_blocks=False):
    """-> (atom_pred [B,N,nd], edge_pred [B,N,N,ch]) and, with return_blocks, a list of (h [B,N,D], e [B,N,N,De]) after every
    block (rows / pairs outside the masks are zeroed in the returned copies)."""
    dt = xh.dtype
    p = {(k[7:] if k.startswith('module.') else k): v.to(dt) for k, v in sd.items()}
    B, N, _ = xh.shape
    nm = node_mask.reshape(B, N, 1).to(dt)
    em = edge_mask.reshape(B, N, N, 1).to(dt)
    valid = em[..., 0] > 0
    if cond_x is None:
        cond_x, cond_edge_x = torch.zeros_like(xh), torch.zeros_like(edge_x)
        adj = torch.ones(B, N, N, dtype=dt, device=xh.device)
    else:
        adj = (cond_edge_x[..., 0] >= hp.edge_th).to(dt)
    adj_score = torch.where(adj == 0, torch.full_like(adj, -1e10), adj)

    x = noise_level.to(dt).unsqueeze(-1)
    fr = x * p['time_mlp.0.weights'].unsqueeze(0) * 2 * math.pi
    temb = _lin(p, 'time_mlp.3', F.gelu(_lin(p, 'time_mlp.1', torch.cat([x, fr.sin(), fr.cos()], dim=-1))))     # [B, T]
    st = F.silu(temb)

    h = _lin(p, 'node_emb', torch.cat([xh, cond_x.to(dt)], dim=-1))
    e = _lin(p, 'edge_emb', torch.cat([edge_x, cond_edge_x.to(dt)], dim=-1))
    atom_hids, edge_hids, blocks = [h], [e], []
    H, C, SH, SC = hp.H, hp.C, hp.SH, hp.SC
    for l in range(hp.L):
        pre = 'e_block_%d.' % l
        nmod = _lin(p, pre + 'node_time_mlp.1', st).unsqueeze(1).chunk(6, dim=-1)                  # each [B,1,D]
        emod = _lin(p, pre + 'edge_time_mlp.1', st).reshape(B, 1, 1, -1).chunk(6, dim=-1)          # each [B,1,1,De]
        hm = _mod(_ln(h), nmod[0], nmod[1])
        et = _mod(_ln(e), emod[0], emod[1])
        q = _lin(p, pre + 'attn_mpnn.lin_query', hm).reshape(B, N, SH, SC)
        k = _lin(p, pre + 'attn_mpnn.lin_key', hm).reshape(B, N, SH, SC)
        v = _lin(p, pre + 'attn_mpnn.lin_value', hm).reshape(B, N, H, C)
        t0 = torch.tanh(_lin(p, pre + 'attn_mpnn.lin_edge0', et)).reshape(B, N, N, SH, SC)
        t1 = torch.tanh(_lin(p, pre + 'attn_mpnn.lin_edge1', et)).reshape(B, N, N, H, C)
        # [b, r, c]: target c (query), source r (key / value)
        sc = (q.unsqueeze(1) * k.unsqueeze(2) * t0).sum(-1) / math.sqrt(C)                         # [B,N,N,SH]
        sc = torch.cat([adj_score.unsqueeze(-1), sc], dim=-1)                                      # [B,N,N,H]
        sc = sc.masked_fill(~valid.unsqueeze(-1), float('-inf'))
        mx = sc.max(dim=1, keepdim=True).values
        mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
        w = torch.exp(sc - mx)
        alpha = w / (w.sum(dim=1, keepdim=True) + 1e-16)
        hn = (alpha.unsqueeze(-1) * v.unsqueeze(2) * t1).sum(1).reshape(B, N, H * C)               # [B, N(c), D]

        u = _lin(p, pre + 'node2edge_lin', hn.unsqueeze(1) + hn.unsqueeze(2))
        hx = h + nmod[2] * hn
        hx = _mod(_ln(hx), nmod[3], nmod[4]) * nm
        h = (hx + nmod[5] * _lin(p, pre + 'ff_linear2', F.silu(_lin(p, pre + 'ff_linear1', hx)))) * nm
        e1 = e + emod[2] * u
        e2 = _mod(_ln(e1), emod[3], emod[4])
        e = e2 + emod[5] * _lin(p, pre + 'ff_linear4', F.silu(_lin(p, pre + 'ff_linear3', e2)))
        atom_hids.append(_lin(p, 'node_%d' % l, h))
        edge_hids.append(_lin(p, 'edge_%d' % l, e))
        if return_blocks:
            blocks.append((h * nm, e * em))
    ah = torch.cat(atom_hids, dim=-1)
    eh = torch.cat(edge_hids, dim=-1)
    atom_pred = _mlp3(p, 'node_pred_mlp', ah) * nm
    ep = torch.cat([_mlp3(p, 'edge_exist_mlp', eh), _mlp3(p, 'edge_type_mlp', eh)], dim=-1) * em
    ep = 0.5 * (ep + ep.transpose(1, 2))
    if return_blocks:
        return atom_pred, ep, blocks
    return atom_pred, ep


class OracleModel2D:
    """CPU stand-in with the score-network call signature, backed by forward_dense (checker only)."""

    def __init__(self, sd, hp, dtype=torch.float32):
        self.sd, self.hp, self.dtype = sd, hp, dtype

    def eval(self):
        return self

    def __call__(self, t, xh, node_mask, edge_mask, context=None, **kw):
        c = lambda v: None if v is None else v.to(self.dtype)
        with torch.no_grad():
            ox, oe = forward_dense(self.sd, self.hp, c(xh), node_mask, edge_mask, c(kw['edge_x']), c(kw.get('cond_x')),
                                   c(kw.get('cond_edge_x')), c(kw['noise_level']))
        return ox.to(xh.dtype), oe.to(xh.dtype)


def load_n_nodes_hist(path, name):
    """tests/golden/n_nodes_2d.json -> {'train_n_nodes': {n: count}} in ascending n (the order the reference's table has)."""
    import json
    with open(path) as f:
        raw = json.load(f)[name]
    return {'train_n_nodes': {int(k): int(raw[k]) for k in sorted(raw, key=int)}, 'max_n_nodes': max(int(k) for k in raw)}


def decode_agrees(fx, atom_type, fc, edge_type, n_nodes, margin=1e-3):
    """Compare decodes with a traj2d / samplefn2d fixture wherever every recorded decision margin of the entry exceeds `margin`.
    Returns (number of mismatches, share of real entries excluded)."""
    import numpy as np
    B, N = fx['atom_type'].shape
    node_real = np.arange(N)[None, :] < np.asarray(n_nodes)[:, None]
    edge_real = node_real[:, :, None] & node_real[:, None, :] & ~np.eye(N, dtype=bool)[None]
    ok_atom = node_real & (fx['margin_atom'] > margin)
    bad = int((np.asarray(atom_type)[ok_atom] != fx['atom_type'][ok_atom]).sum())
    excluded, total = int((node_real & ~ok_atom).sum()), int(node_real.sum())
    if 'margin_charge' in fx:
        ok_fc = node_real & (fx['margin_charge'] > margin)
        bad += int((np.asarray(fc)[..., 0][ok_fc] != fx['fc'][..., 0][ok_fc]).sum())
        excluded += int((node_real & ~ok_fc).sum()); total += int(node_real.sum())
    ok_e = edge_real & (fx['margin_exist'] > margin) & (fx['margin_order'] > margin)
    if 'margin_aromatic' in fx:
        ok_e &= fx['margin_aromatic'] > margin
    bad += int((np.asarray(edge_type)[ok_e] != fx['edge_type'][ok_e]).sum())
    excluded += int((edge_real & ~ok_e).sum()); total += int(edge_real.sum())
    return bad, excluded / max(total, 1)

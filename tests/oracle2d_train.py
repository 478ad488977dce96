"""The dense 2-D oracle (tests/oracle2d.py) with training-mode dropout: the same block formulas with the four FFN mask multiplies.

Checker only.  The masks are restated by oracle/philox_ref.dropout_masks (the training kernels' counter-based generator and their
element numbering: node rows, and rows of the dense n x n tile with the diagonal carried); padded entries get a multiplier of 1.
tests/test_train2d_emul.py asserts torch.equal with oracle2d.forward_dense when drop is None.
"""
import math

import torch
from torch.nn import functional as F

from oracle2d import Hyper2D, _lin, _ln, _mod, _mlp3          # noqa: F401


def _dense_masks(drop, l, B, N, dt, device):
    """masks[b][l][site] ([n, .] / [n, n, .] numpy) -> padded [B, N, .] / [B, N, N, .] tensors, ones on padding."""
    out = {}
    for site in ('A1', 'F2', 'A3', 'F4'):
        w = drop[0][l][site].shape[-1]
        full = torch.ones((B, N, w) if site in ('A1', 'F2') else (B, N, N, w), dtype=dt, device=device)
        for b in range(B):
            m = torch.as_tensor(drop[b][l][site]).to(dt).to(device)
            n = m.shape[0]
            if site in ('A1', 'F2'):
                full[b, :n] = m
            else:
                full[b, :n, :n] = m
        out[site] = full
    return out


def forward_dense_drop(sd, hp, xh, node_mask, edge_mask, edge_x, cond_x=None, cond_edge_x=None, noise_level=None, return_blocks=False, drop=None):
    """oracle2d.forward_dense with the four dropout multiplies of EquivariantMixBlock_2D._ff_block_node / _ff_block_edge
    (mol_gnn.py:364-370).  drop: None (identity: the same operations as forward_dense, bit for bit) or the per-molecule, per-block masks
    of oracle/philox_ref.dropout_masks."""
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
        dm = None if drop is None else _dense_masks(drop, l, B, N, dt, xh.device)
        a1 = F.silu(_lin(p, pre + 'ff_linear1', hx))
        f2 = _lin(p, pre + 'ff_linear2', a1 if dm is None else a1 * dm['A1'])
        h = (hx + nmod[5] * (f2 if dm is None else f2 * dm['F2'])) * nm
        e1 = e + emod[2] * u
        e2 = _mod(_ln(e1), emod[3], emod[4])
        a3 = F.silu(_lin(p, pre + 'ff_linear3', e2))
        f4 = _lin(p, pre + 'ff_linear4', a3 if dm is None else a3 * dm['A3'])
        e = e2 + emod[5] * (f4 if dm is None else f4 * dm['F4'])
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

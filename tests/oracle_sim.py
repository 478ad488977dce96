"""CPU oracle of DGT_concat_sim, the 3-D score network WITHOUT extra attention heads.  TEST INFRASTRUCTURE ONLY.

A dense per-molecule restatement in plain PyTorch (float32 or float64, by the dtype of its inputs and state_dict) of what the
reference's class computes in one call.  The top level and the block body are those of DGT_concat (oracle/dgt_oracle.forward_dense):
self-conditioned concatenation, distances from the self-conditioning positions with the batch-global first-step switch, edge_emb,
LN1 + modulate, node2edge sum, gates, both feed-forwards, norm2, Gaussian distances from the current positions, per-block readouts,
three heads, symmetrisation, centre-of-mass removal, NaN guard.  Two things differ:

  * attention (Trans_Layer): 16 learned heads of C = nf / 16 channels; lin_query / lin_key nf -> nf, lin_edge0 nf / 4 -> nf without
    bias; score = sum_ch q_c k_a tanh(lin_edge0 et) / sqrt(C); softmax per target and head over the real incoming edges — no adjacency
    heads, no -1e10; message v_a * tanh(lin_edge1 et) * alpha;
  * coordinate update (CondEquiUpdate): coord_mlp.2 is Linear(nf, 1, bias=False) and iota = tanh(.) as it is — no adjacency
    weighting, no mean over three heads.

There is no extra adjacency: n_extra_heads, trans_name, softmax_inf and edge_quan_th are never read and spatial_cut_off has no effect.
tools/make_golden_sim.py asserts this file against the reference within 1e-5 while it writes the fixtures.

Index convention inside one molecule: tensors are [a, c, ...] with a = row = source, c = column = target; softmax and aggregation
run over a, the position update sums over c.
"""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle.dgt_oracle import _gbf, _lin, _ln, _mlp3, time_embedding


@dataclass
class HyperSim:
    nf: int = 256
    n_layers: int = 8
    n_heads: int = 16
    mlp_ratio: int = 2
    in_node_dim: int = 6
    edge_ch: int = 2
    cond_ch: int = 0              # (time_embedding reads it: there is no conditional variant)

    @staticmethod
    def from_config(config):
        m = config.model
        return HyperSim(nf=m.nf, n_layers=m.n_layers, n_heads=m.n_heads, mlp_ratio=m.mlp_ratio,
                        in_node_dim=config.data.atom_types + int(m.include_fc_charge), edge_ch=m.edge_ch)

    @property
    def de(self):
        return self.nf // 4


def forward_dense(p, hp, xh, node_mask, edge_mask, edge_x, cond_x=None, cond_edge_x=None, noise_level=None,
                  return_intermediates=False):
    bs, N, _ = xh.shape
    D, De, L, H = hp.nf, hp.de, hp.n_layers, hp.n_heads
    C = D // H
    dt = xh.dtype
    n_nodes = node_mask.reshape(bs, N).sum(1).long().tolist()
    has_cond = cond_x is not None
    tau = F.silu(time_embedding(p, hp, noise_level))
    first = True                                                  # batch-global: sum of squared self-conditioning distances == 0
    if has_cond:
        tot = 0.0
        for b in range(bs):
            cp = cond_x[b, :n_nodes[b], 0:3]
            tot = tot + ((cp[:, None, :] - cp[None, :, :]) ** 2).sum()
        first = bool(tot == 0)
    out_x = torch.zeros(bs, N, 3 + hp.in_node_dim, dtype=dt)
    out_e = torch.zeros(bs, N, N, hp.edge_ch, dtype=dt)
    inter, pos_all = [], []
    for b in range(bs):
        n = n_nodes[b]
        tb = tau[b:b + 1]
        x = xh[b, :n, 0:3].clone()
        feat, ex = xh[b, :n, 3:], edge_x[b, :n, :n]
        offd = ~torch.eye(n, dtype=torch.bool)
        if has_cond:
            cpos, cfeat, cex = cond_x[b, :n, 0:3], cond_x[b, :n, 3:], cond_edge_x[b, :n, :n]
        else:
            cpos, cfeat, cex = torch.zeros(n, 3, dtype=dt), torch.zeros_like(feat), torch.zeros_like(ex)
        d2c = ((cpos[:, None, :] - cpos[None, :, :]) ** 2).sum(-1, keepdim=True)
        G0 = torch.zeros(n, n, De, dtype=dt) if first else _gbf(p, 'dist_layer', d2c, tb)
        e = _lin(p, 'edge_emb', torch.cat([ex, cex, G0], dim=-1))
        h = _lin(p, 'node_emb', torch.cat([feat, cfeat], dim=-1))
        ah, eh, blocks = [h], [e], []
        negmask = torch.where(offd, 0.0, float('-inf')).to(dt)      # a == c is no edge
        for l in range(L):
            bk = 'e_block_%d' % l
            diff = x[:, None, :] - x[None, :, :]
            d2 = (diff ** 2).sum(-1, keepdim=True)
            G = _gbf(p, bk + '.dist_layer', d2, tb)
            ns1, nc1, ng1, ns2, nc2, ng2 = _lin(p, bk + '.node_time_mlp.1', tb).chunk(6, dim=1)
            es1, ec1, eg1, es2, ec2, eg2 = _lin(p, bk + '.edge_time_mlp.1', tb).chunk(6, dim=1)
            ht = _ln(h) * (1 + nc1) + ns1
            et = _ln(_lin(p, bk + '.edge_emb', torch.cat([G, e], dim=-1))) * (1 + ec1) + es1
            q = _lin(p, bk + '.attn_mpnn.lin_query', ht).reshape(n, H, C)
            k = _lin(p, bk + '.attn_mpnn.lin_key', ht).reshape(n, H, C)
            v = _lin(p, bk + '.attn_mpnn.lin_value', ht).reshape(n, H, C)
            t0 = torch.tanh(_lin(p, bk + '.attn_mpnn.lin_edge0', et, bias=False)).reshape(n, n, H, C)
            S = (q[None, :, :, :] * k[:, None, :, :] * t0).sum(-1) / math.sqrt(C)          # [a, c, H]
            if n > 1:
                Sm = S + negmask[..., None]
                ex_ = (Sm - Sm.max(dim=0, keepdim=True).values).exp()
                alpha = ex_ / (ex_.sum(0, keepdim=True) + 1e-16)
            else:
                alpha = torch.zeros_like(S)
            t1 = torch.tanh(_lin(p, bk + '.attn_mpnn.lin_edge1', et, bias=False)).reshape(n, n, H, C)
            hhat = (v[:, None, :, :] * t1 * alpha[..., None]).sum(0).reshape(n, D)
            n2e = F.linear(hhat, p[bk + '.node2edge_lin.weight'])
            ehat = n2e[:, None, :] + n2e[None, :, :] + p[bk + '.node2edge_lin.bias']
            hn = _ln(h + ng1 * hhat) * (1 + nc2) + ns2
            en = _ln(e + eg1 * ehat) * (1 + ec2) + es2
            h = hn + ng2 * _lin(p, bk + '.ff_linear2', F.silu(_lin(p, bk + '.ff_linear1', hn)))
            e = en + eg2 * _lin(p, bk + '.ff_linear4', F.silu(_lin(p, bk + '.ff_linear3', en)))
            W = p[bk + '.equi_update.input_lin.weight']
            Wr, Wc, We, Wd = W[:, :D], W[:, D:2 * D], W[:, 2 * D:2 * D + De], W[:, 2 * D + De:]
            pre = (F.linear(h, Wr)[:, None, :] + F.linear(h, Wc)[None, :, :] + F.linear(e, We) + F.linear(G, Wd)
                   + p[bk + '.equi_update.input_lin.bias'])
            sh, sc = _lin(p, bk + '.equi_update.time_mlp.1', tb).chunk(2, dim=1)
            u = _ln(pre) * (1 + sc) + sh
            iota = torch.tanh(F.linear(F.silu(_lin(p, bk + '.equi_update.coord_mlp.0', u)),
                                       p[bk + '.equi_update.coord_mlp.2.weight']))          # [a, c, 1]
            nrm = diff.norm(dim=-1, keepdim=True).clamp(min=1e-8)
            trans = diff / nrm * p[bk + '.equi_update.coord_norm.scale'] * iota * offd[..., None]
            x = x + trans.sum(1)
            x = x - x.mean(0, keepdim=True)
            ah.append(_lin(p, 'node_%d' % l, h))
            eh.append(_lin(p, 'edge_%d' % l, e))
            if return_intermediates:
                blocks.append(dict(h=h.clone(), e=e.clone(), pos=x.clone(), hhat=hhat.clone(), S=S.clone(), alpha=alpha.clone()))
        ehc = torch.cat(eh, dim=-1)
        Ep = torch.cat([_mlp3(p, 'edge_exist_mlp', ehc), _mlp3(p, 'edge_type_mlp', ehc)], dim=-1) * offd[..., None]
        out_e[b, :n, :n] = 0.5 * (Ep + Ep.transpose(0, 1))
        out_x[b, :n, 3:] = _mlp3(p, 'node_pred_mlp', torch.cat(ah, dim=-1))
        pos_all.append(x)
        inter.append(blocks)
    nan = any(bool(torch.isnan(x).any()) for x in pos_all)
    for b in range(bs):
        x = torch.zeros_like(pos_all[b]) if nan else pos_all[b]
        out_x[b, :n_nodes[b], 0:3] = x - x.mean(0, keepdim=True)
    if return_intermediates:
        return out_x, out_e, inter
    return out_x, out_e

"""Shared by the training tests of DGT_concat_sim (tests/test_train_sim_emul.py, tests/test_train_sim_gpu.py).  TEST INFRASTRUCTURE ONLY.

  oracle_param_grads      the sim version of helpers.oracle_param_grads: (pred, edge_pred, {name: d <d_out, outputs> / d parameter}) by
                          autograd through tests/oracle_sim.forward_dense, or through forward_dense_masked when dropout multipliers are given
  forward_dense_masked    oracle_sim.forward_dense restated with the training-mode dropout multipliers of oracle/philox_ref.dropout_masks at
                          the four feed-forward sites of a block (A1, F2 on nodes; A3, F4 on edge pairs): the only live sites — the reference
                          builds this block's Trans_Layer without a dropout argument (mol_gnn.py:116), so the softmax weights are never
                          dropped.  With all-ones multipliers it equals oracle_sim.forward_dense (asserted by the CPU suite).
  selfcond_inputs         random self-conditioning inputs and output gradients, as the 3-D training tests draw them
"""
import math

import torch
import torch.nn.functional as F

import oracle_sim as OS
from oracle.dgt_oracle import _gbf, _lin, _ln, _mlp3, time_embedding

GRAD_REL, K32 = 3e-4, 16.0          # the gradient rule of helpers.compare_grads
DROP_SEED = (0x5DEECE66D << 20) | 0x1234567           # >= 2^32: the key's high word matters (tests/test_train_emul.py)


def drop_masks_for(hp, n_nodes, p, seed):
    from oracle import philox_ref as PR
    return PR.dropout_masks(seed, p, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio)


def forward_dense_masked(p, hp, xh, node_mask, edge_mask, edge_x, cond_x, cond_edge_x, noise_level, drop):
    """drop[b][l] = {'A1': [n, r D], 'F2': [n, D], 'A3': [n, n, r De], 'F4': [n, n, De]} multipliers (0 or 1 / (1 - p))."""
    bs, N, _ = xh.shape
    D, De, L, H = hp.nf, hp.de, hp.n_layers, hp.n_heads
    C = D // H
    dt = xh.dtype
    n_nodes = node_mask.reshape(bs, N).sum(1).long().tolist()
    has_cond = cond_x is not None
    tau = F.silu(time_embedding(p, hp, noise_level))
    first = True
    if has_cond:
        tot = 0.0
        for b in range(bs):
            cp = cond_x[b, :n_nodes[b], 0:3]
            tot = tot + ((cp[:, None, :] - cp[None, :, :]) ** 2).sum()
        first = bool(tot == 0)
    out_x = torch.zeros(bs, N, 3 + hp.in_node_dim, dtype=dt)
    out_e = torch.zeros(bs, N, N, hp.edge_ch, dtype=dt)
    pos_all = []
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
        ah, eh = [h], [e]
        negmask = torch.where(offd, 0.0, float('-inf')).to(dt)
        for l in range(L):
            bk = 'e_block_%d' % l
            m = {k_: torch.as_tensor(v_).to(dt) for k_, v_ in drop[b][l].items()}
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
            S = (q[None, :, :, :] * k[:, None, :, :] * t0).sum(-1) / math.sqrt(C)
            if n > 1:
                Sm = S + negmask[..., None]
                ex_ = (Sm - Sm.max(dim=0, keepdim=True).values).exp()
                alpha = ex_ / (ex_.sum(0, keepdim=True) + 1e-16)
            else:
                alpha = torch.zeros_like(S)
            t1 = torch.tanh(_lin(p, bk + '.attn_mpnn.lin_edge1', et, bias=False)).reshape(n, n, H, C)
            hhat = (v[:, None, :, :] * t1 * alpha[..., None]).sum(0).reshape(n, D)      # (alpha is not dropped: see the module docstring)
            n2e = F.linear(hhat, p[bk + '.node2edge_lin.weight'])
            ehat = n2e[:, None, :] + n2e[None, :, :] + p[bk + '.node2edge_lin.bias']
            hn = _ln(h + ng1 * hhat) * (1 + nc2) + ns2
            en = _ln(e + eg1 * ehat) * (1 + ec2) + es2
            h = hn + ng2 * (_lin(p, bk + '.ff_linear2', F.silu(_lin(p, bk + '.ff_linear1', hn)) * m['A1']) * m['F2'])
            e = en + eg2 * (_lin(p, bk + '.ff_linear4', F.silu(_lin(p, bk + '.ff_linear3', en)) * m['A3']) * m['F4'])
            W = p[bk + '.equi_update.input_lin.weight']
            Wr, Wc, We, Wd = W[:, :D], W[:, D:2 * D], W[:, 2 * D:2 * D + De], W[:, 2 * D + De:]
            pre = (F.linear(h, Wr)[:, None, :] + F.linear(h, Wc)[None, :, :] + F.linear(e, We) + F.linear(G, Wd)
                   + p[bk + '.equi_update.input_lin.bias'])
            sh, sc = _lin(p, bk + '.equi_update.time_mlp.1', tb).chunk(2, dim=1)
            u = _ln(pre) * (1 + sc) + sh
            iota = torch.tanh(F.linear(F.silu(_lin(p, bk + '.equi_update.coord_mlp.0', u)), p[bk + '.equi_update.coord_mlp.2.weight']))
            nrm = diff.norm(dim=-1, keepdim=True).clamp(min=1e-8)
            trans = diff / nrm * p[bk + '.equi_update.coord_norm.scale'] * iota * offd[..., None]
            x = x + trans.sum(1)
            x = x - x.mean(0, keepdim=True)
            ah.append(_lin(p, 'node_%d' % l, h))
            eh.append(_lin(p, 'edge_%d' % l, e))
        ehc = torch.cat(eh, dim=-1)
        Ep = torch.cat([_mlp3(p, 'edge_exist_mlp', ehc), _mlp3(p, 'edge_type_mlp', ehc)], dim=-1) * offd[..., None]
        out_e[b, :n, :n] = 0.5 * (Ep + Ep.transpose(0, 1))
        out_x[b, :n, 3:] = _mlp3(p, 'node_pred_mlp', torch.cat(ah, dim=-1))
        pos_all.append(x)
    nan = any(bool(torch.isnan(x).any()) for x in pos_all)
    for b in range(bs):
        x = torch.zeros_like(pos_all[b]) if nan else pos_all[b]
        out_x[b, :n_nodes[b], 0:3] = x - x.mean(0, keepdim=True)
    return out_x, out_e


def oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e, dtype=torch.float64, drop=None):
    """(pred, edge_pred, {name: d <d_out, outputs> / d parameter}) by autograd through the sim oracle on the CPU."""
    sd = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model.state_dict().items()}
    c = lambda t: None if t is None else t.detach().cpu().to(dtype)
    if drop is None:
        px, pe = OS.forward_dense(sd, hp, c(xh), c(nm), c(em), c(ex), c(cx), c(cex), c(nl))
    else:
        px, pe = forward_dense_masked(sd, hp, c(xh), c(nm), c(em), c(ex), c(cx), c(cex), c(nl), drop)
    ((px * c(d_x)).sum() + (pe * c(d_e)).sum()).backward()
    return px.detach(), pe.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}


def selfcond_inputs(xh, ex, nm, em, selfcond, seed=9):
    """(cond_x, cond_edge_x, d_out_x, d_out_e): the self-conditioning inputs (None, None on a first step) and output gradients that are
    neither symmetric nor masked — the kernels must mask and symmetrise."""
    g = torch.Generator().manual_seed(seed)
    cx = cex = None
    if selfcond:
        cx = torch.randn(xh.shape, generator=g) * nm
        cex = torch.randn(ex.shape, generator=g)
        cex = (cex + cex.transpose(1, 2)) * em.reshape(ex.shape[0], ex.shape[1], ex.shape[1], 1)
    return cx, cex, torch.randn(xh.shape, generator=g), torch.randn(ex.shape, generator=g)


def forward_close(got, want, what):
    """The forward tolerance of the project: |got - want| <= 2e-5 + 1e-4 |want|, elementwise."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    err = (g - w).abs()
    print("%s: max |err| %.3e (max |x| %.3e)" % (what, float(err.max()), float(w.abs().max())))
    assert bool((err <= 2e-5 + 1e-4 * w.abs()).all()), "%s: max |err| %.3e outside 2e-5 + 1e-4 |x|" % (what, float(err.max()))

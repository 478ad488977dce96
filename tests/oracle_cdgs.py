"""Dense torch restatement of the CDGS forward on a flat state_dict (keys `all_modules.<i>...`), the checker of the HIP kernels.

Dtype-generic: the computation runs in the dtype of the state_dict's tensors (float32: the reference's own arithmetic; float64: the
yardstick of helpers.close64), on their device.  Everything is evaluated on the padded [B, N, ...] tensors as the reference does,
which is what makes the edge GroupNorm depend on N: its statistics run over 8 channels x N x N positions, padded ones included.
Message passing is written densely (masked sums over the source atom) instead of through edge lists.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F


def hparams(cfg):
    m = cfg.model
    return SimpleNamespace(nf=m.nf, n_layers=m.n_layers, n_heads=m.n_heads, rw_depth=m.rw_depth, edge_ch=m.edge_ch,
                           atom_ch=cfg.data.atom_types)


def _lin(sd, name, x):
    w = sd[name + '.weight']
    b = sd.get(name + '.bias')
    return F.linear(x, w.reshape(w.shape[0], w.shape[1]), b)       # conv 1x1 weights are matrices with two trailing 1s


def sinusoid(t999, nf):
    half = nf // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float32, device=t999.device) * -(math.log(10000) / (half - 1))).to(t999.dtype)
    arg = t999[:, None] * freq[None, :]
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)


def rw_features(k_step, adj):
    """(landing [B, N, k], code [B, N, N] long): diagonals of AD^2 .. AD^(k+1) and the count of those powers with no walk."""
    AD = adj / (adj.sum(-1, keepdim=True) + 1e-8)
    p, land = AD, []
    code = torch.zeros(adj.shape, dtype=torch.long, device=adj.device)
    for _ in range(k_step):
        p = torch.bmm(p, AD)
        land.append(torch.diagonal(p, dim1=1, dim2=2))
        code = code + (p <= 0).long()
    return torch.stack(land, dim=-1), code


def _block(sd, pre, hp, h, e, adj, nm, em, temb_act):
    """h [B, N, C], e [B, N, N, C] (masked), adj / em [B, N, N], nm [B, N, 1]; returns (h, e) after the block."""
    B, N, C = h.shape
    H, Ch = hp.n_heads, C // hp.n_heads
    gn = lambda name, v: F.group_norm(v.reshape(-1, C), min(C // 4, 32), sd[pre + name + '.weight'], sd[pre + name + '.bias'], 1e-6).reshape(v.shape)
    h_in, e_in = h, e
    he = (e + _lin(sd, pre + 't_edge', temb_act)[:, None, None, :]) * em[..., None]
    hs = (h + _lin(sd, pre + 't_node', temb_act)[:, None, :]) * nm
    # local: GINE, source = first pair index, target = second
    msg = torch.relu(hs[:, :, None, :] + he) * adj[..., None]                     # [b, j, i, c]
    agg = (1 + sd[pre + 'local_model.eps']) * hs + msg.sum(1)
    loc = _lin(sd, pre + 'local_model.nn.2', torch.relu(_lin(sd, pre + 'local_model.nn.0', agg))) * nm
    h_local = gn('norm1_local', h_in + loc)
    # global: edge-gated attention over every real ordered pair
    q = _lin(sd, pre + 'self_attn.lin_query', hs).reshape(B, N, H, Ch)
    k = _lin(sd, pre + 'self_attn.lin_key', hs).reshape(B, N, H, Ch)
    v = _lin(sd, pre + 'self_attn.lin_value', hs).reshape(B, N, H, Ch)
    g0 = torch.tanh(_lin(sd, pre + 'self_attn.lin_edge0', he)).reshape(B, N, N, H, Ch)
    g1 = torch.tanh(_lin(sd, pre + 'self_attn.lin_edge1', he)).reshape(B, N, N, H, Ch)
    logit = (q[:, None] * k[:, :, None] * g0).sum(-1) / math.sqrt(Ch)              # [b, j, i, head]
    live = em[..., None] > 0
    logit = logit.masked_fill(~live, float('-inf'))                               # masked pairs: exp(-inf) = 0, whatever their size
    mx = logit.max(dim=1, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    ex = torch.exp(logit - mx)
    alpha = ex / (ex.sum(1, keepdim=True) + 1e-16)
    att = (v[:, :, None] * g1 * alpha[..., None]).sum(1).reshape(B, N, C)
    h_attn = gn('norm1_attn', h_in + att)
    h = (h_local + h_attn) * nm
    pair = h[:, None, :, :] + h[:, :, None, :]
    ff = lambda a, b, x: _lin(sd, pre + b, F.silu(_lin(sd, pre + a, x)))
    h = gn('norm2_node', h + ff('ff_linear1', 'ff_linear2', h)) * nm
    e = e_in + ff('ff_linear3', 'ff_linear4', pair)
    e = F.group_norm(e.permute(0, 3, 1, 2), min(C // 4, 32), sd[pre + 'norm2_edge.weight'], sd[pre + 'norm2_edge.bias'], 1e-6)
    e = e.permute(0, 2, 3, 1) * em[..., None]
    return h, e


def forward(sd, hp, t, x, node_mask, edge_mask, edge_x, return_blocks=False, return_rw=False):
    """(atom_score [B, N, atom_ch], bond_score [B, N, N, edge_ch]); with return_blocks also the list of (h [B, N, C], e [B, N, N, C])
    after the embeddings and after every block; with return_rw also (landing, code)."""
    any_w = sd['all_modules.0.weight']
    dt, dev = any_w.dtype, any_w.device
    c = lambda v: v.to(device=dev, dtype=dt)
    t, x, edge_x = c(t), c(x), c(edge_x)
    B, N, _ = x.shape
    nm, em = c(node_mask).reshape(B, N, 1), c(edge_mask).reshape(B, N, N)
    M = lambda i: 'all_modules.%d' % i
    L = hp.n_layers
    temb = _lin(sd, M(1), F.silu(_lin(sd, M(0), sinusoid(t * 999, hp.nf))))
    temb_act = F.silu(temb)
    adj = (edge_x[..., 0] >= 0).to(dt) * em
    land, code = rw_features(hp.rw_depth, adj)
    spd = F.one_hot(code, hp.rw_depth + 1).to(dt)
    mask = em[..., None]
    d_cate = _lin(sd, M(2), edge_x[..., 1:]) * mask
    d_exist = _lin(sd, M(3), edge_x[..., :1]) * mask
    d_spd = _lin(sd, M(4), spd) * mask
    e = _lin(sd, M(5), torch.cat([d_cate, d_exist, d_spd], -1)) * mask
    a_deg = _lin(sd, M(6), edge_x.sum(2))                                        # sum over the second atom index, unmasked
    a_cate = _lin(sd, M(7), x)
    a_rw = _lin(sd, M(8), land)
    h = _lin(sd, M(9), torch.cat([a_deg, a_cate, a_rw], -1))
    states = [(h, e)]
    a_hids, b_hids = [], []
    for l in range(L):
        h, e = _block(sd, M(10 + 3 * l) + '.', hp, h, e, adj, nm, em, temb_act)
        states.append((h, e))
        a_hids.append(_lin(sd, M(11 + 3 * l), h))
        b_hids.append(_lin(sd, M(12 + 3 * l), e))
    a_hids, b_hids = torch.cat(a_hids, -1), torch.cat(b_hids, -1)
    h0 = 10 + 3 * L
    head = lambda i, v, m: _lin(sd, M(i + 2), F.silu(_lin(sd, M(i + 1), F.silu(_lin(sd, M(i), v)) * m)))
    atom = head(h0, torch.cat([a_cate, a_hids], -1), nm) * nm
    bond = head(h0 + 3, torch.cat([d_cate, b_hids], -1), mask)
    exist = head(h0 + 6, torch.cat([d_exist, b_hids], -1), mask)
    s = torch.cat([exist, bond], -1)
    s = (s + s.transpose(1, 2)) / 2 * mask
    out = (atom, s)
    if return_blocks:
        out = out + (states,)
    if return_rw:
        out = out + ((land, code),)
    return out

"""The CDGS forward of tests/oracle_cdgs.py with the six dropout sites of a block restated as given multipliers — the checker of the
training path under model.train() (csrc/cdgs_train.hip).

forward_drop(..., drop=None) is oracle_cdgs.forward operation for operation; with drop = {(layer, site): multipliers} every site
multiplies its tensor by the given array, in the reference's call order (models/cdgs.py HybridMPBlock.forward):
    1 h_local  [B, N, C]     2 h_attn  [B, N, C]     3 node FF hidden [B, N, 2C]     4 node FF out [B, N, C]
    5 edge FF hidden [B, N, N, 2C]     6 edge FF out [B, N, N, C]
over the DENSE PADDED tensors: the reference draws its masks at every one of the N x N positions of the edge tile, padded and diagonal
ones included, and its edge GroupNorm reads them all.
drop_masks restates the kernels' masks: site = 8 l + s, element = the flat index of that dense tensor, so
oracle.philox_ref.drop_mul(seed, site, p, count).reshape(shape) is the whole restatement."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle_cdgs as OC
from oracle import philox_ref as PR

SITES = (1, 2, 3, 4, 5, 6)


def site_shapes(B, N, C):
    return {1: (B, N, C), 2: (B, N, C), 3: (B, N, 2 * C), 4: (B, N, C), 5: (B, N, N, 2 * C), 6: (B, N, N, C)}


def drop_masks(seed, p, B, N, n_layers, C, dtype=torch.float64):
    shapes = site_shapes(B, N, C)
    out = {}
    for l in range(n_layers):
        for s in SITES:
            m = PR.drop_mul(seed, 8 * l + s, p, int(np.prod(shapes[s])))
            out[(l, s)] = torch.from_numpy(m.reshape(shapes[s])).to(dtype)
    return out


def drop_mul_window(seed, site, p, start, count):
    """philox_ref.drop_mul for the elements start .. start + count - 1 (any start: philox_ref's own builder begins at element 0 and so
    cannot reach the second counter word, idx >> 34): float32 [count]."""
    p = np.float32(p)
    if p <= 0:
        return np.ones(count, np.float32)
    idx = np.arange(count, dtype=np.uint64) + np.uint64(start)
    quad = idx >> np.uint64(2)
    ctr = np.stack([quad & np.uint64(0xFFFFFFFF), quad >> np.uint64(32), np.full(quad.shape, site, np.uint64),
                    np.full(quad.shape, PR.DROP_TAG, np.uint64)], axis=-1).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    u = np.take_along_axis(PR.philox4x32_10(ctr, key), (idx & np.uint64(3)).astype(np.int64)[:, None], axis=1)[:, 0]
    uni = (u >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(uni < p, np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - p)).astype(np.float32)


def drop_mask_rows(seed, p, layer, site, row0, rows, width):
    """The multipliers of rows row0 .. row0 + rows - 1 of a dense [., width] site tensor (drop_masks restricted to a window of rows)."""
    return drop_mul_window(seed, 8 * layer + site, p, row0 * width, rows * width).reshape(rows, width)


def ones_masks(B, N, n_layers, C, dtype=torch.float64):
    shapes = site_shapes(B, N, C)
    return {(l, s): torch.ones(shapes[s], dtype=dtype) for l in range(n_layers) for s in SITES}


def _block(sd, pre, hp, h, e, adj, nm, em, temb_act, dm, margins=None, taps=None):
    lin = OC._lin
    B, N, C = h.shape
    H, Ch = hp.n_heads, C // hp.n_heads
    gn = lambda name, v: F.group_norm(v.reshape(-1, C), min(C // 4, 32), sd[pre + name + '.weight'], sd[pre + name + '.bias'], 1e-6).reshape(v.shape)
    h_in, e_in = h, e
    he = (e + lin(sd, pre + 't_edge', temb_act)[:, None, None, :]) * em[..., None]
    hs = (h + lin(sd, pre + 't_node', temb_act)[:, None, :]) * nm
    pre_msg = hs[:, :, None, :] + he
    msg = torch.relu(pre_msg) * adj[..., None]
    agg = (1 + sd[pre + 'local_model.eps']) * hs + msg.sum(1)
    pre_nn = lin(sd, pre + 'local_model.nn.0', agg)
    loc = lin(sd, pre + 'local_model.nn.2', torch.relu(pre_nn)) * nm
    if margins is not None:                     # distance of the gradient-carrying ReLU arguments from the kink
        with torch.no_grad():
            m = [pre_nn.abs()[nm.squeeze(-1) > 0].min().item()]
            if bool((adj > 0).any()):
                m.append(pre_msg.abs()[adj > 0].min().item())
            margins.append(min(m))
    h_local = gn('norm1_local', h_in + dm(1, loc))
    q = lin(sd, pre + 'self_attn.lin_query', hs).reshape(B, N, H, Ch)
    k = lin(sd, pre + 'self_attn.lin_key', hs).reshape(B, N, H, Ch)
    v = lin(sd, pre + 'self_attn.lin_value', hs).reshape(B, N, H, Ch)
    g0 = torch.tanh(lin(sd, pre + 'self_attn.lin_edge0', he)).reshape(B, N, N, H, Ch)
    g1 = torch.tanh(lin(sd, pre + 'self_attn.lin_edge1', he)).reshape(B, N, N, H, Ch)
    logit = (q[:, None] * k[:, :, None] * g0).sum(-1) / math.sqrt(Ch)
    live = em[..., None] > 0
    logit = logit.masked_fill(~live, float('-inf'))
    mx = logit.max(dim=1, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    ex = torch.exp(logit - mx)
    alpha = ex / (ex.sum(1, keepdim=True) + 1e-16)
    att = (v[:, :, None] * g1 * alpha[..., None]).sum(1).reshape(B, N, C)
    h_attn = gn('norm1_attn', h_in + dm(2, att))
    h = (h_local + h_attn) * nm
    pair = h[:, None, :, :] + h[:, :, None, :]
    ff = lambda a, b, x, sa, sb: dm(sb, lin(sd, pre + b, dm(sa, F.silu(lin(sd, pre + a, x)))))
    h = gn('norm2_node', h + ff('ff_linear1', 'ff_linear2', h, 3, 4)) * nm
    e = e_in + ff('ff_linear3', 'ff_linear4', pair, 5, 6)
    if taps is not None:                        # what the training path keeps besides h and e: alpha, and the xhat of norm2_edge
        taps.append(dict(alpha=alpha.detach(), xhat=F.group_norm(e.permute(0, 3, 1, 2), min(C // 4, 32), None, None, 1e-6).permute(0, 2, 3, 1).detach()))
    e = F.group_norm(e.permute(0, 3, 1, 2), min(C // 4, 32), sd[pre + 'norm2_edge.weight'], sd[pre + 'norm2_edge.bias'], 1e-6)
    e = e.permute(0, 2, 3, 1) * em[..., None]
    return h, e


def forward_drop(sd, hp, t, x, node_mask, edge_mask, edge_x, drop=None, return_blocks=False, margins=None, taps=None):
    """(atom_score, bond_score[, states]) as oracle_cdgs.forward; drop: None (no dropout) or {(layer, site): multipliers}; margins: a list
    that receives, per block, the smallest |argument| of the two ReLUs (GINE message, GINE nn) over the positions that carry gradient;
    taps: a list that receives, per block, dict(alpha [B, N, N, H] (source, target), xhat [B, N, N, C] of norm2_edge)."""
    lin = OC._lin
    any_w = sd['all_modules.0.weight']
    dt, dev = any_w.dtype, any_w.device
    c = lambda v: v.to(device=dev, dtype=dt)
    t, x, edge_x = c(t), c(x), c(edge_x)
    B, N, _ = x.shape
    nm, em = c(node_mask).reshape(B, N, 1), c(edge_mask).reshape(B, N, N)
    M = lambda i: 'all_modules.%d' % i
    L = hp.n_layers
    temb = lin(sd, M(1), F.silu(lin(sd, M(0), OC.sinusoid(t * 999, hp.nf))))
    temb_act = F.silu(temb)
    adj = (edge_x[..., 0] >= 0).to(dt) * em
    land, code = OC.rw_features(hp.rw_depth, adj)
    spd = F.one_hot(code, hp.rw_depth + 1).to(dt)
    mask = em[..., None]
    d_cate = lin(sd, M(2), edge_x[..., 1:]) * mask
    d_exist = lin(sd, M(3), edge_x[..., :1]) * mask
    d_spd = lin(sd, M(4), spd) * mask
    e = lin(sd, M(5), torch.cat([d_cate, d_exist, d_spd], -1)) * mask
    a_deg = lin(sd, M(6), edge_x.sum(2))
    a_cate = lin(sd, M(7), x)
    a_rw = lin(sd, M(8), land)
    h = lin(sd, M(9), torch.cat([a_deg, a_cate, a_rw], -1))
    states = [(h, e)]
    a_hids, b_hids = [], []
    for l in range(L):
        dm = (lambda s, v: v) if drop is None else (lambda s, v, l=l: v * c(drop[(l, s)]))
        h, e = _block(sd, M(10 + 3 * l) + '.', hp, h, e, adj, nm, em, temb_act, dm, margins, taps)
        states.append((h, e))
        a_hids.append(lin(sd, M(11 + 3 * l), h))
        b_hids.append(lin(sd, M(12 + 3 * l), e))
    a_hids, b_hids = torch.cat(a_hids, -1), torch.cat(b_hids, -1)
    h0 = 10 + 3 * L
    head = lambda i, v, m: lin(sd, M(i + 2), F.silu(lin(sd, M(i + 1), F.silu(lin(sd, M(i), v)) * m)))
    atom = head(h0, torch.cat([a_cate, a_hids], -1), nm) * nm
    bond = head(h0 + 3, torch.cat([d_cate, b_hids], -1), mask)
    exist = head(h0 + 6, torch.cat([d_exist, b_hids], -1), mask)
    s = torch.cat([exist, bond], -1)
    s = (s + s.transpose(1, 2)) / 2 * mask
    return (atom, s, states) if return_blocks else (atom, s)

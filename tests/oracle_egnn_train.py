"""CPU checker of the property classifier's training path: tests/oracle_egnn.py `forward` restated so that autograd sees the state dict
(the original detaches it), and the parameter gradients of <d_out, out> through it in float64 or float32."""
import numpy as np
import torch
import torch.nn.functional as F


def forward(sd, st, h0, x, n_nodes):
    """oracle_egnn.forward on a state dict that is used as given (same dtype as h0 / x, leaves that may require grad): out [B]."""
    B, N = h0.shape[0], h0.shape[1]
    dtype = h0.dtype
    n = torch.as_tensor(np.asarray(n_nodes), dtype=torch.long)
    node = (torch.arange(N).unsqueeze(0) < n.unsqueeze(1))                         # [B, N]
    edge = (node.unsqueeze(1) & node.unsqueeze(2) & ~torch.eye(N, dtype=torch.bool)).to(dtype).unsqueeze(-1)      # [B, N, N, 1]
    lin = lambda name, t: F.linear(t, sd[name + '.weight'], sd[name + '.bias'])
    diff = x.unsqueeze(2) - x.unsqueeze(1)                                          # [B, i, j, 3] = x_i - x_j
    radial = diff.square().sum(-1, keepdim=True)
    h = lin('embedding', h0)
    for l in range(st['n_layers']):
        pre = 'gcl_%d.' % l
        hi, hj = h.unsqueeze(2).expand(B, N, N, -1), h.unsqueeze(1).expand(B, N, N, -1)
        m = F.silu(lin(pre + 'edge_mlp.2', F.silu(lin(pre + 'edge_mlp.0', torch.cat([hi, hj, radial], -1)))))
        if st['attention']:
            m = m * torch.sigmoid(lin(pre + 'att_mlp.0', m))
        agg = (m * edge).sum(2)                                                     # over sources j, row atom i
        feats = [h, agg] + ([h0] if st['node_attr'] else [])
        h = h + lin(pre + 'node_mlp.2', F.silu(lin(pre + 'node_mlp.0', torch.cat(feats, -1))))
    hd = lin('node_dec.2', F.silu(lin('node_dec.0', h))) * node.to(dtype).unsqueeze(-1)
    return lin('graph_dec.2', F.silu(lin('graph_dec.0', hd.sum(1)))).squeeze(-1)


def grads(sd, st, h0, x, n_nodes, d_out, dtype=torch.float64, chunk=None):
    """(out [B], {name: d <d_out, out> / d parameter}) by autograd through `forward` in `dtype`.  chunk: evaluate slices of that many
    molecules and sum the gradients over slices (every molecule's output depends on that molecule alone)."""
    sdg = {(k[7:] if k.startswith('module.') else k): v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    h0, x, d_out = h0.detach().cpu().to(dtype), x.detach().cpu().to(dtype), d_out.detach().cpu().to(dtype)
    n_nodes = list(n_nodes)
    B = len(n_nodes)
    chunk = B if chunk is None else chunk
    outs = []
    for b0 in range(0, B, chunk):
        nn_ = n_nodes[b0:b0 + chunk]
        N = max(nn_)                                                                # padding atoms carry no weight: drop unused width
        out = forward(sdg, st, h0[b0:b0 + chunk, :N], x[b0:b0 + chunk, :N], nn_)
        (out * d_out[b0:b0 + chunk]).sum().backward()
        outs.append(out.detach())
    return torch.cat(outs), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sdg.items()}

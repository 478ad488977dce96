"""Shared by tests/test_egnn_kernels_host.py and tests/test_egnn_kernels_gpu.py: a plain restatement of what the two fused edge kernels
of the property classifier store (csrc/egnn_forward.hip kegnn_edge, csrc/egnn_train.hip kegnn_edge_bwd + kegnn_tgt_sum), in the dtype
asked for, and the seeded inputs of the kernel-level tests.

For an ordered pair (row atom i, source j != i) of one molecule:
    rad = |xc_i - xc_j|^2,  z1 = P[i, :nf] + P[j, nf:] + rad wr,  a = SiLU(z1),  z2 = W2 a + b2,  m = SiLU(z2),
    g = sigmoid(wa . m + ba) (1 without attention),  agg_i = sum_j g m
    c = (dagg_i . m) g (1 - g) (0 without attention),  dm = g dagg_i + c wa,  dz2 = dm SiLU'(z2),  da = W2^T dz2,  dz1 = da SiLU'(z1)
    ea = a, ez2 = dz2, ez1 = dz1 (compact edge rows eoff_b + i (n - 1) + (j < i ? j : j - 1)),
    dP[i, :nf] = sum_j dz1(i, j),  dP[j, nf:] = sum_i dz1(i, j),  Q[i, :nf] = sum_j rad dz1,  Q[i, nf:] = sum_j c m,  qb[i] = sum_j c
tests/test_egnn_kernels_host.py anchors it: the backward arrays are autograd's through the forward part, and the forward part composed
with node_mlp reproduces oracle_egnn.forward."""
import math

import torch
import torch.nn.functional as F

MAIN = [1, 2, 33, 1, 31, 32, 34, 65, 64, 3]      # 266 atoms, 12 300 edges: molecule boundaries inside the 4-wave workgroups
NFS = [64, 128, 192, 256]                        # kegnn_edge<2, true>, <4, true>, <6, false>, <8, false>
OVERFLOW = 88.8                                  # exp(-z) is beyond float32 for z < -88.8
# the saturating regime: multipliers on the benign draws; the gate's by width, set where the float64 restatement meets
# assert_saturating with room on both sides (nf 128 at 3: 46 % of the gates saturated; nf 256 at 3: 7 % of dz1 live)
SAT = dict(P=8.0, xc=3.0, wr=2.0, W2=2.0)
SAT_WA = {64: 3.0, 128: 4.0, 192: 4.0, 256: 1.5}


def seed(regime, nf):
    """one seed per (regime, width): the host tests judge the very draws the GPU tests use"""
    return dict(benign=100, saturating=700, geometry=300, zero_row=400, wide=500)[regime] + nf


def silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def fwd_rows(Pm, xm, i0, i1, wr, W2, b2, wa, ba):
    """Row atoms i0 .. i1 - 1 of ONE molecule (Pm [n, 2 nf], xm [n, >= 3]) against all its atoms as sources: a dict of [r, n(, nf)]
    tensors.  wr / wa / ba may carry a leading row-atom axis ([n, nf], [n, nf], [n]): the per-row-atom copies of the autograd anchor."""
    n, nf = Pm.shape[0], Pm.shape[1] // 2
    d = xm[i0:i1, None, :3] - xm[None, :, :3]
    rad = d.square().sum(-1)                                                  # [r, n]
    wr_ = wr[i0:i1, None, :] if wr.dim() == 2 else wr
    z1 = Pm[i0:i1, None, :nf] + Pm[None, :, nf:] + rad.unsqueeze(-1) * wr_
    a = F.silu(z1)
    z2 = a @ W2.t() + b2
    m = F.silu(z2)
    mask = (torch.arange(i0, i1).unsqueeze(1) != torch.arange(n).unsqueeze(0))
    if wa is not None:
        wa_ = wa[i0:i1, None, :] if wa.dim() == 2 else wa
        ba_ = ba[i0:i1, None] if ba.numel() > 1 else ba
        logit = (m * wa_).sum(-1) + ba_
        g = torch.sigmoid(logit)
    else:
        logit, g = None, torch.ones_like(rad)
    gm = g * mask.to(g.dtype)
    agg = (gm.unsqueeze(-1) * m).sum(1)
    return dict(rad=rad, z1=z1, a=a, z2=z2, m=m, mask=mask, logit=logit, g=g, gm=gm, agg=agg)


def restate(P, xc, wr, W2, b2, wa, ba, n_nodes, dagg=None, dtype=torch.float64, keep=False, rows=64):
    """-> dict: agg [Nn, nf]; with dagg also ea, ez2, ez1 [E, nf], dP [Nn, 2 nf], Q [Nn, 2 nf], qb [Nn].  keep: also z1, z2 [E, nf] and the
    gate logits [E] of the valid pairs (the non-vacuity conditions read them).  Big molecules go in slices of `rows` row atoms."""
    c_ = lambda t: None if t is None else t.detach().cpu().to(dtype)
    P, xc, wr, W2, b2, wa, ba, dagg = map(c_, (P, xc, wr, W2, b2, wa, ba, dagg))
    nf, Nn = wr.shape[0], sum(n_nodes)
    out = dict(agg=torch.zeros(Nn, nf, dtype=dtype))
    per_edge = ['ea', 'ez2', 'ez1'] if dagg is not None else []
    if keep:
        per_edge += ['z1', 'z2', 'logit']
    lists = {k: [] for k in per_edge}
    if dagg is not None:
        out.update(dP=torch.zeros(Nn, 2 * nf, dtype=dtype), Q=torch.zeros(Nn, 2 * nf, dtype=dtype), qb=torch.zeros(Nn, dtype=dtype))
    noff = 0
    for n in n_nodes:
        Pm, xm = P[noff:noff + n], xc[noff:noff + n]
        for i0 in range(0, n, rows):
            i1 = min(n, i0 + rows)
            f = fwd_rows(Pm, xm, i0, i1, wr, W2, b2, wa, ba)
            t0, t1, mask = noff + i0, noff + i1, f['mask']
            out['agg'][t0:t1] = f['agg']
            if keep:
                lists['z1'].append(f['z1'][mask])
                lists['z2'].append(f['z2'][mask])
                lists['logit'].append(f['logit'][mask] if wa is not None else torch.zeros(int(mask.sum()), dtype=dtype))
            if dagg is None:
                continue
            dg = dagg[t0:t1].unsqueeze(1)                                     # [r, 1, nf]
            if wa is not None:
                c = (f['m'] * dg).sum(-1) * f['g'] * (1 - f['g']) * mask.to(dtype)
                dm = f['gm'].unsqueeze(-1) * dg + c.unsqueeze(-1) * wa
            else:
                c = torch.zeros_like(f['rad'])
                dm = f['gm'].unsqueeze(-1) * dg
            dz2 = dm * silu_grad(f['z2'])
            dz1 = (dz2 @ W2) * silu_grad(f['z1'])
            lists['ea'].append(f['a'][mask])
            lists['ez2'].append(dz2[mask])
            lists['ez1'].append(dz1[mask])
            out['dP'][t0:t1, :nf] = dz1.sum(1)
            out['dP'][noff:noff + n, nf:] += dz1.sum(0)
            out['Q'][t0:t1, :nf] = (f['rad'].unsqueeze(-1) * dz1).sum(1)
            out['Q'][t0:t1, nf:] = (c.unsqueeze(-1) * f['m']).sum(1)
            out['qb'][t0:t1] = c.sum(1)
        noff += n
    for k in per_edge:
        width = () if k == 'logit' else (nf,)
        out[k] = torch.cat(lists[k]) if lists[k] else torch.zeros((0,) + width, dtype=dtype)
    return out


def agg_from_ea(ea, W2, b2, wa, ba, n_nodes, dtype):
    """agg [Nn, nf] from stored a rows [E, nf] (compact edge order): the rest of the forward, restated."""
    ea, W2, b2 = ea.detach().cpu().to(dtype), W2.detach().cpu().to(dtype), b2.detach().cpu().to(dtype)
    m = F.silu(ea @ W2.t() + b2)
    if wa is not None:
        m = m * torch.sigmoid(m @ wa.detach().cpu().to(dtype) + ba.detach().cpu().to(dtype)).unsqueeze(-1)
    nf = W2.shape[0]
    agg, e = torch.zeros(sum(n_nodes), nf, dtype=dtype), 0
    t = 0
    for n in n_nodes:
        if n > 1:
            agg[t:t + n] = m[e:e + n * (n - 1)].view(n, n - 1, nf).sum(1)
        e += n * (n - 1)
        t += n
    return agg


def edge_offsets(n_nodes):
    """(noff [B], eoff [B], Nn, E)"""
    noff, eoff, t, e = [], [], 0, 0
    for n in n_nodes:
        noff.append(t)
        eoff.append(e)
        t += n
        e += n * (n - 1)
    return noff, eoff, t, e


def inputs(n_nodes, nf, seed, att=True, regime='benign'):
    """Seeded float32 inputs of one call: dict(P, xc, dagg, wr, W2, b2, wa, ba).  Weights at 1 / sqrt(nf) scale, positions 1.5 randn.
    regime 'saturating': the multipliers SAT / SAT_WA; 'geometry': in the 34-atom molecule of MAIN two atoms share a position (rad = 0) and one
    sits 100 units away; 'zero_row': the dagg row of the last atom of the 33-atom molecule (the row atom whose last chunk holds only its
    own, masked lane) is zero."""
    g = torch.Generator().manual_seed(seed)
    Nn, s = sum(n_nodes), 1.0 / math.sqrt(nf)
    r = lambda *shape: torch.randn(*shape, generator=g)
    d = dict(P=r(Nn, 2 * nf), xc=torch.cat([1.5 * r(Nn, 3), torch.zeros(Nn, 1)], 1), dagg=r(Nn, nf), wr=s * r(nf), W2=s * r(nf, nf), b2=0.5 * r(nf),
             wa=s * r(nf), ba=0.5 * r(1))
    if regime == 'saturating':
        for k, v in dict(SAT, wa=SAT_WA[nf]).items():
            d[k] = d[k] * v
    noff = edge_offsets(n_nodes)[0]
    if regime == 'geometry':
        t = noff[n_nodes.index(34)]
        d['xc'][t + 7] = d['xc'][t + 20]
        d['xc'][t + 33, 0] += 100.0
    if regime == 'zero_row':
        d['dagg'][zero_row_atom(n_nodes)] = 0.0
    if not att:
        d['wa'] = d['ba'] = None
    return d


def zero_row_atom(n_nodes):
    return edge_offsets(n_nodes)[0][n_nodes.index(33)] + 32


def saturation_report(r64, att):
    """The non-vacuity figures of the saturating regime on the float64 restatement (keep=True): a dict of fractions / counts."""
    z1, z2, lg, dz1 = r64['z1'], r64['z2'], r64['logit'], r64['ez1'].abs()
    rep = dict(z2_over=float((z2.abs() > OVERFLOW).double().mean()), z1_over=int((z1.abs() > OVERFLOW).sum()),
               z2_neg_over=int((z2 < -OVERFLOW).sum()), z1_neg_over=int((z1 < -OVERFLOW).sum()),
               dz1_live=float((dz1 > 1e-6 * dz1.max()).double().mean()))
    if att:
        rep.update(gate_sat=float((lg.abs() > 20).double().mean()), gate_live=float((lg.abs() < 2).double().mean()))
    return rep


def assert_saturating(rep, att, what=''):
    """the conditions under which the saturating regime tests what it says ("The EGNN edge kernels one by one")"""
    if att:
        assert rep['gate_sat'] >= 0.5, (what, rep)
        assert rep['gate_live'] >= 0.01, (what, rep)
    assert rep['z2_over'] >= 1e-3 and rep['z1_over'] >= 100, (what, rep)
    assert rep['z2_neg_over'] > 0 and rep['z1_neg_over'] > 0, (what, rep)      # the side on which exp(-z) itself overflows
    assert rep['dz1_live'] >= 0.1, (what, rep)

"""The float64 restatements of the fused training kernels (tests/fused_kernels_common.py) are anchored here, on the CPU:
  * composed into one EquivariantMixBlock (chain A, node pair, attention, chain B, chain C) they reproduce the per-block tensors of the
    dense oracles of DGT_concat, DGT_concat_sim and DGT_concat_2D at float64;
  * every backward restatement equals torch.autograd.grad through its forward restatement at float64.
A restatement written from the kernel's own comments could share the kernel's mistake; one that also reproduces the model cannot.
tests/test_fused_kernels_gpu.py then holds the kernels against these functions."""
import math
import os
import re

import pytest
import torch
from torch.nn import functional as F

from oracle import dgt_oracle as O

import fused_kernels_common as K
import oracle2d as O2
import oracle_sim as OS
from helpers import make_config, make_model, masks, random_inputs

# Composition against the oracle at float64: both sides evaluate the same formulas in a different association (per-row gathers and a
# split input_lin here, dense [n, n] broadcasts there), so they differ by float64 rounding carried through three blocks of unit-gain
# arithmetic: measured worst 2.2e-15.  1e-11 leaves room for other BLAS orders and is four decades below the float32 rounding the
# GPU tests resolve (1e-7); a wrong formula is off by 1e-2 or more.
ANCHOR_TOL = 1e-11
# backward restatement against autograd through the forward restatement, float64, relative to the array's largest entry: both are
# float64 evaluations of the same derivative (a few hundred ulps at most: 1e-13)
AUTOGRAD_TOL = 1e-12


def test_binding_lists_follow_the_header():
    from jodo_amd import capi
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'jodo_hip.h')) as f:
        txt = f.read()
    enums = re.findall(r'enum \{ (JODO_FT_[^}]*)\}', txt)
    assert len(enums) == 2
    names = [[n.strip().split(' ')[0].replace('JODO_FT_', '') for n in e.split(',')] for e in enums]
    assert names[0] == list(capi.FT_OPS) + ['N_OPS']
    assert names[1] == list(capi.FT_SLOTS) + ['N_SLOTS']


def block_params(sd, l, kind):
    bk = 'e_block_%d.' % l
    P = dict(le0=sd[bk + 'attn_mpnn.lin_edge0.weight'], le1=sd[bk + 'attn_mpnn.lin_edge1.weight'], ff3_w=sd[bk + 'ff_linear3.weight'],
             ff3_b=sd[bk + 'ff_linear3.bias'], ff4_w=sd[bk + 'ff_linear4.weight'], ff4_b=sd[bk + 'ff_linear4.bias'], ero_w=sd['edge_%d.weight' % l],
             ero_b=sd['edge_%d.bias' % l], n2e_b=sd[bk + 'node2edge_lin.bias'])
    assert bk + 'attn_mpnn.lin_edge0.bias' not in sd and bk + 'attn_mpnn.lin_edge1.bias' not in sd
    if kind != '2d':
        P.update(edge_emb_w=sd[bk + 'edge_emb.weight'], edge_emb_b=sd[bk + 'edge_emb.bias'], in_w=sd[bk + 'equi_update.input_lin.weight'],
                 in_b=sd[bk + 'equi_update.input_lin.bias'], c0_w=sd[bk + 'equi_update.coord_mlp.0.weight'], c0_b=sd[bk + 'equi_update.coord_mlp.0.bias'],
                 c2_w=sd[bk + 'equi_update.coord_mlp.2.weight'], gbf_means=sd[bk + 'dist_layer.means.weight'].reshape(-1))
        P['gbf_stds'] = sd[bk + 'dist_layer.stds.weight'].reshape(-1)
    return P


def composed_block(sd, l, kind, tp, H, XH, SC, tau, h, e, pos):
    """One EquivariantMixBlock from the restatements (float64): -> h', e', pos', hhat, alpha."""
    bk = 'e_block_%d.' % l
    lin = lambda name, x: F.linear(x, sd[bk + name + '.weight'], sd.get(bk + name + '.bias'))
    D = h.shape[1]
    P = block_params(sd, l, kind)
    emod, nmod = lin('edge_time_mlp.1', tau), lin('node_time_mlp.1', tau)
    if kind == '2d':
        A = K.chain_a_2d(P, tp, e, emod)
    else:
        A = K.chain_a(P, tp, pos, lin('dist_layer.time_mlp.1', tau), e, emod)
    ht = K.node_ln_mod(h, None, tp['node_mol'], nmod, 0, 0, D)['y']
    q, k, v = lin('attn_mpnn.lin_query', ht), lin('attn_mpnn.lin_key', ht), lin('attn_mpnn.lin_value', ht)
    ones = torch.ones(tp['R'], dtype=torch.float64)               # no self-conditioning input: both adjacency flags are 1 everywhere
    AT = K.attn_fwd(tp['nn'], H, XH, SC, q, k, v, A['t0'], A['t1'], ones, ones)
    n2e = F.linear(AT['hhat'], sd[bk + 'node2edge_lin.weight'])
    hn = K.node_ln_mod(h, AT['hhat'], tp['node_mol'], nmod, 2 * D, 3 * D, 4 * D)['y']
    h2 = hn + nmod[tp['node_mol'], 5 * D:] * lin('ff_linear2', F.silu(lin('ff_linear1', hn)))
    one = torch.ones(1, 1, dtype=torch.float64)
    Bc = K.chain_b(P, tp, e, n2e, emod, one, one)
    if kind == '2d':
        return h2, Bc['e_out'], pos, AT['hhat'], AT['alpha'], Bc['ro']
    W = P['in_w']
    Cc = K.chain_c(P, tp, Bc['e_out'], A['G'], F.linear(h2, W[:, :D]), F.linear(h2, W[:, D:2 * D]), lin('equi_update.time_mlp.1', tau))
    iota = Cc['inv'].mean(-1, keepdim=True)                       # (inv * [1, adj2d, adjsp]).mean(-1) with both flags 1; one head: itself
    diff = pos[tp['edge_a']] - pos[tp['edge_c']]
    trans = diff / diff.norm(dim=-1, keepdim=True).clamp(min=1e-8) * sd[bk + 'equi_update.coord_norm.scale'] * iota
    trans = trans * (tp['edge_a'] != tp['edge_c'])[:, None]
    x = pos.clone().index_add_(0, tp['edge_a'], trans)
    mean = torch.zeros(tp['B'], 3, dtype=torch.float64).index_add_(0, tp['node_mol'], x) / torch.tensor(tp['nn'], dtype=torch.float64)[:, None]
    return h2, Bc['e_out'], x - mean[tp['node_mol']], AT['hhat'], AT['alpha'], Bc['ro']


N_NODES = [3, 1, 6, 2, 5]
N_BLOCKS = 3                        # blocks composed (the oracles run their whole network; a block's inputs are the composed outputs of the one before)


def _gbf_pure(p, prefix, d2, tau_silu):
    """dgt_oracle._gbf with every operation in the evaluation's dtype.  The oracle's own version forms sigma = |w| + 1e-5 and the
    normalisation a sigma in FLOAT32 whatever the dtype (its `.float()`), which leaves its float64 Gaussians 2^-24 relative from the
    float64 value of the same formula."""
    ss = F.linear(tau_silu, p[prefix + '.time_mlp.1.weight'], p[prefix + '.time_mlp.1.bias'])
    x = d2 * (ss[..., 0:1] + 1) + ss[..., 1:2]
    return torch.cat([x, K.gauss(x.reshape(-1), p[prefix + '.means.weight'].view(-1), p[prefix + '.stds.weight'].view(-1))[:, 1:].reshape(
        x.shape[:-1] + (-1,))], dim=-1)


@pytest.mark.parametrize('pure_gbf', [True, False])
@pytest.mark.parametrize('kind', ['3d', 'sim'])
def test_composed_restatements_reproduce_the_dense_oracle_3d(kind, pure_gbf, monkeypatch):
    """pure_gbf: against the oracle with its Gaussian layer evaluated purely in float64 (_gbf_pure) the composition agrees at float64
    rounding (ANCHOR_TOL).  Against the oracle as it stands the difference is the oracle's float32 normalisation of the Gaussians:
    two float32 roundings (sigma, a sigma), 2^-23 relative, of features as large as 1 / (a min sigma) (the bound below: 2.3e-5 at the
    test initialisation, whose narrowest Gaussian has sigma 0.002); measured 2.6e-8 after three blocks (Gaussians that narrow are
    rarely lit)."""
    if pure_gbf:
        monkeypatch.setattr(O, '_gbf', _gbf_pure)
        monkeypatch.setattr(OS, '_gbf', _gbf_pure)
    cfg = make_config('vpsde_qm9_uncond_jodo', **({'name': 'DGT_concat_sim'} if kind == 'sim' else {}))
    model = make_model(cfg, 5)
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    hp = (OS.HyperSim if kind == 'sim' else O.Hyper).from_config(cfg)
    xh, ex, nl, _, nm, em = random_inputs(hp, N_NODES, 11)
    fwd = OS.forward_dense if kind == 'sim' else O.forward_dense
    with torch.no_grad():
        _, _, inter = fwd(sd, hp, xh.double(), nm.double(), em.double(), ex.double(), None, None, nl.double(), return_intermediates=True)
        tp = K.mol_topo(N_NODES)
        tau = F.silu(O.time_embedding(sd, hp, nl.double()))
        H = hp.n_heads
        XH = 0 if kind == 'sim' else hp.n_extra_heads
        SC = (hp.nf // H) if kind == 'sim' else hp.sub_ch
        xs = torch.cat([xh[b, :n] for b, n in enumerate(N_NODES)]).double()
        es = torch.cat([ex[b, :n, :n].reshape(n * n, -1) for b, n in enumerate(N_NODES)]).double()
        pos = xs[:, :3].clone()
        h = F.linear(torch.cat([xs[:, 3:], torch.zeros_like(xs[:, 3:])], -1), sd['node_emb.weight'], sd['node_emb.bias'])
        e = F.linear(torch.cat([es, torch.zeros_like(es), torch.zeros(tp['R'], hp.de, dtype=torch.float64)], -1), sd['edge_emb.weight'], sd['edge_emb.bias'])
        worst = 0.0
        for l in range(N_BLOCKS):
            h, e, pos, hhat, alpha, ro = composed_block(sd, l, kind, tp, H, XH, SC, tau, h, e, pos)
            for b, n in enumerate(N_NODES):
                ns, es_ = slice(int(tp['node_off'][b]), int(tp['node_off'][b + 1])), slice(int(tp['edge_off'][b]), int(tp['edge_off'][b + 1]))
                want = inter[b][l]
                for got, ref in ((h[ns], want['h']), (e[es_], want['e'].reshape(n * n, -1)), (pos[ns], want['pos']), (hhat[ns], want['hhat']),
                                 (alpha[es_], want['alpha'].reshape(n * n, -1)),
                                 (ro[es_], F.linear(want['e'], sd['edge_%d.weight' % l], sd['edge_%d.bias' % l]).reshape(n * n, -1))):
                    worst = max(worst, float((got - ref).abs().max()))
    sig = min(float(v.abs().min()) for k_, v in sd.items() if k_.endswith('dist_layer.stds.weight') and k_.startswith('e_block_')) + 1e-5
    bound = ANCHOR_TOL if pure_gbf else 2.0 ** -23 / (K.A_GAUSS * sig)
    print("composed block vs dense oracle (%s, %s Gaussian layer): worst |difference| %.2e, bound %.2e" % (
        kind, 'float64' if pure_gbf else "the oracle's", worst, bound))
    assert worst <= bound


@pytest.mark.parametrize('cfg_name', ['vpsde_zinc_2d_jodo', 'vpsde_moses_2d_jodo'])
def test_composed_restatements_reproduce_the_dense_oracle_2d(cfg_name):
    cfg = make_config(cfg_name)
    model = make_model(cfg, 5)
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    hp = O2.Hyper2D.from_config(cfg)
    B, N = len(N_NODES), max(N_NODES)
    nm, em = masks(N_NODES)
    g = torch.Generator().manual_seed(3)
    xh = (torch.randn(B, N, hp.nd, generator=g) * nm).double()
    ex = torch.randn(B, N, N, hp.ch, generator=g)
    ex = ((ex + ex.transpose(1, 2)) * em.reshape(B, N, N, 1)).double()
    nl = (torch.randn(B, generator=g) * 2).double()
    with torch.no_grad():
        _, _, blocks = O2.forward_dense(sd, hp, xh, nm, em, ex, None, None, nl, return_blocks=True)
        x = nl.unsqueeze(-1)
        fr = x * sd['time_mlp.0.weights'].unsqueeze(0) * 2 * math.pi
        tau = F.silu(F.linear(F.gelu(F.linear(torch.cat([x, fr.sin(), fr.cos()], -1), sd['time_mlp.1.weight'], sd['time_mlp.1.bias'])),
                              sd['time_mlp.3.weight'], sd['time_mlp.3.bias']))
        tp = K.mol_topo(N_NODES)
        xs = torch.cat([xh[b, :n] for b, n in enumerate(N_NODES)])
        es = torch.cat([ex[b, :n, :n].reshape(n * n, -1) for b, n in enumerate(N_NODES)])
        h = F.linear(torch.cat([xs, torch.zeros_like(xs)], -1), sd['node_emb.weight'], sd['node_emb.bias'])
        e = F.linear(torch.cat([es, torch.zeros_like(es)], -1), sd['edge_emb.weight'], sd['edge_emb.bias'])
        worst = 0.0
        for l in range(N_BLOCKS):
            h, e, _, _, _, _ = composed_block(sd, l, '2d', tp, hp.H, hp.XH, hp.SC, tau, h, e, None)
            for b, n in enumerate(N_NODES):
                ns, es_ = slice(int(tp['node_off'][b]), int(tp['node_off'][b + 1])), slice(int(tp['edge_off'][b]), int(tp['edge_off'][b + 1]))
                offd = ~torch.eye(n, dtype=torch.bool)              # the oracle zeroes the diagonal pairs of the copies it returns
                worst = max(worst, float((h[ns] - blocks[l][0][b, :n]).abs().max()))
                if n > 1:
                    worst = max(worst, float((e[es_].reshape(n, n, -1)[offd] - blocks[l][1][b, :n, :n][offd]).abs().max()))
    print("composed block vs dense oracle (%s): worst |difference| %.2e" % (cfg_name, worst))
    assert worst <= ANCHOR_TOL


# ---- backward restatements against autograd through the forward restatements ---------------------------------------------------------
def rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def leaf(t):
    return t.clone().requires_grad_(True)


D_AG = K.dims(128, 2, 126, 3, 8)


def setup(seed=0, R=45, p=0.1):
    g = torch.Generator().manual_seed(seed)
    tp = K.rand_topo(R, seed)
    return g, tp, K.rand_params(D_AG, seed + 1), p


def test_bwd_c_is_the_gradient_of_chain_c():
    g, tp, P, _ = setup()
    D, De, R = D_AG['D'], D_AG['De'], tp['R']
    e_in, G = leaf(K.randn64(g, R, De)), leaf(K.randn64(g, R, De))
    hr, hc, qmod = K.randn64(g, tp['Nn'], D), K.randn64(g, tp['Nn'], D), K.randn64(g, tp['B'], 2 * D, scale=0.5)
    Pl = dict(P, c2_w=leaf(P['c2_w']), c0_w=leaf(P['c0_w']), c0_b=leaf(P['c0_b']))
    f = K.chain_c(Pl, tp, e_in, G, hr, hc, qmod)
    dinv, de0 = K.randn64(g, R, D_AG['nco']), K.randn64(g, R, De)
    f['u'].retain_grad(); f['c0a'].retain_grad()
    ge, gG, gc0 = torch.autograd.grad((f['inv'] * dinv).sum(), [e_in, G, Pl['c0_b']], retain_graph=True)
    b = K.bwd_c(P, tp, f['inv'].detach(), dinv, f['c0pre'].detach(), f['xh'].detach(), f['rs'].detach(), qmod, de0)
    gu, gpre = torch.autograd.grad((f['inv'] * dinv).sum(), [f['u'], f['c0pre']], retain_graph=True)
    assert rel(b['de'] - de0, ge) <= AUTOGRAD_TOL and rel(b['dG'], gG) <= AUTOGRAD_TOL
    assert rel(b['dc0'], gpre) <= AUTOGRAD_TOL and rel(b['du'], gu) <= AUTOGRAD_TOL and rel(b['dc0'].sum(0), gc0) <= AUTOGRAD_TOL
    # dinv' is the gradient of the tanh's argument, dpre that of input_lin's output (through its bias)
    Pb = dict(P, in_b=leaf(P['in_b']))
    f2 = K.chain_c(Pb, tp, e_in.detach(), G.detach(), hr, hc, qmod)
    assert rel(b['dpre'].sum(0), torch.autograd.grad((f2['inv'] * dinv).sum(), [Pb['in_b']])[0]) <= AUTOGRAD_TOL
    z = leaf(torch.atanh(f['inv'].detach()))
    assert rel(b['dinv'], torch.autograd.grad((torch.tanh(z) * dinv).sum(), [z])[0]) <= 1e-9


def test_bwd_b_is_the_gradient_of_chain_b():
    g, tp, P, p = setup(1)
    De, R, HID = D_AG['De'], tp['R'], D_AG['r'] * D_AG['De']
    seed = (5 << 32) | 77
    m3, m4 = K.drop_masks(seed, 3, p, R, HID, torch.float64), K.drop_masks(seed, 4, p, R, De, torch.float64)
    assert 0 < float((m3 == 0).double().mean()) < 0.3 and 0 < float((m4 == 0).double().mean()) < 0.3
    e_in, n2e, emod = leaf(K.randn64(g, R, De)), K.randn64(g, tp['Nn'], De), leaf(K.randn64(g, tp['B'], 6 * De, scale=0.5))
    Pl = dict(P, ff3_b=leaf(P['ff3_b']), ff4_b=leaf(P['ff4_b']))
    f = K.chain_b(Pl, tp, e_in, n2e, emod, m3, m4)
    de_out = K.randn64(g, R, De)
    loss = (f['e_out'] * de_out).sum()
    ge, gmod, gb3, gb4, gen = torch.autograd.grad(loss, [e_in, emod, Pl['ff3_b'], Pl['ff4_b'], f['en']])
    b = K.bwd_b(P, tp, de_out, f['f4'].detach(), f['f3'].detach(), f['xh'].detach(), f['rs'].detach(), emod.detach(), m3, m4)
    assert rel(b['de_prev'], ge) <= AUTOGRAD_TOL and rel(b['dhid'].sum(0), gb3) <= AUTOGRAD_TOL and rel(b['df4'].sum(0), gb4) <= AUTOGRAD_TOL
    assert rel(b['den'], gen) <= AUTOGRAD_TOL
    # f4d feeds the gate gradient: d g2[b] = sum over the molecule's rows of de_out f4d
    dg2 = torch.zeros(tp['B'], De, dtype=torch.float64).index_add_(0, tp['edge_mol'], de_out * b['f4d'])
    assert rel(dg2, gmod[:, 5 * De:]) <= AUTOGRAD_TOL
    assert bool((b['dhid'][m3 == 0] == 0).all()) and bool((b['f4d'][m4 == 0] == 0).all())


def test_bwd_a_is_the_gradient_of_chain_a():
    g, tp, P, _ = setup(2)
    D, De, QK, R = D_AG['D'], D_AG['De'], D_AG['QK'], tp['R']
    pos, gm = K.randn64(g, tp['Nn'], 3, scale=0.5), K.randn64(g, tp['B'], 2, scale=0.3)
    e_in, emod = leaf(K.randn64(g, R, De)), K.randn64(g, tp['B'], 6 * De, scale=0.5)
    Pl = dict(P, edge_emb_b=leaf(P['edge_emb_b']))
    f = K.chain_a(Pl, tp, pos, gm, e_in, emod)
    d0, d1 = K.randn64(g, R, QK), K.randn64(g, R, D)            # gradients of the tanh outputs; the kernel takes those of the arguments
    loss = (f['t0'] * d0).sum() + (f['t1'] * d1).sum()
    ge, gb, get = torch.autograd.grad(loss, [e_in, Pl['edge_emb_b'], f['et']], retain_graph=True)
    W = P['edge_emb_w']
    dt0, dt1 = d0 * (1 - f['t0'].detach() ** 2), d1 * (1 - f['t1'].detach() ** 2)
    dG0, dep0 = K.randn64(g, R, De), K.randn64(g, R, De)
    b = K.bwd_a(P, tp, dt1, dt0, f['xh'].detach(), f['rs'].detach(), emod, dG0, dep0)
    assert rel(b['det'], get) <= AUTOGRAD_TOL and rel(b['de_prev'] - dep0, ge) <= AUTOGRAD_TOL and rel(b['de1'].sum(0), gb) <= AUTOGRAD_TOL
    Gl = leaf(f['G'].detach())
    e1 = F.linear(torch.cat([Gl, e_in.detach()], -1), W, P['edge_emb_b'])
    xh, _ = K.ln_rs(e1)
    m = tp['edge_mol']
    et = xh * (1 + emod[m, De:2 * De]) + emod[m, :De]
    gG = torch.autograd.grad((torch.tanh(F.linear(et, P['le0'])) * d0).sum() + (torch.tanh(F.linear(et, P['le1'])) * d1).sum(), [Gl])[0]
    assert rel(b['dG'] - dG0, gG) <= AUTOGRAD_TOL
    # the 2-D form: the same chain with LayerNorm1 on e itself
    e2 = leaf(K.randn64(g, R, De))
    f2 = K.chain_a_2d(P, tp, e2, emod)
    g2 = torch.autograd.grad((f2['t0'] * d0).sum() + (f2['t1'] * d1).sum(), [e2])[0]
    b2 = K.bwd_a_2d(P, tp, d1 * (1 - f2['t1'].detach() ** 2), d0 * (1 - f2['t0'].detach() ** 2), f2['xh'].detach(), f2['rs'].detach(), emod, dep0)
    assert rel(b2['de_prev'] - dep0, g2) <= AUTOGRAD_TOL


def test_node_ln_mod_bwd_is_the_gradient_of_node_ln_mod():
    g = torch.Generator().manual_seed(4)
    rows, Fw, B = 9, 128, 3
    row_mol = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2])
    a, res, mods = leaf(K.randn64(g, rows, Fw)), leaf(K.randn64(g, rows, Fw)), K.randn64(g, B, 6 * Fw, scale=0.5)
    f = K.node_ln_mod(a, res, row_mol, mods, 2 * Fw, 3 * Fw, 4 * Fw)
    dy, dx0 = K.randn64(g, rows, Fw), K.randn64(g, rows, Fw)
    ga, gr = torch.autograd.grad((f['y'] * dy).sum(), [a, res])
    b = K.node_ln_mod_bwd(dy, f['xh'].detach(), f['rs'].detach(), row_mol, mods, 4 * Fw, dx0)
    assert rel(b['dx'] - dx0, ga) <= AUTOGRAD_TOL
    assert rel((b['dx'] - dx0) * mods[row_mol][:, 2 * Fw:3 * Fw], gr) <= AUTOGRAD_TOL


@pytest.mark.parametrize('XH', [2, 0])
def test_attn_bwd_is_the_gradient_of_attn_fwd(XH):
    g = torch.Generator().manual_seed(6)
    nn, D, H = [1, 2, 5, 3], 128, 16
    SC = D // (H - XH) if XH == 0 else (H * (D // H)) // (H - XH)
    QK = (H - XH) * SC
    tp = K.mol_topo(nn)
    q, k, v = leaf(K.randn64(g, tp['Nn'], QK)), leaf(K.randn64(g, tp['Nn'], QK)), leaf(K.randn64(g, tp['Nn'], D))
    z0, z1 = leaf(K.randn64(g, tp['R'], QK)), leaf(K.randn64(g, tp['R'], D))
    adj2d, adjsp = (torch.rand(tp['R'], generator=g) < 0.7).double(), (torch.rand(tp['R'], generator=g) < 0.7).double()
    t0, t1 = torch.tanh(z0), torch.tanh(z1)
    f = K.attn_fwd(nn, H, XH, SC, q, k, v, t0, t1, adj2d, adjsp)
    dh = K.randn64(g, tp['Nn'], D)
    want = torch.autograd.grad((f['hhat'] * dh).sum(), [q, k, v, z0, z1])
    b = K.attn_bwd(nn, H, XH, SC, dh, q.detach(), k.detach(), v.detach(), t0.detach(), t1.detach(), f['alpha'].detach())
    for name, w in zip(('dq', 'dk', 'dv', 'dt0', 'dt1'), want):
        assert rel(b[name], w) <= AUTOGRAD_TOL, name
    assert bool((f['alpha'][tp['edge_a'] == tp['edge_c']] == 0).all())


def test_gbf_bwd_is_the_gradient_of_the_gaussian_layer():
    g = torch.Generator().manual_seed(7)
    R, De, B = 70, 32, 4
    P = K.rand_params(K.dims(128, 2, 126, 3, 8), 9)
    row_mol = torch.sort(torch.randint(0, B, (R,), generator=g)).values
    d2, gm = leaf(K.randn64(g, R).abs()), K.randn64(g, B, 2, scale=0.3)
    means, stds = leaf(P['gbf_means']), leaf(P['gbf_stds'])
    G = K.gauss(d2 * (gm[row_mol, 0] + 1) + gm[row_mol, 1], means, stds)
    dG, dd0 = K.randn64(g, R, De), K.randn64(g, R)
    gd, gmn, gsd = torch.autograd.grad((G * dG).sum(), [d2, means, stds])
    b = K.gbf_bwd(d2.detach(), row_mol, gm, P['gbf_means'], P['gbf_stds'], dG, dd0)
    assert rel(b['dd2'] - dd0, gd) <= AUTOGRAD_TOL and rel(b['part_m'].sum(0), gmn) <= AUTOGRAD_TOL and rel(b['part_s'].sum(0), gsd) <= AUTOGRAD_TOL
    assert b['part_m'].shape == (3, De - 1) and bool((P['gbf_stds'] < 0).any())
    assert rel(b['dxp'] * (gm[row_mol, 0] + 1), gd) <= AUTOGRAD_TOL

"""CPU checks behind tests/test_cdgs_kernels_gpu.py (the launch sequences of the CDGS training step one by one against float64):

  * the anchors of the yardstick: the forward restatements of tests/cdgs_kernels_common.py, composed into the prologue and one block,
    are the dense oracle (oracle_cdgs.forward / oracle_cdgs_train.forward_drop) in float64, with and without dropout masks, alpha and
    the xhat of norm2_edge included; every backward restatement is autograd through its own forward restatement;
  * the test entry jodo_cdgs_train_debug_op through the host emulation build of the same kernel source (tests/emulcdgs), on the small
    shapes (N <= 12, column sums up to 6 209 rows), with the comparisons, guard bands and refusals of the device file;
  * the conditions on the inputs, decided by the float64 restatement alone;
  * the name lists of jodo_amd.capi against the header's enums."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import cdgs_kernels_common as K
import cdgs_train_common as C
import oracle_cdgs as OC
import oracle_cdgs_train as OCT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, 'tests', 'emulcdgs')


@pytest.fixture(scope='module')
def hs():
    subprocess.run(['make', '-C', EMUL_DIR, 'libjodo_cdgs_train_emul.so'], check=True, capture_output=True)
    h = K.Harness('cpu', ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_cdgs_train_emul.so')))
    yield h
    print('worst err / bound per op (host emulation): ' + ', '.join('%s %.3f' % kv for kv in sorted(h.ratios.items())))


def test_name_lists_are_the_headers_enums():
    from jodo_amd import capi
    text = open(os.path.join(ROOT, 'include', 'jodo_hip.h')).read()
    names = re.findall(r'JODO_CT_(\w+)', ' '.join(re.findall(r'enum \{ (JODO_CT_[^}]*)\}', text)))
    ops = [n for n in names if n.startswith('OP_')]
    slots = [n for n in names if not n.startswith('OP_') and not n.startswith('N_')]
    assert tuple(ops) == capi.CT_OPS and tuple(slots) == capi.CT_SLOTS
    assert sorted('OP_' + k for k in K.OPS) == sorted(capi.CT_OPS)


# ---- anchors ----------------------------------------------------------------------------------------------------------------------------
def block_from_restatements(sd, pre, c, h, e, adj, temb_act, seed, p, layer=0):
    """One HybridMPBlock as the step runs it: the restated ops in the step's order, plain float64 Linears between them.
    -> (h, e, alpha, xhat of norm2_edge)"""
    lin = OC._lin
    geo = dict(n_nodes=c['n_nodes'], N=c['N'], isc=K.ISC)
    op = lambda name, **kw: K.restate(name, dict(geo, **kw), torch.float64)
    drop = lambda site: dict(drop_p=p, drop_seed=seed, drop_site=8 * layer + site)
    B, N = c['B'], c['N']
    he = op('ADDT', mode=2, X=e.reshape(B * N * N, -1), TB=lin(sd, pre + 't_edge', temb_act))['Y'].reshape(e.shape)
    hs_ = op('ADDT', mode=1, X=h.reshape(B * N, -1), TB=lin(sd, pre + 't_node', temb_act))['Y'].reshape(h.shape)
    agg = op('GINE', EPS=sd[pre + 'local_model.eps'], HS=hs_, HE=he, ADJ=adj)['AGG']
    g1 = op('RELU', X=lin(sd, pre + 'local_model.nn.0', agg).reshape(B * N, -1))['Y'].reshape(h.shape)
    loc = lin(sd, pre + 'local_model.nn.2', g1)
    gn = lambda name, **kw: op('GN_FWD', GAMMA=sd[pre + name + '.weight'], BETA=sd[pre + name + '.bias'], **kw)
    hc = gn('norm1_local', H=h, A=loc, amask=1, **drop(1))['Y']
    q, k, v = (lin(sd, pre + 'self_attn.lin_' + n, hs_) for n in ('query', 'key', 'value'))
    g0, g1e = torch.tanh(lin(sd, pre + 'self_attn.lin_edge0', he)), torch.tanh(lin(sd, pre + 'self_attn.lin_edge1', he))
    att = op('ATTN_FWD', Q=q, K=k, V=v, G0=g0, G1=g1e)
    hc = gn('norm1_attn', H=h, A=att['ATT'], acc=1, Y=hc, **drop(2))['Y']
    a1 = F.silu(lin(sd, pre + 'ff_linear1', hc)) * K.multipliers(drop(3), (B, N, 2 * h.shape[-1]), torch.float64)
    h_out = gn('norm2_node', H=hc, A=lin(sd, pre + 'ff_linear2', a1), **drop(4))['Y']
    pair = op('PAIR', X=hc)['Y']
    a3 = F.silu(lin(sd, pre + 'ff_linear3', pair)) * K.multipliers(drop(5), (B, N, N, 2 * h.shape[-1]), torch.float64)
    f4 = op('SCALE', mode=0, X=lin(sd, pre + 'ff_linear4', a3).reshape(B * N * N, -1), **drop(6))['Y'].reshape(e.shape)
    en = op('EGN_FWD', XHAT=f4 + e, GAMMA=sd[pre + 'norm2_edge.weight'], BETA=sd[pre + 'norm2_edge.bias'])
    return h_out, en['Y'], att['ALPHA'], en['XHAT']


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_forward_restatements_compose_into_the_oracle(p):
    c = C.random_case('w12')
    _, _, sd = C.model_for('qm9')
    sd64 = {k: v.double() for k, v in sd.items()}
    hp = c['hp']
    seed = 4242
    masks_ = OCT.drop_masks(seed, p, c['B'], c['N'], hp.n_layers, hp.nf) if p > 0 else None
    args = (sd64, hp, c['t'], c['x'], c['nm'], c['em'], c['ex'])
    taps = []
    with torch.no_grad():
        _, _, states = OCT.forward_drop(*args, drop=masks_, return_blocks=True, taps=taps)
        if p == 0:
            plain = OC.forward(*args, return_blocks=True, return_rw=True)
            assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(states, plain[2]))
            rw = K.rw_restate(c['ex'], c['n_nodes'], c['N'], hp.rw_depth, torch.float64)
            land, code = plain[3]
            assert torch.equal(rw['CNT'], code.double()) and torch.equal(rw['ADJ'], (c['ex'][..., 0] >= 0).double() * c['em'].reshape(rw['ADJ'].shape).double())
            d_rw = max(float((rw['LAND'] - land).abs().max()), float((rw['DEG'] - c['ex'].double().sum(2)).abs().max()))
            print('prologue: restatement against oracle_cdgs.rw_features %.1e' % d_rw)
            assert d_rw <= 1e-15
        temb_act = F.silu(OC._lin(sd64, 'all_modules.1', F.silu(OC._lin(sd64, 'all_modules.0', OC.sinusoid(c['t'].double() * 999, hp.nf)))))
        adj = K.rw_restate(c['ex'], c['n_nodes'], c['N'], hp.rw_depth, torch.float64)['ADJ']
        worst = 0.0
        for l in (0, 1):
            h, e, alpha, xhat = block_from_restatements(sd64, 'all_modules.%d.' % (10 + 3 * l), c, states[l][0], states[l][1], adj, temb_act, seed, p, l)
            for what, got, want in (('h', h, states[l + 1][0]), ('e', e, states[l + 1][1]), ('alpha', alpha, taps[l]['alpha']), ('xhat', xhat, taps[l]['xhat'])):
                dist = float((got - want).abs().max()) / float(want.abs().max())
                print('block %d from the restatements against the oracle, dropout %g: %-5s %.1e of max |.| = %.2f' % (l, p, what, dist, float(want.abs().max())))
                worst = max(worst, dist)
    assert worst <= 1e-13                                        # float64 rounding (F.group_norm against the plain two-pass statistics)


def test_backward_restatements_are_autograd_through_the_forward_restatements():
    n_nodes, N = [9, 4, 7, 2], 12
    dist = {}

    def grads(fwd, leaves, douts):
        xs = [v.double().clone().requires_grad_(True) for v in leaves]
        outs = fwd(*xs)
        sum((o * g.double()).sum() for o, g in zip(outs, douts)).backward()
        return [x.grad for x in xs]

    def note(op, pairs):
        dist[op] = max(float((a - b).abs().max() / max(float(b.abs().max()), 1e-300)) for a, b in pairs)

    geo = dict(n_nodes=n_nodes, N=N, isc=K.ISC)
    rs = lambda op, d: K.restate(op, d, torch.float64)
    d = K.conditioned('GINE_BWD', n_nodes, N, 1)
    ghs, ghe = grads(lambda hs_, he: [rs('GINE', dict(d, HS=hs_, HE=he))['AGG']], [d['HS'], d['HE']], [d['DAGG']])
    r = rs('GINE_BWD', d)
    note('GINE_BWD', [(r['DHS'], ghs), (r['DHE'], ghe)])
    d = K.inputs('PAIR_BWD', n_nodes, N, 2)
    (gx,) = grads(lambda x: [rs('PAIR', dict(geo, X=x))['Y']], [torch.randn(4, N, K.D)], [d['X']])
    note('PAIR_BWD', [(rs('PAIR_BWD', d)['Y'], gx)])
    for hard, acc in ((None, 0), (True, 0)):
        d = K.inputs('GN_BWD', n_nodes, N, 3, hard)
        x = torch.randn(4, N, K.D, generator=torch.Generator().manual_seed(3)).double()
        if hard:
            x[:, :, 0:8], x[:, :, 8:16] = 0.375, 1e3 + 1e-2 * torch.randn(4, N, 8, generator=torch.Generator().manual_seed(4)).double()
        f = K.restate('GN_FWD', dict(geo, H=x, A=torch.zeros_like(x), GAMMA=d['GAMMA'], BETA=torch.zeros(K.D)), torch.float64)
        dd = dict(d, XHAT=f['XHAT'], RSTD=f['RSTD'])
        (gx,) = grads(lambda x_: [rs('GN_FWD', dict(geo, H=x_, A=torch.zeros_like(x_), GAMMA=d['GAMMA'], BETA=torch.zeros(K.D)))['Y']], [x], [d['DY']])
        note('GN_BWD' + (' hard' if hard else ''), [(rs('GN_BWD', dd)['DX'], gx)])
        # the norm weights: the masked column sums
        gg, gb = grads(lambda ga, be: [rs('GN_FWD', dict(geo, H=x, A=torch.zeros_like(x), GAMMA=ga, BETA=be))['Y']], [d['GAMMA'], torch.zeros(K.D)], [d['DY']])
        ng = rs('NORM_GRADS', dict(geo, mode=1, DY=d['DY'].reshape(-1, K.D), XHAT=f['XHAT'].reshape(-1, K.D)))
        note('NORM_GRADS mode 1' + (' hard' if hard else ''), [(ng['DBETA'], gb), (ng['DGAMMA'], gg)])
    for hard in (None, 'mean'):
        d = K.inputs('EGN_BWD', n_nodes, N, 5, hard)
        x = K._tile_values(4, N, K.D, torch.Generator().manual_seed(5), hard, n_nodes).double()
        f = rs('EGN_FWD', dict(geo, XHAT=x, GAMMA=d['GAMMA'], BETA=torch.zeros(K.D)))
        gx, gg, gb = grads(lambda x_, ga, be: [rs('EGN_FWD', dict(geo, XHAT=x_, GAMMA=ga, BETA=be))['Y']], [x, d['GAMMA'], torch.zeros(K.D)], [d['DY']])
        note('EGN_BWD' + (' hard' if hard else ''), [(rs('EGN_BWD', dict(d, XHAT=f['XHAT'], RSTD=f['RSTD']))['DX'], gx)])
        ng = rs('NORM_GRADS', dict(geo, mode=2, DY=d['DY'].reshape(-1, K.D), XHAT=f['XHAT'].reshape(-1, K.D)))
        note('NORM_GRADS mode 2' + (' hard' if hard else ''), [(ng['DBETA'], gb), (ng['DGAMMA'], gg)])
    for hard in (None, True):
        d = K.conditioned('ATTN_BWD', n_nodes, N, 7, hard)
        t0, t1 = torch.atanh(d['G0'].double().clamp(-1 + 1e-12, 1 - 1e-12)), torch.atanh(d['G1'].double().clamp(-1 + 1e-12, 1 - 1e-12))
        dd = dict(d, G0=torch.tanh(t0), G1=torch.tanh(t1))
        dd['ALPHA'] = rs('ATTN_FWD', dd)['ALPHA']
        fwd = lambda q, k, v, a, b: [rs('ATTN_FWD', dict(dd, Q=q, K=k, V=v, G0=torch.tanh(a), G1=torch.tanh(b)))['ATT']]
        gq, gk, gv, g0, g1 = grads(fwd, [d['Q'], d['K'], d['V'], t0, t1], [d['DATT']])
        r = rs('ATTN_BWD', dd)
        note('ATTN_BWD' + (' hard' if hard else ''), [(r['DQ'], gq), (r['DK'], gk), (r['DV'], gv), (r['DT0'], g0), (r['DT1'], g1)])
        # d logit: the gradient of an offset added to the logits
        (gl,) = grads(lambda z: [rs('ATTN_FWD', dict(dd, LOGIT_OFFSET=z))['ATT']], [torch.zeros(4, N, N, K.H)], [d['DATT']])
        note('ATTN_BWD d logit' + (' hard' if hard else ''), [(r['DAL'], gl)])
    for k, v in dist.items():
        print('backward restatement against autograd, %-24s relative distance %.1e' % (k, v))
    assert max(dist.values()) <= 1e-12, dist


# ---- the conditions on the inputs: the yardstick alone ---------------------------------------------------------------------------------------
def test_input_conditions_hold_on_the_float64_restatement():
    for n_nodes, N in K.SMALL + K.WIDE[:2]:
        d = K.conditioned('GINE_BWD', n_nodes, N, K.case_seed('GINE_BWD', N, 0))
        assert K.relu_margin(d) > K.RELU_MARGIN
        for i, (tag, hard, kw) in enumerate(K.VARIANTS['RW']):
            d = K.conditioned('RW', n_nodes, N, K.case_seed('RW', N, i), hard)
            assert K.rw_decided(d), (tag, N)
    for n_nodes, N in K.SMALL[2:]:
        for op in ('ATTN_FWD', 'ATTN_BWD'):
            d = K.conditioned(op, n_nodes, N, K.case_seed(op, N, 1), True)
            assert K.sharp_heads(d), (op, N)
            logit = K.attn_alpha(d['Q'].double(), d['K'].double(), d['G0'].double(), K.masks(n_nodes, N)[1], K.ISC)[1]
            assert float(logit[..., 0].nan_to_num(neginf=0.0).abs().max()) == 0.0           # head 0: all logits equal
            assert 55 < float(logit.nan_to_num(neginf=0.0).abs().max()) < 120, float(logit.nan_to_num(neginf=0.0).abs().max())
    # n = 1: no source, alpha exactly 0; n = 2: one source, alpha = 1 / (1 + 1e-16)
    d = K.inputs('ATTN_FWD', [2, 1], 2, 1, True)
    al = K.restate('ATTN_FWD', d)['ALPHA']
    assert float(al[1].abs().max()) == 0.0 and float(al[0, 1, 0, 3]) == 1.0 / (1.0 + 1e-16) and float(al[0, 0, 0].abs().max()) == 0.0


def test_one_row_cases_carry_the_whole_sum():
    """dy non-zero on ONE live row: the float64 column sums ARE that row, so a lost tail, chunk or group shows at full size"""
    seen = set()
    for rows, mode, one in K.norm_grads_cases():
        if one is None:
            continue
        n_nodes, N = K.norm_grads_geometry(rows, mode)
        assert float(K.live_rows(dict(n_nodes=n_nodes, N=N, mode=mode), rows, torch.float64)[one]) == 1.0
        seen.add(('last', rows) if one == max(K.single_rows(rows, mode, n_nodes, N)) else ('second group' if one >= 2048 else 'other', rows))
    assert ('last', 2113) in seen and ('second group', 2113) in seen and ('last', K.COLSUM_GROUPS) in seen
    rows = K.COLSUM_GROUPS
    assert (rows + 63) // 64 == 98 and 98 // 32 == 3 and 98 % 32 == 2 and rows % 64 == 1


# ---- the entry through the host emulation build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', range(len(K.SMALL)))
@pytest.mark.parametrize('op', K.TILED)
def test_every_op_through_the_emulation_build(hs, op, shape):
    n_nodes, N = K.SMALL[shape]
    K.run_variants(hs, op, n_nodes, N)


@pytest.mark.parametrize('rows,mode,one_row', K.norm_grads_cases())
def test_column_sums_through_the_emulation_build(hs, rows, mode, one_row):
    K.run_norm_grads(hs, rows, mode, one_row)


@pytest.mark.parametrize('op', ['ATTN_FWD', 'EGN_FWD', 'GINE'])
def test_each_molecule_alone_through_the_emulation_build(hs, op):
    K.molecule_alone(hs, op, [9, 4, 7, 2], 12, 31)


def test_hard_sets_end_where_they_must(hs):
    """n = 1: alpha exactly 0; n = 2: 1 / (1 + 1e-16) = 1 in float32; equal channels / a constant tile: xhat exactly 0, rstd 1 / sqrt(1e-6);
    EGN with an n = 1 molecule: nothing live, e_out and d pre exactly 0 there whatever the padded rows hold"""
    (_, d, got, _), = K.run_variants(hs, 'ATTN_FWD', [2, 1], 2, [('hard', True, {})])
    assert K.is_zero(got['ALPHA'][1]) and K.is_zero(got['ATT'][1]) and bool((got['ALPHA'][0, 1, 0] == 1.0).all()) and bool((got['ALPHA'][0, 0, 1] == 1.0).all())
    (_, d, got, _), = K.run_variants(hs, 'GN_FWD', [12, 1, 5], 12, [('hard', True, {})])
    assert K.is_zero(got['XHAT'][:, :, 0:8]) and float((got['RSTD'][:, :, 0] - 1000).abs().max()) < 1e-3
    (_, d, got, _), = K.run_variants(hs, 'EGN_FWD', [12, 1, 5], 12, [('constant', 'constant', {})])
    assert K.is_zero(got['XHAT'][0]) and float((got['RSTD'][0] - 1000).abs().max()) < 1e-3 and K.is_zero(got['Y'][1])
    (_, d, got, _), = K.run_variants(hs, 'EGN_BWD', [12, 1, 5], 12, [('benign', None, {})])
    assert K.is_zero(got['DX'][1]) and not K.is_zero(got['DX'][2][5:])          # n = 1: nothing live; n = 5: the padded rows carry gradient


def test_entry_refusals_through_the_emulation_build(hs):
    K.refusals(hs)

"""The float64 restatement of the classifier's two fused edge kernels (tests/egnn_kernels_common.py) is anchored here, on the CPU:
  * every backward array equals torch.autograd.grad through the forward part (ez1 / ez2: the gradients of retained z1 / z2; Q / qb: the
    gradients of per-row-atom copies of wr, wa, ba), with and without attention;
  * on the four fixture cases of tests/egnn_train_common.py, P built from `embedding` and `edge_mlp.0` of the seeded state dict and the
    restated agg put through node_mlp reproduce the first hidden state of oracle_egnn.forward at float64;
  * the inputs of the GPU tests' saturating, geometry and zero-row regimes do what they are there for (evaluated on the restatement
    alone, so they are known good before a GPU is involved);
  * the test entry jodo_egnn_debug_edge refuses bad arguments before it touches a device.
tests/test_egnn_kernels_gpu.py then holds the kernels against these functions."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import egnn_kernels_common as K
import egnn_train_common as C
import oracle_egnn as OE

# both sides are float64 evaluations of the same expression in another association: a few hundred ulps at most, relative to the array's
# largest entry (measured 2e-16 .. 5e-16); a wrong formula is off by 1e-2 or more
TOL = 1e-12


@pytest.mark.parametrize('att', [True, False])
def test_backward_restatement_is_autograd_through_the_forward_restatement(att):
    n_nodes, nf = [1, 2, 5, 9], 64
    d = K.inputs(n_nodes, nf, 5, att)
    r = K.restate(d['P'], d['xc'], d['wr'], d['W2'], d['b2'], d['wa'], d['ba'], n_nodes, d['dagg'], torch.float64)
    dd = {k: (None if v is None else v.double()) for k, v in d.items()}
    P = dd['P'].clone().requires_grad_(True)
    Nn = sum(n_nodes)
    wr_rows = dd['wr'].expand(Nn, nf).clone().requires_grad_(True)
    wa_rows = dd['wa'].expand(Nn, nf).clone().requires_grad_(True) if att else None
    ba_rows = dd['ba'].expand(Nn).clone().requires_grad_(True) if att else None
    loss, z1s, z2s, masks, t = 0.0, [], [], [], 0
    for n in n_nodes:
        f = K.fwd_rows(P[t:t + n], dd['xc'][t:t + n], 0, n, wr_rows[t:t + n], dd['W2'], dd['b2'], wa_rows[t:t + n] if att else None,
                       ba_rows[t:t + n] if att else None)
        f['z1'].retain_grad()
        f['z2'].retain_grad()
        z1s.append(f['z1'])
        z2s.append(f['z2'])
        masks.append(f['mask'])
        assert float((f['agg'].detach() - r['agg'][t:t + n]).abs().max()) <= TOL * float(r['agg'].abs().max())
        loss = loss + (f['agg'] * dd['dagg'][t:t + n]).sum()
        t += n
    loss.backward()
    want = dict(dP=P.grad, ez1=torch.cat([z.grad[m] for z, m in zip(z1s, masks)]), ez2=torch.cat([z.grad[m] for z, m in zip(z2s, masks)]),
                Q=torch.cat([wr_rows.grad, wa_rows.grad if att else torch.zeros(Nn, nf, dtype=torch.float64)], 1),
                qb=ba_rows.grad if att else torch.zeros(Nn, dtype=torch.float64))
    for k, w in want.items():
        scale = max(float(w.abs().max()), 1e-300)
        err = float((r[k] - w).abs().max())
        print("%s: |restated - autograd| / scale %.2e" % (k, err / scale))
        assert r[k].shape == w.shape and err <= TOL * scale, k
    for z, m in zip(z1s + z2s, masks + masks):                # the masked pairs (j = i) carry no gradient at all
        assert float(z.grad[~m].abs().max()) == 0.0 if (~m).any() else True


@pytest.mark.parametrize('tag', C.CASES)
def test_forward_restatement_composed_with_node_mlp_is_the_oracles_first_layer(tag):
    _, st, sd, h0, x, n_nodes, _ = C.case(tag)
    nf, att = st['hidden_nf'], bool(st['attention'])
    with torch.no_grad():
        _, hidden = OE.forward(sd, st, h0, x, n_nodes, torch.float64)
        s = {k: v.double() for k, v in sd.items()}
        real = torch.cat([torch.arange(n) + b * h0.shape[1] for b, n in enumerate(n_nodes)])
        a0 = h0.double().reshape(-1, h0.shape[2])[real]
        xc = x.double().reshape(-1, 3)[real]
        h = F.linear(a0, s['embedding.weight'], s['embedding.bias'])
        w0, b0 = s['gcl_0.edge_mlp.0.weight'], s['gcl_0.edge_mlp.0.bias']
        P = torch.cat([h @ w0[:, :nf].t() + b0, h @ w0[:, nf:2 * nf].t()], 1)
        r = K.restate(P, xc, w0[:, 2 * nf], s['gcl_0.edge_mlp.2.weight'], s['gcl_0.edge_mlp.2.bias'], s['gcl_0.att_mlp.0.weight'][0] if att else None,
                      s['gcl_0.att_mlp.0.bias'] if att else None, n_nodes, None, torch.float64)
        feats = [h, r['agg']] + ([a0] if st['node_attr'] else [])
        t = F.silu(F.linear(torch.cat(feats, 1), s['gcl_0.node_mlp.0.weight'], s['gcl_0.node_mlp.0.bias']))
        h1 = h + F.linear(t, s['gcl_0.node_mlp.2.weight'], s['gcl_0.node_mlp.2.bias'])
    err, scale = float((h1 - hidden[0]).abs().max()), float(hidden[0].abs().max())
    print("%s: |composed - oracle| / scale %.2e" % (tag, err / scale))
    assert err <= TOL * scale


@pytest.mark.parametrize('att', [True, False])
@pytest.mark.parametrize('nf', K.NFS)
def test_saturating_inputs_saturate(nf, att):
    d = K.inputs(K.MAIN, nf, K.seed('saturating', nf), att, 'saturating')
    r64 = K.restate(d['P'], d['xc'], d['wr'], d['W2'], d['b2'], d['wa'], d['ba'], K.MAIN, d['dagg'], torch.float64, keep=True)
    r32 = K.restate(d['P'], d['xc'], d['wr'], d['W2'], d['b2'], d['wa'], d['ba'], K.MAIN, d['dagg'], torch.float32)
    rep = K.saturation_report(r64, att)
    print(nf, att, rep)
    K.assert_saturating(rep, att, 'nf %d' % nf)
    for k in ('agg', 'ea', 'ez2', 'ez1', 'dP', 'Q', 'qb'):
        assert bool(torch.isfinite(r64[k]).all()) and bool(torch.isfinite(r32[k]).all()), k
        scale = float(r64[k].abs().max())
        print("  %s: scale %.3e, float32 restatement %.2e of it" % (k, scale, float((r32[k].double() - r64[k]).abs().max()) / max(scale, 1e-300)))


def test_geometry_and_zero_row_inputs():
    n_nodes = K.MAIN
    noff, eoff, Nn, E = K.edge_offsets(n_nodes)
    assert (Nn, E) == (266, 12300)
    d = K.inputs(n_nodes, 64, 1, True, 'geometry')
    b = n_nodes.index(34)
    xm = d['xc'][noff[b]:noff[b] + 34, :3].double()
    rad = (xm[:, None] - xm[None]).square().sum(-1)
    assert int((rad == 0).sum()) == 34 + 2 and float(rad.max()) > 9e3
    r = K.restate(d['P'], d['xc'], d['wr'], d['W2'], d['b2'], d['wa'], d['ba'], n_nodes, d['dagg'], torch.float64)
    assert all(bool(torch.isfinite(v).all()) for v in r.values())
    d = K.inputs(n_nodes, 64, 1, True, 'zero_row')
    t = K.zero_row_atom(n_nodes)
    b = n_nodes.index(33)
    assert t == noff[b] + 32 and float(d['dagg'][t].abs().max()) == 0.0 and float(d['dagg'][t - 1].abs().max()) > 0
    r = K.restate(d['P'], d['xc'], d['wr'], d['W2'], d['b2'], d['wa'], d['ba'], n_nodes, d['dagg'], torch.float64)
    e0 = eoff[b] + 32 * 32
    for k, v in (('dP', r['dP'][t, :64]), ('Q', r['Q'][t]), ('qb', r['qb'][t]), ('ez1', r['ez1'][e0:e0 + 32]), ('ez2', r['ez2'][e0:e0 + 32])):
        assert float(v.abs().max()) == 0.0, k
    assert float(r['dP'][t, 64:].abs().max()) > 0 and float(r['ez1'][e0 - 1].abs().max()) > 0       # the atom as a source still counts


def test_binding_lists_follow_the_header():
    from jodo_amd import capi
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'jodo_hip.h')) as f:
        txt = f.read()
    enums = re.findall(r'enum \{ (JODO_ET_[^}]*)\}', txt)
    assert len(enums) == 2
    names = [[n.strip().split(' ')[0].replace('JODO_ET_', '') for n in e.split(',')] for e in enums]
    assert names[0] == list(capi.ET_OPS) + ['N_OPS']
    assert names[1] == list(capi.ET_SLOTS) + ['N_SLOTS']


def test_entry_refuses_bad_arguments_before_it_touches_a_device():
    """Pointers are made-up aligned addresses: every call here must return before anything dereferences them."""
    from jodo_amd import capi
    ARG, UNSUPPORTED = -1, -3
    nf = 64

    def args(op, n_nodes, nf=nf, att=True, fix=None):
        n = np.asarray(n_nodes, dtype=np.int32)
        Nn, E = int(n.sum()), int((n * (n - 1)).sum())
        a = capi.EgnnEdgeTestArgs()
        a.op, a.nf, a.B, a.grid_cap, a.n_nodes = op, nf, len(n), 0, n.ctypes.data
        cnt = dict(P=Nn * 2 * nf, XC=Nn * 4, DAGG=Nn * nf, WR=nf, W2=nf * nf, B2=nf, WA=nf, BA=1, DESC=3 * len(n) + Nn, IMG=2 * nf * nf, AGG=Nn * nf,
                   EA=E * nf, EZ2=E * nf, EZ1=E * nf, DP=Nn * 2 * nf, Q=Nn * 2 * nf, QB=Nn)
        for i, k in enumerate(capi.ET_SLOTS):
            if not att and k in ('WA', 'BA'):
                continue
            a.a[i], a.n[i] = 0x10000 * (i + 1), cnt[k]
        for k, (p, c) in (fix or {}).items():
            i = capi.ET_SLOTS.index(k)
            a.a[i] = a.a[i] if p is None else p
            a.n[i] = a.n[i] if c is None else c
        return a, n

    def call(*ar, **kw):
        a, keep = args(*ar, **kw)
        rc = capi.egnn_debug_edge(a)
        return rc, capi.lib().jodo_last_error().decode()

    rc, msg = call(1, [3, 4], nf=96)
    assert rc == UNSUPPORTED and 'hidden_nf 96' in msg, msg
    rc, msg = call(1, [3, 0])
    assert rc == ARG and 'n_nodes[1] = 0' in msg, msg
    rc, msg = call(0, [256])
    assert rc == UNSUPPORTED and 'n_nodes[0] = 256' in msg, msg
    rc, msg = call(1, [3, 4], fix=dict(EZ1=(None, 18 * nf - 1)))
    assert rc == ARG and 'array ez1 has %d elements, the op touches %d' % (18 * nf - 1, 18 * nf) in msg, msg
    rc, msg = call(0, [3, 4], fix=dict(AGG=(None, 7 * nf + 1)))
    assert rc == ARG and 'array agg has' in msg, msg
    rc, msg = call(0, [3, 4], fix=dict(IMG=(None, 2 * nf * nf - 1)))
    assert rc == ARG and 'array img has' in msg, msg
    rc, msg = call(1, [3, 4], fix=dict(DAGG=(0x20004, None)))
    assert rc == ARG and 'array dagg is not 16-byte aligned' in msg, msg
    rc, msg = call(1, [3, 4], fix=dict(P=(0, None)))
    assert rc == ARG and 'array p is a null pointer' in msg, msg
    rc, msg = call(1, [3, 4], fix=dict(BA=(0, None)))       # attention needs both wa and ba
    assert rc == ARG and 'array ba is a null pointer' in msg, msg
    rc, msg = call(2, [3, 4])
    assert rc == ARG and 'unknown op' in msg, msg
    a, keep = args(0, [3])
    a.grid_cap = -1
    assert capi.egnn_debug_edge(a) == ARG
    a.grid_cap, a.B = 0, 0
    assert capi.egnn_debug_edge(a) == ARG

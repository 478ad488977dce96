"""The two fused edge kernels of the property classifier (csrc/egnn_forward.hip kegnn_edge; csrc/egnn_train.hip kegnn_edge_bwd followed
by kegnn_tgt_sum) on their own against float64, through the test entry jodo_egnn_debug_edge.  The network-level tests see the backward
only through parameter gradients, every one a sum over all atoms or edges of the batch; here EVERY element of the seven arrays the
kernels store (agg; ea, ez2, ez1 per edge; dP, Q, qb per atom) is compared with the restatement of tests/egnn_kernels_common.py
(anchored to autograd and to the model by tests/test_egnn_kernels_host.py), in all four instantiations (nf 64, 128: W2 in LDS; 192, 256:
W2 streamed, z2 / dz2 parked in LDS), with and without attention.

Around every call (the harness of tests/test_fused_kernels_gpu.py): outputs start as NaN, every array sits between two guard bands of
512 floats that are compared bit for bit afterwards, inputs must come back unchanged, and the call is repeated and must give the same
bits.  Tolerances are the project's two rules with both yardsticks from the restatement alone: helpers.close64 for agg and ea, the
gradient rule |got - r64| <= max(GRAD_REL max |r64|, K32 max |r32 - r64|) for the others (dP and Q by halves: P_src / P_tgt and
dw_r / dw_a are different quantities).  No array needed a bound of its own.

Shapes: MAIN = [1, 2, 33, 1, 31, 32, 34, 65, 64, 3] (266 atoms: no multiple of 4; molecule boundaries inside the 4-wave workgroups;
n = 33 gives row atom 32 a last chunk whose only lane is its own, masked one; 31 .. 34 and 64 / 65 straddle the 32-source chunk; n = 1
has no sources); n = 255 and 224 (eight chunks, the last with 31 sources / seven full chunks; compact edge rows up to 64 770 per
molecule); [1, 1, 1] (no edge at all)."""
import ctypes

import numpy as np
import pytest
import torch

import egnn_kernels_common as K
from test_fused_kernels_gpu import DEV, Buf, check_bwd, check_fwd

pytestmark = pytest.mark.gpu

IN_SLOTS = ('P', 'XC', 'DAGG', 'WR', 'W2', 'B2', 'WA', 'BA')
OUT_SLOTS = {0: ('AGG',), 1: ('EA', 'EZ2', 'EZ1', 'DP', 'Q', 'QB')}
ARG, UNSUPPORTED = -1, -3


def capi():
    from jodo_amd import capi as c
    return c


class Case:
    """The guarded device arrays of one (inputs, n_nodes, nf): inputs, scratch, NaN-poisoned outputs."""

    def __init__(self, d, n_nodes, nf):
        self.n_nodes, self.nf = list(n_nodes), nf
        _, _, Nn, E = K.edge_offsets(n_nodes)
        self.Nn, self.E, self.att = Nn, E, d['wa'] is not None
        self.ins = {k.upper(): Buf(v) for k, v in d.items() if v is not None}
        self.scratch = dict(DESC=Buf((3 * len(n_nodes) + Nn,)), IMG=Buf((2 * nf * nf,)))
        self.outs = dict(AGG=Buf((Nn, nf)), EA=Buf((E, nf)), EZ2=Buf((E, nf)), EZ1=Buf((E, nf)), DP=Buf((Nn, 2 * nf)), Q=Buf((Nn, 2 * nf)), QB=Buf((Nn,)))
        self.bufs = list(self.ins.values()) + list(self.scratch.values()) + list(self.outs.values())

    def call(self, op, grid_cap=0, nf=None, n_nodes=None, override=None):
        """-> (return code, error text).  override: slot -> (tensor view or None, element count or None) in place of the Buf's own."""
        c = capi()
        a = c.EgnnEdgeTestArgs()
        n = np.ascontiguousarray(self.n_nodes if n_nodes is None else n_nodes, dtype=np.int32)
        a.op, a.nf, a.B, a.grid_cap, a.n_nodes = op, self.nf if nf is None else nf, len(n), grid_cap, n.ctypes.data
        slots = dict(self.ins)
        slots.update(self.scratch)
        slots.update(self.outs)
        for name, b in slots.items():
            i = c.ET_SLOTS.index(name)
            view, cnt = (override or {}).get(name, (None, None))
            a.a[i] = (b.view if view is None else view).data_ptr()
            a.n[i] = b.view.numel() if cnt is None else cnt
        rc = c.egnn_debug_edge(a, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        msg = c.lib().jodo_last_error()
        return rc, (msg.decode() if msg else '')

    def intact(self, what):
        assert all(b.guards_ok() for b in self.bufs), "%s: a guard band was written" % what
        for k, b in self.ins.items():
            assert torch.equal(b.bits(), b.init.view(torch.int32)), "%s: the input %s was modified" % (what, k)

    def run(self, op, grid_cap=0, what=''):
        """One op, twice: -> slot -> stored array (CPU).  Guards, inputs, NaN left behind and run-to-run bits are checked here."""
        names = OUT_SLOTS[op]
        for b in self.outs.values():
            b.reset()
        rc, msg = self.call(op, grid_cap)
        assert rc == 0, "%s: %s" % (what, msg)
        got = {k: self.outs[k].view.detach().cpu().clone() for k in names}
        first = {k: self.outs[k].bits() for k in names}
        self.intact(what)
        for k in names:
            assert not bool(torch.isnan(got[k]).any()), "%s: %s has elements the kernel never wrote (or NaN)" % (what, k)
        for k in self.outs:                                  # the other op's arrays keep their NaN
            if k not in names:
                assert bool(torch.isnan(self.outs[k].view).all()), "%s: %s was written by the wrong op" % (what, k)
        for b in self.outs.values():
            b.reset()
        rc, msg = self.call(op, grid_cap)
        assert rc == 0, "%s (second run): %s" % (what, msg)
        for k in names:
            assert torch.equal(self.outs[k].bits(), first[k]), "%s: %s differs between two runs" % (what, k)
        self.intact(what + ' (second run)')
        return got


def both(d, n_nodes, **kw):
    args = (d['P'], d['xc'], d['wr'], d['W2'], d['b2'], d['wa'], d['ba'], n_nodes, d['dagg'])
    return K.restate(*args, dtype=torch.float32), K.restate(*args, dtype=torch.float64, **kw)


def compare(label, fwd, bwd, r32, r64, nf):
    """every stored element against the restatement; empty arrays (no edge) have nothing to compare"""
    check_fwd(label, 'agg', fwd['AGG'], r32['agg'], r64['agg'])
    if r64['ea'].numel():
        check_fwd(label, 'ea', bwd['EA'], r32['ea'], r64['ea'])
        check_bwd(label, 'ez2', bwd['EZ2'], r32['ez2'], r64['ez2'])
        check_bwd(label, 'ez1', bwd['EZ1'], r32['ez1'], r64['ez1'])
    else:
        assert bwd['EA'].numel() == bwd['EZ2'].numel() == bwd['EZ1'].numel() == 0
    check_bwd(label, 'dP.src', bwd['DP'][:, :nf], r32['dP'][:, :nf], r64['dP'][:, :nf])
    check_bwd(label, 'dP.tgt', bwd['DP'][:, nf:], r32['dP'][:, nf:], r64['dP'][:, nf:])
    check_bwd(label, 'Q.wr', bwd['Q'][:, :nf], r32['Q'][:, :nf], r64['Q'][:, :nf])
    check_bwd(label, 'Q.wa', bwd['Q'][:, nf:], r32['Q'][:, nf:], r64['Q'][:, nf:])
    check_bwd(label, 'qb', bwd['QB'], r32['qb'], r64['qb'])


def run_and_compare(label, d, n_nodes, nf, r=None):
    case = Case(d, n_nodes, nf)
    fwd, bwd = case.run(0, what=label + ' forward'), case.run(1, what=label + ' backward')
    r32, r64 = r if r is not None else both(d, n_nodes)
    compare(label, fwd, bwd, r32, r64, nf)
    return case, fwd, bwd, r64


def is_zero(t):
    return bool(((t.contiguous().view(torch.int32) & 0x7FFFFFFF) == 0).all())


# ---- the main batch, every instantiation, with and without attention -------------------------------------------------------------------
@pytest.mark.parametrize('att', [True, False])
@pytest.mark.parametrize('nf', K.NFS)
def test_main_batch_benign(nf, att):
    d = K.inputs(K.MAIN, nf, K.seed('benign', nf), att)
    run_and_compare('edge nf%d att%d benign' % (nf, att), d, K.MAIN, nf)


@pytest.mark.parametrize('att', [True, False])
@pytest.mark.parametrize('nf', K.NFS)
def test_main_batch_saturating(nf, att):
    """exp(-z) beyond float32 in both SiLUs and in the gate, gates at exactly 0 and 1 beside live ones: everything stays finite and inside
    the same two rules.  The conditions that make this regime what it says are asserted on the float64 restatement."""
    d = K.inputs(K.MAIN, nf, K.seed('saturating', nf), att, 'saturating')
    r32, r64 = both(d, K.MAIN, keep=True)
    K.assert_saturating(K.saturation_report(r64, att), att, 'nf %d' % nf)
    _, fwd, bwd, _ = run_and_compare('edge nf%d att%d saturating' % (nf, att), d, K.MAIN, nf, (r32, r64))
    for k, v in list(fwd.items()) + list(bwd.items()):
        assert bool(torch.isfinite(v).all()), "nf %d: %s is not finite" % (nf, k)


@pytest.mark.parametrize('att', [True, False])
@pytest.mark.parametrize('nf', K.NFS)
def test_geometry_edges_and_a_zero_row(nf, att):
    """Two atoms at one position (rad = 0) and one atom 100 units away (rad 1e4: the first SiLU saturates both ways) inside the 34-atom
    molecule; then a row atom whose dagg row is zero: everything it owns is exactly zero, what it gives as a source is not."""
    d = K.inputs(K.MAIN, nf, K.seed('geometry', nf), att, 'geometry')
    run_and_compare('edge nf%d att%d geometry' % (nf, att), d, K.MAIN, nf)
    d = K.inputs(K.MAIN, nf, K.seed('zero_row', nf), att, 'zero_row')
    _, _, bwd, r64 = run_and_compare('edge nf%d att%d zero row' % (nf, att), d, K.MAIN, nf)
    noff, eoff, _, _ = K.edge_offsets(K.MAIN)
    t, b = K.zero_row_atom(K.MAIN), K.MAIN.index(33)
    e0 = eoff[b] + 32 * 32
    assert is_zero(bwd['DP'][t, :nf]) and is_zero(bwd['Q'][t]) and is_zero(bwd['QB'][t]), "the zero row's own sums are not exactly zero"
    assert is_zero(bwd['EZ1'][e0:e0 + 32]) and is_zero(bwd['EZ2'][e0:e0 + 32]), "the zero row's edge rows are not exactly zero"
    assert not is_zero(bwd['DP'][t, nf:]) and not is_zero(bwd['EZ1'][e0 - 1]) and not is_zero(bwd['EA'][e0:e0 + 32])


# ---- wide molecules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nf,n_nodes', [(64, [255, 224]), (192, [255, 1])])
def test_wide_molecules(nf, n_nodes):
    d = K.inputs(n_nodes, nf, K.seed('wide', nf), True)
    run_and_compare('edge nf%d wide' % nf, d, n_nodes, nf)


# ---- no edge at all ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nf', [64, 192])
def test_molecules_of_one_atom(nf):
    n_nodes = [1, 1, 1]
    d = K.inputs(n_nodes, nf, 9, True)
    case = Case(d, n_nodes, nf)
    assert case.E == 0 and case.outs['EZ1'].view.numel() == 0
    fwd, bwd = case.run(0, what='E = 0 forward'), case.run(1, what='E = 0 backward')
    assert is_zero(fwd['AGG']) and is_zero(bwd['DP']) and is_zero(bwd['Q']) and is_zero(bwd['QB'])


# ---- properties, per instantiation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nf', K.NFS)
def test_grid_and_molecule_independence_and_consistency(nf):
    """grid_cap 1 (one workgroup, 67 trips of the persistent loop: the LDS-staged W2, or the per-wave z2 / dz2 columns, are reused across
    trips), 2 and the production cap give the same bits; every molecule alone gives the bits of its rows in the batch; the backward's
    recomputed a, put through the rest of the forward restatement, is the forward kernel's agg (loose: the sharp checks are above)."""
    n_nodes = K.MAIN
    d = K.inputs(n_nodes, nf, K.seed('benign', nf), True)
    case = Case(d, n_nodes, nf)
    base = {}
    for cap in (0, 1, 2):
        got = dict(case.run(0, cap, 'cap %d forward' % cap), **case.run(1, cap, 'cap %d backward' % cap))
        for k, v in got.items():
            if cap == 0:
                base[k] = v
            else:
                assert torch.equal(v.view(torch.int32), base[k].view(torch.int32)), "nf %d: %s differs between grid_cap %d and the production cap" % (nf, k, cap)
    noff, eoff, _, _ = K.edge_offsets(n_nodes)
    for b, n in enumerate(n_nodes):
        t0, e0 = noff[b], eoff[b]
        one = {k: (None if v is None else (v[t0:t0 + n] if k in ('P', 'xc', 'dagg') else v)) for k, v in d.items()}
        alone = Case(one, [n], nf)
        got = dict(alone.run(0, what='molecule %d alone forward' % b), **alone.run(1, what='molecule %d alone backward' % b))
        for k, v in got.items():
            ref = base[k][e0:e0 + n * (n - 1)] if k in ('EA', 'EZ2', 'EZ1') else base[k][t0:t0 + n]
            assert torch.equal(v.view(torch.int32), ref.view(torch.int32)), "nf %d: %s of molecule %d (n = %d) alone differs from the batch" % (nf, k, b, n)
    a32 = K.agg_from_ea(base['EA'], d['W2'], d['b2'], d['wa'], d['ba'], n_nodes, torch.float32)
    a64 = K.agg_from_ea(base['EA'], d['W2'], d['b2'], d['wa'], d['ba'], n_nodes, torch.float64)
    check_fwd('edge nf%d consistency' % nf, 'agg(ea)', base['AGG'], a32, a64)


# ---- the entry refuses what the kernels were not built for ----------------------------------------------------------------------------------
def test_entry_refusals():
    """No kernel runs here: every call comes back with an error code, and every poisoned output still holds its NaN."""
    nf, n_nodes = 64, [3, 4]
    d = K.inputs(n_nodes, nf, 3, True)
    case = Case(d, n_nodes, nf)
    before = {k: b.bits() for k, b in case.outs.items()}
    rc, msg = case.call(1, override=dict(EZ2=(None, 18 * nf + 1)))
    assert rc == ARG and 'array ez2 has %d elements, the op touches %d' % (18 * nf + 1, 18 * nf) in msg, msg
    rc, msg = case.call(0, override=dict(P=(None, 7 * 2 * nf - 1)))
    assert rc == ARG and 'array p has' in msg, msg
    rc, msg = case.call(1, nf=96)
    assert rc == UNSUPPORTED and 'hidden_nf 96' in msg, msg
    rc, msg = case.call(1, n_nodes=[7, 0])
    assert rc == ARG and 'n_nodes[1] = 0' in msg, msg
    rc, msg = case.call(0, n_nodes=[256])
    assert rc == UNSUPPORTED and 'n_nodes[0] = 256' in msg, msg
    rc, msg = case.call(1, n_nodes=[4, 3, 1])               # other counts than the arrays were made for
    assert rc == ARG and 'elements, the op touches' in msg, msg
    odd = case.ins['DAGG'].view.view(-1)[1:]
    rc, msg = case.call(1, override=dict(DAGG=(odd, 7 * nf)))
    assert rc == ARG and 'array dagg is not 16-byte aligned' in msg, msg
    rc, msg = case.call(2)
    assert rc == ARG and 'unknown op' in msg, msg
    torch.cuda.synchronize()
    for k, b in case.outs.items():
        assert torch.equal(b.bits(), before[k]) and bool(torch.isnan(b.view).all()), k
    case.intact('refusals')

"""Every fused training kernel (jodo_amd/csrc/train_fused.hip) on its own against float64, through the test entry
jodo_train_debug_fused (csrc/train_debug.hip).  The network-level tests see these kernels only through parameter gradients and final
outputs; here EVERY array a kernel stores is compared with the restatement of tests/fused_kernels_common.py (anchored to the models by
tests/test_fused_kernels_host.py), at the row counts where the 32-row strips go ragged and with molecule ids changing inside strips.

Around every call: outputs start as NaN (an element never written is seen), every array sits between two guard bands of 512 floats
of a fixed bit pattern that are compared bit for bit afterwards (a tail-lane write past an array's end is seen although the
workspace arena of the training step would have hidden it), inputs must come back unchanged, and the call is repeated and must give
the same bits.

Tolerances are the project's two rules with both yardsticks from the restatement alone: forward arrays helpers.close64 (2e-5 +
1e-4 |x|, or 4 x the float32 restatement's distance from float64), backward arrays the gradient rule |got - r64| <=
max(GRAD_REL max |r64|, K32 max |r32 - r64|) per array.  No op needed a bound of its own."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fused_kernels_common as K
import oracle2d as O2
from helpers import close64, make_config
from train_scale_common import GRAD_REL, K32

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 512, 0x5A5AC3C3
DEV = 'cuda:0'
SEED = (0x1234 << 32) | 0x9E3779B9           # a dropout seed above 2^32: both key words of the generator are in use
RATIOS = {}


def capi():
    from jodo_amd import capi as c
    return c


class Buf:
    """A float32 device array between two guard bands.  init: a CPU tensor (its values are the array's contents before every call) or a
    shape (NaN before every call)."""

    def __init__(self, init):
        if isinstance(init, torch.Tensor):
            self.init = init.detach().to(torch.float32).contiguous()
        else:
            self.init = torch.full(tuple(init), float('nan'), dtype=torch.float32)
        n = self.init.numel()
        self.full = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
        self.view = self.full[GUARD:GUARD + n].view(torch.float32).view(self.init.shape)
        self.reset()

    def reset(self):
        self.view.copy_(self.init)

    def keep(self):
        """the present contents become the contents before every later call (the packed operands, once packed)"""
        self.init = self.view.detach().cpu().clone()

    def guards_ok(self):
        n = self.init.numel()
        return bool((self.full[:GUARD] == PATTERN).all()) and bool((self.full[GUARD + n:] == PATTERN).all())

    def bits(self):
        return self.view.detach().cpu().contiguous().view(torch.int32).clone()


def call(op, sc, tp, slots):
    """-> (return code, error text).  sc: scalar fields; tp: host topology arrays; slots: name -> Buf, or (tensor view, element count)."""
    c = capi()
    a = c.FusedTestArgs()
    a.op = c.FT_OPS.index(op)
    for k, v in sc.items():
        setattr(a, k, v)
    host, total = [], 0
    for k in c.FT_TOPO:
        if tp.get(k) is not None:
            arr = np.ascontiguousarray(np.asarray(tp[k]), dtype=np.int32)
            host.append(arr)
            total += arr.size
            setattr(a, k, arr.ctypes.data)
    topo_dev = torch.empty(total + 8, dtype=torch.int32, device=DEV)
    a.topo_dev, a.topo_dev_count = topo_dev.data_ptr(), total + 8
    for name, b in slots.items():
        i = c.FT_SLOTS.index(name)
        if b is None:
            continue
        view, n = (b.view, b.view.numel()) if isinstance(b, Buf) else b
        a.a[i], a.n[i] = view.data_ptr(), n
    rc = c.train_debug_fused(a, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    msg = c.lib().jodo_last_error()
    return rc, (msg.decode() if msg else '')


def note(label, ratio):
    """worst err / bound per op label (the figures of DESIGN.md's table are the maxima of the lines check_fwd / check_bwd print)"""
    RATIOS[label] = max(RATIOS.get(label, 0.0), ratio)


def check_fwd(label, what, got, r32, r64):
    g, a, b = got.detach().cpu().double(), r32.double(), r64.double()
    assert g.shape == b.shape, (label, what, g.shape, b.shape)
    assert not bool(torch.isnan(g).any()), "%s: %s has elements the kernel never wrote" % (label, what)
    err = (g - b).abs()
    e32 = float((a - b).abs().max())
    ratio = float((err / torch.clamp(2e-5 + 1e-4 * b.abs(), min=4.0 * e32)).max())
    print("  %-22s %-8s fwd  err %.2e  float32 restatement %.2e  err / bound %.3f" % (label, what, float(err.max()), e32, ratio))
    note(label, ratio)
    close64(got, r32, r64, what='%s %s' % (label, what))


def check_bwd(label, what, got, r32, r64):
    g, a, b = got.detach().cpu().double(), r32.double(), r64.double()
    assert g.shape == b.shape, (label, what, g.shape, b.shape)
    assert not bool(torch.isnan(g).any()), "%s: %s has elements the kernel never wrote" % (label, what)
    err, e32 = float((g - b).abs().max()), float((a - b).abs().max())
    bound = max(GRAD_REL * max(float(b.abs().max()), 1e-12), K32 * e32)
    print("  %-22s %-8s bwd  err %.2e  float32 restatement %.2e  err / bound %.3f" % (label, what, err, e32, err / bound))
    note(label, err / bound)
    assert err <= bound, "%s %s: max |HIP - f64| %.3e, bound %.3e (scale %.3e, float32 restatement %.3e)" % (label, what, err, bound, float(b.abs().max()), e32)


def run_op(label, op, sc, tp, ins, outs, refs=None, rule=None, poison=()):
    """One op through the entry, twice.  ins: slot -> Buf (read only: must come back unchanged; None: a NULL pointer); outs: slot -> Buf;
    refs: slot -> (r32, r64) compared under `rule` (check_fwd / check_bwd); poison: output slots that must keep their NaN.
    -> slot -> the stored array (CPU)."""
    slots = dict(ins)
    slots.update(outs)
    bufs = [b for b in slots.values() if isinstance(b, Buf)]
    for b in outs.values():
        b.reset()
    rc, msg = call(op, sc, tp, slots)
    assert rc == 0, "%s: %s" % (label, msg)
    got = {k: b.view.detach().cpu().clone() for k, b in outs.items()}
    first = {k: b.bits() for k, b in outs.items()}
    assert all(b.guards_ok() for b in bufs), "%s: a guard band was written" % label
    for k, b in ins.items():
        if isinstance(b, Buf):
            assert torch.equal(b.bits(), b.init.view(torch.int32)), "%s: the input %s was modified" % (label, k)
    for k in poison:
        assert bool(torch.isnan(got[k]).all()), "%s: %s is written although the header says it is skipped" % (label, k)
    for k, (r32, r64) in (refs or {}).items():
        rule(label, k, got[k], r32, r64)
    for b in outs.values():
        b.reset()
    rc, msg = call(op, sc, tp, slots)
    assert rc == 0, "%s (second run): %s" % (label, msg)
    for k, b in outs.items():
        assert torch.equal(b.bits(), first[k]), "%s: %s differs between two runs" % (label, k)
    assert all(b.guards_ok() for b in bufs), "%s: a guard band was written (second run)" % label
    return got


def both(fn, *args, **kw):
    """the restatement at float32 and at float64 -> slot -> (r32, r64)"""
    r32, r64 = fn(*args, dtype=torch.float32, **kw), fn(*args, dtype=torch.float64, **kw)
    return {k: (r32[k], r64[k]) for k in r64}


def f32(t):
    return t.float().double()


# ---- the operand images (k_pack): exact copies, compared bit for bit ----------------------------------------------------------------
def pack_layout(d):
    De, D, r = d['De'], d['D'], d['r']
    qkp = (d['QK'] + 31) // 32 * 32
    L, o = {}, 0
    for k, n in (('ee', De * 2 * De), ('l0', qkp * De), ('l1', D * De), ('ff3', r * De * De), ('ff4', De * r * De), ('ero', 32 * De),
                 ('in_eg', D * 2 * De), ('c0', D * D), ('tab', 3 * De)):
        L[k] = o
        o += n
    L['total'] = o = (o + 63) // 64 * 64
    for k, n in (('c0t', D * D), ('int_eg', 2 * De * D), ('ff4t', r * De * De), ('ff3t', De * r * De), ('l1t', De * D), ('l0t', De * D), ('eet', 2 * De * De)):
        L[k] = o
        o += n
    L['total_bwd'] = (o + 63) // 64 * 64
    return L


def image(M, K_):
    """[out, in] -> [out block][quad][lane][4] in the natural maps (register R of half h = feature (R / 16) 32 + 16 h + R % 16 on both
    sides); rows and columns the matrix does not have are zero."""
    M = M.float().numpy()
    nb, kq = (M.shape[0] + 31) // 32, K_ // 8
    pad = np.zeros((nb * 32, K_), np.float32)
    pad[:M.shape[0], :M.shape[1]] = M
    lane = np.arange(64)
    i, kh = lane & 31, lane >> 5
    row = np.arange(nb)[:, None, None, None] * 32 + (((i >> 2) & 1) * 16 + (i & 3) + 4 * (i >> 3))[None, None, :, None]
    R = np.arange(kq)[None, :, None, None] * 4 + np.arange(4)[None, None, None, :]
    col = (R // 16) * 32 + kh[None, None, :, None] * 16 + R % 16
    return torch.from_numpy(pad[np.broadcast_to(row, (nb, kq, 64, 4)), np.broadcast_to(col, (nb, kq, 64, 4))].reshape(-1).copy())


def expected_images(d, P, L, which):
    D, De, r = d['D'], d['De'], d['r']
    W = P.get('in_w')
    items = dict(ee=lambda: image(P['edge_emb_w'], 2 * De), l0=lambda: image(P['le0'], De), l1=lambda: image(P['le1'], De),
                 ff3=lambda: image(P['ff3_w'], De), ff4=lambda: image(P['ff4_w'], r * De), ero=lambda: image(P['ero_w'], De),
                 in_eg=lambda: image(W[:, 2 * D:], 2 * De), c0=lambda: image(P['c0_w'], D), c0t=lambda: image(P['c0_w'].t(), D),
                 int_eg=lambda: image(W[:, 2 * D:].t(), D), ff4t=lambda: image(P['ff4_w'].t(), De), ff3t=lambda: image(P['ff3_w'].t(), r * De),
                 l1t=lambda: image(P['le1'].t(), D), l0t=lambda: image(P['le0'].t(), D), eet=lambda: image(P['edge_emb_w'].t(), De))
    return {k: (L[k], items[k]()) for k in which}


def pack_and_check(d, P, pbufs, two_d):
    """Runs the two pack ops into a NaN-poisoned buffer and compares the whole buffer bit for bit: the images where they belong, the
    Gaussian table to float32 rounding, NaN everywhere else (nothing outside the images is written)."""
    L = pack_layout(d)
    packed = Buf((L['total_bwd'],))
    sc = dict(D=d['D'], De=d['De'], r=d['r'], QK=d['QK'], ce=d['ce'], nco=d['nco'])
    fwd_items = ('l0', 'l1', 'ff3', 'ff4', 'ero') if two_d else ('ee', 'l0', 'l1', 'ff3', 'ff4', 'ero', 'in_eg', 'c0')
    bwd_items = ('ff4t', 'ff3t', 'l1t', 'l0t') if two_d else ('c0t', 'int_eg', 'ff4t', 'ff3t', 'l1t', 'l0t', 'eet')
    exp = torch.full((L['total_bwd'],), float('nan'), dtype=torch.float32)
    for step, op, items in ((0, 'PACK_2D' if two_d else 'PACK', fwd_items), (1, 'PACK_2D_BWD' if two_d else 'PACK_BWD', bwd_items)):
        ins = {k.upper(): pbufs[k] for k in pbufs}
        got = run_op(op, op, sc, {}, ins, {'PACKED': packed})['PACKED']
        for k, (off, img) in expected_images(d, P, L, items).items():
            exp[off:off + img.numel()] = img
        g, e = got.clone(), exp.clone()
        if not two_d:                                    # the Gaussian table [3][De]: mu | 1 / sigma | 1 / (2.5066272 sigma), k = 0: 0 | 1 | 0
            De = d['De']
            sd = P['gbf_stds'].float().abs() + 1e-5
            tab = torch.cat([torch.zeros(1), P['gbf_means'].float(), torch.ones(1), 1 / sd, torch.zeros(1), 1 / (2.5066272 * sd)])
            t0 = L['tab']
            assert torch.allclose(g[t0:t0 + 3 * De], tab, rtol=3e-7, atol=0), op
            g[t0:t0 + 3 * De] = 0
            e[t0:t0 + 3 * De] = 0
        assert torch.equal(g.view(torch.int32), e.view(torch.int32)), "%s: the packed images differ from the natural map" % op
        note(op, 0.0)
        packed.keep()
        exp = got.clone()
    return packed, sc


def param_bufs(P):
    return {k: Buf(v) for k, v in P.items()}


def topo_host(tp):
    return {k: tp[k].numpy() if isinstance(tp[k], torch.Tensor) else tp[k] for k in tp if k in capi().FT_TOPO}


# ---- the per-edge chains ----------------------------------------------------------------------------------------------------------
CHAIN_CASES = [(i, 95) for i in range(len(K.DIMS_3D))] + [(i, R) for i in (0, 5) for R in (1, 31, 32, 33)]


@pytest.mark.parametrize('di,R', CHAIN_CASES)
def test_chains_3d(di, R):
    d = K.DIMS_3D[di]
    D, De, r, QK, ce, nco = d['D'], d['De'], d['r'], d['QK'], d['ce'], d['nco']
    HID = r * De
    tp = K.rand_topo(R, 100 + di)
    th = topo_host(tp)
    B, Nn = tp['B'], tp['Nn']
    P = K.rand_params(d, 200 + di)
    pb = param_bufs(P)
    packed, sc = pack_and_check(d, P, pb, False)
    sc.update(R=R, Nn=Nn, B=B, save=1)
    g = torch.Generator().manual_seed(300 + di * 7 + R)
    pslots = {k.upper(): v for k, v in pb.items()}
    pslots['PACKED'] = packed
    tag = 'D%d nco%d' % (D, nco)

    # chain A
    pos, gm = K.randn64(g, Nn, 3, scale=0.5), K.randn64(g, B, 2, scale=0.3)
    e_in, emod = K.randn64(g, R, De), K.randn64(g, B, 6 * De, scale=0.5)
    ra = both(K.chain_a, P, tp, pos, gm, e_in, emod)
    ins = dict(pslots, POS=Buf(pos), GM=Buf(gm), E_IN=Buf(e_in), EMOD=Buf(emod))
    shapes = dict(D2=(R,), G=(R, De), XH=(R, De), RS=(R,), ET=(R, De), T0=(R, QK), T1=(R, D))
    names = dict(D2='d2', G='G', XH='xh', RS='rs', ET='et', T0='t0', T1='t1')
    outs = {k: Buf(s) for k, s in shapes.items()}
    a1 = run_op('fused_chain_a', 'CHAIN_A', sc, th, ins, outs, {k: ra[n] for k, n in names.items()}, check_fwd)
    a0 = run_op('fused_chain_a save=0', 'CHAIN_A', dict(sc, save=0), th, ins, outs, poison=('D2', 'XH', 'RS', 'ET'))
    for k in ('G', 'T0', 'T1'):
        assert torch.equal(a0[k].view(torch.int32), a1[k].view(torch.int32)), "chain A: %s differs between save = 0 and save = 1" % k

    # chain B: the readout goes into columns eh_col .. eh_col + ce - 1 of a wider head input
    n2e = K.randn64(g, Nn, De)
    ld_eh, eh_col = ce + 24, 12
    eh0 = K.randn64(g, R, ld_eh)
    bref = {}
    for p in (0.0, 0.1):
        m3 = K.drop_masks(SEED, 11, p, R, HID, torch.float64)
        m4 = K.drop_masks(SEED, 12, p, R, De, torch.float64)
        rb = both(K.chain_b, P, tp, e_in, n2e, emod, m3, m4)
        eh_ref = tuple(torch.cat([eh0[:, :eh_col].to(t.dtype), t, eh0[:, eh_col + ce:].to(t.dtype)], dim=1) for t in rb['ro'])
        scb = dict(sc, drop_p=p, seed=SEED, site_a3=11, site_f4=12, ld_eh=ld_eh, eh_col=eh_col)
        ins = dict(pslots, E_IN=Buf(e_in), N2E=Buf(n2e), EMOD=Buf(emod))
        shapes = dict(XH=(R, De), RS=(R,), EN=(R, De), F3=(R, HID), A3=(R, HID), F4=(R, De), E_OUT=(R, De))
        names = dict(XH='xh', RS='rs', EN='en', F3='f3', A3='a3', F4='f4', E_OUT='e_out')
        outs = {k: Buf(s) for k, s in shapes.items()}
        outs['EH'] = Buf(eh0)
        refs = {k: rb[n] for k, n in names.items()}
        refs['EH'] = eh_ref
        lab = 'fused_chain_b p=%g' % p
        b1 = run_op(lab, 'CHAIN_B', scb, th, ins, outs, refs, check_fwd)
        side = torch.ones(ld_eh, dtype=torch.bool)
        side[eh_col:eh_col + ce] = False
        assert torch.equal(b1['EH'][:, side].view(torch.int32), eh0.float()[:, side].view(torch.int32)), "chain B wrote beside its readout columns"
        if p > 0:
            assert bool((b1['A3'][m3 == 0] == 0).all()) and 0 < int((m3 == 0).sum()), "chain B: a3 is not zero where the restated mask is"
        b0 = run_op(lab + ' save=0', 'CHAIN_B', dict(scb, save=0), th, ins, outs, poison=('XH', 'RS', 'EN', 'F3', 'A3', 'F4'))
        for k in ('E_OUT', 'EH'):
            assert torch.equal(b0[k].view(torch.int32), b1[k].view(torch.int32)), "chain B: %s differs between save = 0 and save = 1" % k
        bref[p] = (rb, m3, m4)

    # chain C
    e2, G = K.randn64(g, R, De), f32(ra['G'][1])
    hr, hc, qmod = K.randn64(g, Nn, D), K.randn64(g, Nn, D), K.randn64(g, B, 2 * D, scale=0.5)
    rc_ = both(K.chain_c, P, tp, e2, G, hr, hc, qmod)
    ins = dict(pslots, E_IN=Buf(e2), G=Buf(G), HR=Buf(hr), HC=Buf(hc), QMOD=Buf(qmod))
    shapes = dict(XH=(R, D), RS=(R,), U=(R, D), C0PRE=(R, D), C0A=(R, D), INV=(R, nco))
    names = dict(XH='xh', RS='rs', U='u', C0PRE='c0pre', C0A='c0a', INV='inv')
    outs = {k: Buf(s) for k, s in shapes.items()}
    c1 = run_op('fused_chain_c ' + tag, 'CHAIN_C', sc, th, ins, outs, {k: rc_[n] for k, n in names.items()}, check_fwd)
    c0 = run_op('fused_chain_c save=0', 'CHAIN_C', dict(sc, save=0), th, ins, outs, poison=('XH', 'RS', 'U', 'C0PRE', 'C0A'))
    assert torch.equal(c0['INV'].view(torch.int32), c1['INV'].view(torch.int32)), "chain C: inv differs between save = 0 and save = 1"

    # chain C': saved activations = the float64 restatement's, rounded to float32
    sv = {k: f32(v[1]) for k, v in rc_.items()}
    dinv, de0 = K.randn64(g, R, nco), K.randn64(g, R, De)
    rbc = both(K.bwd_c, P, tp, sv['inv'], dinv, sv['c0pre'], sv['xh'], sv['rs'], qmod, de0)
    ins = dict(pslots, INV=Buf(sv['inv']), C0PRE=Buf(sv['c0pre']), XH=Buf(sv['xh']), RS=Buf(sv['rs']), QMOD=Buf(qmod))
    outs = dict(DINV=Buf(dinv), DC0=Buf((R, D)), DU=Buf((R, D)), DPRE=Buf((R, D)), DE=Buf(de0), DG=Buf((R, De)))
    names = dict(DINV='dinv', DC0='dc0', DU='du', DPRE='dpre', DE='de', DG='dG')
    run_op('fused_bwd_c ' + tag, 'BWD_C', sc, {'edge_mol': th['edge_mol']}, ins, outs, {k: rbc[n] for k, n in names.items()}, check_bwd)

    # chain B'
    de_out = K.randn64(g, R, De)
    for p in (0.0, 0.1):
        rb, m3, m4 = bref[p]
        sv = {k: f32(v[1]) for k, v in rb.items()}
        rbb = both(K.bwd_b, P, tp, de_out, sv['f4'], sv['f3'], sv['xh'], sv['rs'], emod, m3, m4)
        scb = dict(sc, drop_p=p, seed=SEED, site_a3=11, site_f4=12)
        ins = dict(pslots, DE_OUT=Buf(de_out), F4=Buf(sv['f4']), F3=Buf(sv['f3']), XH=Buf(sv['xh']), RS=Buf(sv['rs']), EMOD=Buf(emod))
        outs = dict(F4D=Buf((R, De)), DF4=Buf((R, De)), DHID=Buf((R, HID)), DEN=Buf((R, De)), DE_PREV=Buf((R, De)))
        names = dict(F4D='f4d', DF4='df4', DHID='dhid', DEN='den', DE_PREV='de_prev')
        bb = run_op('fused_bwd_b p=%g' % p, 'BWD_B', scb, {'edge_mol': th['edge_mol']}, ins, outs, {k: rbb[n] for k, n in names.items()}, check_bwd)
        if p > 0:                                       # the backward regenerates the forward's masks
            assert bool((bb['F4D'][m4 == 0] == 0).all()) and bool((bb['DHID'][m3 == 0] == 0).all())
            assert bool((bb['F4D'][m4 != 0] != 0).all()), "chain B': f4d is zero where the restated mask keeps the element"

    # chain A'
    sv = {k: f32(v[1]) for k, v in ra.items()}
    dt1, dt0 = K.randn64(g, R, D), K.randn64(g, R, QK)
    dG0, dep0 = K.randn64(g, R, De), K.randn64(g, R, De)
    rba = both(K.bwd_a, P, tp, dt1, dt0, sv['xh'], sv['rs'], emod, dG0, dep0)
    ins = dict(pslots, DT1=Buf(dt1), DT0=Buf(dt0), XH=Buf(sv['xh']), RS=Buf(sv['rs']), EMOD=Buf(emod))
    outs = dict(DET=Buf((R, De)), DE1=Buf((R, De)), DG=Buf(dG0), DE_PREV=Buf(dep0))
    names = dict(DET='det', DE1='de1', DG='dG', DE_PREV='de_prev')
    run_op('fused_bwd_a', 'BWD_A', sc, {'edge_mol': th['edge_mol']}, ins, outs, {k: rba[n] for k, n in names.items()}, check_bwd)


def dims_2d(cfg_name):
    cfg = make_config(cfg_name)
    hp = O2.Hyper2D.from_config(cfg)
    return dict(D=hp.D, De=hp.De, r=hp.r, QK=hp.SH * hp.SC, nco=3, ce=(2 * hp.De) // cfg.model.n_layers)


@pytest.mark.parametrize('cfg_name', ['vpsde_zinc_2d_jodo', 'vpsde_moses_2d_jodo'])
@pytest.mark.parametrize('R', K.ROWS)
def test_chains_2d(cfg_name, R):
    d = dims_2d(cfg_name)
    D, De, r, QK, ce = d['D'], d['De'], d['r'], d['QK'], d['ce']
    assert QK == 255
    HID = r * De
    tp = K.rand_topo(R, 400 + R)
    th = topo_host(tp)
    B, Nn = tp['B'], tp['Nn']
    P = {k: v for k, v in K.rand_params(d, 500).items() if k in ('le0', 'le1', 'ff3_w', 'ff3_b', 'ff4_w', 'ff4_b', 'ero_w', 'ero_b', 'n2e_b')}
    pb = param_bufs(P)
    packed, sc = pack_and_check(d, P, {k: pb[k] for k in ('le0', 'le1', 'ff3_w', 'ff4_w', 'ero_w')}, True)
    sc.update(R=R, Nn=Nn, B=B, save=1)
    g = torch.Generator().manual_seed(600 + R)
    pslots = {k.upper(): v for k, v in pb.items()}
    pslots['PACKED'] = packed
    em_only = {'edge_mol': th['edge_mol']}

    e_in, emod = K.randn64(g, R, De), K.randn64(g, B, 6 * De, scale=0.5)
    ra = both(K.chain_a_2d, P, tp, e_in, emod)
    ins = dict(pslots, E_IN=Buf(e_in), EMOD=Buf(emod))
    shapes = dict(XH=(R, De), RS=(R,), ET=(R, De), T0=(R, QK), T1=(R, D))
    names = dict(XH='xh', RS='rs', ET='et', T0='t0', T1='t1')
    outs = {k: Buf(s) for k, s in shapes.items()}
    a1 = run_op('fused2d_chain_a', 'CHAIN_A_2D', sc, em_only, ins, outs, {k: ra[n] for k, n in names.items()}, check_fwd)
    a0 = run_op('fused2d_chain_a save=0', 'CHAIN_A_2D', dict(sc, save=0), em_only, ins, outs, poison=('XH', 'RS', 'ET'))
    for k in ('T0', 'T1'):
        assert torch.equal(a0[k].view(torch.int32), a1[k].view(torch.int32))

    sv = {k: f32(v[1]) for k, v in ra.items()}
    dt1, dt0, dep0 = K.randn64(g, R, D), K.randn64(g, R, QK), K.randn64(g, R, De)
    rba = both(K.bwd_a_2d, P, tp, dt1, dt0, sv['xh'], sv['rs'], emod, dep0)
    ins = dict(pslots, DT1=Buf(dt1), DT0=Buf(dt0), XH=Buf(sv['xh']), RS=Buf(sv['rs']), EMOD=Buf(emod))
    outs = dict(DET=Buf((R, De)), DE_PREV=Buf(dep0))
    run_op('fused2d_bwd_a', 'BWD_A_2D', sc, em_only, ins, outs, dict(DET=rba['det'], DE_PREV=rba['de_prev']), check_bwd)

    # chain B / B' on the 2-D operand images (QK = 255 is outside fused_available: chain B has a predicate of its own)
    n2e, p = K.randn64(g, Nn, De), 0.1
    m3, m4 = K.drop_masks(SEED, 3, p, R, HID, torch.float64), K.drop_masks(SEED, 4, p, R, De, torch.float64)
    rb = both(K.chain_b, P, tp, e_in, n2e, emod, m3, m4)
    ld_eh, eh_col = ce + 8, 4
    eh0 = K.randn64(g, R, ld_eh)
    scb = dict(sc, drop_p=p, seed=SEED, site_a3=3, site_f4=4, ld_eh=ld_eh, eh_col=eh_col)
    ins = dict(pslots, E_IN=Buf(e_in), N2E=Buf(n2e), EMOD=Buf(emod))
    names = dict(XH='xh', RS='rs', EN='en', F3='f3', A3='a3', F4='f4', E_OUT='e_out')
    outs = {k: Buf(rb[n][1].shape) for k, n in names.items()}
    outs['EH'] = Buf(eh0)
    refs = {k: rb[n] for k, n in names.items()}
    refs['EH'] = tuple(torch.cat([eh0[:, :eh_col].to(t.dtype), t, eh0[:, eh_col + ce:].to(t.dtype)], dim=1) for t in rb['ro'])
    run_op('fused_chain_b 2-D', 'CHAIN_B', scb, th, ins, outs, refs, check_fwd)
    sv = {k: f32(v[1]) for k, v in rb.items()}
    de_out = K.randn64(g, R, De)
    rbb = both(K.bwd_b, P, tp, de_out, sv['f4'], sv['f3'], sv['xh'], sv['rs'], emod, m3, m4)
    ins = dict(pslots, DE_OUT=Buf(de_out), F4=Buf(sv['f4']), F3=Buf(sv['f3']), XH=Buf(sv['xh']), RS=Buf(sv['rs']), EMOD=Buf(emod))
    outs = dict(F4D=Buf((R, De)), DF4=Buf((R, De)), DHID=Buf((R, HID)), DEN=Buf((R, De)), DE_PREV=Buf((R, De)))
    names = dict(F4D='f4d', DF4='df4', DHID='dhid', DEN='den', DE_PREV='de_prev')
    run_op('fused_bwd_b 2-D', 'BWD_B', scb, em_only, ins, outs, {k: rbb[n] for k, n in names.items()}, check_bwd)


# ---- node rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Fw', [128, 256, 384])
def test_node_pair(Fw):
    g = torch.Generator().manual_seed(700 + Fw)
    for rows in (1, 63, 64, 65):
        B = min(5, rows)
        row_mol = torch.sort(torch.randint(0, B, (rows,), generator=g)).values
        a, res, mods = K.randn64(g, rows, Fw), K.randn64(g, rows, Fw), K.randn64(g, B, 6 * Fw, scale=0.5)
        tp = {'row_mol': row_mol.numpy()}
        for with_res in (False, True):
            g_off, sh_off, sc_off = (2 * Fw, 3 * Fw, 4 * Fw) if with_res else (0, 0, Fw)
            sc = dict(D=Fw, Nn=rows, B=B, ldm=6 * Fw, g_off=g_off, sh_off=sh_off, sc_off=sc_off)
            rf = both(K.node_ln_mod, a, res if with_res else None, row_mol, mods, g_off, sh_off, sc_off)
            ins = dict(E_IN=Buf(a), N2E=Buf(res) if with_res else None, MODS=Buf(mods))
            outs = dict(XH=Buf((rows, Fw)), RS=Buf((rows,)), E_OUT=Buf((rows, Fw)))
            run_op('fused_node_ln_mod', 'NODE_LN_MOD', sc, tp, ins, outs, dict(XH=rf['xh'], RS=rf['rs'], E_OUT=rf['y']), check_fwd)
            xh, rs, dy, dx0 = f32(rf['xh'][1]), f32(rf['rs'][1]), K.randn64(g, rows, Fw), K.randn64(g, rows, Fw)
            for acc in (0, 1):
                rbw = both(K.node_ln_mod_bwd, dy, xh, rs, row_mol, mods, sc_off, dx0 if acc else None)
                ins = dict(DE_OUT=Buf(dy), XH=Buf(xh), RS=Buf(rs), MODS=Buf(mods))
                outs = dict(DE_PREV=Buf(dx0) if acc else Buf((rows, Fw)))
                run_op('fused_node_ln_mod_bwd', 'NODE_LN_MOD_BWD', dict(sc, acc=acc), tp, ins, outs, dict(DE_PREV=rbw['dx']), check_bwd)


# ---- attention ------------------------------------------------------------------------------------------------------------------------
ATT_NN = [1, 2, 16, 17, 65]                       # no pair at all (an empty softmax), one pair, one past a 16-source group, a second wave's share


@pytest.mark.parametrize('D,XH', [(128, 2), (256, 2), (384, 2), (256, 0), (128, 0)])
def test_attention(D, XH):
    H = 16
    C = D // H
    SC = (H * C) // (H - XH)
    QK = (H - XH) * SC
    tp = K.mol_topo(ATT_NN)
    R, Nn = tp['R'], tp['Nn']
    th = {k: tp[k].numpy() if isinstance(tp[k], torch.Tensor) else np.asarray(tp[k]) for k in ('node_mol', 'nn', 'node_off', 'edge_off')}
    g = torch.Generator().manual_seed(800 + D + XH)
    F3 = 2 * QK + D
    qkv = K.randn64(g, Nn, F3)                       # q | k | v side by side, as the merged projection leaves them
    t0, t1 = torch.tanh(K.randn64(g, R, QK)).float().double(), torch.tanh(K.randn64(g, R, D)).float().double()
    adj2d, adjsp = (torch.rand(R, generator=g) < 0.7).double(), (torch.rand(R, generator=g) < 0.7).double()
    q, k, v = qkv[:, :QK], qkv[:, QK:2 * QK], qkv[:, 2 * QK:]
    rf = both(K.attn_fwd, ATT_NN, H, XH, SC, q, k, v, t0, t1, adj2d, adjsp)
    alpha = f32(rf['alpha'][1])
    dhhat = K.randn64(g, Nn, D)
    rb = both(K.attn_bwd, ATT_NN, H, XH, SC, dhhat, q, k, v, t0, t1, alpha)
    sc = dict(D=D, H=H, XH=XH, SC=SC, N=max(ATT_NN), R=R, Nn=Nn, B=len(ATT_NN), ldqk=F3, ldv=F3, ldd_qk=F3, ldd_v=F3, inv_sqrt_c=1.0 / math.sqrt(C))
    bq = Buf(qkv)
    n_all = bq.view.numel()
    flat = bq.view.view(-1)
    qs = dict(Q=(flat, n_all), K=(flat[QK:], n_all - QK), V=(flat[2 * QK:], n_all - 2 * QK))
    fwd_bits = {}
    for one_wave in (0, 1):
        form = 'one wave' if one_wave else 'several waves'
        ins = dict(qs, T0=Buf(t0), T1=Buf(t1), ADJ2D=Buf(adj2d) if XH >= 1 else None, ADJSP=Buf(adjsp) if XH >= 2 else None)
        outs = dict(ALPHA=Buf((R, H)), HHAT=Buf((Nn, D)))
        got = run_op('fused_attn_fwd (%s)' % form, 'ATTN_FWD', dict(sc, one_wave=one_wave), th, ins, outs, dict(ALPHA=rf['alpha'], HHAT=rf['hhat']), check_fwd)
        assert bq.guards_ok() and torch.equal(bq.bits(), bq.init.view(torch.int32))
        fwd_bits[one_wave] = got
        dqkv = Buf((Nn, F3))
        dflat = dqkv.view.view(-1)
        ins = dict(qs, T0=Buf(t0), T1=Buf(t1), DHHAT=Buf(dhhat), ALPHA=Buf(alpha))
        outs = dict(DS=Buf((R, H)), DT1=Buf((R, D)), DT0=Buf((R, QK)))
        slots_d = dict(DQ=(dflat, n_all), DK=(dflat[QK:], n_all - QK), DV=(dflat[2 * QK:], n_all - 2 * QK))
        ins.update(slots_d)
        run_op('fused_attn_bwd (%s)' % form, 'ATTN_BWD', dict(sc, one_wave=one_wave), th, ins, outs,
               dict(DS=rb['dS'], DT1=rb['dt1'], DT0=rb['dt0']), check_bwd)
        assert dqkv.guards_ok()
        dg = dqkv.view.detach().cpu()
        lab = 'fused_attn_bwd (%s)' % form
        check_bwd(lab, 'dq', dg[:, :QK], *rb['dq'])
        check_bwd(lab, 'dk', dg[:, QK:2 * QK], *rb['dk'])
        check_bwd(lab, 'dv', dg[:, 2 * QK:], *rb['dv'])
        first = dqkv.bits()
        dqkv.reset()
        rc, msg = call('ATTN_BWD', dict(sc, one_wave=one_wave), th, dict(ins, **outs))
        assert rc == 0, msg
        assert torch.equal(dqkv.bits(), first), "attention backward: dq | dk | dv differ between two runs"
    for k in ('ALPHA', 'HHAT'):                       # the header's promise: the forms share every sum's order
        assert torch.equal(fwd_bits[0][k].view(torch.int32), fwd_bits[1][k].view(torch.int32)), "attention forward: %s differs between the forms" % k


# ---- Gaussian layer backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('De', [32, 64, 96])
def test_gbf_bwd(De):
    g = torch.Generator().manual_seed(900 + De)
    P = K.rand_params(K.dims(4 * De, 2, 4 * De - 2, 3, 8), 901)
    means, stds = P['gbf_means'], P['gbf_stds']
    assert bool((stds < 0).any())
    for rows in (31, 32, 33, 95):
        B = 6
        row_mol = torch.sort(torch.randint(0, B, (rows,), generator=g)).values
        d2, gm = K.randn64(g, rows).abs(), K.randn64(g, B, 2, scale=0.3)
        nch = (rows + 31) // 32
        for acc, ldg, gcol in ((0, De, 0), (1, De + 12, 4)):
            dGw = K.randn64(g, rows, ldg)
            dd0 = K.randn64(g, rows)
            rf = both(K.gbf_bwd, d2, row_mol, gm, means, stds, dGw[:, gcol:gcol + De], dd0 if acc else None)
            sc = dict(De=De, R=rows, B=B, ldg=ldg, gcol=gcol, acc=acc)
            ins = dict(D2=Buf(d2), GM=Buf(gm), GBF_MEANS=Buf(means), GBF_STDS=Buf(stds), DG=Buf(dGw))
            outs = dict(DXP=Buf((rows,)), DD2=Buf(dd0) if acc else Buf((rows,)), PART_M=Buf((nch, De - 1)), PART_S=Buf((nch, De - 1)))
            run_op('fused_gbf_bwd', 'GBF_BWD', sc, {'edge_mol': row_mol.numpy()}, ins, outs,
                   dict(DXP=rf['dxp'], DD2=rf['dd2'], PART_M=rf['part_m'], PART_S=rf['part_s']), check_bwd)


# ---- the entry refuses what the kernels were not built for ----------------------------------------------------------------------------------
def test_entry_refusals():
    """No kernel runs here: every call must come back with an error code and a text that names the problem."""
    d = K.DIMS_3D[0]
    D, De, QK, R = d['D'], d['De'], d['QK'], 33
    tp = K.rand_topo(R, 1)
    th = topo_host(tp)
    sc = dict(D=D, De=De, r=d['r'], QK=QK, ce=d['ce'], nco=d['nco'], R=R, Nn=tp['Nn'], B=tp['B'], save=1)
    L = pack_layout(d)
    slots = dict(PACKED=Buf((L['total_bwd'],)), EDGE_EMB_B=Buf((De,)), POS=Buf((tp['Nn'], 3)), GM=Buf((tp['B'], 2)), E_IN=Buf((R, De)),
                 EMOD=Buf((tp['B'], 6 * De)), D2=Buf((R,)), G=Buf((R, De)), XH=Buf((R, De)), RS=Buf((R,)), ET=Buf((R, De)), T0=Buf((R, QK)), T1=Buf((R, D)))
    before = {k: b.bits() for k, b in slots.items()}
    c = capi()
    ARG, UNSUPPORTED = -1, -3

    rc, msg = call('CHAIN_A', dict(sc, D=192, De=48), th, slots)
    assert rc == UNSUPPORTED and 'fused_available is false' in msg and 'D 192' in msg, msg
    rc, msg = call('CHAIN_A', dict(sc, QK=127), th, slots)
    assert rc == UNSUPPORTED and 'QK 127' in msg, msg
    rc, msg = call('CHAIN_A', dict(sc, nco=2), th, slots)
    assert rc == UNSUPPORTED and 'nco 2' in msg, msg
    rc, msg = call('CHAIN_B', dict(sc, ce=33), th, slots)
    assert rc == UNSUPPORTED and 'fused_chain_b_available is false' in msg, msg
    rc, msg = call('CHAIN_A_2D', dict(sc, QK=D + 1), th, slots)
    assert rc == UNSUPPORTED and 'fused2d_available is false' in msg, msg
    rc, msg = call('ATTN_FWD', dict(sc, H=16, XH=2, SC=9, N=193), th, slots)
    assert rc == UNSUPPORTED and 'fused_attention_available is false' in msg and 'N 193' in msg, msg
    rc, msg = call('NODE_LN_MOD', dict(sc, D=192), th, slots)
    assert rc == UNSUPPORTED and 'F in {128, 256, 384}' in msg, msg
    rc, msg = call('GBF_BWD', dict(sc, De=130), th, slots)
    assert rc == UNSUPPORTED and 'De 130' in msg, msg

    bad = dict(th)
    bad['edge_mol'] = th['edge_mol'].copy()
    bad['edge_mol'][3] = tp['B']
    rc, msg = call('CHAIN_A', sc, bad, slots)
    assert rc == ARG and 'edge_mol[3] = %d is out of range' % tp['B'] in msg, msg
    bad = dict(th)
    bad['edge_c'] = th['edge_c'].copy()
    bad['edge_c'][R - 1] = -1
    rc, msg = call('CHAIN_A', sc, bad, slots)
    assert rc == ARG and 'edge_c[%d] = -1 is out of range' % (R - 1) in msg, msg

    short = dict(slots)
    short['T1'] = (slots['T1'].view, R * D - 1)
    rc, msg = call('CHAIN_A', sc, th, short)
    assert rc == ARG and 'array t1 has %d floats, the op touches %d' % (R * D - 1, R * D) in msg, msg
    short = dict(slots)
    short['PACKED'] = (slots['PACKED'].view, L['total_bwd'] - 1)
    rc, msg = call('CHAIN_A', sc, th, short)
    assert rc == ARG and 'array packed has' in msg, msg
    null = dict(slots)
    null['EMOD'] = None
    rc, msg = call('CHAIN_A', sc, th, null)
    assert rc == ARG and 'array emod is a null pointer' in msg, msg
    odd = dict(slots)
    odd['E_IN'] = (slots['E_IN'].view.view(-1)[1:], R * De)
    rc, msg = call('CHAIN_A', sc, th, odd)
    assert rc == ARG and 'array e_in is not 16-byte aligned' in msg, msg
    rc, msg = call('CHAIN_A', sc, dict(th, edge_a=None), slots)
    assert rc == ARG and 'topology array edge_a is a null pointer' in msg, msg
    rc, msg = call('CHAIN_A', dict(sc, R=0), th, slots)
    assert rc == ARG and 'non-positive count' in msg, msg

    # attention: offsets that do not follow nn
    at = K.mol_topo([2, 3])
    ah = {k: at[k].numpy() if isinstance(at[k], torch.Tensor) else np.asarray(at[k]) for k in ('node_mol', 'nn', 'node_off', 'edge_off')}
    asc = dict(D=128, H=16, XH=2, SC=9, N=3, R=at['R'], Nn=at['Nn'], B=2, ldqk=126, ldv=128, ldd_qk=126, ldd_v=128)
    bad = dict(ah)
    bad['edge_off'] = ah['edge_off'].copy()
    bad['edge_off'][1] = 5
    rc, msg = call('ATTN_FWD', asc, bad, slots)
    assert rc == ARG and 'not consistent with nn' in msg, msg
    bad = dict(ah)
    bad['node_mol'] = ah['node_mol'].copy()
    bad['node_mol'][2] = 0
    rc, msg = call('ATTN_FWD', asc, bad, slots)
    assert rc == ARG and 'node_mol[2] = 0 is out of range' in msg, msg
    rc, msg = call('ATTN_FWD', dict(asc, N=2), ah, slots)
    assert rc == ARG and 'nn[1] = 3 is out of range' in msg, msg

    a = c.FusedTestArgs()
    a.op = len(c.FT_OPS)
    assert c.train_debug_fused(a) == ARG and b'unknown op' in c.lib().jodo_last_error()
    torch.cuda.synchronize()
    for k, b in slots.items():                           # nothing ran: every array still holds what it held
        assert torch.equal(b.bits(), before[k]) and b.guards_ok(), k

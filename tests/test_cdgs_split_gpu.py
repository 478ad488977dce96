"""GPU: the opt-in split-bf16 ("bf16x3") form of CDGS — `model.bf16x3 = True`: every row GEMM over node rows and edge rows (kc_gemm_s)
on the bf16 MFMA with three-term operands, six retained products per K16 step (csrc/dgt_split.h).

Gates, as for the 2-D model (tests/test_dgt2d_split_gpu.py).  The forward tolerance (atol 2e-5 + rtol 1e-4) is hundreds of times the fp32
error on these weights, so a dropped mid * mid product (2^-16 relative) would pass it.  The kernel gate and the block-1 gate therefore
compare ERRORS AGAINST FLOAT64: the split form may be at most 2 x as far from float64 as the exact-fp32 form of the same kernel (the
factor of tests/test_split_gate.py); after one block the yardstick is the larger of the default HIP path's and the float32 oracle's
distance from float64 on the same inputs.  The whole network is then held to the fixtures and to the float64 oracle at the default
path's own bounds (helpers.close64 with K64, fwd_close at 2e-5 + 1e-4 |x|)."""
import ctypes
import random

import numpy as np
import pytest
import torch

from jodo_amd import capi
from jodo_amd import sampling as S
from jodo_amd.models import get_node_dist, load_dataset_info
from jodo_amd.utils import get_data_inverse_scaler
from helpers import K64, close64, load_fixture, make_config
from test_cdgs_gpu import (CFG, DEV, EDGE_CASES, _MODELS, _replay, _samplefn_setup, _scheduler, call, fwd_close, inputs, make_model, oracle_32_64,
                           shared_model)
import oracle2d as O2

pytestmark = pytest.mark.gpu
D = 256
d = lambda v: None if v is None else v.to(DEV)


@pytest.fixture(autouse=True)
def _switches_off():
    yield
    for _, model in list(_MODELS.values()):                  # the sibling's shared models go back to the default path
        model.bf16x3 = False
        model.max_blocks = -1


def call_split(model, *args, split=True):
    model.bf16x3 = split
    out = call(model, *args)
    if split:
        assert model.last_flags.tolist() == [0, 0, 0, 1]
    else:
        assert model.last_flags is None
    return out


# ---- 1. kernel gate: the production row GEMM in both forms on caller-packed weights ---------------------------------------------------
def _pack(W):
    n_out, n_in = W.shape
    f = np.zeros(n_out * n_in, dtype=np.float32)
    s = np.zeros(n_out * n_in * 3, dtype=np.uint16)
    Wc = np.ascontiguousarray(W, dtype=np.float32)
    capi.check(capi.lib().jodo_debug_pack_split(Wc.ctypes.data_as(ctypes.c_void_p), n_out, n_in, f.ctypes.data_as(ctypes.c_void_p),
                                                s.ctypes.data_as(ctypes.c_void_p)), 'pack_split')
    return f, s


_GEMM_W = {}


def _gemm_weights(K, n_out):
    if (K, n_out) not in _GEMM_W:
        g = torch.Generator().manual_seed(1000 * K + n_out)
        W = (torch.rand(n_out, K, generator=g) * 2 - 1) / 16
        bias = torch.randn(n_out, generator=g)
        f, s = _pack(W.numpy())
        _GEMM_W[(K, n_out)] = (W, bias, torch.from_numpy(f).to(DEV), torch.from_numpy(s.view(np.int16)).to(DEV))
    return _GEMM_W[(K, n_out)]


_ACT64 = {0: lambda v: v, 1: torch.nn.functional.silu, 2: torch.relu, 3: torch.tanh}


def _gate(what, mode, xin, x64, rows, K, n_out, with_bias, act, residual=False, desc=None, xadd=None, ldadd=0):
    """Both forms of the production GEMM on the same packed weights against float64.  xin: what the kernel reads (mode 0 / 1: [rows, K];
    mode 2: the node rows); x64 [rows, K]: the rows the MFMAs see, in float64 (for modes 1 / 2 the fp32 sums the kernels form, widened)."""
    W, bias, wf, ws = _gemm_weights(K, n_out)
    y64 = x64 @ W.double().t()
    if with_bias:
        y64 = y64 + bias.double()
    y64 = _ACT64[act](y64)
    g = torch.Generator().manual_seed(rows + 7)
    res = torch.randn(rows, n_out, generator=g) if residual else None
    if residual:
        y64 = y64 + res.double()
    xd, bd = d(xin), d(bias) if with_bias else None
    cfgp, B, N, n_ptr, desc_dev = desc if desc is not None else (None, 0, 0, None, None)
    err = {}
    for split, w in ((0, wf), (1, ws)):
        y = torch.full((rows + 1, n_out), float('nan'), device=DEV)      # one guard row: the row tail clamp reads, never writes, past `rows`
        if residual:
            y[:rows] = d(res)                                             # R aliases Y
        capi.check(capi.lib().jodo_debug_gemm_cdgs(split, mode, cfgp, B, N, n_ptr, capi.ptr(desc_dev), capi.ptr(xd), K, rows, K, n_out,
                                                   capi.ptr(w), capi.ptr(bd), act, capi.ptr(xadd), ldadd, capi.ptr(y) if residual else None,
                                                   capi.ptr(y), n_out, capi.current_stream_ptr()), 'debug_gemm_cdgs')
        torch.cuda.synchronize()
        assert bool(torch.isnan(y[rows]).all()) and bool(torch.isfinite(y[:rows]).all())
        err[split] = float((y[:rows].cpu().double() - y64).abs().max())
    print('%s: err fp32 form %.3e, split form %.3e, ratio %.2f' % (what, err[0], err[1], err[1] / max(err[0], 1e-30)))
    if K == 256:
        assert err[0] < 5e-6                                 # the exact form: a K = 256 fp32 fma chain (tests/test_split_gate.py)
    assert err[1] <= 2.0 * err[0], err


def _x(rows, K, seed):
    return torch.randn(rows, K, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('rows', [1, 33, 65, 130])
def test_split_gemm_rows(rows):
    x = _x(rows, 256, rows)
    _gate('mode 0 rows %d' % rows, 0, x, x.double(), rows, 256, 512, False, 0)


# NB = 16 / 8 / 24 / 3 / 16 / 1: groups of 8 output blocks with and without a tail; nk = 11 is odd, nk = 2 the shortest
@pytest.mark.parametrize('K,n_out', [(256, 512), (512, 256), (256, 768), (256, 96), (704, 512), (128, 32)])
def test_split_gemm_shapes(K, n_out):
    x = _x(65, K, K + n_out)
    _gate('mode 0 K %d n_out %d' % (K, n_out), 0, x, x.double(), 65, K, n_out, True, 1)
    _gate('mode 0 K %d n_out %d plain' % (K, n_out), 0, x, x.double(), 65, K, n_out, False, 0)


@pytest.mark.parametrize('epilogue', ['plain', 'bias-silu', 'bias-relu', 'tanh', 'bias-residual'])
def test_split_gemm_epilogues(epilogue):
    with_bias, act, residual = {'plain': (False, 0, False), 'bias-silu': (True, 1, False), 'bias-relu': (True, 2, False),
                                'tanh': (False, 3, False), 'bias-residual': (True, 0, True)}[epilogue]
    x = _x(130, 512, 5)
    _gate('mode 0 ' + epilogue, 0, x, x.double(), 130, 512, 256, with_bias, act, residual)


def _descriptor(n_nodes):
    cfg, model = shared_model('qm9')
    B, N = len(n_nodes), max(n_nodes)
    n_host = np.ascontiguousarray(n_nodes, dtype=np.int32)
    n_ptr = n_host.ctypes.data_as(ctypes.c_void_p)
    L = capi.lib()
    lay = (ctypes.c_int64 * 8)()
    cfgp = ctypes.byref(model._cfg_struct)
    capi.check(L.jodo_cdgs_layout(cfgp, B, N, n_ptr, lay), 'layout')
    desc = torch.empty(int(lay[0]), dtype=torch.int32)
    capi.check(L.jodo_cdgs_fill_desc(cfgp, B, N, n_ptr, ctypes.c_void_p(desc.data_ptr()), ctypes.c_int64(int(lay[0]))), 'fill_desc')
    return (cfgp, B, N, n_ptr, desc.to(DEV)), n_host, int(lay[3])


# R = 1 / 8 / 512 / 593 edge rows: a one-row launch, one partial tile, the exact strip boundary, one molecule past it
DESCS = {'R=1': [1], 'R=8': [2, 2], 'R=512': [8] * 8, 'R=593': [8] * 7 + [9]}


@pytest.mark.parametrize('case', sorted(DESCS))
def test_split_gemm_mode1_row_plus_time_shift(case):
    n_nodes = DESCS[case]
    desc, n_host, R = _descriptor(n_nodes)
    assert R == sum(n * n for n in n_nodes)
    L, lyr = 8, 3
    x = _x(R, D, R)
    tm = _x(len(n_nodes), 2 * D * L, R + 1)                   # per-molecule shift rows with the forward's stride 2 D L
    off = lyr * 2 * D + D
    mol = torch.repeat_interleave(torch.arange(len(n_nodes)), torch.tensor([n * n for n in n_nodes]))
    xsum = x + tm[mol, off:off + D]                           # fp32, as the kernels add before their MFMAs
    tmd = d(tm)
    _gate('mode 1 ' + case, 1, x, xsum.double(), R, D, 2 * D, False, 3, desc=desc, xadd=tmd.view(-1)[off:], ldadd=2 * D * L)


@pytest.mark.parametrize('case', sorted(DESCS))
def test_split_gemm_mode2_gathered_pair_sums(case):
    n_nodes = DESCS[case]
    desc, n_host, R = _descriptor(n_nodes)
    hc = _x(sum(n_nodes), D, R + 2)
    rr, cc, noff = [], [], 0
    for n in n_nodes:
        for r in range(n):
            for c in range(n):
                rr.append(noff + r)
                cc.append(noff + c)
        noff += n
    xsum = hc[torch.tensor(rr)] + hc[torch.tensor(cc)]        # h_r + h_c in fp32
    _gate('mode 2 ' + case, 2, hc, xsum.double(), R, D, 2 * D, True, 1, desc=desc)


def test_debug_gemm_refuses_bad_arguments():
    x = torch.zeros(8, 64, device=DEV)
    L = capi.lib()
    desc, _, R = _descriptor([2, 2])
    cfgp, B, N, n_ptr, dd = desc
    ok = lambda **kw: L.jodo_debug_gemm_cdgs(*[kw.get(k, v) for k, v in (
        ('split', 1), ('mode', 0), ('cfg', cfgp), ('B', B), ('N', N), ('n', n_ptr), ('desc', capi.ptr(dd)), ('x', capi.ptr(x)), ('ldx', 64),
        ('rows', 8), ('K', 64), ('n_out', 32), ('w', capi.ptr(x)), ('bias', None), ('act', 0), ('xadd', None), ('ldadd', 0), ('res', None),
        ('y', capi.ptr(x)), ('ldy', 32), ('stream', None))])
    assert ok(n_out=48, ldy=48) == -1                         # n_out not a multiple of 32
    assert ok(K=96, ldx=96) == -1                             # K not a multiple of 64
    assert ok(split=0, K=32, ldx=32) == -1
    assert ok(x=None) == -1 and ok(w=None) == -1 and ok(y=None) == -1
    assert ok(mode=2, rows=7) == -1                           # modes 1 / 2: rows must be the descriptor's edge rows (8)
    assert b'edge rows' in L.jodo_last_error()
    assert ok(mode=1, rows=8) == -1                           # mode 1 without its shift rows
    assert ok(mode=2, desc=None) == -1
    assert ok(mode=3) == -1 and ok(act=4) == -1
    torch.cuda.synchronize()


# ---- 2. block-1 gate -----------------------------------------------------------------------------------------------------------------------
def _offdiag(n_nodes):
    rows, idx, off = [], [], 0
    for b, n in enumerate(n_nodes):
        for r in range(n):
            for c in range(n):
                if r != c:
                    rows.append(off + r * n + c)
                    idx.append((b, r, c))
        off += n * n
    diag = torch.ones(off, dtype=torch.bool)
    if rows:
        diag[torch.tensor(rows)] = False
    return torch.tensor(rows, dtype=torch.long), idx, diag


@pytest.mark.parametrize('n_nodes', [[1], [2], [8] * 7 + [9], [1, 29, 7, 2]], ids=['one-atom', 'one-pair', '65-atoms', 'mixed'])
def test_first_block_is_as_close_to_float64_as_fp32_arithmetic(n_nodes):
    cfg, model = shared_model('qm9')
    t, x, ex, nm, em = inputs(cfg, n_nodes, 31)
    r32, r64 = oracle_32_64(cfg, model, t, x, ex, nm, em, return_blocks=True)
    (h32, e32), (h64, e64) = r32[2][1], r64[2][1]
    compact = lambda h: torch.cat([h[b, :n] for b, n in enumerate(n_nodes)]).double()
    rows, idx, diag = _offdiag(n_nodes)
    bi, ri, ci = (torch.tensor([q[k] for q in idx], dtype=torch.long) for k in range(3))
    dense = lambda e: e[bi, ri, ci].double()
    err = {}
    for name, split in (('default', False), ('split', True)):
        model.max_blocks = 1
        call_split(model, t, x, ex, nm, em, split=split)
        h, e = model.debug_state()
        e = e.cpu()
        assert float(e[diag].abs().max()) == 0.0              # the diagonal rows are exactly zero between blocks, in both forms
        err[name] = (float((h.cpu().double() - compact(h64)).abs().max()),
                     float((e[rows].double() - dense(e64)).abs().max()) if len(idx) else 0.0)
    err['oracle32'] = (float((compact(h32) - compact(h64)).abs().max()), float((dense(e32) - dense(e64)).abs().max()) if len(idx) else 0.0)
    for k, what in ((0, 'h'), (1, 'e')):
        yard = max(err['default'][k], err['oracle32'][k])
        print('%s after block 1, %s: |err64| split %.3e, default %.3e, float32 oracle %.3e, ratio %.2f' % (
            what, n_nodes, err['split'][k], err['default'][k], err['oracle32'][k], err['split'][k] / max(yard, 1e-30)))
        assert err['split'][k] <= 2.0 * yard, (what, err)


# ---- 3. the whole network with the switch on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['qm9', 'geom'])
def test_forward_matches_reference_fixture(which):
    fx = load_fixture('fwd_cdgs_%s.npz' % which)
    cfg, model = shared_model(which, int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    nm, em = S.build_masks(n_nodes, max(n_nodes), 'cpu')
    t = lambda k: torch.from_numpy(fx[k])
    got = call_split(model, t('t'), t('x'), t('edge_x'), nm, em)
    fwd_close(got[0], t('out_x'), which + ' split x')
    fwd_close(got[1], t('out_e'), which + ' split e')


def test_blocks_match_reference_fixture():
    fx = load_fixture('blocks_cdgs_qm9.npz')
    cfg, model = shared_model('qm9', int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    nm, em = S.build_masks(n_nodes, max(n_nodes), 'cpu')
    t = lambda k: torch.from_numpy(fx[k])
    rows, _, diag = _offdiag(n_nodes)
    for l in range(cfg.model.n_layers):
        model.max_blocks = l + 1
        call_split(model, t('t'), t('x'), t('edge_x'), nm, em)
        h, e = model.debug_state()
        fwd_close(h, torch.from_numpy(fx['h'][l]), 'split h after block %d' % l)
        fwd_close(e.cpu()[rows], torch.from_numpy(fx['e'][l]), 'split e after block %d' % l)
        assert float(e.cpu()[diag].abs().max()) == 0.0


def check64_split(cfg, model, n_nodes, seed, what, N=None, symmetric=True):
    """tests/test_cdgs_gpu.py check64 with the switch on; the exact path on the same inputs must give other bits."""
    t, x, ex, nm, em = inputs(cfg, n_nodes, seed, N, symmetric)
    exact = call_split(model, t, x, ex, nm, em, split=False)
    got = call_split(model, t, x, ex, nm, em)
    r32, r64 = oracle_32_64(cfg, model, t, x, ex, nm, em)
    close64(got[0], r32[0], r64[0], 'bf16x3 ' + what + ' x', k=K64)
    close64(got[1], r32[1], r64[1], 'bf16x3 ' + what + ' e', k=K64)
    B, N = ex.shape[0], ex.shape[1]
    assert float((got[0].cpu() * (1 - nm)).abs().max()) == 0.0
    assert float((got[1].cpu() * (1 - em.reshape(B, N, N, 1))).abs().max()) == 0.0
    assert torch.equal(got[1], got[1].transpose(1, 2))
    if sum(n_nodes) > 1:
        assert not (torch.equal(got[0], exact[0]) and torch.equal(got[1], exact[1])), "the split kernels did not run"
    return got


@pytest.mark.parametrize('case', sorted(EDGE_CASES))
def test_size_edges(case):
    cfg, model = shared_model('qm9')
    check64_split(cfg, model, EDGE_CASES[case], 41, case)


@pytest.mark.parametrize('B', [63, 64, 65])
def test_batch_sizes_around_a_gemm_strip(B):
    cfg, model = shared_model('qm9')
    check64_split(cfg, model, [1 + (b % 3) for b in range(B)], 43, 'B=%d' % B)


def test_asymmetric_edge_input_and_a_batch_padded_wider_than_its_maximum():
    cfg, model = shared_model('qm9')
    check64_split(cfg, model, [9, 21, 1, 2, 14], 59, 'asymmetric', symmetric=False)
    check64_split(cfg, model, [9, 4, 7, 2], 31, 'padded to 12', N=12)


# ---- 4. the exact path is untouched ----------------------------------------------------------------------------------------------------------
def _direct_exact(model, t, x, ex):
    """The unchanged jodo_cdgs_forward entry on the last call's plan and packed blob, with a workspace of its own."""
    plan = model._last_plan
    _, blob, woff_c, n_woff = model._packed
    t, x, ex = (d(v).float().contiguous() for v in (t, x, ex))
    out_x, out_e = torch.full_like(x, float('nan')), torch.full_like(ex, float('nan'))
    ws = torch.zeros_like(plan['ws'])
    capi.check(capi.lib().jodo_cdgs_forward(ctypes.byref(model._cfg_struct), plan['B'], plan['N'], plan['n_nodes'].ctypes.data_as(ctypes.c_void_p),
                                            capi.ptr(plan['desc']), capi.ptr(blob), woff_c, n_woff, capi.ptr(t), capi.ptr(x), capi.ptr(ex),
                                            capi.ptr(out_x), capi.ptr(out_e), capi.ptr(ws), -1, capi.current_stream_ptr()), 'jodo_cdgs_forward')
    torch.cuda.synchronize()
    return out_x, out_e


@pytest.mark.parametrize('n_nodes', [[1], [8] * 7 + [9], [1, 29, 7, 2]], ids=['one-atom', '65-atoms', 'mixed'])
def test_the_exact_path_is_untouched_and_the_split_form_is_deterministic(n_nodes):
    cfg, model = shared_model('qm9')
    t, x, ex, nm, em = inputs(cfg, n_nodes, 37)
    nmd, emd = d(nm), d(em)                                   # one mask storage: every call below uses the same plan
    args = (t, x, ex, nmd, emd)
    a = call_split(model, *args, split=False)
    assert model.last_flags is None
    b = _direct_exact(model, t, x, ex)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])            # the default path is the unchanged entry, bit for bit
    plan = model._last_plan
    s1 = call_split(model, *args)
    s2 = call_split(model, *args)
    assert model._last_plan is plan
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])        # two split calls: the same bits
    c = call_split(model, *args, split=False)                             # ... and the exact path does not depend on a split call before it
    assert model.last_flags is None and model._last_plan is plan
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    b2 = _direct_exact(model, t, x, ex)
    assert torch.equal(b[0], b2[0]) and torch.equal(b[1], b2[1])


# ---- 5. the tape follows the weights -----------------------------------------------------------------------------------------------------------
def test_tape_follows_the_weights():
    cfg = make_config(CFG['qm9'])
    model = make_model(cfg, 7)
    n_nodes = [7, 12, 3]
    args = inputs(cfg, n_nodes, 6)

    def fresh_output():
        twin = make_model(cfg, 19)
        twin.load_state_dict(model.state_dict())
        return call_split(twin, *args)

    base = call_split(model, *args)
    tape0 = model._tape[1]
    with torch.no_grad():                                    # an in-place update that bumps the tensor version (an optimiser step)
        model.all_modules[10 + 3 * 2].ff_linear3.weight.add_(0.01)       # both are read from the tape only
        model.all_modules[10 + 3 * 5].self_attn.lin_edge1.weight.add_(0.01)
    upd = call_split(model, *args)
    assert model._tape[1] is not tape0 and model._tape[0] is model._packed
    want = fresh_output()
    assert torch.equal(upd[0], want[0]) and torch.equal(upd[1], want[1])
    assert not torch.equal(upd[0], base[0]) and not torch.equal(upd[1], base[1])       # (the comparison above is not one of unchanged outputs)
    model.load_state_dict(make_model(cfg, 23).state_dict())
    assert model._packed is None and model._tape is None
    upd2 = call_split(model, *args)
    want = fresh_output()
    assert torch.equal(upd2[0], want[0]) and torch.equal(upd2[1], want[1])
    assert not torch.equal(upd2[0], upd[0]) and not torch.equal(upd2[1], upd[1])
    with torch.no_grad():                                    # a `.data` write bumps nothing: the caller says so
        model.all_modules[10 + 3 * 8].weight.data.mul_(1.5)              # the atom head's first layer
        model.all_modules[10].ff_linear4.weight.data.mul_(1.5)
    model.invalidate_packed_weights()
    assert model._packed is None and model._tape is None
    upd3 = call_split(model, *args)
    want = fresh_output()
    assert torch.equal(upd3[0], want[0]) and torch.equal(upd3[1], want[1])
    assert not torch.equal(upd3[0], upd2[0]) and not torch.equal(upd3[1], upd2[1])


def test_first_switch_on_under_graph_capture_is_refused(monkeypatch):
    cfg = make_config(CFG['qm9'])
    model = make_model(cfg, 7)
    t, x, ex, nm, em = inputs(cfg, [3, 5], 6)
    args = (t, x, ex, d(nm), d(em))
    call_split(model, *args, split=False)                    # plan and blob exist; no tape yet
    model.bf16x3 = True
    with monkeypatch.context() as m:                         # (no capture is started: the model asks torch whether one is running)
        m.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        with pytest.raises(RuntimeError, match='one eager call with bf16x3 = True first'):
            call(model, *args)
        assert model._tape is None
    call_split(model, *args)                                 # eager: builds the tape
    with monkeypatch.context() as m:                         # ... after which a captured call finds it
        m.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        call_split(model, *args)


# ---- 6. rounds ------------------------------------------------------------------------------------------------------------------------------------
def test_ancestral_trajectory_fixture_replayed_with_the_switch_on():
    fx = load_fixture('traj_cdgs_qm9_anc5.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain']))
    model.bf16x3 = True
    ns, steps, n_nodes = _scheduler(cfg), int(fx['steps']), fx['n_nodes'].tolist()
    nm, em = S.build_masks(n_nodes, max(n_nodes), DEV)
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond, noise_fn=_replay(fx))
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    assert model.last_flags[3].item() == 1
    ex_, ee_ = (x_mean.cpu() - torch.from_numpy(fx['x_mean'])).abs().max().item(), (e_mean.cpu() - torch.from_numpy(fx['edge_x_mean'])).abs().max().item()
    print('bf16x3 free-running end state: max |err|', ex_, ee_)
    assert ex_ <= 1e-3 and ee_ <= 1e-3
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_mean.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_mean.clone(), em,
                                        cfg.data.compress_edge)
    bad, excluded = O2.decode_agrees(fx, one_hot.argmax(2).cpu().numpy(), fc.cpu().numpy(), et.cpu().numpy(), n_nodes)
    print('bf16x3 decodes: mismatches', bad, 'excluded share', excluded)
    assert bad == 0
    assert excluded <= float(fx['margin_cap']) and float(fx['margin_shares'].max()) <= float(fx['margin_cap']) == 0.05


def test_sampling_fn_with_the_switch_on_reproduces_the_reference_run():
    fx, cfg, model, ns, dist = _samplefn_setup()             # the single-device DataParallel wrapper; the switch goes on the inner module
    model.module.bf16x3 = True
    batch, seed = int(fx['batch']), int(fx['seed'])
    inv = get_data_inverse_scaler(cfg)
    fn = S.get_sampling_fn(cfg, ns, dist, batch, batch, inv, return_raw=True, cpu_noise=True)
    torch.manual_seed(seed)
    random.seed(seed)
    mols = fn(model)
    assert model.module.last_flags[3].item() == 1
    assert [int(m[1].shape[0]) for m in mols] == fx['n_nodes'].tolist()
    at, fc, et = np.zeros_like(fx['atom_type']), np.zeros_like(fx['fc']), np.zeros_like(fx['edge_type'])
    for b, (pos, a, e, q) in enumerate(mols):
        n = a.shape[0]
        assert pos is None
        at[b, :n], et[b, :n, :n] = a.numpy(), e.numpy()
    bad, excluded = O2.decode_agrees(fx, at, fc, et, fx['n_nodes'].tolist())
    print('bf16x3 samplefn_cdgs: mismatches', bad, 'excluded share', excluded)
    assert bad == 0 and excluded <= 0.05
    graphed = S.get_sampling_fn(cfg, ns, dist, batch, batch, inv, hip_graph=True, return_raw=True)
    with pytest.raises(NotImplementedError, match='graph replay'):
        graphed(model)

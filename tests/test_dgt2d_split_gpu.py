"""GPU: the opt-in split-bf16 ("bf16x3") form of DGT_concat_2D — `model.bf16x3 = True`: the node GEMMs (k2d_gemm_s) and the pair
update (k2d_pair_s) on the bf16 MFMA with three-term operands, six retained products per K16 step (csrc/dgt_split.h).

Gates.  The forward tolerance (atol 2e-5 + rtol 1e-4) is about 400 x the fp32 error on these weights, so a dropped mid * mid product
(2^-16 relative) would pass it.  The kernel gate and the block-1 gate therefore compare ERRORS AGAINST FLOAT64: the split form may be
at most 2 x as far from float64 as the exact-fp32 form of the same kernel (the factor of tests/test_split_gate.py); after one block the
yardstick is the larger of the default HIP path's and the float32 oracle's distance from float64 on the same inputs.  The whole network
is then held to the fixtures and to the float64 oracle at the default path's own bounds."""
import ctypes

import numpy as np
import pytest
import torch

from jodo_amd import capi, fused
from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.graphed import GraphedAncestralRound2D
from jodo_amd.mix_dpm_solver import DPM_Solver_2D
from jodo_amd.models import utils as mutils
from helpers import K64, close64, load_fixture, make_config, make_model, masks, state_dict_cpu
from test_dgt2d_gpu import fwd_close, sym_inputs
import oracle2d as O2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFG = 'vpsde_zinc_2d_jodo'
BATCHES = [[1], [2], [38, 27], [1, 38, 7, 2]]        # one row, no pairs | one pair | 65 rows, 1054 pairs (a part-filled last strip) | mixed
BATCH_IDS = ['one-atom', 'one-pair', '65-rows', 'mixed']
d = lambda v: None if v is None else v.to(DEV)


def call(model, xh, nm, em, ex, cx, cex, nl, split=True):
    model.bf16x3 = split
    with torch.no_grad():
        out = model(nl, xh, nm, em, edge_x=ex, cond_x=cx, cond_edge_x=cex, noise_level=nl)
    assert model.last_flags[3].item() == (1 if split else 0)
    return out


def cond_inputs(cfg, xh, ex, nm, em, seed):
    """self-conditioning inputs for a batch of sym_inputs: masked node tensor, symmetric masked edge tensor"""
    g = torch.Generator().manual_seed(seed)
    B, N = ex.shape[0], ex.shape[1]
    cx = torch.randn(xh.shape, generator=g) * nm
    cex = torch.randn(ex.shape, generator=g)
    cex = (cex + cex.transpose(1, 2)) * 0.5 * em.reshape(B, N, N, 1)
    return cx, cex


@pytest.fixture(scope='module')
def zinc():
    cfg = make_config(CFG)
    model = make_model(cfg, 7, DEV)
    sd = state_dict_cpu(model)
    return cfg, model, sd, {k: v.double() for k, v in sd.items()}, O2.Hyper2D.from_config(cfg)


@pytest.fixture(autouse=True)
def _switches_off(request):
    yield
    if 'zinc' in request.fixturenames:
        model = request.getfixturevalue('zinc')[1]
        model.bf16x3 = model.pair_attention = model.force_directed = False
        model.max_blocks = -1


_ORACLE = {}


def oracle(zinc, key, xh, nm, em, ex, cx, cex, nl):
    """(float32, float64) dense oracle with the per-block states, computed once per input set and shared between the tests"""
    if key not in _ORACLE:
        _, _, sd, sd64, hp = zinc
        f64 = lambda v: None if v is None else v.double()
        with torch.no_grad():
            r32 = O2.forward_dense(sd, hp, xh, nm, em, ex, cx, cex, nl, return_blocks=True)
            r64 = O2.forward_dense(sd64, hp, xh.double(), nm, em, ex.double(), f64(cx), f64(cex), nl.double(), return_blocks=True)
        _ORACLE[key] = (r32, r64)
    return _ORACLE[key]


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


@pytest.mark.parametrize('epilogue', ['plain', 'bias-silu'])
# NB = 2 below the form's NOB = 8 | NB = 8: a full walk | NB = 5: no multiple of NOB | NB = 17: three output-block groups, a tail of one
@pytest.mark.parametrize('K,n_out', [(256, 64), (512, 256), (768, 160), (256, 544)])
@pytest.mark.parametrize('rows', [1, 33, 65, 130])
def test_split_gemm_is_as_good_as_the_fp32_gemm(rows, K, n_out, epilogue):
    W, bias, wf, ws = _gemm_weights(K, n_out)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, K, generator=g)
    y64 = x.double() @ W.double().t()
    if epilogue == 'bias-silu':
        y64 = torch.nn.functional.silu(y64 + bias.double())
    xd, bd = d(x), d(bias) if epilogue == 'bias-silu' else None
    err = {}
    for split, w in ((0, wf), (1, ws)):
        y = torch.full((rows + 1, n_out), float('nan'), device=DEV)       # one guard row: the row tail clamp reads, never writes, past `rows`
        capi.check(capi.lib().jodo_debug_gemm2d(split, capi.ptr(xd), rows, K, n_out, capi.ptr(w), capi.ptr(bd), 1 if bd is not None else 0,
                                                capi.ptr(y), capi.current_stream_ptr()), 'debug_gemm2d')
        torch.cuda.synchronize()
        assert bool(torch.isnan(y[rows]).all()) and bool(torch.isfinite(y[:rows]).all())
        err[split] = float((y[:rows].cpu().double() - y64).abs().max())
    print('rows %d K %d n_out %d %s: err fp32 form %.3e, split form %.3e, ratio %.2f' % (rows, K, n_out, epilogue, err[0], err[1],
                                                                                         err[1] / max(err[0], 1e-30)))
    if K == 256:
        assert err[0] < 5e-6                                  # the exact form: a K = 256 fp32 fma chain (tests/test_split_gate.py)
    assert err[1] <= 2.0 * err[0], err


def test_debug_gemm_refuses_bad_arguments():
    x = torch.zeros(4, 64, device=DEV)
    L = capi.lib()
    assert L.jodo_debug_gemm2d(0, capi.ptr(x), 4, 64, 48, capi.ptr(x), None, 0, capi.ptr(x), None) == -1       # n_out not a multiple of 32
    assert L.jodo_debug_gemm2d(1, capi.ptr(x), 4, 96, 32, capi.ptr(x), None, 0, capi.ptr(x), None) == -1       # K not a multiple of 64
    assert L.jodo_debug_gemm2d(1, None, 4, 64, 32, capi.ptr(x), None, 0, capi.ptr(x), None) == -1


# ---- 2. block-1 gate -----------------------------------------------------------------------------------------------------------------------
def _pair_rows(n_nodes):
    """(workspace row, b, r, c) of every ordered pair r != c: the unordered pair's row, as test_blocks_match_reference_fixture maps it"""
    rows, idx, off = [], [], 0
    for b, n in enumerate(n_nodes):
        for r in range(n):
            for c in range(n):
                if r != c:
                    rows.append(off + min(r, c) * n + max(r, c))
                    idx.append((b, r, c))
        off += n * n
    return torch.tensor(rows, dtype=torch.long), idx


@pytest.mark.parametrize('cond', [False, True], ids=['first-step', 'conditioned'])
@pytest.mark.parametrize('shared', [True, False], ids=['shared-level', 'per-molecule-levels'])
@pytest.mark.parametrize('n_nodes', BATCHES, ids=BATCH_IDS)
def test_first_block_is_as_close_to_float64_as_fp32_arithmetic(zinc, n_nodes, shared, cond):
    cfg, model = zinc[0], zinc[1]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 31, shared_level=0.4 if shared else None)
    cx, cex = cond_inputs(cfg, xh, ex, nm, em, 32) if cond else (None, None)
    r32, r64 = oracle(zinc, (tuple(n_nodes), shared, cond), xh, nm, em, ex, cx, cex, nl)
    (h32, e32), (h64, e64) = r32[2][0], r64[2][0]
    compact = lambda h: torch.cat([h[b, :n] for b, n in enumerate(n_nodes)]).double()
    rows, idx = _pair_rows(n_nodes)
    bi, ri, ci = (torch.tensor([t[k] for t in idx], dtype=torch.long) for k in range(3))
    dense = lambda e: e[bi, ri, ci].double()
    model.max_blocks = 1
    args = (d(xh), d(nm), d(em), d(ex), d(cx), d(cex), d(nl))
    err = {}
    for name, split in (('default', False), ('split', True)):
        call(model, *args, split=split)
        h, e = model.debug_state()
        err[name] = (float((h.cpu().double() - compact(h64)).abs().max()),
                     float((e.cpu()[rows].double() - dense(e64)).abs().max()) if len(idx) else 0.0)
    err['oracle32'] = (float((compact(h32) - compact(h64)).abs().max()), float((dense(e32) - dense(e64)).abs().max()) if len(idx) else 0.0)
    for k, what in ((0, 'h'), (1, 'e')):
        yard = max(err['default'][k], err['oracle32'][k])
        print('%s after block 1, %s: |err64| split %.3e, default %.3e, float32 oracle %.3e, ratio %.2f' % (
            what, n_nodes, err['split'][k], err['default'][k], err['oracle32'][k], err['split'][k] / max(yard, 1e-30)))
        assert err['split'][k] <= 2.0 * yard, (what, err)


# ---- 3. the whole network with the switch on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_forward_matches_reference_fixture(which):
    fx = load_fixture('fwd2d_%s.npz' % which)
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    o1 = call(model, t('xh'), nm, em, t('edge_x'), None, None, t('noise_level'))
    assert model.last_flags[0].item() == 1
    fwd_close(o1[0], torch.from_numpy(fx['out1_x']), which + ' split first step x')
    fwd_close(o1[1], torch.from_numpy(fx['out1_e']), which + ' split first step e')
    o2 = call(model, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'))
    fwd_close(o2[0], torch.from_numpy(fx['out2_x']), which + ' split self-conditioned x')
    fwd_close(o2[1], torch.from_numpy(fx['out2_e']), which + ' split self-conditioned e')


def test_blocks_match_reference_fixture():
    fx = load_fixture('blocks2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    rows, _ = _pair_rows(n_nodes)
    for l in range(cfg.model.n_layers):
        model.max_blocks = l + 1
        call(model, t('xh'), nm, em, t('edge_x'), t('cond_x'), t('cond_edge_x'), t('noise_level'))
        h, e = model.debug_state()
        fwd_close(h, torch.from_numpy(fx['h'][l]), 'split h after block %d' % l)
        fwd_close(e.cpu()[rows], torch.from_numpy(fx['e'][l]), 'split e after block %d' % l)


def _direct_exact(model, args):
    """The unchanged jodo_dgt2d_forward entry on the last call's plan and packed blob, with flags and a workspace of its own."""
    xh, nm, em, ex, cx, cex, nl = args
    plan = model._last_plan
    _, blob, woff_c, n_woff = model._packed
    out_x, out_e = torch.full_like(xh, float('nan')), torch.full_like(ex, float('nan'))
    flags, ws = torch.zeros_like(plan['flags']), torch.zeros_like(plan['ws'])
    capi.check(capi.lib().jodo_dgt2d_forward(ctypes.byref(model._cfg_struct), plan['B'], plan['N'], plan['n_nodes'].ctypes.data_as(ctypes.c_void_p),
                                             capi.ptr(plan['desc']), capi.ptr(blob), woff_c, n_woff, capi.ptr(xh), capi.ptr(ex), capi.ptr(cx),
                                             capi.ptr(cex), capi.ptr(nl), capi.ptr(out_x), capi.ptr(out_e), capi.ptr(flags), capi.ptr(ws), 0, -1,
                                             capi.current_stream_ptr()), 'jodo_dgt2d_forward')
    torch.cuda.synchronize()
    assert flags[3].item() == 0
    return out_x, out_e


@pytest.mark.parametrize('n_nodes', BATCHES, ids=BATCH_IDS)
def test_batches_against_float64_and_the_exact_path_is_untouched(zinc, n_nodes):
    cfg, model = zinc[0], zinc[1]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 31)
    cx, cex = cond_inputs(cfg, xh, ex, nm, em, 32)
    r32, r64 = oracle(zinc, (tuple(n_nodes), False, True), xh, nm, em, ex, cx, cex, nl)
    args = tuple(d(v).contiguous() for v in (xh, nm, em, ex, cx, cex, nl))
    a = call(model, *args, split=False)
    b = _direct_exact(model, args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])           # the default path is the unchanged entry, bit for bit
    s = call(model, *args, split=True)
    close64(s[0], r32[0], r64[0], 'bf16x3 %s nodes' % n_nodes, k=K64)
    close64(s[1], r32[1], r64[1], 'bf16x3 %s edges' % n_nodes, k=K64)
    if sum(n_nodes) > 1:
        assert not (torch.equal(s[0], a[0]) and torch.equal(s[1], a[1])), "the split kernels did not run"
    c = call(model, *args, split=False)                                 # ... and does not depend on a split call on the same plan before it
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ---- 4. invariants under the switch -----------------------------------------------------------------------------------------------------------
def test_invariants_determinism_and_the_other_switches(zinc):
    cfg, model, sd, sd64, hp = zinc
    n_nodes = [1, 38, 7, 2]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 31)
    cx, cex = cond_inputs(cfg, xh, ex, nm, em, 32)
    _, r64 = oracle(zinc, (tuple(n_nodes), False, True), xh, nm, em, ex, cx, cex, nl)
    B, N = len(n_nodes), max(n_nodes)
    emd = em.reshape(B, N, N, 1)
    args = (d(xh), d(nm), d(em), d(ex), d(cx), d(cex), d(nl))
    a = call(model, *args)
    b = call(model, *args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float((a[0].cpu() * (1 - nm)).abs().max()) == 0.0 and float((a[1].cpu() * (1 - emd)).abs().max()) == 0.0
    assert torch.equal(a[1], a[1].transpose(1, 2))
    # the directed fallback (2 P items in the pair update) on symmetric inputs ...
    model.force_directed = True
    f = call(model, *args)
    model.force_directed = False
    assert model.last_flags[0].item() == 0
    fwd_close(f[0], r64[0], 'bf16x3 force_directed x')
    fwd_close(f[1], r64[1], 'bf16x3 force_directed e')
    assert torch.equal(f[1], f[1].transpose(1, 2))
    # ... and on genuinely asymmetric edge inputs
    g = torch.Generator().manual_seed(12)
    asym = torch.randn(B, N, N, cfg.model.edge_ch, generator=g) * emd
    casym = torch.randn(B, N, N, cfg.model.edge_ch, generator=g) * emd
    got = call(model, d(xh), d(nm), d(em), d(asym), d(cx), d(casym), d(nl))
    assert model.last_flags[0].item() == 0
    with torch.no_grad():
        want = O2.forward_dense(sd64, hp, xh.double(), nm, em, asym.double(), cx.double(), casym.double(), nl.double())
    fwd_close(got[0], want[0], 'bf16x3 asymmetric x')
    fwd_close(got[1], want[1], 'bf16x3 asymmetric e')
    assert torch.equal(got[1], got[1].transpose(1, 2))
    # the pair-symmetric attention walk together with the switch
    model.pair_attention = True
    p = call(model, *args)
    assert model.last_flags.tolist()[2:4] == [1, 1]
    fwd_close(p[0], r64[0], 'bf16x3 + pair_attention x')
    fwd_close(p[1], r64[1], 'bf16x3 + pair_attention e')
    model.pair_attention = False
    call(model, *args)
    assert model.last_flags.tolist()[2:4] == [0, 1]


# ---- 5. the tape follows the weights -----------------------------------------------------------------------------------------------------------
def test_tape_follows_the_weights():
    cfg = make_config(CFG)
    model = make_model(cfg, 7, DEV)
    n_nodes = [7, 12, 3]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 6)
    args = (d(xh), d(nm), d(em), d(ex), None, None, d(nl))

    def fresh_output():
        twin = make_model(cfg, 19, DEV)
        twin.load_state_dict(model.state_dict())
        return call(twin, *args)

    base = call(model, *args)
    tape0 = model._tape[1]
    with torch.no_grad():                                    # an in-place update that bumps the tensor version (an optimiser step)
        model.e_block_2.ff_linear1.weight.add_(0.01)         # both live in the tape only (node GEMM, pair update)
        model.e_block_5.ff_linear3.weight.add_(0.01)
    upd = call(model, *args)
    assert model._tape[1] is not tape0 and model._tape[0] is model._packed
    want = fresh_output()
    assert torch.equal(upd[0], want[0]) and torch.equal(upd[1], want[1])
    assert not torch.equal(upd[0], base[0]) and not torch.equal(upd[1], base[1])       # (the comparison above is not one of unchanged outputs)
    model.load_state_dict(make_model(cfg, 23).state_dict())
    assert model._packed is None
    upd2 = call(model, *args)
    want = fresh_output()
    assert torch.equal(upd2[0], want[0]) and torch.equal(upd2[1], want[1])
    assert not torch.equal(upd2[0], upd[0]) and not torch.equal(upd2[1], upd[1])
    with torch.no_grad():                                    # a `.data` write bumps nothing: the caller says so
        model.node_pred_mlp[0].weight.data.mul_(1.5)
        model.e_block_0.ff_linear4.weight.data.mul_(1.5)
    model.invalidate_packed_weights()
    assert model._packed is None and model._tape is None
    upd3 = call(model, *args)
    want = fresh_output()
    assert torch.equal(upd3[0], want[0]) and torch.equal(upd3[1], want[1])
    assert not torch.equal(upd3[0], upd2[0]) and not torch.equal(upd3[1], upd2[1])


def test_first_switch_on_under_graph_capture_is_refused(monkeypatch):
    cfg = make_config(CFG)
    model = make_model(cfg, 7, DEV)
    xh, ex, nl, nm, em = sym_inputs(cfg, [3, 5], 6)
    args = (d(xh), d(nm), d(em), d(ex), None, None, d(nl))
    call(model, *args, split=False)                          # plan and blob exist; no tape yet
    model.bf16x3 = True
    with monkeypatch.context() as m:                         # (no capture is started: the model asks torch whether one is running)
        m.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        with torch.no_grad(), pytest.raises(RuntimeError, match='one eager call with bf16x3 = True first'):
            model(args[6], args[0], args[1], args[2], edge_x=args[3], cond_x=None, cond_edge_x=None, noise_level=args[6])
        assert model._tape is None
    call(model, *args)                                       # eager: builds the tape
    with monkeypatch.context() as m:                         # ... after which a captured call finds it
        m.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        call(model, *args)


# ---- 6. rounds ------------------------------------------------------------------------------------------------------------------------------------
def _schedule(cfg):
    return NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)


def test_graph_replay_equals_the_eager_device_noise_round():
    steps, key, n_nodes = 6, (13, 2, 4), [5, 3, 9]
    cfg = make_config(CFG)
    model = make_model(cfg, 7, DEV, head_gain=8.0)
    model.bf16x3 = True
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    g = torch.Generator().manual_seed(21)
    z = d(mutils.sample_gaussian_with_mask((B, N, nd), 'cpu', nm, generator=g))
    ez = d(mutils.sample_symmetric_edge_feature_noise(B, N, ch, em, generator=g).contiguous())
    nm, em = d(nm), d(em)
    ns = _schedule(cfg)
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond)
    try:
        sampler.device_noise = fused.DeviceNoise.for_rank(*key)
        with torch.no_grad():
            want = [v.clone() for v in sampler.sampling(model, z, nm, em, ez, None)]
        assert model.last_flags[3].item() == 1
        sampler.device_noise = fused.DeviceNoise.for_rank(*key)
        with torch.no_grad():
            rnd = GraphedAncestralRound2D(sampler, model, nm, em)
            got = rnd.run(z, ez)
        torch.cuda.synchronize()
    finally:
        sampler.device_noise = None
    assert rnd.graph is not None and model.last_flags[3].item() == 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_ancestral_trajectory_fixture_replayed_with_the_switch_on():
    fx = load_fixture('traj2d_zinc_anc5.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    model.bf16x3 = True
    ns = _schedule(cfg)
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    replay = lambda i, kind, like: torch.from_numpy(fx['node_noise' if kind == 'node' else 'edge_noise'][i]).to(like.device)
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, int(fx['steps'])), cfg.model.pred_data, cfg.model.self_cond, noise_fn=replay)
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    assert model.last_flags[3].item() == 1
    ex_, ee_ = (x_mean.cpu() - torch.from_numpy(fx['x_mean'])).abs().max().item(), (e_mean.cpu() - torch.from_numpy(fx['edge_x_mean'])).abs().max().item()
    print('bf16x3 ancestral end state: max |err|', ex_, ee_)
    assert ex_ <= 1e-3 and ee_ <= 1e-3


def test_dpm_trajectory_fixture_replayed_with_the_switch_on():
    fx = load_fixture('traj2d_zinc_dpm_single2.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.sampling.method, cfg.sampling.steps = 'dpm_2d', int(fx['steps'])
    cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = str(fx['dpm_solver_method']), int(fx['dpm_solver_order'])
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    model.bf16x3 = True
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    solver = DPM_Solver_2D(_schedule(cfg), cfg)
    x_end, e_end = solver.sampling(model, d(torch.from_numpy(fx['z'])), nm, em, d(torch.from_numpy(fx['edge_z'])), None)
    assert model.last_flags[3].item() == 1
    ex_, ee_ = (x_end.cpu() - torch.from_numpy(fx['x_end'])).abs().max().item(), (e_end.cpu() - torch.from_numpy(fx['edge_x_end'])).abs().max().item()
    print('bf16x3 dpm_2d end state: max |err|', ex_, ee_)
    assert ex_ <= 1e-3 and ee_ <= 1e-3
    assert torch.equal(e_end, e_end.transpose(1, 2))

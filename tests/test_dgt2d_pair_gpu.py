"""GPU: the pair-symmetric attention walk of DGT_concat_2D (model.pair_attention = True; csrc/dgt2d_forward.hip k2d_attn_pair) against
the reference's fixtures, the float64 dense oracle (tests/oracle2d.py) and the directed walk.

Bound: the project's forward tolerance atol 2e-5 + rtol 1e-4 |want| of tests/test_dgt2d_gpu.py, unchanged — the pair walk evaluates the
same fp32 expressions per edge and differs from the directed walk in the summation order of a target's softmax only.  Pair against
directed: twice that bound, both being within it of the reference.  Every test that expects the pair walk asserts last_flags[2] == 1."""
import os

import numpy as np
import pytest
import torch

from jodo_amd import fused
from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.graphed import GraphedAncestralRound2D
from jodo_amd.models import get_node_dist
from jodo_amd.models import utils as mutils
from jodo_amd.utils import get_data_inverse_scaler
from helpers import load_fixture, make_config, make_model, state_dict_cpu, masks, GOLDEN
import oracle2d as O2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL, RTOL = 2e-5, 1e-4
CFG = {'zinc': 'vpsde_zinc_2d_jodo', 'moses': 'vpsde_moses_2d_jodo'}
d = lambda v: None if v is None else v.to(DEV)

EDGE_SIZES = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64]     # odd / even half offset; ends on, crosses and fills a wave; the maximal width
GAP_SIZES = [40, 33, 30, 7, 50, 3]                   # groups (50, 40, 33, 3) and (30, 7): unused slots, 40 atoms across waves 1 and 2


def fwd_close(got, want, what, factor=1.0):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = factor * (ATOL + RTOL * want.abs())
    print('%s: max |err| %.3e, worst err / bound %.3f' % (what, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all()), "%s: max |err| %g, worst err / bound %g" % (what, err.max().item(), (err / bound).max().item())


def call(model, xh, nm, em, ex, cx, cex, nl, pair=True, walked=None):
    """One forward; walked = 1 / 0: assert which attention walk did the work (default: the pair walk when it was asked for)."""
    model.pair_attention = pair
    with torch.no_grad():
        out = model(nl, xh, nm, em, edge_x=ex, cond_x=cx, cond_edge_x=cex, noise_level=nl)
    if pair:
        assert model.last_flags[2].item() == (1 if walked is None else walked)
    return out


def sym_inputs(cfg, n_nodes, seed, shared_level=None, cond=False):
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), int(max(n_nodes))
    nm, em = masks(n_nodes)
    emd = em.reshape(B, N, N, 1)
    xh = torch.randn(B, N, nd, generator=g) * nm
    ex = torch.randn(B, N, N, ch, generator=g)
    ex = (ex + ex.transpose(1, 2)) * emd
    nl = torch.full((B,), float(shared_level)) if shared_level is not None else torch.randn(B, generator=g) * 2
    cx = cex = None
    if cond:
        cx = torch.randn(B, N, nd, generator=g) * nm
        cex = torch.randn(B, N, N, ch, generator=g)
        cex = (cex + cex.transpose(1, 2)) * 0.5 * emd
    return xh, ex, cx, cex, nl, nm, em


@pytest.fixture(scope='module')
def zinc():
    cfg = make_config(CFG['zinc'])
    return cfg, make_model(cfg, 7, DEV)


@pytest.fixture(autouse=True)
def _switches_off(request):
    yield
    if 'zinc' in request.fixturenames:
        model = request.getfixturevalue('zinc')[1]
        model.pair_attention = model.force_directed = False
        model.max_blocks = -1


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_forward_matches_reference_fixture(which):
    fx = load_fixture('fwd2d_%s.npz' % which)
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    n_nodes = fx['n_nodes'].tolist()
    assert {1, 2}.issubset(n_nodes)
    nm, em = masks(n_nodes, DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    o1 = call(model, t('xh'), nm, em, t('edge_x'), None, None, t('noise_level'))
    fwd_close(o1[0], torch.from_numpy(fx['out1_x']), which + ' first step x')
    fwd_close(o1[1], torch.from_numpy(fx['out1_e']), which + ' first step e')
    o2 = call(model, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'))
    fwd_close(o2[0], torch.from_numpy(fx['out2_x']), which + ' self-conditioned x')
    fwd_close(o2[1], torch.from_numpy(fx['out2_e']), which + ' self-conditioned e')


def test_blocks_match_reference_fixture():
    fx = load_fixture('blocks2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    rows, off = [], 0
    for n in n_nodes:
        rows += [off + min(r, c) * n + max(r, c) for r in range(n) for c in range(n) if r != c]
        off += n * n
    rows = torch.tensor(rows)
    for l in range(cfg.model.n_layers):
        model.max_blocks = l + 1
        call(model, t('xh'), nm, em, t('edge_x'), t('cond_x'), t('cond_edge_x'), t('noise_level'))
        h, e = model.debug_state()
        fwd_close(h, torch.from_numpy(fx['h'][l]), 'h after block %d' % l)
        fwd_close(e.cpu()[rows], torch.from_numpy(fx['e'][l]), 'e after block %d' % l)


# ---- 2. + 3. small shapes against the float64 oracle, and against the directed walk ----------------------------------------------------
@pytest.mark.parametrize('shared', [True, False], ids=['shared-level', 'per-molecule-levels'])
@pytest.mark.parametrize('cond', [False, True], ids=['first-step', 'conditioned'])
@pytest.mark.parametrize('n_nodes', [EDGE_SIZES, GAP_SIZES], ids=['edge-sizes', 'gaps-and-straddle'])
def test_small_shapes_against_float64_oracle_and_directed(zinc, n_nodes, cond, shared):
    cfg, model = zinc
    xh, ex, cx, cex, nl, nm, em = sym_inputs(cfg, n_nodes, 31, shared_level=0.4 if shared else None, cond=cond)
    B, N = len(n_nodes), max(n_nodes)
    emd = em.reshape(B, N, N, 1)
    if cond:                                             # the adjacency head sees both sides of the threshold
        live = cex[..., 0][em.reshape(B, N, N) > 0]
        assert bool((live >= model.edge_th).any()) and bool((live < model.edge_th).any())
    got = call(model, d(xh), d(nm), d(em), d(ex), d(cx), d(cex), d(nl))
    assert model.last_flags.tolist()[:3] == [1, 1 if shared else 0, 1]
    om = O2.OracleModel2D(state_dict_cpu(model), O2.Hyper2D.from_config(cfg), dtype=torch.float64)
    f64 = lambda v: None if v is None else v.double()
    want = om(None, xh.double(), nm, em, edge_x=ex.double(), cond_x=f64(cx), cond_edge_x=f64(cex), noise_level=nl.double())
    fwd_close(got[0], want[0], 'pair walk x')
    fwd_close(got[1], want[1], 'pair walk e')
    ref = call(model, d(xh), d(nm), d(em), d(ex), d(cx), d(cex), d(nl), pair=False)
    fwd_close(got[0], ref[0], 'pair against directed x', factor=2.0)
    fwd_close(got[1], ref[1], 'pair against directed e', factor=2.0)
    assert torch.equal(got[1], got[1].transpose(1, 2))
    assert float((got[0].cpu() * (1 - nm)).abs().max()) == 0.0 and float((got[1].cpu() * (1 - emd)).abs().max()) == 0.0


# ---- 4. more groups than the persistent grid has workgroups ----------------------------------------------------------------------------
def test_many_groups_against_directed(zinc):
    cfg, model = zinc
    torch.manual_seed(5)
    n_nodes = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), cfg.data.info_name)).sample(2000).tolist()
    xh, ex, _, _, nl, nm, em = sym_inputs(cfg, n_nodes, 17, shared_level=0.7)
    dx, dnm, dem, dex, dnl = d(xh), d(nm), d(em), d(ex), d(nl)
    p1 = call(model, dx, dnm, dem, dex, None, None, dnl)
    assert model._last_plan['pair_groups'] > 256
    p2 = call(model, dx, dnm, dem, dex, p1[0], p1[1], dnl)
    r2 = call(model, dx, dnm, dem, dex, p1[0], p1[1], dnl, pair=False)
    fwd_close(p2[0], r2[0], 'B = 2000 pair against directed x', factor=2.0)
    fwd_close(p2[1], r2[1], 'B = 2000 pair against directed e', factor=2.0)
    assert torch.equal(p2[1], p2[1].transpose(1, 2))
    assert float((p2[0] * (1 - dnm)).abs().max()) == 0.0
    assert float((p2[1] * (1 - dem.reshape(p2[1].shape[0], p2[1].shape[1], p2[1].shape[1], 1))).abs().max()) == 0.0


# ---- 5. determinism and batch independence, bit for bit --------------------------------------------------------------------------------
def test_bitwise_determinism_and_batch_independence(zinc):
    cfg, model = zinc
    n_nodes = [38, 9, 64, 2, 33, 20, 5]
    xh, ex, cx, cex, nl, nm, em = sym_inputs(cfg, n_nodes, 3, shared_level=-0.3, cond=True)
    a = call(model, d(xh), d(nm), d(em), d(ex), d(cx), d(cex), d(nl))
    b = call(model, d(xh), d(nm), d(em), d(ex), d(cx), d(cex), d(nl))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    def subset(idx):
        """the molecules idx as a batch of their own (padded to their own width)"""
        ns = [n_nodes[i] for i in idx]
        N = max(ns)
        s = torch.tensor(idx)
        nm_, em_ = masks(ns)
        o = call(model, d(xh[s][:, :N]), d(nm_), d(em_), d(ex[s][:, :N, :N]), d(cx[s][:, :N]), d(cex[s][:, :N, :N]), d(nl[s]))
        return {i: (o[0][k, :n_nodes[i]], o[1][k, :n_nodes[i], :n_nodes[i]]) for k, i in enumerate(idx)}

    want = {i: (a[0][i, :n], a[1][i, :n, :n]) for i, n in enumerate(n_nodes)}
    for idx in ([0], [2], [3], [4], [5, 3, 0, 6, 2, 1, 4], [4, 6, 0], [2, 2, 4, 4, 3]):        # alone, shuffled, other company
        for i, (ox, oe) in subset(idx).items():
            assert torch.equal(ox, want[i][0]) and torch.equal(oe, want[i][1]), (idx, i)


# ---- 6. fallback ------------------------------------------------------------------------------------------------------------------------
def test_fallback_to_the_directed_walk(zinc):
    cfg, model = zinc
    n_nodes = [9, 27, 1, 2, 16]
    xh, ex, _, _, nl, nm, em = sym_inputs(cfg, n_nodes, 4)
    B, N = len(n_nodes), max(n_nodes)
    g = torch.Generator().manual_seed(12)
    asym = torch.randn(B, N, N, cfg.model.edge_ch, generator=g) * em.reshape(B, N, N, 1)
    a = call(model, d(xh), d(nm), d(em), d(asym), None, None, d(nl), walked=0)
    assert model.last_flags[0].item() == 0
    r = call(model, d(xh), d(nm), d(em), d(asym), None, None, d(nl), pair=False)
    assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1])
    model.force_directed = True
    a = call(model, d(xh), d(nm), d(em), d(ex), None, None, d(nl), walked=0)
    r = call(model, d(xh), d(nm), d(em), d(ex), None, None, d(nl), pair=False)
    model.force_directed = False
    assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1])
    # and back: the record follows the walk
    call(model, d(xh), d(nm), d(em), d(ex), None, None, d(nl))
    call(model, d(xh), d(nm), d(em), d(ex), None, None, d(nl), pair=False)
    assert model.last_flags[2].item() == 0


# ---- 7. callers -------------------------------------------------------------------------------------------------------------------------
def test_trajectory_free_running_and_teacher_forced():
    fx = load_fixture('traj2d_zinc_anc5.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    model.pair_attention = True
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    steps = int(fx['steps'])
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    replay = lambda i, kind, like: torch.from_numpy(fx['node_noise' if kind == 'node' else 'edge_noise'][i]).to(like.device)
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond, noise_fn=replay)
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    assert model.last_flags[2].item() == 1
    ex_, ee_ = (x_mean.cpu() - torch.from_numpy(fx['x_mean'])).abs().max().item(), (e_mean.cpu() - torch.from_numpy(fx['edge_x_mean'])).abs().max().item()
    print('free-running end state: max |err|', ex_, ee_)
    assert ex_ <= 1e-3 and ee_ <= 1e-3
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_mean.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_mean.clone(), em,
                                        cfg.data.compress_edge)
    bad, excluded = O2.decode_agrees(fx, one_hot.argmax(2).cpu().numpy(), fc.cpu().numpy(), et.cpu().numpy(), n_nodes)
    assert bad == 0 and excluded <= float(fx['margin_cap'])
    t = lambda k, i: torch.from_numpy(fx[k][i]).to(DEV)
    for i in range(steps):
        cx, cex = (None, None) if i == 0 else (t('step_pred_x', i - 1), t('step_pred_e', i - 1))
        got = call(model, t('step_x', i), nm, em, t('step_edge_x', i), cx, cex, t('step_noise_level', i))
        fwd_close(got[0], torch.from_numpy(fx['step_pred_x'][i]), 'teacher-forced step %d x' % i)
        fwd_close(got[1], torch.from_numpy(fx['step_pred_e'][i]), 'teacher-forced step %d e' % i)


def test_graph_replay_equals_the_eager_device_noise_round():
    steps, key, n_nodes = 5, (13, 2, 4), [1, 5, 9, 33, 2]
    cfg = make_config(CFG['zinc'])
    model = make_model(cfg, 7, DEV, head_gain=8.0)
    model.pair_attention = True
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    g = torch.Generator().manual_seed(21)
    z = d(mutils.sample_gaussian_with_mask((B, N, nd), 'cpu', nm, generator=g))
    ez = d(mutils.sample_symmetric_edge_feature_noise(B, N, ch, em, generator=g).contiguous())
    nm, em = d(nm), d(em)
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond)
    try:
        sampler.device_noise = fused.DeviceNoise.for_rank(*key)
        with torch.no_grad():
            want = [v.clone() for v in sampler.sampling(model, z, nm, em, ez, None)]
        assert model.last_flags[2].item() == 1
        sampler.device_noise = fused.DeviceNoise.for_rank(*key)
        with torch.no_grad():
            rnd = GraphedAncestralRound2D(sampler, model, nm, em)
            got = rnd.run(z, ez)
        torch.cuda.synchronize()
    finally:
        sampler.device_noise = None
    assert rnd.graph is not None and model.last_flags[2].item() == 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_runs_under_single_device_dataparallel():
    cfg = make_config(CFG['moses'])
    cfg.device = torch.device(DEV)
    model = mutils.create_model(cfg, wrap='dataparallel')
    inner = model.module
    inner.pair_attention = True
    n_nodes = [5, 9, 2]
    xh, ex, _, _, nl, nm, em = sym_inputs(cfg, n_nodes, 8)
    nmd, emd = d(nm), d(em)
    with torch.no_grad():
        a = model(d(nl), d(xh), nmd, emd, edge_x=d(ex), cond_x=None, cond_edge_x=None, noise_level=d(nl))
        b = model(d(nl), d(xh), nmd, emd, edge_x=d(ex), cond_x=a[0], cond_edge_x=a[1], noise_level=d(nl))
    assert len(inner._plans) == 1 and inner.last_flags[2].item() == 1
    om = O2.OracleModel2D(state_dict_cpu(inner), O2.Hyper2D.from_config(cfg))
    want = om(None, xh, nm, em, edge_x=ex, cond_x=a[0].cpu(), cond_edge_x=a[1].cpu(), noise_level=nl)
    fwd_close(b[0], want[0], 'DataParallel x')
    fwd_close(b[1], want[1], 'DataParallel e')


# ---- 8. weights follow updates ----------------------------------------------------------------------------------------------------------
def test_weight_updates_reach_the_pair_kernel():
    cfg = make_config(CFG['zinc'])
    model = make_model(cfg, 7, DEV)
    n_nodes = [7, 12, 3]
    xh, ex, _, _, nl, nm, em = sym_inputs(cfg, n_nodes, 6)
    nmd, emd = d(nm), d(em)
    hp = O2.Hyper2D.from_config(cfg)

    def check(tag, masks_=None):
        m_ = masks_ or (nmd, emd)
        got = call(model, d(xh), m_[0], m_[1], d(ex), None, None, d(nl))
        want = O2.OracleModel2D(state_dict_cpu(model), hp)(None, xh, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)
        fwd_close(got[0], want[0], tag + ' x')
        fwd_close(got[1], want[1], tag + ' e')
        return got

    # Sizes of the changes, from the dense oracle on the CPU: lin_edge1 x 3 in all blocks moves the node output by 1.3e-3,
    # lin_edge0 x 4 on top of it by 2.5e-4; the forward bound at these outputs (|x| <= 0.15) is 3.5e-5, so a kernel that kept the old
    # weights fails the oracle comparison, and the thresholds below sit between that bound and the oracle's change.
    blocks = [getattr(model, 'e_block_%d' % l).attn_mpnn for l in range(cfg.model.n_layers)]
    base = check('initial weights')
    with torch.no_grad():
        for a in blocks:
            a.lin_edge1.weight.data.mul_(3.0)
    model.invalidate_packed_weights()
    upd = check('after .data.mul_ + invalidate_packed_weights')
    assert float((upd[0] - base[0]).abs().max()) > 3e-4
    with torch.no_grad():
        for a in blocks:
            a.lin_edge0.weight.data.mul_(4.0)
    upd2 = check('after .data.mul_ seen by a new batch', masks([7, 12, 3], DEV))
    assert float((upd2[0] - upd[0]).abs().max()) > 1e-4
    fresh = make_model(cfg, 19)
    model.load_state_dict(fresh.state_dict())
    upd3 = check('after load_state_dict')
    assert float((upd3[0] - upd2[0]).abs().max()) > 1e-3

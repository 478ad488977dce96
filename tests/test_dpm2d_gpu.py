"""GPU: DPM-Solver++ for the 2-D models — the update kernel jodo_dpm_update_2d against the float32 framework expression on the device,
the fused solver against the op-by-op solver, the reference-derived trajectories tests/golden/traj2d_*_dpm_*.npz with the HIP model
(free-running and teacher-forced), graph replay (GraphedDPMRound2D) against the eager solver, and the public sampling function with
sampling.method = 'dpm_2d'.

Bounds: the kernel rounds every product and sum on its own, in the order of the framework expression a * base - b * P - c * (c2 * (DA - DB)),
so it is compared with that expression bit for bit (torch.equal; the project's bound for the 3-D fused update, 2e-6 absolute in
tests/test_dgt_gpu.py, is implied).  Fused against op-by-op solver: 2e-6 absolute, as the 3-D test.  Trajectories: end state within 1e-3,
decodes equal outside the recorded margins, every recorded evaluation within the forward bound atol 2e-5 + rtol 1e-4 (what the
traj2d_*_anc5 test asks)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from jodo_amd import capi, fused
from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.graphed import GraphedDPMRound2D
from jodo_amd.mix_dpm_solver import DPM_Solver_2D
from jodo_amd.models import get_node_dist
from jodo_amd.models import utils as mutils
from jodo_amd.utils import get_data_inverse_scaler
from helpers import load_fixture, make_config, make_model, masks, GOLDEN
import oracle2d as O2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL, RTOL = 2e-5, 1e-4
CFG = {'zinc': 'vpsde_zinc_2d_jodo', 'moses': 'vpsde_moses_2d_jodo'}
FIXTURES = ['traj2d_zinc_dpm_single2.npz', 'traj2d_zinc_dpm_single3.npz', 'traj2d_zinc_dpm_single1.npz', 'traj2d_zinc_dpm_multi2.npz',
            'traj2d_moses_dpm_single2.npz']
VARIANTS = [('singlestep_fixed', 2, 6), ('singlestep_fixed', 3, 6), ('singlestep_fixed', 1, 3), ('multistep', 2, 5)]
d = lambda v: v.to(DEV)


def fwd_close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = ATOL + RTOL * want.abs()
    print('%s: max |err| %.3e, worst err / bound %.3f' % (what, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all()), "%s: max |err| %g, worst err / bound %g" % (what, err.max().item(), (err / bound).max().item())


def dpm_config(cfg_name, steps, method=None, order=None):
    cfg = make_config(cfg_name)
    cfg.sampling.method, cfg.sampling.steps = 'dpm_2d', int(steps)
    if method is not None:
        cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = str(method), int(order)
    return cfg


def schedule(cfg):
    return NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def update_2d(n_nodes, coef, base, P, DA, DB, table=None, out=None):
    """jodo_dpm_update_2d through the C ABI.  coef = (a, b, c, c2); table = (step, stride, col): the table form with the coefficients in
    row `step` of a device table whose other entries are NaN; out = (x_out, edge_out) or fresh NaN-filled tensors."""
    B, N, nd = base[0].shape
    ch = base[1].shape[-1]
    nn = d(torch.tensor(n_nodes, dtype=torch.int32))
    xo, eo = out if out is not None else (torch.full_like(base[0], float('nan')), torch.full_like(base[1], float('nan')))
    c8, tab, step, stride, col = (ctypes.c_float * 8)(*coef, 0.0, 0.0, 0.0, 0.0), None, None, 0, 0
    if table is not None:
        row, stride, col = table
        host = torch.full((row + 2, stride), float('nan'))
        host[row, col:col + 4] = torch.tensor(coef)
        tab, step, c8 = d(host), d(torch.tensor([row], dtype=torch.int32)), None
    capi.check(capi.lib().jodo_dpm_update_2d(B, N, nd, ch, capi.ptr(nn), c8, capi.ptr(tab), capi.ptr(step), stride, col,
                                             *[capi.ptr(t) for pair in (base, P, DA, DB) for t in pair], capi.ptr(xo), capi.ptr(eo),
                                             capi.current_stream_ptr()), 'jodo_dpm_update_2d')
    torch.cuda.synchronize()
    return xo, eo


def kernel_inputs(n_nodes, nd, ch, seed):
    """Four (node, edge) pairs of magnitude at most 4, non-zero on padding and on the diagonal; every edge tensor is symmetric except that
    its strict upper triangle sits one ulp above the mirrored lower one — an output that depends on the upper triangle shows."""
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), max(n_nodes)
    up = torch.triu(torch.ones(N, N, dtype=torch.bool), 1).reshape(1, N, N, 1)
    pairs = []
    for _ in range(4):
        x = torch.rand(B, N, nd, generator=g) * 7.9 - 3.95
        e = torch.rand(B, N, N, ch, generator=g) * 7.9 - 3.95
        low = torch.tril(e.permute(0, 3, 1, 2), 0)
        sym = (low + torch.tril(e.permute(0, 3, 1, 2), -1).transpose(-1, -2)).permute(0, 2, 3, 1).contiguous()
        e = torch.where(up, torch.nextafter(sym, torch.full_like(sym, 8.0)), sym)
        assert float(x.abs().max()) <= 4 and float(e.abs().max()) <= 4 and float(e.abs().min()) > 0 and float(x.abs().min()) > 0
        pairs.append((d(x), d(e.contiguous())))
    return pairs


PATTERNS = {'c = 0': (0.83, -0.41, 0.0, 1.0), 'c > 0': (0.61, -0.72, 0.37, 1.0), 'c < 0': (0.55, -0.8, -1.9, 1.0),
            'c2 != 1': (0.7, -0.52, -0.26, 1.0 / 0.83)}


@pytest.mark.parametrize('which,n_nodes', [('zinc', [9, 1, 38, 17, 2]), ('moses', [27, 3, 1, 14])])
def test_update_kernel_equals_the_framework_expression(which, n_nodes):
    cfg = make_config(CFG[which])
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes, DEV)
    emd = em.reshape(B, N, N, 1)
    base, P, DA, DB = kernel_inputs(n_nodes, nd, ch, 11)
    for name, coef in PATTERNS.items():
        a, b, c, c2 = (torch.tensor(v, dtype=torch.float32) for v in coef)
        coef = tuple(float(v) for v in (a, b, c, c2))                      # the float32 values, as the solver hands them over
        ref = [a * base[k] - b * P[k] - c * (c2 * (DA[k] - DB[k])) for k in range(2)]      # float32, one rounding per operation
        low = torch.tril(ref[1].permute(0, 3, 1, 2), -1)
        want_x, want_e = ref[0] * nm, (low + low.transpose(-1, -2)).permute(0, 2, 3, 1) * emd      # cell (b, r, c), r > c, both ways
        xo, eo = update_2d(n_nodes, coef, base, P, DA, DB)
        ex, ee = (xo - want_x).abs().max().item(), (eo - want_e).abs().max().item()
        print(which, name, 'max |err| nodes %.3e edges %.3e' % (ex, ee))
        assert ex <= 2e-6 and ee <= 2e-6                                   # nan-prefilled outputs: every element was written
        assert torch.equal(xo, want_x) and torch.equal(eo, want_e)
        assert torch.equal(eo, eo.transpose(1, 2))
        assert float((xo * (1 - nm)).abs().max()) == 0.0 and float((eo * (1 - emd)).abs().max()) == 0.0      # padding, diagonal
        assert float(xo[nm.expand_as(xo) > 0].abs().min()) > 0.0 and float(eo[emd.expand_as(eo) > 0].abs().min()) > 0.0
        # the one-ulp offset of the upper triangle reaches the framework expression there, not the kernel's output
        upper = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1).reshape(1, N, N, 1) & (emd > 0)
        assert not torch.equal(ref[1][upper.expand_as(eo)], eo[upper.expand_as(eo)])
        # table form with a device step counter, row 3 / stride 16 / column 8: the same bits
        xt, et = update_2d(n_nodes, coef, base, P, DA, DB, table=(3, 16, 8))
        assert torch.equal(xt, xo) and torch.equal(et, eo)
        # in place: the outputs are the update's own base
        xb, eb = base[0].clone(), base[1].clone()
        xi, ei = update_2d(n_nodes, coef, (xb, eb), P, DA, DB, out=(xb, eb))
        assert xi.data_ptr() == xb.data_ptr() and torch.equal(xi, xo) and torch.equal(ei, eo)


def test_update_entry_rejects_bad_arguments():
    base, P, DA, DB = kernel_inputs([2, 3], 4, 2, 1)
    L, nn, st = capi.lib(), d(torch.tensor([2, 3], dtype=torch.int32)), capi.current_stream_ptr()
    tens = [capi.ptr(t) for pair in (base, P, DA, DB) for t in pair] + [capi.ptr(base[0].clone()), capi.ptr(base[1].clone())]
    c8 = (ctypes.c_float * 8)(1, 1, 0, 1, 0, 0, 0, 0)
    tab, step = d(torch.zeros(2, 8)), d(torch.zeros(1, dtype=torch.int32))
    assert L.jodo_dpm_update_2d(2, 3, 4, 2, capi.ptr(nn), None, None, None, 0, 0, *tens, st) != 0            # neither form
    assert L.jodo_dpm_update_2d(2, 3, 4, 2, capi.ptr(nn), c8, capi.ptr(tab), capi.ptr(step), 8, 0, *tens, st) != 0      # both forms
    assert L.jodo_dpm_update_2d(2, 3, 4, 2, capi.ptr(nn), None, capi.ptr(tab), None, 8, 0, *tens, st) != 0   # table without a counter
    assert L.jodo_dpm_update_2d(2, 3, 4, 2, capi.ptr(nn), None, capi.ptr(tab), capi.ptr(step), 8, 4, *tens, st) != 0    # columns past the row
    assert L.jodo_dpm_update_2d(2, 0, 4, 2, capi.ptr(nn), c8, None, None, 0, 0, *tens, st) != 0
    assert L.jodo_dpm_update_2d(2, 3, 4, 2, None, c8, None, None, 0, 0, *tens, st) != 0
    with pytest.raises(ValueError):
        fused.dpm_update_2d(object(), [1, 1, 0, 1, 0, 0, 0, 0], base[0], base[1][:, :2], P, DA, DB, nn)
    with pytest.raises(TypeError):
        cpu = lambda pair: (pair[0].cpu(), pair[1].cpu())
        fused.dpm_update_2d(type('S', (), {})(), [1, 1, 0, 1, 0, 0, 0, 0], base[0].cpu(), base[1].cpu(), cpu(P), cpu(DA), cpu(DB), nn.cpu())
    torch.cuda.synchronize()


# ---- the solver --------------------------------------------------------------------------------------------------------------------
class Fake(torch.nn.Module):
    """Deterministic stand-in for the score network (that of test_fused_dpm_update_equals_framework_update without the position lines)."""

    def forward(self, t, x, node_mask, edge_mask, edge_x=None, noise_level=None, cond_x=None, cond_edge_x=None, context=None):
        e = torch.tanh(edge_x * 0.7 + 0.1 * noise_level.reshape(-1, 1, 1, 1))
        out = torch.tanh(x * 0.5 + 0.2) * node_mask
        if cond_x is not None:
            out = out + 0.1 * cond_x
        return out, (e + e.transpose(1, 2)) * edge_mask.reshape(edge_x.shape[0], edge_x.shape[1], edge_x.shape[2], 1)


@pytest.mark.parametrize('method,order,nfe', VARIANTS)
def test_fused_solver_equals_the_op_by_op_solver(method, order, nfe):
    cfg = dpm_config(CFG['zinc'], nfe, method, order)
    n_nodes = [9, 1, 29, 17, 2]
    nm, em = masks(n_nodes, DEV)
    B, N = len(n_nodes), max(n_nodes)
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    g = torch.Generator().manual_seed(321)
    nm_c, em_c = masks(n_nodes)
    z = d(mutils.sample_gaussian_with_mask((B, N, nd), 'cpu', nm_c, generator=g))
    ez = d(mutils.sample_symmetric_edge_feature_noise(B, N, ch, em_c, generator=g).contiguous())
    outs = []
    for fused_on in (False, True):
        solver = DPM_Solver_2D(schedule(cfg), cfg, fused=fused_on)
        outs.append(solver.sampling(Fake(), z, nm, em, ez, None))
    for a, b in zip(*outs):
        err = (a - b).abs().max().item()
        print(method, order, 'fused vs op-by-op: max |err| %.3e' % err)
        assert err < 2e-6
    assert float((outs[1][0] * (1 - nm)).abs().max()) == 0.0 and torch.equal(outs[1][1], outs[1][1].transpose(1, 2))
    assert outs[1][0].data_ptr() not in {t.data_ptr() for t in solver._dpm_bufs.x}            # clones, not the ring's buffers


def _fixture_setup(fname):
    fx = load_fixture(fname)
    cfg = dpm_config(str(fx['cfg_name']), fx['steps'], fx['dpm_solver_method'], fx['dpm_solver_order'])
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    n_nodes = fx['n_nodes'].tolist()
    return fx, cfg, model, n_nodes, masks(n_nodes, DEV)


@pytest.mark.parametrize('fname', FIXTURES)
def test_reference_trajectory_free_running(fname):
    fx, cfg, model, n_nodes, (nm, em) = _fixture_setup(fname)
    solver = DPM_Solver_2D(schedule(cfg), cfg)
    x_end, e_end = solver.sampling(model, d(torch.from_numpy(fx['z'])), nm, em, d(torch.from_numpy(fx['edge_z'])), None)
    ex_, ee_ = (x_end.cpu() - torch.from_numpy(fx['x_end'])).abs().max().item(), (e_end.cpu() - torch.from_numpy(fx['edge_x_end'])).abs().max().item()
    print(fname, 'free-running end state: max |err|', ex_, ee_)
    assert ex_ <= 1e-3 and ee_ <= 1e-3
    assert torch.equal(e_end, e_end.transpose(1, 2))
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_end.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_end.clone(), em,
                                        cfg.data.compress_edge)
    bad, excluded = O2.decode_agrees(fx, one_hot.argmax(2).cpu().numpy(), fc.cpu().numpy(), et.cpu().numpy(), n_nodes)
    print(fname, 'decodes: mismatches', bad, 'excluded share', excluded)
    assert bad == 0
    assert excluded <= float(fx['margin_cap']) and float(fx['margin_shares'].max()) <= float(fx['margin_cap']) == 0.05
    # the device decode of the same end state: the same decisions
    at, q, bt = fused.decode_2d(cfg, x_end, e_end, fused.n_nodes_from_mask(nm))
    assert torch.equal(at.cpu().long(), one_hot.argmax(2).cpu() * nm[..., 0].cpu().long()) and torch.equal(bt.cpu().float(), et.cpu())


@pytest.mark.parametrize('fname', FIXTURES)
def test_reference_trajectory_teacher_forced(fname):
    fx, cfg, model, n_nodes, (nm, em) = _fixture_setup(fname)
    t = lambda k, i: torch.from_numpy(fx[k][i]).to(DEV)
    for i in range(int(fx['steps'])):
        cx, cex = (None, None) if i == 0 else (t('step_pred_x', i - 1), t('step_pred_e', i - 1))
        nl = t('step_noise_level', i)
        with torch.no_grad():
            got = model(nl, t('step_x', i), nm, em, edge_x=t('step_edge_x', i), cond_x=cx, cond_edge_x=cex, noise_level=nl)
        fwd_close(got[0], torch.from_numpy(fx['step_pred_x'][i]), '%s teacher-forced evaluation %d x' % (fname, i))
        fwd_close(got[1], torch.from_numpy(fx['step_pred_e'][i]), '%s teacher-forced evaluation %d e' % (fname, i))


# ---- graph replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,end_step', [('singlestep_fixed', 5), ('multistep', 10)])
def test_graph_replay_equals_the_eager_solver(method, end_step):
    cfg = dpm_config(CFG['zinc'], 10, method, 2)
    model = make_model(cfg, 7, DEV, head_gain=8.0)
    n_nodes = [1, 5, 9, 33, 2]
    B, N = len(n_nodes), max(n_nodes)
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    nm_c, em_c = masks(n_nodes)
    g = torch.Generator().manual_seed(21)
    z = d(mutils.sample_gaussian_with_mask((B, N, nd), 'cpu', nm_c, generator=g))
    ez = d(mutils.sample_symmetric_edge_feature_noise(B, N, ch, em_c, generator=g).contiguous())
    nm, em = d(nm_c), d(em_c)
    solver = DPM_Solver_2D(schedule(cfg), cfg)
    want_x, want_e = solver.sampling(model, z, nm, em, ez, None)
    rnd = GraphedDPMRound2D(solver, model, nm, em)
    got_x, got_e = rnd.run(z, ez)
    torch.cuda.synchronize()
    assert rnd.graph is not None and int(rnd.step.item()) == end_step == rnd.K
    print(method, 'graph vs eager: max |diff|', (got_x - want_x).abs().max().item(), (got_e - want_e).abs().max().item())
    assert torch.equal(got_x, want_x) and torch.equal(got_e, want_e)
    assert bool(torch.isfinite(got_x).all() and torch.isfinite(got_e).all()) and float(got_x.abs().max()) > 0
    for bad in (('singlestep_fixed', 1), ('singlestep_fixed', 3)):
        with pytest.raises(NotImplementedError):
            GraphedDPMRound2D(DPM_Solver_2D(schedule(cfg), dpm_config(CFG['zinc'], 6, *bad)), model, nm, em)


# ---- the public entry --------------------------------------------------------------------------------------------------------------
class _FixedNodes:
    """nodes_dist stand-in: returns preset atom counts (consumes no random numbers)."""

    def __init__(self, rounds):
        self.rounds, self.calls = rounds, 0

    def sample(self, n):
        out = torch.tensor(self.rounds[self.calls])
        self.calls += 1
        assert len(out) == n
        return out


def _same_mols(a, b):
    return len(a) == len(b) and all(m[0] is None and w[0] is None and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(m[1:], w[1:]))
                                    for m, w in zip(a, b))


def _entry_setup(steps=6):
    cfg = dpm_config(CFG['zinc'], steps)
    cfg.device = torch.device(DEV)
    model = mutils.create_model(cfg, wrap='dataparallel_keys')            # the wrapper create_model gives by default
    from jodo_amd.models import deterministic_init_
    deterministic_init_(model.module, seed=42)
    with torch.no_grad():
        sd = model.module.state_dict()
        for k in ('node_pred_mlp.4.weight', 'edge_type_mlp.4.weight', 'edge_exist_mlp.4.weight'):
            sd[k].mul_(8.0)
    model.module.invalidate_packed_weights()
    dist = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k'))
    return cfg, model, schedule(cfg), dist, get_data_inverse_scaler(cfg)


def test_public_entry_dpm_2d_on_gpu():
    cfg, model, ns, dist, inv = _entry_setup()
    runs = []
    for _ in range(2):
        fn = S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, hip_graph=True, seed=8, return_raw=True)
        torch.manual_seed(8)                                 # atom counts and the initial z / edge_z are torch draws
        runs.append(fn(model))
    assert len(runs[0]) == 5 and _same_mols(runs[0], runs[1])
    assert len({int(m[1].shape[0]) for m in runs[0]}) > 1
    # eager, whatever the noise option says: the same molecules (nothing is drawn after the initial state)
    for kw in (dict(), dict(device_noise=True), dict(device_noise=False)):
        fn = S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, seed=8, return_raw=True, **kw)
        torch.manual_seed(8)
        assert _same_mols(fn(model), runs[0])
    # hip_graph goes with every noise option; what the graph does not cover says so when the function is built
    S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, hip_graph=True, device_noise=False)
    S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, hip_graph=True, cpu_noise=True)
    cfg3 = dpm_config(CFG['zinc'], 6, 'singlestep_fixed', 3)
    cfg3.device = cfg.device
    with pytest.raises(NotImplementedError, match='order 2'):
        S.get_sampling_fn(cfg3, ns, dist, 5, 5, inv, hip_graph=True)
    # the pair-symmetric attention walk (opt-in on the model) under the solver, eager and replayed
    inner = model.module
    inner.pair_attention = True
    try:
        for hip_graph in (False, True):
            fn = S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, hip_graph=hip_graph, seed=8, return_raw=True)
            torch.manual_seed(8)
            mols = fn(model)
            assert len(mols) == 5 and int(inner.last_flags[2].item()) == 1
            assert [int(m[1].shape[0]) for m in mols] == [int(m[1].shape[0]) for m in runs[0]]
    finally:
        inner.pair_attention = False


@pytest.mark.parametrize('hip_graph', [False, True])
def test_two_dpm_2d_rounds_through_one_sampling_fn(hip_graph):
    """get_sampling_fn builds ONE DPM_Solver_2D and reuses it for every round.  Two rounds with the same batch size and padded width but
    different atom counts: the second must equal the same round sampled through a fresh solver (same generator state) — nothing of
    round 1 (atom counts, ring buffers, self-conditioning state) may leak into it."""
    cfg, model, ns, _, inv = _entry_setup()
    r1, r2 = [27, 5, 9, 14, 3], [8, 27, 2, 20, 11]

    def run_rounds(lists, state=None):
        if state is not None:
            torch.set_rng_state(state[0]); torch.cuda.set_rng_state(state[1], DEV)
        fn = S.get_sampling_fn(cfg, ns, _FixedNodes([sum(lists, [])]), 5, 5 * len(lists), inv, return_raw=True, hip_graph=hip_graph)
        return fn(model)

    torch.manual_seed(31)
    both = run_rounds([r1, r2])
    torch.manual_seed(31)
    first = run_rounds([r1])
    state = (torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
    second = run_rounds([r2], state)
    assert len(both) == 10 and _same_mols(both, first + second)
    assert [int(m[1].shape[0]) for m in both] == r1 + r2
    assert not _same_mols(both[:5], both[5:])

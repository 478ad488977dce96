"""CPU: DPM-Solver++ for the 2-D models (mix_dpm_solver.DPM_Solver_2D, sampling.method 'dpm_2d') on the op-by-op path with the dense
oracle model (tests/oracle2d.OracleModel2D): the reference-derived trajectories tests/golden/traj2d_*_dpm_*.npz (the reference's own
DPM_Solver_hybrid run with three zero position columns, tools/make_golden_2d.dpm_fixture), the update formula restated in float64, the
public entry's method selection, and a sharded round in 'parity' mode over gloo with a rank whose share is empty.

Bounds: end state within 1e-3 and decodes equal outside the recorded margins (what the traj2d_*_anc5 host test asks); the float64
restatement within 8 * 2^-24 * (|a base| + |b P| + |c c2| (|DA| + |DB|)) per element — at most six float32 roundings, each of an
intermediate no larger than that sum."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.mix_dpm_solver import DPM_Solver_2D, DPM_Solver_hybrid
from jodo_amd.models import get_node_dist
from jodo_amd.utils import get_data_inverse_scaler
from helpers import load_fixture, make_config, make_model, state_dict_cpu, masks, GOLDEN
import oracle2d as O2

FIXTURES = ['traj2d_zinc_dpm_single2.npz', 'traj2d_zinc_dpm_single3.npz', 'traj2d_zinc_dpm_single1.npz', 'traj2d_zinc_dpm_multi2.npz',
            'traj2d_moses_dpm_single2.npz']
SEED = 77


def dpm_config(cfg_name, steps, method=None, order=None):
    cfg = make_config(cfg_name)
    cfg.sampling.method, cfg.sampling.steps = 'dpm_2d', int(steps)
    if method is not None:
        cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = str(method), int(order)
    return cfg


def schedule(cfg):
    return NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)


class Counting:
    """The model with a record of its calls (noise level and whether a self-conditioning input came with it)."""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, t, x, node_mask, edge_mask, **kw):
        self.calls.append((float(kw['noise_level'][0]), kw.get('cond_x') is not None))
        return self.model(t, x, node_mask, edge_mask, **kw)


@pytest.mark.parametrize('fname', FIXTURES)
def test_dpm_solver_2d_reproduces_reference_trajectory_on_cpu(fname):
    fx = load_fixture(fname)
    assert int(fx['torch_num_threads']) == 8
    cfg = dpm_config(str(fx['cfg_name']), fx['steps'], fx['dpm_solver_method'], fx['dpm_solver_order'])
    om = Counting(O2.OracleModel2D(state_dict_cpu(make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain']))), O2.Hyper2D.from_config(cfg)))
    n_nodes = fx['n_nodes'].tolist()
    assert 1 in n_nodes and 2 in n_nodes and cfg.data.max_node in n_nodes and 4 <= int(fx['steps']) <= 6
    nm, em = masks(n_nodes)
    solver = DPM_Solver_2D(schedule(cfg), cfg)
    z, ez = torch.from_numpy(fx['z']), torch.from_numpy(fx['edge_z'])
    x_end, e_end = solver.sampling(om, z, nm, em, ez, None)
    # NFE evaluations at the recorded noise levels, self-conditioned from the second on
    assert len(om.calls) == int(fx['steps']) == fx['step_noise_level'].shape[0]
    assert np.allclose([c[0] for c in om.calls], fx['step_noise_level'][:, 0], rtol=1e-6, atol=1e-6)
    assert [c[1] for c in om.calls] == [False] + [True] * (int(fx['steps']) - 1)
    ex, ee = (x_end - torch.from_numpy(fx['x_end'])).abs().max().item(), (e_end - torch.from_numpy(fx['edge_x_end'])).abs().max().item()
    print(fname, 'end state err', ex, ee)
    assert ex < 1e-3 and ee < 1e-3
    assert torch.equal(e_end, e_end.transpose(1, 2))
    B, N = len(n_nodes), max(n_nodes)
    assert float((x_end * (1 - nm)).abs().max()) == 0.0 and float((e_end * (1 - em.reshape(B, N, N, 1))).abs().max()) == 0.0
    assert x_end.data_ptr() != z.data_ptr() and torch.equal(z, torch.from_numpy(fx['z']))      # a result of its own, inputs untouched
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_end.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_end.clone(), em,
                                        cfg.data.compress_edge)
    bad, excluded = O2.decode_agrees(fx, one_hot.argmax(2).numpy(), fc.numpy(), et.numpy(), n_nodes)
    print(fname, 'decodes: mismatches', bad, 'excluded share', excluded)
    assert bad == 0 and excluded <= float(fx['margin_cap']) == 0.05
    assert float(fx['margin_shares'].max()) <= 0.05
    assert len(np.unique(fx['atom_type'][nm[..., 0].numpy() > 0])) >= 2 and len(np.unique(fx['edge_type'])) >= 2


def test_defaults_and_rejected_variants():
    cfg = dpm_config('vpsde_zinc_2d_jodo', 6)
    assert 'dpm_solver_method' not in cfg.sampling and 'dpm_solver_order' not in cfg.sampling      # the 2-D configs carry neither key
    sv = DPM_Solver_2D(schedule(cfg), cfg)
    assert isinstance(sv, DPM_Solver_hybrid) and (sv.method, sv.order, sv.steps) == ('singlestep_fixed', 2, 6)
    assert sv.noise_draws_per_round() == 0
    for method, order in (('singlestep_fixed', 4), ('multistep', 3), ('multistep', 1), ('adaptive', 2)):
        with pytest.raises(ValueError):
            DPM_Solver_2D(schedule(cfg), dpm_config('vpsde_zinc_2d_jodo', 6, method, order))
    cfg.model.self_cond = False
    with pytest.raises(AssertionError):
        DPM_Solver_2D(schedule(cfg), cfg)


# coefficient patterns of the solver's variants: (a, b, c, c2) with None where the variant leaves the term out
PATTERNS = {'first order': (0.83, -0.41, None, None), 'single-step second': (0.61, -0.72, -0.37, None),
            'single-step third': (0.55, -0.8, 1.9, None), 'multistep second': (0.7, -0.52, -0.26, 1.0 / 0.83)}


@pytest.mark.parametrize('name', sorted(PATTERNS))
def test_update_formula_restated_in_float64(name):
    a, b, c, c2 = (None if v is None else torch.tensor(v, dtype=torch.float32) for v in PATTERNS[name])
    g = torch.Generator().manual_seed(5)
    B, N, nd, ch = 3, 7, 10, 2
    r = lambda *s: torch.randn(*s, generator=g)
    base, P, DA, DB = ((r(B, N, nd), r(B, N, N, ch)) for _ in range(4))
    cfg = dpm_config('vpsde_zinc_2d_jodo', 4)
    sv = DPM_Solver_2D(schedule(cfg), cfg)
    nm, _ = masks([7, 3, 1])
    got = sv._update(None, base[0], base[1], P, DA, DB, None, nm, None, None, False, a, b, c, c2)
    d = lambda v: 0.0 if v is None else float(v)
    c2_ = 1.0 if c2 is None else float(c2)
    for k in range(2):
        want = d(a) * base[k].double() - d(b) * P[k].double() - d(c) * (c2_ * (DA[k].double() - DB[k].double()))
        bound = 8 * 2.0 ** -24 * (abs(d(a)) * base[k].abs() + abs(d(b)) * P[k].abs() + abs(d(c) * c2_) * (DA[k].abs() + DB[k].abs())).double()
        err = (got[k].double() - want).abs()
        print(name, 'nodes' if k == 0 else 'edges', 'max err', err.max().item(), 'worst err / bound', (err / bound).max().item())
        assert got[k].dtype == torch.float32 and bool((err <= bound).all())


def _setup(steps=4, batch=4):
    cfg = dpm_config('vpsde_zinc_2d_jodo', steps)
    cfg.device = 'cpu'
    model = O2.OracleModel2D(state_dict_cpu(make_model(cfg, 5, head_gain=30.0)), O2.Hyper2D.from_config(cfg))
    nodes_dist = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k'))
    return cfg, model, schedule(cfg), nodes_dist, get_data_inverse_scaler(cfg)


def _builder(cfg, ns, nodes_dist, inv, batch, samples, **kw):
    return S._get_sampling_fn_2d(cfg, ns, nodes_dist, batch, samples, inv, 1e-3, **kw)


def _same(a, b):
    eq = lambda x, y: (x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and torch.equal(x, y))
    return len(a) == len(b) and all(len(m) == len(w) and all(eq(x, y) for x, y in zip(m, w)) for m, w in zip(a, b))


def test_public_entry_selects_the_solver_by_method():
    cfg, model, ns, nodes_dist, inv = _setup()
    counted = Counting(model)
    counted.eval = lambda: counted
    fn = _builder(cfg, ns, nodes_dist, inv, 4, 4, return_raw=True)       # the private builder: the seam that takes a CPU model
    torch.manual_seed(SEED)
    mols = fn(counted)
    assert len(mols) == 4 and len(counted.calls) == 4                    # one round, 4 NFE
    assert all(m[0] is None and m[1].shape[0] == m[2].shape[0] == m[2].shape[1] for m in mols)
    assert fn.last_indices == [0, 1, 2, 3]
    # deterministic after the initial draw: the same seed gives the same molecules, and cpu_noise draws the same initial state
    torch.manual_seed(SEED)
    assert _same(_builder(cfg, ns, nodes_dist, inv, 4, 4, return_raw=True)(model), mols)
    torch.manual_seed(SEED)
    assert _same(_builder(cfg, ns, nodes_dist, inv, 4, 4, return_raw=True, cpu_noise=True, device_noise=False)(model), mols)
    # the ancestral sampler is another procedure: 4 steps of it make another 4 evaluations and draw per step
    cfg_a, _, _, _, _ = _setup()
    cfg_a.sampling.method = 'ancestral'
    torch.manual_seed(SEED)
    _builder(cfg_a, ns, nodes_dist, inv, 4, 4, return_raw=True)(model)
    after_ancestral = torch.rand(1)
    torch.manual_seed(SEED)
    fn(model)
    assert not torch.equal(torch.rand(1), after_ancestral)               # the solver drew less
    # the public entry builds it on a CPU config too, and still refuses what it refused
    S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv)
    S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv, device_noise=False)
    for kw in (dict(hip_graph=True), dict(device_noise=True), dict(shard=(0, 2))):
        with pytest.raises(NotImplementedError, match='needs a GPU device'):
            S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv, **kw)
    with pytest.raises(NotImplementedError, match='needs a GPU device'):
        _builder(cfg, ns, nodes_dist, inv, 4, 4, hip_graph=True)
    cfg.sampling.method = 'fast'
    with pytest.raises(NotImplementedError, match='fast'):
        S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv)
    with pytest.raises(NotImplementedError, match='dpm_2d'):             # the message points to the new name
        S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv)
    cfg.sampling.method = 'dpm'
    with pytest.raises(ValueError, match='Invalid sampling method'):
        S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv)
    cfg3 = make_config('vpsde_qm9_uncond_jodo')                          # a 3-D config does not know the 2-D name
    cfg3.device, cfg3.sampling.method = 'cpu', 'dpm_2d'
    with pytest.raises(ValueError, match='Invalid sampling method'):
        S.get_sampling_fn(cfg3, ns, nodes_dist, 4, 4, inv)


# ---- parity mode over gloo, world size 2 (the pattern of tests/test_sampling2d_host.py) --------------------------------------------
ROUNDS = ((5, 5), (1, 2))          # (batch, samples): one round dealt 3 + 2; two rounds of one molecule, rank 1's share empty in both


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _by_value(m):
    return tuple(None if t is None else t.numpy().copy() for t in m)


def _sample_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from jodo_amd.dist import gather_sampled
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    cfg, model, ns, nodes_dist, inv = _setup()
    out = []
    for batch, samples in ROUNDS:
        torch.manual_seed(1234 + rank)                   # whatever the process did before must not matter
        fn = _builder(cfg, ns, nodes_dist, inv, batch, samples, shard=(rank, world), shard_mode='parity', seed=SEED)
        mols = fn(model)
        full = gather_sampled(fn.last_decoded, fn.last_indices, with_pos=False)
        assert len(mols) == len(fn.last_indices) and all(r[0] is None for r in fn.last_decoded)
        out.append((fn.last_indices, [_by_value(m) for m in full]))
    q.put((rank, out))                                   # by value (no shared-memory handles)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_dpm_2d_parity_mode_reproduces_the_unsharded_run():
    threads = torch.get_num_threads()
    torch.set_num_threads(2)                  # as the workers: CPU GEMM blocking (hence low bits) depends on the thread count
    try:
        cfg, model, ns, nodes_dist, inv = _setup()
        want = []
        for batch, samples in ROUNDS:
            torch.manual_seed(SEED)
            want.append(_builder(cfg, ns, nodes_dist, inv, batch, samples, return_raw=True)(model))
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_sample_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)
        idx = [[res[r][1][k][0] for r in range(2)] for k in range(len(ROUNDS))]
        assert idx[0] == [[0, 1, 2], [3, 4]]
        assert idx[1] == [[0, 1], []]                                       # rank 1 held nothing and stayed in step
        for _, out in res:
            for k, (_, full) in enumerate(out):
                got = [tuple(None if a is None else torch.from_numpy(a) for a in m) for m in full]
                assert _same(got, want[k])
        assert len({int(m[1].shape[0]) for m in want[0]}) > 1               # not a degenerate batch
    finally:
        torch.set_num_threads(threads)

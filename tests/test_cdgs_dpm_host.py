"""CPU: the noise-prediction form of DPM_Solver_2D (sampling.method 'dpm_2d' on CDGS: pred_data = False, self_cond = False) on the
op-by-op path, with the dense oracle tests/oracle_cdgs.py as the network.

What pins it: (1) the new route ends in the very bits of the existing data-form class run on a wrapper that returns
(x - sigma_t eps) / alpha_t — and that class is pinned to the reference's solver trajectories (tests/test_dpm2d_host.py); (2) the record
of the network calls; (3) the fp32 round against the same round in float64 inside the forward bound 2e-5 + 1e-4 |x|; (4) an analytic
network whose probability-flow solution is known in closed form, for the orders of convergence; (5) refusals and defaults; (6) the
public entry on a CPU device, its CPU-noise replay and two parity shards over gloo."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.mix_dpm_solver import DPM_Solver_2D, DPM_Solver_hybrid
from jodo_amd.models import get_model_class, get_node_dist, load_dataset_info, deterministic_init_
from jodo_amd.utils import get_data_inverse_scaler
from helpers import make_config, masks
import oracle_cdgs as OC

CFG = 'vpsde_qm9_2d_cdgs'
N_NODES = [9, 1, 2, 5]
VARIANTS = {'single1': ('singlestep_fixed', 1, 5), 'single2': ('singlestep_fixed', 2, 6), 'single3': ('singlestep_fixed', 3, 6),
            'multi2': ('multistep', 2, 6)}
ATOL, RTOL = 2e-5, 1e-4
SEED = 77
_SD = {}


def dpm_config(cfg_name, steps, method=None, order=None):
    cfg = make_config(cfg_name)
    cfg.sampling.method, cfg.sampling.steps = 'dpm_2d', int(steps)
    if method is not None:
        cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = str(method), int(order)
    return cfg


def schedule(cfg):
    return NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)


def weights(dtype=torch.float32):
    """The seeded weights of the traj_cdgs_qm9_anc5 recipe (seed 21, head gain 1), built once."""
    if dtype not in _SD:
        if torch.float32 not in _SD:
            model = deterministic_init_(get_model_class('CDGS')(make_config(CFG)), seed=21)
            _SD[torch.float32] = {k: v.detach().float().clone() for k, v in model.state_dict().items()}
        _SD[dtype] = {k: v.to(dtype) for k, v in _SD[torch.float32].items()}
    return _SD[dtype]


class OracleCDGS:
    """The dense oracle with the score network's call signature and a record of its calls."""

    depends_on_padded_width = True            # as the HIP model declares it: parity shards keep the round's width

    def __init__(self, dtype=torch.float32):
        self.sd, self.hp, self.calls = weights(dtype), OC.hparams(make_config(CFG)), []

    def eval(self):
        return self

    def __call__(self, t, x, node_mask, edge_mask, context=None, **kw):
        self.calls.append(dict(t=t.clone(), kw={k: v for k, v in kw.items() if k != 'edge_x'}, context=context))
        with torch.no_grad():
            return OC.forward(self.sd, self.hp, t, x, node_mask, edge_mask, kw['edge_x'])


class AsDataPrediction:
    """A noise-predicting network presented as a data-predicting one: x0 = (x - sigma_t eps) / alpha_t with the schedule calls of the
    solver's own conversion.  The self-conditioning inputs that the data-form solver passes are ignored."""

    def __init__(self, net, ns):
        self.net, self.ns = net, ns

    def __call__(self, t, x, node_mask, edge_mask, context=None, **kw):
        eps_x, eps_e = self.net(t, x, node_mask, edge_mask, edge_x=kw['edge_x'])
        t0 = t[0]                                                     # the solver's scalar time (vec_t = ones * t)
        alpha_t, sigma_t = torch.exp(self.ns.marginal_log_mean_coeff(t0)), self.ns.marginal_std(t0)
        return (x - sigma_t * eps_x) / alpha_t, (kw['edge_x'] - sigma_t * eps_e) / alpha_t


def initial_state(cfg, n_nodes, seed, dtype=torch.float32, nd=None, ch=None):
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    nd = cfg.data.atom_types + int(cfg.model.include_fc_charge) if nd is None else nd
    ch = cfg.model.edge_ch if ch is None else ch
    z = torch.randn(B, N, nd, generator=g) * nm
    ez = torch.randn(B, N, N, ch, generator=g)
    ez = torch.tril(ez.permute(0, 3, 1, 2), -1).permute(0, 2, 3, 1)
    ez = (ez + ez.transpose(1, 2)) * em.reshape(B, N, N, 1)
    return z.to(dtype), ez.to(dtype), nm, em


def noise_round(name, dtype=torch.float32):
    method, order, steps = VARIANTS[name]
    cfg = dpm_config(CFG, steps, method, order)
    net = OracleCDGS(dtype)
    z, ez, nm, em = initial_state(cfg, N_NODES, 3, dtype)
    solver = DPM_Solver_2D(schedule(cfg), cfg)
    return solver, net, (z, ez, nm, em), solver.sampling(net, z, nm, em, ez, None)


# ---- 1. the very bits of the pinned data-form solver on the equivalent x0 network ------------------------------------------------------
@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_noise_form_equals_the_data_form_on_the_converted_network(name):
    method, order, steps = VARIANTS[name]
    solver, net, (z, ez, nm, em), (x_end, e_end) = noise_round(name)
    assert solver.noise_form
    cfg_d = dpm_config(CFG, steps, method, order)
    cfg_d.model.pred_data = cfg_d.model.self_cond = True
    ns = schedule(cfg_d)
    data_solver = DPM_Solver_2D(ns, cfg_d)
    assert not data_solver.noise_form
    inner = OracleCDGS()
    x_ref, e_ref = data_solver.sampling(AsDataPrediction(inner, ns), z, nm, em, ez, None)
    assert len(inner.calls) == len(net.calls) == steps
    print(name, 'max |x_end|', x_end.abs().max().item(), 'max |e_end|', e_end.abs().max().item())
    assert torch.equal(x_end, x_ref) and torch.equal(e_end, e_ref)
    assert bool(torch.isfinite(x_end).all()) and float(x_end.abs().max()) > 0
    assert torch.equal(e_end, e_end.transpose(1, 2))                  # the oracle's edge output is exactly symmetric
    B, N = len(N_NODES), max(N_NODES)
    assert float((x_end * (1 - nm)).abs().max()) == 0.0 and float((e_end * (1 - em.reshape(B, N, N, 1))).abs().max()) == 0.0


# ---- 2. the record of the network calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['single2', 'multi2'])
def test_call_record(name):
    method, order, steps = VARIANTS[name]
    solver, net, (z, ez, nm, em), (x_end, e_end) = noise_round(name)
    ns = solver.noise_schedule
    if method == 'multistep':
        grid = list(solver.get_time_steps('time_uniform', ns.T, 1. / ns.total_N, steps, 'cpu')[:-1])
    else:
        K, grid = steps // 2, []
        outer = solver.get_time_steps('time_uniform', ns.T, 1. / ns.total_N, K, 'cpu')
        for k in range(K):
            lam = ns.marginal_lambda(solver.get_time_steps('time_uniform', outer[k].item(), outer[k + 1].item(), 2, 'cpu'))
            grid += [outer[k], solver.second_order_coefficients(outer[k], outer[k + 1], (lam[1] - lam[0]) / (lam[-1] - lam[0]))['s1']]
    assert len(net.calls) == steps == len(grid)                       # exactly NFE evaluations
    for call, t in zip(net.calls, grid):
        assert call['t'].shape == (len(N_NODES),) and torch.equal(call['t'], torch.ones(len(N_NODES)) * t)
        assert call['kw'].get('cond_x') is None and call['kw'].get('cond_edge_x') is None
        assert torch.equal(call['kw']['noise_level'], torch.ones(len(N_NODES)) * ns.get_noiseLevel(t))
    assert solver.cond_x is None and solver.cond_edge_x is None      # nothing is carried between evaluations
    z0, ez0, _, _ = initial_state(dpm_config(CFG, steps), N_NODES, 3)
    assert torch.equal(z, z0) and torch.equal(ez, ez0)                # the inputs are untouched
    assert x_end.data_ptr() != z.data_ptr() and e_end.data_ptr() != ez.data_ptr()


# ---- 3. fp32 against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_fp32_round_against_float64(name):
    _, _, _, got = noise_round(name)
    _, _, _, want = noise_round(name, torch.float64)
    for g, w, what in zip(got, want, ('x', 'e')):
        assert g.dtype == torch.float32 and w.dtype == torch.float64
        err = (g.double() - w).abs()
        bound = ATOL + RTOL * w.abs()
        print('%s %s: max |err| %.3e at max |x| %.3e, worst err / bound %.4f' % (name, what, err.max().item(), w.abs().max().item(),
                                                                                   (err / bound).max().item()))
        assert bool((err <= bound).all())


# ---- 4. an analytic network: data N(0, s^2) ---------------------------------------------------------------------------------------------
S_DATA = 0.5
NFES = (6, 12, 24, 48)


class GaussianEps:
    """The exact noise prediction for data N(0, s^2): eps = sigma_t x / (alpha_t^2 s^2 + sigma_t^2)."""

    def __init__(self, ns):
        self.ns = ns

    def __call__(self, t, x, node_mask, edge_mask, context=None, **kw):
        t0 = t[0]
        alpha, sigma = torch.exp(self.ns.marginal_log_mean_coeff(t0)), self.ns.marginal_std(t0)
        k = sigma / (alpha ** 2 * S_DATA ** 2 + sigma ** 2)
        return k * x, k * kw['edge_x']


def analytic_error(method, order, steps):
    cfg = dpm_config('vpsde_zinc_2d_jodo', steps, method, order)
    cfg.model.pred_data = cfg.model.self_cond = False
    ns = schedule(cfg)
    z, ez, nm, em = initial_state(cfg, [5, 3, 1, 2], 11)
    assert z.shape[-1] == 10 and ez.shape[-1] == 2                    # ZINC-shaped tensors
    x_end, e_end = DPM_Solver_2D(ns, cfg).sampling(GaussianEps(ns), z, nm, em, ez, None)
    var = lambda t: (torch.exp(ns.marginal_log_mean_coeff(t)).double() ** 2 * S_DATA ** 2 + ns.marginal_std(t).double() ** 2)
    scale = torch.sqrt(var(torch.tensor(1. / ns.total_N)) / var(torch.tensor(float(ns.T))))
    num = ((x_end.double() - scale * z.double()).square().sum() + (e_end.double() - scale * ez.double()).square().sum()).sqrt()
    den = ((scale * z.double()).square().sum() + (scale * ez.double()).square().sum()).sqrt()
    return float(num / den)


def test_orders_of_convergence_on_the_gaussian_model():
    err = {name: [analytic_error(m, o, n) for n in NFES] for name, (m, o, _) in VARIANTS.items()}
    for name in sorted(err):
        print(name, ' '.join('%d: %.3e' % (n, e) for n, e in zip(NFES, err[name])))
    for name, row in err.items():
        assert all(a > b for a, b in zip(row, row[1:])), name         # the error falls strictly with the number of evaluations
    ratio = err['single1'][2] / err['single1'][3]
    print('order 1, 24 -> 48 evaluations: ratio %.3f' % ratio)
    assert 1.8 <= ratio <= 2.2
    assert err['single2'][3] <= 2.5e-3


# ---- 5. refusals and defaults -------------------------------------------------------------------------------------------------------------
def test_refusals_and_defaults():
    cfg = dpm_config(CFG, 6)
    assert cfg.model.pred_data is False and cfg.model.self_cond is False
    assert 'dpm_solver_method' not in cfg.sampling and 'dpm_solver_order' not in cfg.sampling
    assert 'dpm_solver_method' not in make_config('vpsde_geom_2d_cdgs').sampling and 'dpm_solver_order' not in make_config('vpsde_geom_2d_cdgs').sampling
    sv = DPM_Solver_2D(schedule(cfg), cfg)
    assert isinstance(sv, DPM_Solver_hybrid) and (sv.method, sv.order, sv.steps) == ('singlestep_fixed', 2, 6) and sv.noise_form
    assert sv.noise_draws_per_round() == 0
    cfg.model.self_cond = True                                        # (False, True): refused, as AncestralSampler_2D refuses it
    with pytest.raises(AssertionError):
        DPM_Solver_2D(schedule(cfg), cfg)
    cfg.model.pred_data, cfg.model.self_cond = True, False            # (True, False): refused as before
    with pytest.raises(AssertionError):
        DPM_Solver_2D(schedule(cfg), cfg)
    for method, order in (('singlestep_fixed', 4), ('multistep', 3), ('adaptive', 2)):
        with pytest.raises(ValueError):
            DPM_Solver_2D(schedule(cfg), dpm_config(CFG, 6, method, order))


# ---- 6. the public entry on a CPU device ---------------------------------------------------------------------------------------------------
def _setup(steps=6):
    cfg = dpm_config(CFG, steps)
    cfg.device = 'cpu'
    return cfg, OracleCDGS(), schedule(cfg), get_node_dist(load_dataset_info(cfg.data.info_name)), get_data_inverse_scaler(cfg)


def _same(a, b):
    eq = lambda x, y: (x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and torch.equal(x, y))
    return len(a) == len(b) and all(len(m) == len(w) and all(eq(x, y) for x, y in zip(m, w)) for m, w in zip(a, b))


def test_public_entry_on_a_cpu_device():
    cfg, model, ns, nodes_dist, inv = _setup()
    fn = S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv, return_raw=True)
    torch.manual_seed(SEED)
    mols = fn(model)
    assert len(mols) == 4 and len(model.calls) == 6                   # one round, 6 evaluations
    assert all(m[0] is None and m[1].shape[0] == m[2].shape[0] == m[2].shape[1] for m in mols)
    assert fn.last_indices == [0, 1, 2, 3]
    torch.manual_seed(SEED)
    assert _same(S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv, return_raw=True, cpu_noise=True)(model), mols)
    for kw in (dict(hip_graph=True), dict(shard=(0, 2))):
        with pytest.raises(NotImplementedError, match='needs a GPU device'):
            S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv, **kw)
    cfg_f = copy.deepcopy(cfg)
    cfg_f.sampling.method = 'fast'
    with pytest.raises(NotImplementedError, match='dpm_2d'):
        S.get_sampling_fn(cfg_f, ns, nodes_dist, 4, 4, inv)


# parity mode over gloo, world size 2 (the pattern of tests/test_dpm2d_host.py); the private builder is the seam that shards a CPU model
ROUNDS = ((4, 4), (1, 2))          # (batch, samples): one round dealt 2 + 2; two rounds of one molecule, rank 1's share empty in both


def _builder(cfg, ns, nodes_dist, inv, batch, samples, **kw):
    return S._get_sampling_fn_2d(cfg, ns, nodes_dist, batch, samples, inv, 1e-3, **kw)


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


def test_two_parity_shards_partition_the_unsharded_run():
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
        assert idx[0] == [[0, 1], [2, 3]]
        assert idx[1] == [[0, 1], []]                                       # rank 1 held nothing and stayed in step
        for _, out in res:
            for k, (_, full) in enumerate(out):
                got = [tuple(None if a is None else torch.from_numpy(a) for a in m) for m in full]
                # (positions, atom types, bonds): this config has no formal charge — an empty [n, 0] tensor from the round itself,
                # zeros [n] once gathered
                assert cfg.model.include_fc_charge is False and all(m[3].numel() == 0 for m in want[k])
                assert _same([m[:3] for m in got], [m[:3] for m in want[k]])
        assert len({int(m[1].shape[0]) for m in want[0]}) > 1               # not a degenerate batch
    finally:
        torch.set_num_threads(threads)

"""GPU: DPM-Solver++ rounds of the noise-predicting CDGS network (sampling.method 'dpm_2d' in the solver's noise form).

1. jodo_eps_to_data_2d against the framework expression (x - sigma * eps) / alpha, bit for bit on everything it reads, with the regions
   it must not read poisoned; its aliased calls; its table form and jodo_step_begin_t.
2. The eager GPU round (HIP forward, conversion kernel, update kernel) against the same round on the CPU in float64 (dense oracle),
   inside the forward bound 2e-5 + 1e-4 |x| per element.
3. GraphedDPMRound2D in the noise form returns the very bits of DPM_Solver_2D.sampling — which is also what shows that the CDGS forward
   can be captured — with and without bf16x3, and on a second round with other atom counts.
4. The public entry under the single-device DataParallel wrapper: replay, the device decode, parity shards, perf shards."""
import ctypes
import random

import pytest
import torch

from jodo_amd import capi, fused, sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.graphed import GraphedDPMRound2D
from jodo_amd.mix_dpm_solver import DPM_Solver_2D
from jodo_amd.models import get_node_dist, load_dataset_info, get_model_class, deterministic_init_
from jodo_amd.models import utils as mutils
from jodo_amd.utils import get_data_inverse_scaler
from helpers import make_config
import oracle_cdgs as OC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL, RTOL = 2e-5, 1e-4
CFG = {'qm9': 'vpsde_qm9_2d_cdgs', 'geom': 'vpsde_geom_2d_cdgs'}
VARIANTS = {'single1': ('singlestep_fixed', 1, 5), 'single2': ('singlestep_fixed', 2, 6), 'single3': ('singlestep_fixed', 3, 6),
            'multi2': ('multistep', 2, 6)}
_MODELS = {}


def dpm_config(which, steps, method=None, order=None):
    cfg = make_config(CFG[which])
    cfg.sampling.method, cfg.sampling.steps = 'dpm_2d', int(steps)
    if method is not None:
        cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = str(method), int(order)
    return cfg


def schedule(cfg):
    return NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)


def shared_model(which):
    """One model per config (seed 21, head gain 1: the traj_cdgs_qm9_anc5 recipe); the tests leave its weights alone."""
    if which not in _MODELS:
        cfg = make_config(CFG[which])
        _MODELS[which] = deterministic_init_(get_model_class('CDGS')(cfg), seed=21).to(DEV).eval()
    return _MODELS[which]


def initial_state(cfg, n_nodes, seed):
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = S.build_masks(list(n_nodes), N, 'cpu')
    z = torch.randn(B, N, cfg.data.atom_types, generator=g) * nm
    ez = torch.randn(B, N, N, cfg.model.edge_ch, generator=g)
    ez = torch.tril(ez.permute(0, 3, 1, 2), -1).permute(0, 2, 3, 1)
    ez = (ez + ez.transpose(1, 2)) * em.reshape(B, N, N, 1)
    return z, ez, nm, em


# ---- 1. the conversion kernel ----------------------------------------------------------------------------------------------------------------
KB, KN, KCOUNTS = 3, 7, [7, 3, 1]


def kernel_case(nd, ch, seed=5):
    """(x, e, eps_x, eps_e) with NaN wherever the kernel must not read, their NaN-free twins, and the masks of what is read."""
    g = torch.Generator().manual_seed(seed)
    n = torch.tensor(KCOUNTS)
    real = (torch.arange(KN)[None, :] < n[:, None])                                     # [B, N]
    r, c = torch.arange(KN)[:, None], torch.arange(KN)[None, :]
    low = (r > c)[None] & real[:, :, None]                                              # cell (b, r, c) with c < r < n_b
    mk = lambda *s: torch.randn(*s, generator=g)
    clean = [mk(KB, KN, nd), mk(KB, KN, KN, ch), mk(KB, KN, nd), mk(KB, KN, KN, ch)]
    nan = torch.tensor(float('nan'))
    poisoned = [torch.where((real[..., None] if t.dim() == 3 else low[..., None]), t, nan) for t in clean]
    return [t.to(DEV) for t in poisoned], [t.to(DEV) for t in clean], real.to(DEV), low.to(DEV)


def expected(alpha, sigma, clean, real, low):
    """The framework expression of the solver's CPU path, per element in the kernel's op order (evaluated on the CPU: there the
    quotient by a scalar is a division, on the device the framework multiplies by the scalar's reciprocal); edges mirrored from the
    lower triangle."""
    x, e, eps_x, eps_e = (t.cpu() for t in clean)
    real, low = real.cpu(), low.cpu()
    dx = torch.where(real[..., None], (x - sigma * eps_x) / alpha, torch.zeros_like(x))
    de = torch.where(low[..., None], (e - sigma * eps_e) / alpha, torch.zeros_like(e))
    return dx.to(DEV), (de + de.transpose(1, 2)).to(DEV)


def marginals(t):
    ns = schedule(make_config(CFG['qm9']))
    tt = torch.tensor(float(t))
    return torch.exp(ns.marginal_log_mean_coeff(tt)), ns.marginal_std(tt)                # float32 scalars


class _Holder:
    pass


@pytest.mark.parametrize('nd,ch', [(4, 2), (5, 3), (16, 2)])
def test_conversion_kernel_equals_the_framework_expression(nd, ch):
    n_dev = torch.tensor(KCOUNTS, dtype=torch.int32, device=DEV)
    poisoned, clean, real, low = kernel_case(nd, ch)
    for t in (1.0, 0.37, 1e-3):
        alpha, sigma = marginals(t)
        want = expected(alpha, sigma, clean, real, low)
        nan_out = lambda: (torch.full_like(clean[0], float('nan')), torch.full_like(clean[1], float('nan')))
        got = fused.eps_to_data_2d(_Holder(), float(alpha), float(sigma), *poisoned, n_dev, out=nan_out())
        for g_, w_ in zip(got, want):
            assert not bool(torch.isnan(g_).any())                                      # every element written, nothing poisoned read
            assert torch.equal(g_, w_)
        assert torch.equal(got[1], got[1].transpose(1, 2))
        assert float(got[1].diagonal(dim1=1, dim2=2).abs().max()) == 0.0
        assert float(got[0][~real].abs().max()) == 0.0
        # the ring on the holder object: outputs that are none of the inputs
        ring = fused.eps_to_data_2d(_Holder(), float(alpha), float(sigma), *poisoned, n_dev)
        assert torch.equal(ring[0], want[0]) and torch.equal(ring[1], want[1])
        assert all(o.data_ptr() not in {p.data_ptr() for p in poisoned} for o in ring)
        # aliased: d = the eps buffers, d = the x buffers
        for pair in ((2, 3), (0, 1)):
            ins = [p.clone() for p in poisoned]
            out = fused.eps_to_data_2d(_Holder(), float(alpha), float(sigma), *ins, n_dev, out=(ins[pair[0]], ins[pair[1]]))
            assert out[0] is ins[pair[0]] and torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


@pytest.mark.parametrize('stride,col', [(8, 0), (16, 0), (16, 8)])
def test_conversion_kernel_table_form_and_time_fetch(stride, col):
    nd, ch, rows = 5, 3, 4
    n_dev = torch.tensor(KCOUNTS, dtype=torch.int32, device=DEV)
    poisoned, clean, real, low = kernel_case(nd, ch, seed=9)
    g = torch.Generator().manual_seed(2)
    tab_host = torch.randn(rows, stride, generator=g)                                   # every other column holds something else
    times = (1.0, 0.7, 0.2, 1e-3)
    for k, t in enumerate(times):
        alpha, sigma = marginals(t)
        tab_host[k, col + 4], tab_host[k, col + 5], tab_host[k, col + 6] = t, alpha, sigma
    tab = tab_host.to(DEV)
    L, st = capi.lib(), capi.current_stream_ptr()
    for row in (0, rows - 1):
        step = torch.tensor([row], dtype=torch.int32, device=DEV)
        alpha, sigma = tab_host[row, col + 5], tab_host[row, col + 6]
        host = fused.eps_to_data_2d(_Holder(), float(alpha), float(sigma), *poisoned, n_dev)
        dx, de = torch.full_like(clean[0], float('nan')), torch.full_like(clean[1], float('nan'))
        capi.check(L.jodo_eps_to_data_2d(KB, KN, nd, ch, capi.ptr(n_dev), 0.0, 0.0, capi.ptr(tab), capi.ptr(step), stride, col,
                                         *[capi.ptr(p) for p in poisoned], capi.ptr(dx), capi.ptr(de), st), 'jodo_eps_to_data_2d')
        assert torch.equal(dx, host[0]) and torch.equal(de, host[1])                     # bit-identical to the host-scalar form
        want = expected(alpha, sigma, clean, real, low)
        assert torch.equal(dx, want[0]) and torch.equal(de, want[1])
        t_out, nl_out = torch.full((KB,), float('nan'), device=DEV), torch.full((KB,), float('nan'), device=DEV)
        capi.check(L.jodo_step_begin_t(KB, capi.ptr(tab), capi.ptr(step), stride, col, capi.ptr(t_out), capi.ptr(nl_out), st), 'jodo_step_begin_t')
        assert torch.equal(t_out.cpu(), tab_host[row, col + 4].expand(KB)) and torch.equal(nl_out.cpu(), tab_host[row, col + 7].expand(KB))
        t_only = torch.full((KB,), float('nan'), device=DEV)
        capi.check(L.jodo_step_begin_t(KB, capi.ptr(tab), capi.ptr(step), stride, col, capi.ptr(t_only), None, st), 'jodo_step_begin_t')
        assert torch.equal(t_only, t_out)
    # a row that does not hold the 8 columns is refused, as jodo_dpm_update_2d refuses it
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert L.jodo_eps_to_data_2d(KB, KN, nd, ch, capi.ptr(n_dev), 0.0, 0.0, capi.ptr(tab), capi.ptr(step), stride, stride - 4,
                                 *[capi.ptr(p) for p in poisoned], capi.ptr(poisoned[2]), capi.ptr(poisoned[3]), st) != 0


# ---- 2. the eager GPU round against the float64 CPU round ------------------------------------------------------------------------------------
class Oracle64:
    def __init__(self, model, cfg):
        self.sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
        self.hp = OC.hparams(cfg)

    def __call__(self, t, x, node_mask, edge_mask, context=None, **kw):
        with torch.no_grad():
            return OC.forward(self.sd, self.hp, t, x, node_mask, edge_mask, kw['edge_x'])


ROUND_CASES = {'qm9 single1': ('qm9', 'single1', [9, 1, 2, 5]), 'qm9 single2': ('qm9', 'single2', [9, 1, 2, 5]),
               'qm9 single3': ('qm9', 'single3', [9, 1, 2, 5]), 'qm9 multi2': ('qm9', 'multi2', [9, 1, 2, 5]),
               'geom single2': ('geom', 'single2', [5, 9, 2])}


@pytest.mark.parametrize('case', sorted(ROUND_CASES))
def test_eager_round_against_the_float64_cpu_round(case):
    which, name, n_nodes = ROUND_CASES[case]
    method, order, steps = VARIANTS[name]
    cfg = dpm_config(which, steps, method, order)
    model = shared_model(which)
    z, ez, nm, em = initial_state(cfg, n_nodes, 3)
    d = lambda v: v.to(DEV)
    z_dev, ez_dev = d(z), d(ez)
    got = DPM_Solver_2D(schedule(cfg), cfg).sampling(model, z_dev, d(nm), d(em), ez_dev, None)
    want = DPM_Solver_2D(schedule(cfg), cfg).sampling(Oracle64(model, cfg), z.double(), nm, em, ez.double(), None)
    B, N = len(n_nodes), max(n_nodes)
    for g_, w_, what in zip(got, want, ('x', 'e')):
        err = (g_.cpu().double() - w_).abs()
        bound = ATOL + RTOL * w_.abs()
        print('%s %s: max |err| %.3e at max |x| %.3e, worst err / bound %.4f' % (case, what, err.max().item(), w_.abs().max().item(),
                                                                                  (err / bound).max().item()))
        assert g_.dtype == torch.float32 and bool((err <= bound).all())
    assert torch.equal(got[1], got[1].transpose(1, 2))
    assert float((got[0].cpu() * (1 - nm)).abs().max()) == 0.0 and float((got[1].cpu() * (1 - em.reshape(B, N, N, 1))).abs().max()) == 0.0
    assert torch.equal(z_dev.cpu(), z) and got[0].data_ptr() != z_dev.data_ptr()          # inputs untouched, results of their own


# ---- 3. replay equals eager --------------------------------------------------------------------------------------------------------------------
def _eager_and_replayed(solver, model, cfg, n_nodes, seed):
    z, ez, nm, em = (v.to(DEV) for v in initial_state(cfg, n_nodes, seed))
    with torch.no_grad():
        eager = solver.sampling(model, z, nm, em, ez, None)
        replayed = GraphedDPMRound2D(solver, model, nm, em).run(z, ez)
    torch.cuda.synchronize()
    return eager, replayed


@pytest.mark.parametrize('bf16x3', [False, True])
@pytest.mark.parametrize('name,steps', [('single2', 8), ('multi2', 5)])
def test_replay_returns_the_bits_of_the_eager_round(name, steps, bf16x3):
    method, order, _ = VARIANTS[name]
    cfg = dpm_config('qm9', steps, method, order)
    model = shared_model('qm9')
    solver = DPM_Solver_2D(schedule(cfg), cfg)
    assert solver.noise_form and GraphedDPMRound2D.supports(solver)
    try:
        model.bf16x3 = bf16x3
        model.invalidate_packed_weights()                  # the eager first step has to pack the blob and, with the switch on, the tape
        for n_nodes, seed in (([4, 4], 5), ([9, 1, 2, 5], 6)):              # the second round: same solver, other atom counts
            eager, replayed = _eager_and_replayed(solver, model, cfg, n_nodes, seed)
            assert bool(torch.isfinite(replayed[0]).all()) and float(replayed[0].abs().max()) > 0
            assert torch.equal(eager[0], replayed[0]) and torch.equal(eager[1], replayed[1])
            if bf16x3:
                assert int(model.last_flags[3]) == 1
            else:
                assert model.last_flags is None
    finally:
        model.bf16x3 = False
        model.invalidate_packed_weights()


def test_replay_refuses_the_other_orders():
    model = shared_model('qm9')
    _, _, nm, em = (v.to(DEV) for v in initial_state(make_config(CFG['qm9']), [4, 4], 5))
    for name in ('single1', 'single3'):
        method, order, steps = VARIANTS[name]
        cfg = dpm_config('qm9', steps, method, order)
        with pytest.raises(NotImplementedError, match='graph replay'):
            GraphedDPMRound2D(DPM_Solver_2D(schedule(cfg), cfg), model, nm, em)


# ---- 4. the public entry on the device ----------------------------------------------------------------------------------------------------------
def _same_mols(a, b):
    return len(a) == len(b) and all(m[0] is None and w[0] is None and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(m[1:], w[1:]))
                                    for m, w in zip(a, b))


def test_public_entry_under_dataparallel():
    cfg = dpm_config('qm9', 6)
    cfg.device = torch.device(DEV)
    model = mutils.create_model(cfg, wrap='dataparallel')    # the reference's wrapper, over the one device
    deterministic_init_(model.module, seed=21)
    model.module.invalidate_packed_weights()
    ns, nodes_dist, inv = schedule(cfg), get_node_dist(load_dataset_info(cfg.data.info_name)), get_data_inverse_scaler(cfg)
    batch, seed = 4, 77

    def run(**kw):
        fn = S.get_sampling_fn(cfg, ns, nodes_dist, batch, batch, inv, return_raw=True, **kw)
        torch.manual_seed(seed)
        random.seed(seed)
        return fn, fn(model)

    _, mols = run(cpu_noise=True)
    assert len(mols) == batch and all(m[0] is None and m[1].shape[0] == m[2].shape[0] == m[2].shape[1] for m in mols)
    _, graphed = run(cpu_noise=True, hip_graph=True)
    assert _same_mols(graphed, mols)                         # the same molecules under the same seed
    _, plain = run()
    _, plain_graphed = run(hip_graph=True)
    assert _same_mols(plain_graphed, plain)
    for order in (1, 3):                                     # the variants that replay does not cover keep raising
        cfg_o = dpm_config('qm9', 6, 'singlestep_fixed', order)
        cfg_o.device = cfg.device
        with pytest.raises(NotImplementedError, match='hip_graph'):
            S.get_sampling_fn(cfg_o, ns, nodes_dist, batch, batch, inv, hip_graph=True)
    # two parity shards together are the unsharded run (each share padded to the round's width)
    parts, idx = [], []
    for rank in (0, 1):
        sh = S.get_sampling_fn(cfg, ns, nodes_dist, batch, batch, inv, shard=(rank, 2), shard_mode='parity', seed=seed, return_raw=True)
        parts += sh(model)
        idx += sh.last_indices
        assert len(sh.last_decoded) == 1 and sh.last_decoded[0][1].is_cuda          # the device decode ran
    assert idx == list(range(batch)) and _same_mols(parts, mols)
    # perf shards: disjoint index sets that cover the round
    sets = []
    for rank in (0, 1):
        sh = S.get_sampling_fn(cfg, ns, nodes_dist, batch, batch, inv, shard=(rank, 2), shard_mode='perf', seed=seed, return_raw=True,
                               hip_graph=bool(rank))
        assert len(sh(model)) == len(sh.last_indices)
        sets.append(set(sh.last_indices))
    assert not (sets[0] & sets[1]) and sets[0] | sets[1] == set(range(batch))

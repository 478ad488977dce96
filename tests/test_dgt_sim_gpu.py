"""DGT_concat_sim on the GPU: the HIP path (csrc/dgt_kernels_attn.h SIM, csrc/dgt_kernels_wide.h NC = 1) against the reference's
recorded outputs (tools/make_golden_sim.py) and the float64 oracle tests/oracle_sim.py, at the project's tolerances: single forward
atol 2e-5 + rtol 1e-4 (helpers.close64 on fresh inputs), per-block tensors 1e-4, K-step trajectories atol 1e-3 with bit-exact
decodes wherever the recorded decision margin exceeds 1e-3."""
import pytest
import torch

import oracle_sim as OS
from helpers import (SPREAD_THREADS, check_decodes, close64, debug_fetch, load_fixture, make_config, make_model, masks,
                     reference_blocks_dense, state_dict_cpu)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAME = 'DGT_concat_sim'
QM9, GEOM = 'vpsde_qm9_uncond_jodo', 'vpsde_geom_uncond_jodo'


def sim_config(cfg_name, **over):
    return make_config(cfg_name, name=NAME, **over)


def close(got, want, atol=2e-5, rtol=1e-4):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    assert bool((err <= atol + rtol * want.abs()).all()), "max err %.3e (bound %.1e + %.0e*|x|)" % (err.max().item(), atol, rtol)


def run(model, xh, ex, nl, nm, em, cx=None, cex=None):
    d = lambda x: None if x is None else x.to(DEV)
    with torch.no_grad():
        out = model(d(nl), d(xh), d(nm), d(em), edge_x=d(ex), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(nl))
    torch.cuda.synchronize()
    return out[0].cpu(), out[1].cpu()


def random_inputs(hp, n_nodes, seed, symmetric=True, N=None):
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), int(N or max(n_nodes))
    from jodo_amd.sampling import build_masks
    nm, em = build_masks(list(n_nodes), N, 'cpu')
    xh = torch.randn(B, N, 3 + hp.in_node_dim, generator=g) * nm
    ex = torch.randn(B, N, N, hp.edge_ch, generator=g)
    if symmetric:
        ex = ex + ex.transpose(1, 2)
    ex = ex * em.reshape(B, N, N, 1)
    return xh, ex, torch.randn(B, generator=g) * 2, nm, em


def oracle_32_64(sd, hp, xh, nm, em, ex, cx, cex, nl):
    """The float32 and the float64 oracle on the same inputs; above 128 atoms the float32 one again at other thread counts, the
    largest distance riding along as `.yard` (the spread yardstick of helpers.oracle_32_64 / close64)."""
    def ev(dtype):
        c = lambda t: None if t is None else t.detach().cpu().to(dtype)
        p = sd if dtype == torch.float32 else {k: v.double() for k, v in sd.items()}
        with torch.no_grad():
            return OS.forward_dense(p, hp, c(xh), c(nm), c(em), c(ex), c(cx), c(cex), c(nl))
    r32, r64 = ev(torch.float32), ev(torch.float64)
    if int(nm.reshape(nm.shape[0], -1).sum(1).max()) > 128:
        yard = [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]
        keep = torch.get_num_threads()
        try:
            for th in SPREAD_THREADS:
                torch.set_num_threads(th)
                yard = [max(y, float((a.double() - b).abs().max())) for y, a, b in zip(yard, ev(torch.float32), r64)]
        finally:
            torch.set_num_threads(keep)
        for t, y in zip(r32, yard):
            t.yard = y
    return r32, r64


def check64(got, sd, hp, xh, nm, em, ex, cx, cex, nl, what):
    r32, r64 = oracle_32_64(sd, hp, xh, nm, em, ex, cx, cex, nl)
    close64(got[0], r32[0], r64[0], what + ' nodes')
    close64(got[1], r32[1], r64[1], what + ' edges')
    return r32


# ---- the reference's recorded outputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ['fwd_sim_qm9.npz', 'fwd_sim_geom.npz'])
def test_hip_matches_reference_fixture(fname):
    fx = load_fixture(fname)
    model = make_model(sim_config(str(fx['cfg_name'])), int(fx['seed']), DEV)
    nm, em = masks(fx['n_nodes'].tolist())
    t = lambda k: torch.from_numpy(fx[k])
    o1 = run(model, t('xh'), t('edge_x'), t('noise_level'), nm, em)
    close(o1[0], t('out1_x'))
    close(o1[1], t('out1_e'))
    o2 = run(model, t('xh'), t('edge_x'), t('noise_level'), nm, em, t('out1_x'), t('out1_e'))
    close(o2[0], t('out2_x'))
    close(o2[1], t('out2_e'))
    flags = model.last_flags.cpu().tolist()
    assert flags[0] == 0 and flags[4] == 0                           # NaN guard silent, pair path
    # asymmetric edge_x: the directed kernels (device flag), the reference's semantics
    oa = run(model, t('xh'), t('asym_edge_x'), t('noise_level'), nm, em, t('out1_x'), t('out1_e'))
    close(oa[0], t('out_asym_x'))
    close(oa[1], t('out_asym_e'))
    flags = model.last_flags.cpu().tolist()
    assert flags[0] == 0 and flags[4] == 1


# ---- the float64 oracle on fresh inputs --------------------------------------------------------------------------------------
ORACLE_CASES = {
    # no edges (n = 1), the single offset d = n / 2 (n = 2), even and odd circulant walks
    'qm9': (QM9, [29, 1, 2, 18, 18, 7, 23], 1.0, 0),
    # multi-strip, odd chunking of the sources, larger activations
    'strips': (QM9, [5] * 20 + [19] * 14, 1.5, 3),
    # the GEOM config: 10 blocks, mlp_ratio 4, three bond channels
    'geom': (GEOM, [70, 33, 12, 1, 2], 1.5, 0),
    # one molecule above a 128-lane attention group (the smallest such size) beside a small one: directed-mode items by size; the
    # reference's initialisation scale
    'big': (QM9, [129, 6], 1.0, 0),
}


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_hip_matches_float64_oracle(case):
    cfg_name, n_nodes, gain, chunk = ORACLE_CASES[case]
    cfg = sim_config(cfg_name)
    model = make_model(cfg, 5, DEV, gain=gain, coord_scale=0.05)
    model.max_chunk = chunk
    hp = OS.HyperSim.from_config(cfg)
    sd = state_dict_cpu(model)
    xh, ex, nl, nm, em = random_inputs(hp, n_nodes, seed=len(n_nodes))
    o1 = run(model, xh, ex, nl, nm, em)
    r1 = check64(o1, sd, hp, xh, nm, em, ex, None, None, nl, case + ' first step')
    o2 = run(model, xh, ex, nl, nm, em, r1[0], r1[1])
    check64(o2, sd, hp, xh, nm, em, ex, r1[0], r1[1], nl, case + ' self-conditioned')
    flags = model.last_flags.cpu().tolist()
    assert flags[0] == 0 and flags[4] == 0


def test_per_block_intermediates():
    """h, edge state and positions after EVERY block against the reference's own per-block tensors at atol 1e-4."""
    from jodo_amd import capi
    fx = load_fixture('blocks_sim_qm9.npz')
    cfg = sim_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    hp = OS.HyperSim.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    args = (t('noise_level'), t('xh'), nm, em)
    kw = dict(edge_x=t('edge_x'), cond_x=t('out1_x'), cond_edge_x=t('out1_e'), noise_level=t('noise_level'))
    with torch.no_grad():
        o = model(*args, **kw)
    close(o[0], t('out2_x'))
    close(o[1], t('out2_e'))
    order = sorted(range(len(n_nodes)), key=lambda b: -n_nodes[b])           # the plan's order: descending n, stable
    Nn, rows, D, De = sum(n_nodes), sum(n * n for n in n_nodes), hp.nf, hp.de
    handle = model._last_plan['handle']
    try:
        for l in range(hp.n_layers):
            capi.check(capi.lib().jodo_debug_set_max_blocks(handle, l + 1), 'set_max_blocks')
            with torch.no_grad():
                model(*args, **kw)
            assert model._last_plan['handle'] is handle
            h = debug_fetch(model, 0, Nn * D).reshape(Nn, D)
            e = debug_fetch(model, 1, rows * De).reshape(rows, De)
            pos = debug_fetch(model, 2, Nn * 4).reshape(Nn, 4)[:, :3]
            ref = reference_blocks_dense(fx, l)
            no, eo = 0, 0
            for b in order:
                n = n_nodes[b]
                rh, re, rp = ref[b]
                offd = ~torch.eye(n, dtype=torch.bool)
                gp = pos[no:no + n] - pos[no:no + n].mean(0, keepdim=True)      # the kernels centre once, at the end
                ge = e[eo:eo + n * n].reshape(n, n, De)
                for name, got, want in (('h', h[no:no + n], rh), ('e', ge[offd], re[offd]), ('pos', gp, rp)):
                    err = (got - want).abs().max().item() if want.numel() else 0.0
                    assert err < 1e-4, "block %d molecule %d %s: %.3e" % (l, b, name, err)
                no += n
                eo += n * n
    finally:
        capi.check(capi.lib().jodo_debug_set_max_blocks(handle, -1), 'set_max_blocks')


@pytest.mark.parametrize("cfg_name,n_nodes", [(QM9, [1, 2, 3, 4, 9, 10, 18, 29, 28]), (GEOM, [44, 45, 7])])
def test_pair_path_equals_directed_path(cfg_name, n_nodes):
    """Symmetric inputs take the pair kernels (device flag [4] = 0); forcing the directed kernels on the same inputs gives the same
    result within 1e-5, and both match the oracle."""
    cfg = sim_config(cfg_name)
    hp = OS.HyperSim.from_config(cfg)
    xh, ex, nl, nm, em = random_inputs(hp, n_nodes, seed=11)
    m_pair = make_model(cfg, 3, DEV, gain=1.5, coord_scale=0.05)
    m_dir = make_model(cfg, 3, DEV, gain=1.5, coord_scale=0.05)
    m_dir.force_directed = True
    sd = state_dict_cpu(m_pair)
    cx = cex = None
    for step in (1, 2):
        a = run(m_pair, xh, ex, nl, nm, em, cx, cex)
        assert m_pair.last_flags.cpu().tolist()[4] == 0
        b = run(m_dir, xh, ex, nl, nm, em, cx, cex)
        assert m_dir.last_flags.cpu().tolist()[4] == 1
        r32 = check64(a, sd, hp, xh, nm, em, ex, cx, cex, nl, 'pair path, step %d' % step)
        check64(b, sd, hp, xh, nm, em, ex, cx, cex, nl, 'directed path, step %d' % step)
        close(a[0], b[0], atol=1e-5)
        close(a[1], b[1], atol=1e-5)
        cx, cex = r32


def test_invariants():
    """Rotation (positions equivariant, the rest invariant), permutation of the batch, padding: exact zeros on it, and a wider
    padded width changes nothing; exact symmetry; run-to-run determinism."""
    cfg = sim_config(QM9)
    model = make_model(cfg, 4, DEV, gain=1.5, coord_scale=0.05)
    hp = OS.HyperSim.from_config(cfg)
    n_nodes = [12, 29, 3, 17]
    xh, ex, nl, nm, em = random_inputs(hp, n_nodes, seed=2)
    xh[:, :, :3] -= xh[:, :, :3].sum(1, keepdim=True) / nm.sum(1, keepdim=True) * nm
    x1, e1 = run(model, xh, ex, nl, nm, em)
    B, N = len(n_nodes), max(n_nodes)
    assert torch.equal(e1, e1.transpose(1, 2))
    assert (x1 * (1 - nm)).abs().max() == 0 and (e1 * (1 - em.reshape(B, N, N, 1))).abs().max() == 0
    assert x1[:, :, :3].sum(1).abs().max() < 1e-5
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(0)))
    xr = xh.clone()
    xr[:, :, :3] = xh[:, :, :3] @ q
    x2, e2 = run(model, xr, ex, nl, nm, em)
    close(x2[:, :, :3], x1[:, :, :3] @ q, atol=2e-5)
    close(x2[:, :, 3:], x1[:, :, 3:], atol=2e-5)
    close(e2, e1, atol=2e-5)
    perm = [2, 0, 3, 1]
    nmp, emp = masks([n_nodes[p] for p in perm])
    x4, e4 = run(model, xh[perm], ex[perm], nl[perm], nmp, emp)
    close(x4, x1[perm], atol=1e-5)
    close(e4, e1[perm], atol=1e-5)
    # three more padded columns: the real part is the same computation (same plan contents, another dense layout)
    from jodo_amd.sampling import build_masks
    nmw, emw = build_masks(n_nodes, N + 3, 'cpu')
    xw, ew = torch.zeros(B, N + 3, xh.shape[2]), torch.zeros(B, N + 3, N + 3, ex.shape[3])
    xw[:, :N], ew[:, :N, :N] = xh, ex
    x5, e5 = run(model, xw, ew, nl, nmw, emw)
    assert torch.equal(x5[:, :N], x1) and torch.equal(e5[:, :N, :N], e1)
    assert x5[:, N:].abs().max() == 0 and e5[:, N:].abs().max() == 0 and e5[:, :, N:].abs().max() == 0
    x6, e6 = run(model, xh, ex, nl, nm, em)
    assert torch.equal(x6, x1) and torch.equal(e6, e1)


def test_ignored_config_keys_change_no_bit():
    """A user who changes only model.name keeps n_extra_heads = 2 in the config: the same bits as with 0, and as with other values
    of the keys the reference's class never reads."""
    hp = OS.HyperSim.from_config(sim_config(QM9))
    xh, ex, nl, nm, em = random_inputs(hp, [9, 1, 2, 16], seed=6)
    outs = []
    for over in (dict(n_extra_heads=2), dict(n_extra_heads=0), dict(softmax_inf=False, edge_quan_th=0.4, spatial_cut_off=0.5,
                                                                    trans_name='Trans_Layer')):
        model = make_model(sim_config(QM9, **over), 5, DEV, gain=1.5)
        o1 = run(model, xh, ex, nl, nm, em)
        outs.append(o1 + run(model, xh, ex, nl, nm, em, o1[0], o1[1]))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


# ---- samplers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_on", [True, False])
def test_ancestral_trajectory(fused_on):
    """The reference's recorded 5-step trajectory (its own draws replayed); fused_on: the per-step update is the fused kernel."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import AncestralSampler
    from jodo_amd.utils import get_self_cond_fn
    fx = load_fixture('traj_sim_qm9_anc5.npz')
    cfg = sim_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    ns = NoiseScheduleVP(cfg.sde.schedule)
    noise = {'node': torch.from_numpy(fx['node_noise']).to(DEV), 'edge': torch.from_numpy(fx['edge_noise']).to(DEV)}
    sampler = AncestralSampler(ns, torch.linspace(ns.T, 1e-3, int(fx['steps'])), True, True, True, get_self_cond_fn(cfg),
                               noise_fn=lambda i, kind, like: noise[kind][i], fused=fused_on)
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    close(x_mean, torch.from_numpy(fx['x_mean']), atol=1e-3, rtol=0)
    close(e_mean, torch.from_numpy(fx['edge_x_mean']), atol=1e-3, rtol=0)
    check_decodes(cfg, fx, x_mean, e_mean, nm, em)
    model.unpin_paths()


@pytest.mark.parametrize("fused_on", [True, False])
def test_dpm_solver_trajectory(fused_on):
    """The reference's recorded DPM_Solver_hybrid run (single-step, order 2, NFE 6; its position-noise draws replayed)."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.mix_dpm_solver import DPM_Solver_hybrid
    fx = load_fixture('traj_sim_qm9_dpm_single2.npz')
    cfg = sim_config(str(fx['cfg_name']))
    cfg.sampling.steps, cfg.sampling.method = int(fx['nfe']), 'fast'
    cfg.sampling.dpm_solver_method, cfg.sampling.dpm_solver_order = str(fx['method']), int(fx['order'])
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    pn = torch.from_numpy(fx['pos_noise']).to(DEV)
    solver = DPM_Solver_hybrid(NoiseScheduleVP(cfg.sde.schedule), cfg, noise_fn=lambda i, kind, like: pn[i], fused=fused_on)
    with torch.no_grad():
        x, e = solver.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    close(x, torch.from_numpy(fx['x_mean']), atol=1e-3, rtol=0)
    close(e, torch.from_numpy(fx['edge_x_mean']), atol=1e-3, rtol=0)
    check_decodes(cfg, fx, x, e, nm, em)
    model.unpin_paths()


class _FixedNodes:
    def __init__(self, n_nodes):
        self.n = torch.as_tensor(n_nodes)

    def sample(self, k):
        assert k == self.n.numel()
        return self.n.clone()


@pytest.mark.parametrize("method", ['ancestral', 'fast'])
def test_graph_replayed_round_equals_eager_device_noise_round(method):
    """One get_sampling_fn round (shard = (0, 1): device noise, fused decode), eager and as a replayed HIP graph: the same draws, the
    same kernels, the same molecules bit for bit.  Both kinds of round: the ancestral step and the DPM outer step."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    cfg = sim_config(QM9)
    cfg.device = torch.device(DEV)
    cfg.sampling.steps, cfg.sampling.method = 6, method
    cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = 'singlestep_fixed', 2
    model = make_model(cfg, 12, DEV, head_gain=10.0)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    n_nodes = [27, 5, 9, 1, 14, 2]
    runs = []
    for hip_graph in (False, True):
        fn = get_sampling_fn(cfg, ns, _FixedNodes(n_nodes), len(n_nodes), len(n_nodes), get_data_inverse_scaler(cfg), shard=(0, 1),
                             shard_mode='perf', seed=31, device_noise=True, hip_graph=hip_graph, return_raw=True)
        torch.manual_seed(31)
        runs.append(fn(model))
    assert [int(m[0].shape[0]) for m in runs[0]] == n_nodes and len(runs[1]) == len(n_nodes)
    for a, b in zip(*runs):
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(bool(torch.isfinite(m[0]).all()) for m in runs[0])
    assert not any(p.get('pinned') for p in model._plans.values())       # the round unpinned what it pinned


def test_split_bf16_and_training_are_refused():
    cfg = sim_config(QM9)
    model = make_model(cfg, 4, DEV)
    hp = OS.HyperSim.from_config(cfg)
    xh, ex, nl, nm, em = (t.to(DEV) for t in random_inputs(hp, [4, 6], seed=4))
    call = lambda: model(nl, xh, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)
    with pytest.raises(NotImplementedError, match='inference'):
        call()                                                       # grad enabled: a training call
    with torch.no_grad():
        model.split_bf16 = True
        with pytest.raises(NotImplementedError, match='split-bf16'):
            call()
        model.split_bf16 = False
        out = call()
    assert bool(torch.isfinite(out[0]).all()) and not out[0].requires_grad

"""GPU: the HIP CDGS network (jodo_amd/models/cdgs.py, csrc/cdgs_forward.hip) against the reference's fixtures and the dense CPU oracle
(tests/oracle_cdgs.py).  Against fixtures the forward bound atol 2e-5 + rtol 1e-4 applies as it stands; on fresh inputs the rule is
helpers.close64 (float64 oracle, K64 = 4 times the float32 oracle's own error where that is larger); a 5-step trajectory within 1e-3
with identical decodes wherever the recorded decision margin exceeds 1e-3 (the tolerances of tests/test_dgt2d_gpu.py)."""
import random

import numpy as np
import pytest
import torch

from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.models import get_node_dist, load_dataset_info, get_model_class, deterministic_init_
from jodo_amd.models import utils as mutils
from jodo_amd.utils import get_data_inverse_scaler
from helpers import load_fixture, make_config, close64
import oracle2d as O2
import oracle_cdgs as OC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL, RTOL = 2e-5, 1e-4
CFG = {'qm9': 'vpsde_qm9_2d_cdgs', 'geom': 'vpsde_geom_2d_cdgs'}
_MODELS, _SD64 = {}, {}


def fwd_close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = ATOL + RTOL * want.abs()
    print('%s: max |err| %.3e, worst err / bound %.3f' % (what, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all()), "%s: max |err| %g, worst err / bound %g" % (what, err.max().item(), (err / bound).max().item())


def head_keys(L):
    h0 = 10 + 3 * L
    return ['all_modules.%d.weight' % (h0 + 2), 'all_modules.%d.weight' % (h0 + 5), 'all_modules.%d.weight' % (h0 + 8)]


def make_model(cfg, seed, head_gain=1.0):
    model = deterministic_init_(get_model_class('CDGS')(cfg), seed=seed)
    if head_gain != 1.0:
        with torch.no_grad():
            for k in head_keys(cfg.model.n_layers):
                model.state_dict()[k].mul_(head_gain)
    return model.to(DEV).eval()


def shared_model(which, seed=7):
    """One model per config for the tests that do not touch the weights."""
    if (which, seed) not in _MODELS:
        cfg = make_config(CFG[which])
        _MODELS[(which, seed)] = (cfg, make_model(cfg, seed))
    return _MODELS[(which, seed)]


def inputs(cfg, n_nodes, seed, N=None, symmetric=True):
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), int(N or max(n_nodes))
    nm, em = S.build_masks(list(n_nodes), N, 'cpu')
    x = torch.randn(B, N, cfg.data.atom_types, generator=g) * nm
    ex = torch.randn(B, N, N, cfg.model.edge_ch, generator=g)
    if symmetric:
        ex = ex + ex.transpose(1, 2)
    ex = ex * em.reshape(B, N, N, 1)
    t = torch.rand(B, generator=g) * 0.999 + 1e-3
    return t, x, ex, nm, em


def call(model, t, x, ex, nm, em):
    d = lambda v: v.to(DEV)
    with torch.no_grad():
        return model(d(t), d(x), d(nm), d(em), edge_x=d(ex))


def oracle_32_64(cfg, model, t, x, ex, nm, em, **kw):
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    key = id(model)
    if key not in _SD64 or any(not torch.equal(a.float(), b) for a, b in zip(_SD64[key].values(), sd.values())):
        _SD64.clear()
        _SD64[key] = {k: v.double() for k, v in sd.items()}
    hp = OC.hparams(cfg)
    with torch.no_grad():
        return OC.forward(sd, hp, t, x, nm, em, ex, **kw), OC.forward(_SD64[key], hp, t, x, nm, em, ex, **kw)


def check64(cfg, model, n_nodes, seed, what, N=None, symmetric=True, edit=None):
    t, x, ex, nm, em = inputs(cfg, n_nodes, seed, N, symmetric)
    if edit is not None:
        ex = edit(ex) * em.reshape(ex.shape[0], ex.shape[1], ex.shape[1], 1)
    got = call(model, t, x, ex, nm, em)
    r32, r64 = oracle_32_64(cfg, model, t, x, ex, nm, em)
    close64(got[0], r32[0], r64[0], what + ' x')
    close64(got[1], r32[1], r64[1], what + ' e')
    B, N = ex.shape[0], ex.shape[1]
    assert float((got[0].cpu() * (1 - nm)).abs().max()) == 0.0
    assert float((got[1].cpu() * (1 - em.reshape(B, N, N, 1))).abs().max()) == 0.0
    assert torch.equal(got[1], got[1].transpose(1, 2))
    return got, r64


# ---- 1. the reference's fixtures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['qm9', 'geom'])
def test_forward_matches_reference_fixture(which):
    fx = load_fixture('fwd_cdgs_%s.npz' % which)
    cfg, model = shared_model(which, int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    nm, em = S.build_masks(n_nodes, max(n_nodes), 'cpu')
    t = lambda k: torch.from_numpy(fx[k])
    got = call(model, t('t'), t('x'), t('edge_x'), nm, em)
    fwd_close(got[0], t('out_x'), which + ' x')
    fwd_close(got[1], t('out_e'), which + ' e')


def test_blocks_match_reference_fixture():
    fx = load_fixture('blocks_cdgs_qm9.npz')
    cfg, model = shared_model('qm9', int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    nm, em = S.build_masks(n_nodes, max(n_nodes), 'cpu')
    t = lambda k: torch.from_numpy(fx[k])
    rows, off = [], 0                                        # fixture order: real ordered pairs (b, r, c) row-major
    for n in n_nodes:
        rows += [off + r * n + c for r in range(n) for c in range(n) if r != c]
        off += n * n
    diag = torch.ones(off, dtype=torch.bool)
    diag[torch.tensor(rows)] = False
    try:
        for l in range(cfg.model.n_layers):
            model.max_blocks = l + 1
            call(model, t('t'), t('x'), t('edge_x'), nm, em)
            h, e = model.debug_state()
            fwd_close(h, torch.from_numpy(fx['h'][l]), 'h after block %d' % l)
            fwd_close(e.cpu()[torch.tensor(rows)], torch.from_numpy(fx['e'][l]), 'e after block %d' % l)
            assert float(e.cpu()[diag].abs().max()) == 0.0       # the diagonal rows are zero between blocks
    finally:
        model.max_blocks = -1


# ---- 2. the edge GroupNorm runs over the padded tensor ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_nodes,wide', [([9, 4, 7, 2], 12), ([29, 11, 17], 33)])
def test_scores_follow_the_padded_width(n_nodes, wide):
    cfg, model = shared_model('qm9')
    n = max(n_nodes)
    a, _ = check64(cfg, model, n_nodes, 31, 'padded to its own maximum %d' % n)
    t, x, ex, nm, em = inputs(cfg, n_nodes, 31)
    pad = lambda v, dims: torch.nn.functional.pad(v, (0, 0) + (0, wide - n) * dims)
    nmw, emw = S.build_masks(n_nodes, wide, 'cpu')
    xw, exw = pad(x, 1), pad(ex, 2)
    got = call(model, t, xw, exw, nmw, emw)
    r32, r64 = oracle_32_64(cfg, model, t, xw, exw, nmw, emw)
    close64(got[0], r32[0], r64[0], 'padded to %d x' % wide)
    close64(got[1], r32[1], r64[1], 'padded to %d e' % wide)
    # the same molecules, two widths: far apart (a kernel that normalises over n cannot pass both)
    for k, (p, q) in enumerate(((a[0].cpu(), got[0].cpu()[:, :n]), (a[1].cpu(), got[1].cpu()[:, :n, :n]))):
        ratio = float(((p - q).abs() / (ATOL + RTOL * p.abs())).max())
        print('width %d vs %d, output %d: max difference / bound %.1f' % (n, wide, k, ratio))
        assert ratio > 100.0


# ---- 3. size edges, against the float64 oracle ---------------------------------------------------------------------------------------------
# Boundaries of the kernels: kc_gemm works on strips of 64 rows (two tiles of 32) and 128 output columns, so the atom count Nn, the edge
# row count R = sum n^2 and the batch size B (time MLP rows) are taken to both sides of 32 / 64; kc_rw walks n^2 entries 256 at a time
# (n = 16 is exactly one pass, n = 17 the first with a second); kc_estats splits a molecule's n^2 rows four ways (n = 1: three empty
# parts).  The plan groups nothing: one workgroup per molecule, atom or edge row, so the batch-size boundaries are those of the row GEMMs.
EDGE_CASES = {
    'B=1': [13],
    'n=1 alone (no pairs)': [1],
    'n=2': [2, 2],
    'one fills N, the rest single atoms': [29, 1, 1, 1],
    'n=16|17 (kc_rw pass boundary)': [16, 17],
    'Nn=32, R=128 (tile boundaries)': [4] * 8,
    'Nn=33 (one atom above a tile)': [4] * 7 + [5],
    'Nn=64, R=512 (strip boundaries)': [8] * 8,
    'Nn=65 (one atom above a strip)': [8] * 7 + [9],
}


@pytest.mark.parametrize('case', sorted(EDGE_CASES))
def test_size_edges(case):
    cfg, model = shared_model('qm9')
    check64(cfg, model, EDGE_CASES[case], 41, case)


@pytest.mark.parametrize('B', [63, 64, 65])
def test_batch_sizes_around_a_gemm_strip(B):
    cfg, model = shared_model('qm9')
    check64(cfg, model, [1 + (b % 3) for b in range(B)], 43, 'B=%d' % B)


def test_adjacency_edges():
    """Existence channel negative everywhere (empty adjacency, degree 0), non-negative everywhere (complete), and exact 0.0 entries
    (which count as edges), one molecule each plus a random one."""
    cfg, model = shared_model('qm9')

    def edit(ex):
        ex = ex.clone()
        ex[0, ..., 0] = -ex[0, ..., 0].abs() - 0.1
        ex[1, ..., 0] = ex[1, ..., 0].abs()
        ex[2, ..., 0] = torch.where(ex[2, ..., 0] > 0.3, torch.zeros(()), -ex[2, ..., 0].abs() - 0.1)
        return ex

    got, _ = check64(cfg, model, [7, 6, 9, 5], 47, 'adjacency edges', edit=edit)
    code, land = model.debug_rw()
    assert int(code[:49].min()) == cfg.model.rw_depth and float(land[:7].abs().max()) == 0.0       # no walks at all
    assert int(code[49:49 + 36].reshape(6, 6)[0, 1]) == 0                                          # complete graph: every power has a walk
    t, x, ex, nm, em = inputs(cfg, [7, 6, 9, 5], 47)
    z = edit(ex)[2, :9, :9, 0]
    assert int(((z == 0) & ~torch.eye(9, dtype=torch.bool)).sum()) >= 2                             # the zeros are there


def test_geom_config_at_max_node():
    cfg, model = shared_model('geom')
    check64(cfg, model, [181, 5], 53, 'GEOM [181, 5]')


# ---- 4. random-walk features alone ---------------------------------------------------------------------------------------------------------
def _graph_batch(graphs, ch):
    N = max(n for n, _ in graphs)
    ex = -torch.ones(len(graphs), N, N, ch)
    for b, (n, edges) in enumerate(graphs):
        for i, j in edges:
            ex[b, i, j, 0] = ex[b, j, i, 0] = 1.0
    return ex


def test_random_walk_features():
    cfg, model = shared_model('geom')                       # rw_depth 16
    chain = (20, [(i, i + 1) for i in range(19)])
    ring7, ring8 = (7, [(i, (i + 1) % 7) for i in range(7)]), (8, [(i, (i + 1) % 8) for i in range(8)])
    two = (9, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)])
    full = (6, [(i, j) for i in range(6) for j in range(i + 1, 6)])
    graphs = [chain, ring7, ring8, two, full]
    n_nodes = [g[0] for g in graphs]
    B, N = len(graphs), max(n_nodes)
    nm, em = S.build_masks(n_nodes, N, 'cpu')
    ex = _graph_batch(graphs, cfg.model.edge_ch) * em.reshape(B, N, N, 1)
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(B, N, cfg.data.atom_types, generator=g) * nm, torch.rand(B, generator=g)
    try:
        model.max_blocks = 0
        call(model, t, x, ex, nm, em)
        code, land = model.debug_rw()
    finally:
        model.max_blocks = -1
    adj = (ex[..., 0] >= 0).float() * em.reshape(B, N, N)
    want_land, want_code = OC.rw_features(cfg.model.rw_depth, adj)
    code, land, no, eo = code.cpu(), land.cpu(), 0, 0
    for b, n in enumerate(n_nodes):
        assert torch.equal(code[eo:eo + n * n].reshape(n, n).long(), want_code[b, :n, :n]), 'distance code of graph %d' % b
        assert float((land[no:no + n] - want_land[b, :n]).abs().max()) <= 1e-6
        no += n
        eo += n * n
    # the chain is bipartite: the code is the count of empty powers, not the breadth-first distance
    c = code[:400].reshape(20, 20)
    assert int(c[0, 1]) == 8 and int(c[0, 2]) == 8 and int(c[0, 19]) == 16 and int(c[0, 17]) == 15
    assert int(want_code[3, 0, 3]) == 16 and int(want_code[4, 0, 1]) == 0          # other component: never; complete graph: always


# ---- 5. asymmetric inputs: the directed walk -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['qm9', 'geom'])
def test_asymmetric_edge_input_matches_oracle(which):
    cfg, model = shared_model(which)
    check64(cfg, model, [9, 21, 1, 2, 14], 59, which + ' asymmetric', symmetric=False)


# ---- 6. determinism and molecule order ----------------------------------------------------------------------------------------------------------
def test_bit_identical_repeat_and_molecule_permutation():
    cfg, model = shared_model('qm9')
    n_nodes = [11, 29, 1, 2, 23, 17]
    t, x, ex, nm, em = inputs(cfg, n_nodes, 61)
    a = call(model, t, x, ex, nm, em)
    b = call(model, t, x, ex, nm, em)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    perm = torch.tensor([4, 0, 5, 1, 3, 2])
    p = call(model, t[perm], x[perm], ex[perm], nm[perm], em.reshape(6, -1)[perm].reshape(-1, 1))
    fwd_close(p[0], a[0].cpu()[perm], 'permuted molecules x')
    fwd_close(p[1], a[1].cpu()[perm], 'permuted molecules e')


# ---- 7. weight updates reach the kernels ------------------------------------------------------------------------------------------------------
def test_weight_updates_reach_the_kernels():
    cfg = make_config(CFG['qm9'])
    model = make_model(cfg, 7)
    n_nodes = [7, 12, 3]
    t, x, ex, nm, em = inputs(cfg, n_nodes, 67)
    d = lambda v: v.to(DEV)
    nmd, emd = d(nm), d(em)

    def check(tag, masks_=None):
        m_ = masks_ or (nmd, emd)
        with torch.no_grad():
            got = model(d(t), d(x), m_[0], m_[1], edge_x=d(ex))
        r32, r64 = oracle_32_64(cfg, model, t, x, ex, nm, em)
        close64(got[0], r32[0], r64[0], tag + ' x')
        close64(got[1], r32[1], r64[1], tag + ' e')
        return got

    base = check('initial weights')
    blk = model.all_modules[10 + 3 * 2]
    with torch.no_grad():
        blk.self_attn.lin_edge1.weight.mul_(1.5)             # in place: bumps the version counter
        blk.norm2_edge.weight.mul_(1.3)
    upd = check('after an in-place update')
    assert float((upd[0] - base[0]).abs().max()) > 1e-4
    with torch.no_grad():
        blk.local_model.eps.fill_(0.7)                       # the GINE buffer is part of the packed weights
    upd1 = check('after an eps update')
    assert float((upd1[0] - upd[0]).abs().max()) > 1e-5
    with torch.no_grad():
        model.all_modules[-1].weight.data.mul_(3.0)          # `.data`: no version bump; the fingerprint of a new batch catches it
    upd2 = check('after .data.mul_ seen by a new batch', (d(nm.clone()), d(em.clone())))
    assert float((upd2[1] - upd1[1]).abs().max()) > 1e-4
    with torch.no_grad():
        model.all_modules[0].bias.data.add_(0.5)
    model.invalidate_packed_weights()
    upd3 = check('after .data.add_ + invalidate_packed_weights')
    assert float((upd3[0] - upd2[0]).abs().max()) > 1e-5
    fresh = deterministic_init_(get_model_class('CDGS')(cfg), seed=19)
    model.load_state_dict(fresh.state_dict())
    upd4 = check('after load_state_dict')
    assert float((upd4[0] - upd3[0]).abs().max()) > 1e-4


# ---- 8. sampling -------------------------------------------------------------------------------------------------------------------------------
def _replay(fx):
    return lambda i, kind, like: torch.from_numpy(fx['node_noise' if kind == 'node' else 'edge_noise'][i]).to(like.device)


def _scheduler(cfg):
    return NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)


def test_trajectory_free_running_and_teacher_forced():
    fx = load_fixture('traj_cdgs_qm9_anc5.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain']))
    ns, steps, n_nodes = _scheduler(cfg), int(fx['steps']), fx['n_nodes'].tolist()
    nm, em = S.build_masks(n_nodes, max(n_nodes), DEV)
    assert cfg.model.pred_data is False and cfg.model.self_cond is False                # the eager noise-prediction branch
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond, noise_fn=_replay(fx))
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    ex_, ee_ = (x_mean.cpu() - torch.from_numpy(fx['x_mean'])).abs().max().item(), (e_mean.cpu() - torch.from_numpy(fx['edge_x_mean'])).abs().max().item()
    print('free-running end state: max |err|', ex_, ee_)
    assert ex_ <= 1e-3 and ee_ <= 1e-3
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_mean.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_mean.clone(), em,
                                        cfg.data.compress_edge)
    bad, excluded = O2.decode_agrees(fx, one_hot.argmax(2).cpu().numpy(), fc.cpu().numpy(), et.cpu().numpy(), n_nodes)
    print('decodes: mismatches', bad, 'excluded share', excluded)
    assert bad == 0
    assert excluded <= float(fx['margin_cap']) and float(fx['margin_shares'].max()) <= float(fx['margin_cap']) == 0.05
    for i in range(steps):
        t = lambda k: torch.from_numpy(fx[k][i])
        got = call(model, t('step_t'), t('step_x'), t('step_edge_x'), nm.cpu(), em.cpu())
        fwd_close(got[0], t('step_pred_x'), 'teacher-forced step %d x' % i)
        fwd_close(got[1], t('step_pred_e'), 'teacher-forced step %d e' % i)


def _samplefn_setup():
    fx = load_fixture('samplefn_cdgs_qm9.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.device = torch.device(DEV)
    cfg.sampling.steps = int(fx['steps'])
    model = mutils.create_model(cfg, wrap='dataparallel')    # the reference's wrapper, over the one device
    deterministic_init_(model.module, seed=int(fx['model_seed']))
    with torch.no_grad():
        sd = model.module.state_dict()
        for k in head_keys(cfg.model.n_layers):
            sd[k].mul_(float(fx['head_gain']))
    model.module.invalidate_packed_weights()
    return fx, cfg, model, _scheduler(cfg), get_node_dist(load_dataset_info(cfg.data.info_name))


def _same_mols(a, b):
    return len(a) == len(b) and all(m[0] is None and w[0] is None and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(m[1:], w[1:]))
                                    for m, w in zip(a, b))


def test_sampling_fn_reproduces_reference_run_and_parity_shards_partition_it():
    fx, cfg, model, ns, dist = _samplefn_setup()
    batch, seed = int(fx['batch']), int(fx['seed'])
    inv = get_data_inverse_scaler(cfg)
    fn = S.get_sampling_fn(cfg, ns, dist, batch, batch, inv, return_raw=True, cpu_noise=True)
    torch.manual_seed(seed)
    random.seed(seed)
    mols = fn(model)
    assert [int(m[1].shape[0]) for m in mols] == fx['n_nodes'].tolist()
    at, fc, et = np.zeros_like(fx['atom_type']), np.zeros_like(fx['fc']), np.zeros_like(fx['edge_type'])
    for b, (pos, a, e, q) in enumerate(mols):
        n = a.shape[0]
        assert pos is None
        at[b, :n], et[b, :n, :n] = a.numpy(), e.numpy()
    bad, excluded = O2.decode_agrees(fx, at, fc, et, fx['n_nodes'].tolist())
    print('samplefn_cdgs: mismatches', bad, 'excluded share', excluded)
    assert bad == 0 and excluded <= 0.05
    # two parity shards together are the unsharded run, molecule for molecule (each share padded to the round's width: this model's
    # scores depend on it)
    parts, idx = [], []
    for rank in (0, 1):
        sh = S.get_sampling_fn(cfg, ns, dist, batch, batch, inv, shard=(rank, 2), shard_mode='parity', seed=seed, return_raw=True)
        parts += sh(model)
        idx += sh.last_indices
        assert len(sh.last_decoded) == 1 and sh.last_decoded[0][1].is_cuda          # the device decode ran
    assert idx == list(range(batch)) and _same_mols(parts, mols)


def test_runs_under_single_device_dataparallel_and_reuses_its_plan():
    cfg = make_config(CFG['geom'])
    cfg.device = torch.device(DEV)
    model = mutils.create_model(cfg, wrap='dataparallel')
    inner = deterministic_init_(model.module, seed=3)
    t, x, ex, nm, em = inputs(cfg, [5, 9, 2], 71)
    d = lambda v: v.to(DEV)
    nmd, emd = d(nm), d(em)
    with torch.no_grad():
        model(d(t), d(x), nmd, emd, edge_x=d(ex), noise_level=d(t))
        plans = len(inner._plans)
        b = model(d(t), d(x), nmd, emd, edge_x=d(ex), noise_level=d(t))
    assert len(inner._plans) == plans == 1                   # the second call found the first one's descriptor and workspace
    r32, r64 = oracle_32_64(cfg, inner, t, x, ex, nm, em)
    close64(b[0], r32[0], r64[0], 'DataParallel x')
    close64(b[1], r32[1], r64[1], 'DataParallel e')
    with pytest.raises(RuntimeError, match='cannot be replicated'):
        inner._replicate_for_data_parallel()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    cfg, model = shared_model('qm9')
    t, x, ex, nm, em = inputs(cfg, [4, 3], 73)
    d = lambda v: v.to(DEV)
    with pytest.raises(NotImplementedError, match='inference only'):
        model(d(t), d(x), d(nm), d(em), edge_x=d(ex))                                  # grad enabled, parameters require grad
    n_nodes = [182]
    nm, em = S.build_masks(n_nodes, 182, DEV)
    with torch.no_grad(), pytest.raises(NotImplementedError, match='181'):
        model(torch.ones(1, device=DEV), torch.zeros(1, 182, 5, device=DEV), nm, em, edge_x=torch.zeros(1, 182, 182, 2, device=DEV))
    cfg2 = make_config(CFG['qm9'])
    cfg2.device = torch.device(DEV)
    cfg2.sampling.steps = 3
    fn = S.get_sampling_fn(cfg2, _scheduler(cfg2), get_node_dist(load_dataset_info(cfg2.data.info_name)), 4, 4, get_data_inverse_scaler(cfg2),
                           hip_graph=True, return_raw=True)
    with pytest.raises(NotImplementedError, match='graph replay'):
        fn(model)
    try:
        model.split_bf16 = True
        with torch.no_grad(), pytest.raises(NotImplementedError, match='split_bf16'):
            call(model, t, x, ex, *S.build_masks([4, 3], 4, 'cpu'))
    finally:
        model.split_bf16 = False

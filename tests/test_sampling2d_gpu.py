"""GPU: the production form of a 2-D sampling round — in-kernel noise (jodo_sampler_step_2d_rng against the numpy restatement of
the generator, oracle/philox_ref.py), graph replay (GraphedAncestralRound2D against the update formula on its own recorded tensors and
against an eager device-noise round, bit for bit), the device decode (jodo_decode_2d against post_process_2D), and the public
sampling function's options on a GPU device.

Tolerances: the in-kernel draws against the restatement at the project's Philox tolerance atol 2e-5 + rtol 1e-5 (float32 log / sincos of
the device against numpy's float64 ones, as tests/test_callers_gpu.py uses for the 3-D kernel); the mean c_x x + c_pred pred at atol 1e-6
(two rounded products and one sum of O(1) values, as test_sampler_step_2d_kernel_matches_torch)."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from jodo_amd import capi, fused
from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.graphed import GraphedAncestralRound2D
from jodo_amd.models import get_node_dist
from jodo_amd.models import utils as mutils
from jodo_amd.utils import get_data_inverse_scaler
from helpers import load_fixture, make_config, make_model, masks, GOLDEN
from oracle import philox_ref as PR
import oracle2d as O2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PH_ATOL, PH_RTOL = 2e-5, 1e-5
CFG = {'zinc': 'vpsde_zinc_2d_jodo', 'moses': 'vpsde_moses_2d_jodo'}
d = lambda v: v.to(DEV)


def ph_close(got, want, what):
    got, want = got.detach().cpu().double(), torch.as_tensor(want).double()
    err = (got - want).abs()
    bound = PH_ATOL + PH_RTOL * want.abs()
    print('%s: max |err| %.3e, worst err / bound %.3f' % (what, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all()), what


def step_rng(n_nodes, c_x, c_pred, sigma, seed, draw, x, e, pred, epred, table_step=None):
    """jodo_sampler_step_2d_rng through the C ABI; table_step = s: the table form with the coefficients in row s of a device table
    and `draw` handed over as draw - s."""
    B, N, nd = x.shape
    ch = e.shape[-1]
    nn = d(torch.tensor(n_nodes, dtype=torch.int32))
    out = [torch.full_like(x, float('nan')), torch.full_like(e, float('nan')), torch.full_like(x, float('nan')), torch.full_like(e, float('nan'))]
    tab = step = None
    if table_step is not None:
        tab = torch.full((table_step + 2, 4), float('nan'))
        tab[table_step] = torch.tensor([c_x, c_pred, sigma, 0.0])
        tab, step = d(tab), d(torch.tensor([table_step], dtype=torch.int32))
        c_x = c_pred = sigma = 0.0
        draw -= table_step
    capi.check(capi.lib().jodo_sampler_step_2d_rng(B, N, nd, ch, capi.ptr(nn), c_x, c_pred, sigma, capi.ptr(tab), capi.ptr(step), seed, draw,
                                                   capi.ptr(x), capi.ptr(e), capi.ptr(pred), capi.ptr(epred), *[capi.ptr(t) for t in out],
                                                   capi.current_stream_ptr()), 'jodo_sampler_step_2d_rng')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('n_nodes,nd,ch', [([1, 4, 9], 10, 2), ([38, 2, 27], 7, 3)])
def test_in_kernel_noise_is_the_philox_restatement(n_nodes, nd, ch):
    B, N = len(n_nodes), max(n_nodes)
    seed, draw = 0x1234567890ABCDEF, 11
    x, e = torch.zeros(B, N, nd, device=DEV), torch.zeros(B, N, N, ch, device=DEV)
    xn, en, xm, em_ = step_rng(n_nodes, 0.0, 0.0, 1.0, seed, draw, x, e, x, e)
    ph_close(xn, PR.node_noise(seed, draw, n_nodes, N, nd)[..., 3:], 'node noise')
    ph_close(en, PR.edge_noise(seed, draw, n_nodes, N, ch), 'edge noise')
    assert float(xm.abs().max()) == 0.0 and float(em_.abs().max()) == 0.0
    assert torch.equal(en, en.transpose(1, 2))
    nm, em = masks(n_nodes)
    assert float((xn.cpu() * (1 - nm)).abs().max()) == 0.0                                   # padding, and the diagonal with it
    assert float((en.cpu() * (1 - em.reshape(B, N, N, 1))).abs().max()) == 0.0
    assert float(xn.cpu()[nm.expand_as(xn) > 0].abs().min()) > 0.0                           # every real entry drew something
    tab = step_rng(n_nodes, 0.0, 0.0, 1.0, seed, draw, x, e, x, e, table_step=3)
    for a, b in zip(tab, (xn, en, xm, em_)):
        assert torch.equal(a, b)
    other = step_rng(n_nodes, 0.0, 0.0, 1.0, seed, draw + 1, x, e, x, e)
    assert not torch.equal(other[1], en) and not torch.equal(other[0], xn)


def test_update_arithmetic_with_in_kernel_noise():
    g = torch.Generator().manual_seed(2)                     # the state and predictions of test_sampler_step_2d_kernel_matches_torch
    n_nodes = [4, 9, 1]
    B, N, nd, ch = 3, 9, 10, 2
    nm, em = masks(n_nodes)
    x, pred = torch.randn(B, N, nd, generator=g) * nm, torch.randn(B, N, nd, generator=g) * nm
    emd = em.reshape(B, N, N, 1)
    sym = lambda v: (torch.tril(v.permute(0, 3, 1, 2), -1) + torch.tril(v.permute(0, 3, 1, 2), -1).transpose(-1, -2)).permute(0, 2, 3, 1) * emd
    e, epred = sym(torch.randn(B, N, N, ch, generator=g)).contiguous(), sym(torch.randn(B, N, N, ch, generator=g)).contiguous()
    seed, draw = 99, 4
    xn, en, xm, emn = step_rng(n_nodes, 0.9, 0.2, 0.3, seed, draw, d(x), d(e), d(pred), d(epred))
    assert torch.allclose(xm.cpu(), 0.9 * x + 0.2 * pred, atol=1e-6) and torch.allclose(emn.cpu(), 0.9 * e + 0.2 * epred, atol=1e-6)
    ph_close(xn - xm, 0.3 * PR.node_noise(seed, draw, n_nodes, N, nd)[..., 3:], 'x_next - x_mean')
    ph_close(en - emn, 0.3 * PR.edge_noise(seed, draw, n_nodes, N, ch), 'edge_next - edge_mean')
    tab = step_rng(n_nodes, 0.9, 0.2, 0.3, seed, draw, d(x), d(e), d(pred), d(epred), table_step=1)
    for a, b in zip(tab, (xn, en, xm, emn)):
        assert torch.equal(a, b)
    # the fused wrapper on ping-pong buffers: same values, the draw counter moves by one
    bufs, rng = fused.StepBuffers(d(x), d(e)), fused.DeviceNoise(seed, draw)
    got = fused.sampler_step_2d_rng(bufs, d(torch.tensor(n_nodes, dtype=torch.int32)), 0.9, 0.2, 0.3, d(x), d(e), d(pred), d(epred), rng)
    assert rng.draw == draw + 1 and all(torch.equal(a, b) for a, b in zip(got, (xn, en, xm, emn)))


def _round_setup(which, n_nodes, steps, seed=21):
    cfg = make_config(CFG[which])
    model = make_model(cfg, 7, DEV, head_gain=8.0)                 # the trajectory fixtures' gain: predictions of O(1)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    g = torch.Generator().manual_seed(seed)
    z = mutils.sample_gaussian_with_mask((B, N, nd), 'cpu', nm, generator=g)
    ez = mutils.sample_symmetric_edge_feature_noise(B, N, ch, em, generator=g).contiguous()
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond)
    return cfg, model, sampler, d(z), d(ez), d(nm), d(em)


def _eager_round(sampler, model, z, ez, nm, em, key):
    sampler.device_noise = fused.DeviceNoise.for_rank(*key)
    try:
        with torch.no_grad():
            xm, emn = sampler.sampling(model, z, nm, em, ez, None)
        return xm.clone(), emn.clone(), sampler.device_noise.draw
    finally:
        sampler.device_noise = None


def test_eager_sampler_with_device_noise():
    cfg, model, sampler, z, ez, nm, em = _round_setup('zinc', [1, 5, 9], 3)
    a = _eager_round(sampler, model, z, ez, nm, em, (5, 0, 0))
    b = _eager_round(sampler, model, z, ez, nm, em, (5, 0, 0))
    c = _eager_round(sampler, model, z, ez, nm, em, (5, 0, 1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    assert a[2] == 3                                         # one draw index per step
    assert bool(torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all())
    # noise_fn wins over device_noise: replayed zeros leave the draw counter alone
    sampler.device_noise = fused.DeviceNoise(1)
    sampler.noise_fn = lambda i, kind, like: torch.zeros_like(like)
    try:
        with torch.no_grad():
            sampler.sampling(model, z, nm, em, ez, None)
        assert sampler.device_noise.draw == 0
    finally:
        sampler.noise_fn = sampler.device_noise = None


@pytest.mark.parametrize('which,n_nodes', [('zinc', [1, 5, 9, 33, 2]), ('moses', [3, 27])])
def test_graph_replay_equals_the_eager_device_noise_round(which, n_nodes):
    steps, key = 5, (13, 2, 4)
    cfg, model, sampler, z, ez, nm, em = _round_setup(which, n_nodes, steps)
    want_x, want_e, _ = _eager_round(sampler, model, z, ez, nm, em, key)
    sampler.device_noise = fused.DeviceNoise.for_rank(*key)
    try:
        with torch.no_grad():
            rnd = GraphedAncestralRound2D(sampler, model, nm, em, record=True)
            got_x, got_e = rnd.run(z, ez)
        torch.cuda.synchronize()
        assert sampler.device_noise.draw == steps and rnd.rng_base == 0
    finally:
        sampler.device_noise = None
    assert rnd.graph is not None and [h['step'] for h in rnd.history] == [1, 2, 3, 4]      # the warm-up step, then three replays
    N, nd, ch = max(n_nodes), z.shape[-1], ez.shape[-1]
    for h in rnd.history:
        i = h['step']
        c_x, c_pred, sigma = (float(v) for v in S.posterior_coefficients(sampler.noise_scheduler, sampler.t_array[i], sampler.s_array[i])[:3])
        c_x, c_pred, sigma = (torch.tensor(v, dtype=torch.float32) for v in (c_x, c_pred, sigma))
        assert torch.allclose(h['x_mean'].cpu(), c_x * h['x_prev'].cpu() + c_pred * h['pred'].cpu(), atol=1e-6)
        assert torch.allclose(h['e_mean'].cpu(), c_x * h['e_prev'].cpu() + c_pred * h['epred'].cpu(), atol=1e-6)
        draw = rnd.rng_base + i
        ph_close(h['x'] - h['x_mean'], float(sigma) * PR.node_noise(sampler_seed(key), draw, n_nodes, N, nd)[..., 3:], '%s step %d node' % (which, i))
        ph_close(h['e'] - h['e_mean'], float(sigma) * PR.edge_noise(sampler_seed(key), draw, n_nodes, N, ch), '%s step %d edge' % (which, i))
        assert torch.equal(h['e'], h['e'].transpose(1, 2))
    assert torch.equal(got_x, want_x) and torch.equal(got_e, want_e)


def sampler_seed(key):
    return fused.DeviceNoise.for_rank(*key).seed


def _decode_inputs(cfg, n_nodes, seed):
    """Random inputs over every bucket of the bond rule and both aromatic outcomes, with exact ties between atom channels and values
    exactly on the decision thresholds: with the configs' normalisation (atom / edge factors 2 and 1, centred) the inverse scaler maps
    x to (2 x + 1) / 2 resp. (x + 1) / 2, exactly in float32 for the small dyadic values used here — 0 lands on 0.5 (bond exists,
    aromatic, order bucket 1.5).  The order thresholds of 3 * ch1 are visited at the nearest float32 input and its two neighbours:
    that hits 1.5 and 2.5 exactly; no float32 input lands on 0.5 (h = (x + 1) / 2 moves in steps of 2^-25 there and 3 h steps over it:
    16777215 2^-25, then 16777218 2^-25), so that threshold is visited from both sides one step apart."""
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), max(n_nodes)
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    xh = torch.randn(B, N, nd, generator=g) * 0.5
    xh[:, ::3, 2] = xh[:, ::3, 5] = 2.0                      # exact tie of two maxima: the first one wins
    xh[:, 1::4, :cfg.data.atom_types] = 0.25                 # all channels equal
    if cfg.model.include_fc_charge:
        xh[:, :, -1] = torch.tensor([0.25, -0.25, 0.75, 0.0, 0.26, -0.74])[torch.randint(0, 6, (B, N), generator=g)]     # 2 x = +-0.5, 1.5: ties of rint
    ex = torch.rand(B, N, N, ch, generator=g) * 2.4 - 1.2    # (x + 1) / 2 in [-0.1, 1.1]
    pick = torch.randint(0, 12, (B, N, N), generator=g)
    ex[..., 0][pick == 0] = 0.0                              # exist exactly on its threshold
    th = []
    for o in (0.5, 1.5, 2.5):                                # x with 3 * ((x + 1) / 2) around o: the nearest float32 and its neighbours
        x0 = np.float32(2.0 * o / 3.0 - 1.0)
        th += [float(np.nextafter(x0, np.float32(-2))), float(x0), float(np.nextafter(x0, np.float32(2)))]
    th = torch.tensor(th)
    sel = pick >= 6
    ex[..., 1][sel] = th[torch.randint(0, 9, (int(sel.sum()),), generator=g)]
    ex[..., 0][pick == 11] = 0.9                             # those certainly exist
    if ch == 3:
        ex[..., 2][pick % 3 == 0] = 0.0                      # aromatic exactly on its threshold
        ex[..., 1][pick == 7] = -0.9                         # no order assigned: the aromatic channel decides
    ex = torch.tril(ex.permute(0, 3, 1, 2), -1)
    ex = (ex + ex.transpose(-1, -2)).permute(0, 2, 3, 1).contiguous()
    return xh, ex


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_device_decode_2d_matches_post_process_2d(which):
    cfg = make_config(CFG[which])
    n_nodes = [38, 1, 2, 17, 27, 9, 30]
    if which == 'moses':
        n_nodes = [min(n, cfg.data.max_node) for n in n_nodes]
    B, N = len(n_nodes), max(n_nodes)
    xh, ex = _decode_inputs(cfg, n_nodes, 31)
    nm, em = masks(n_nodes)
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(xh.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, ex.clone(), em, cfg.data.compress_edge)
    want_at, want_et = (one_hot.argmax(2) * nm[..., 0].long()), et
    at, q, bt = fused.decode_2d(cfg, d(xh), d(ex), d(torch.tensor(n_nodes, dtype=torch.int32)))
    assert at.dtype == torch.uint8 and q.dtype == torch.int8 and bt.dtype == torch.uint8
    assert torch.equal(at.cpu().long(), want_at) and torch.equal(bt.cpu().float(), want_et)
    if cfg.model.include_fc_charge:
        assert torch.equal(q.cpu().long(), fc[..., 0].long())
        assert len(torch.unique(fc)) >= 3
    else:
        assert float(q.abs().max()) == 0 and fc.shape[-1] == 0
    # the inputs did visit every outcome, and padding is zero
    kinds = set(torch.unique(want_et).tolist())
    assert kinds == ({0., 1., 2., 3., 4.} if cfg.model.edge_ch == 3 else {0., 1., 2., 3.})
    if cfg.model.edge_ch == 3:
        hv = (ex[..., 2] + 1) / 2
        real = em.reshape(B, N, N) > 0
        assert bool(((want_et == 0) & (hv >= 0.5) & real).any()) and bool(((want_et == 4) & real).any()) and bool(((hv < 0.5) & (want_et == 0) & real).any())
    assert len(torch.unique(want_at)) >= 3
    assert float((at.cpu() * (1 - nm[..., 0])).abs().max()) == 0 and float((q.cpu() * (1 - nm[..., 0])).abs().max()) == 0
    assert float((bt.cpu() * (1 - em.reshape(B, N, N))).abs().max()) == 0
    # per-molecule tuples in mol_process_2D's format
    mols = fused.mols_from_decoded_2d(at, q, bt, n_nodes, include_fc=cfg.model.include_fc_charge)
    want = S.mol_process_2D(one_hot, fc, n_nodes, et)
    for m, w in zip(mols, want):
        assert m[0] is None and w[0] is None
        assert all(a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) for a, b in zip(m[1:], w[1:]))


def _samplefn_setup(wrap='dataparallel'):
    fx = load_fixture('samplefn2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.device = torch.device(DEV)
    cfg.sampling.steps = int(fx['steps'])
    model = mutils.create_model(cfg, wrap=wrap)
    from jodo_amd.models import deterministic_init_
    deterministic_init_(model.module, seed=int(fx['model_seed']))
    with torch.no_grad():
        sd = model.module.state_dict()
        for k in ('node_pred_mlp.4.weight', 'edge_type_mlp.4.weight', 'edge_exist_mlp.4.weight'):
            sd[k].mul_(float(fx['head_gain']))
    model.module.invalidate_packed_weights()
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    dist = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k'))
    return fx, cfg, model, ns, dist


def _same_mols(a, b):
    return len(a) == len(b) and all(m[0] is None and w[0] is None and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(m[1:], w[1:]))
                                    for m, w in zip(a, b))


def test_public_entry_parity_shard_on_gpu_reproduces_reference_run():
    fx, cfg, model, ns, dist = _samplefn_setup()
    batch, seed = int(fx['batch']), int(fx['seed'])
    inv = get_data_inverse_scaler(cfg)
    fn = S.get_sampling_fn(cfg, ns, dist, batch, batch, inv, shard=(0, 1), shard_mode='parity', seed=seed, return_raw=True)
    random.seed(seed)
    mols = fn(model)
    assert fn.last_indices == list(range(batch))
    assert [int(m[1].shape[0]) for m in mols] == fx['n_nodes'].tolist()
    at, fc, et = np.zeros_like(fx['atom_type']), np.zeros_like(fx['fc']), np.zeros_like(fx['edge_type'])
    for b, (pos, a, e, q) in enumerate(mols):
        n = a.shape[0]
        assert pos is None
        at[b, :n], et[b, :n, :n], fc[b, :n, 0] = a.numpy(), e.numpy(), q.numpy()
    bad, excluded = O2.decode_agrees(fx, at, fc, et, fx['n_nodes'].tolist())
    print('samplefn2d through shard=(0, 1) parity: mismatches', bad, 'excluded share', excluded)
    assert bad == 0 and excluded <= 0.05
    assert len(fn.last_decoded) == 1 and fn.last_decoded[0][0] is None and fn.last_decoded[0][1].is_cuda
    # the unsharded run that replays the CPU draws (cpu_noise) under the same seed: the same molecules, tensor for tensor
    ref = S.get_sampling_fn(cfg, ns, dist, batch, batch, inv, return_raw=True, cpu_noise=True)
    torch.manual_seed(seed)
    random.seed(seed)
    assert _same_mols(mols, ref(model))


def test_public_entry_options_on_gpu():
    fx, cfg, model, ns, dist = _samplefn_setup('dataparallel_keys')       # the wrapper create_model gives by default
    cfg.sampling.steps = 4
    inv = get_data_inverse_scaler(cfg)
    with pytest.raises(ValueError, match='device noise'):
        S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, hip_graph=True, device_noise=False)
    with pytest.raises(NotImplementedError, match='fast'):
        cfg2 = make_config(CFG['zinc'])
        cfg2.device = torch.device(DEV)
        cfg2.sampling.method = 'fast'
        S.get_sampling_fn(cfg2, ns, dist, 5, 5, inv)
    runs = []
    for _ in range(2):
        fn = S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, hip_graph=True, seed=8, return_raw=True)
        torch.manual_seed(8)                                 # atom counts and the initial z / edge_z are torch draws
        runs.append(fn(model))
    assert len(runs[0]) == 5 and _same_mols(runs[0], runs[1])
    # eager with device noise takes the very draws of the graph round: the same molecules
    fn = S.get_sampling_fn(cfg, ns, dist, 5, 5, inv, device_noise=True, seed=8, return_raw=True)
    torch.manual_seed(8)
    assert _same_mols(fn(model), runs[0])

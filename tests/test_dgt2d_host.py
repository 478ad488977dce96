"""CPU: the 2-D model (DGT_concat_2D) — registry, parameter tree, dense oracle against the reference's fixtures, sampler and decode
against recorded trajectories, C packer against the independent Python packer, loud rejection of what is not built."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from jodo_amd import capi, configs
from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.models import get_model_class, get_node_dist, deterministic_init_
from jodo_amd.utils import get_data_inverse_scaler
from helpers import load_fixture, make_config, make_model, state_dict_cpu, masks, GOLDEN
import oracle2d as O2
import py_packing2d as P2

CFGS = ('vpsde_zinc_2d_jodo', 'vpsde_moses_2d_jodo')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_model(cfg_name, seed, head_gain=1.0):
    cfg = make_config(cfg_name)
    model = make_model(cfg, seed, head_gain=head_gain)
    return cfg, O2.OracleModel2D(state_dict_cpu(model), O2.Hyper2D.from_config(cfg))


def test_registry_and_construction():
    cls = get_model_class('DGT_concat_2D')
    for name in CFGS:
        cfg = configs.get(name)
        assert cfg.model.name == 'DGT_concat_2D' and cfg.only_2D and cfg.pred_edge
        assert cfg.eval.batch_size == 2000 and cfg.model.time_dim == 1024 and cfg.model.n_extra_heads == 1
        model = cls(cfg)
        assert sum(p.numel() for p in model.parameters()) > 21e6
    assert configs.get(CFGS[0]).data.atom_types == 9 and configs.get(CFGS[0]).model.include_fc_charge
    assert configs.get(CFGS[1]).data.atom_types == 7 and not configs.get(CFGS[1]).model.include_fc_charge
    assert configs.get(CFGS[1]).model.edge_ch == 3


def test_state_dict_matches_reference_manifest():
    man = json.load(open(os.path.join(GOLDEN, 'sd2d_manifest.json')))
    for name in CFGS:
        model = get_model_class('DGT_concat_2D')(configs.get(name))
        got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        assert len(got) == 235
        assert got == man[name]
        # a reference checkpoint (DataParallel keys stripped) loads strictly
        model.load_state_dict({k: torch.zeros(s) for k, s in man[name]}, strict=True)


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_oracle_reproduces_forward_fixture(which):
    fx = load_fixture('fwd2d_%s.npz' % which)
    assert int(fx['torch_num_threads']) == 8
    cfg, om = _oracle_model(str(fx['cfg_name']), int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    assert 1 in n_nodes and 2 in n_nodes and cfg.data.max_node in n_nodes
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k])
    o1 = om(None, t('xh'), nm, em, edge_x=t('edge_x'), cond_x=None, cond_edge_x=None, noise_level=t('noise_level'))
    o2 = om(None, t('xh'), nm, em, edge_x=t('edge_x'), cond_x=t('out1_x'), cond_edge_x=t('out1_e'), noise_level=t('noise_level'))
    for got, want in ((o1[0], 'out1_x'), (o1[1], 'out1_e'), (o2[0], 'out2_x'), (o2[1], 'out2_e')):
        err = (got - t(want)).abs().max().item()
        print(which, want, 'max err', err)
        assert err < 1e-5


def test_oracle_reproduces_block_fixture():
    fx = load_fixture('blocks2d_zinc.npz')
    cfg, om = _oracle_model(str(fx['cfg_name']), int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        _, _, blocks = O2.forward_dense(om.sd, om.hp, t('xh'), nm, em, t('edge_x'), t('cond_x'), t('cond_edge_x'), t('noise_level'),
                                        return_blocks=True)
    real, emk = nm.reshape(-1) > 0, em.reshape(B, N, N) > 0
    assert len(blocks) == 8
    for l, (h, e) in enumerate(blocks):
        eh = (h.reshape(B * N, -1)[real] - t('h')[l]).abs().max().item()
        ee = (e[emk] - t('e')[l]).abs().max().item()
        print('block', l, eh, ee)
        assert eh < 1e-5 and ee < 1e-5


@pytest.mark.reference
def test_forward_fixture_regenerates_bit_identical(tmp_path):
    from oracle.ref_import import reference_available, load_reference
    if not reference_available():
        pytest.skip("reference not present")
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_golden_2d as G
    old = G.OUT
    G.OUT = str(tmp_path)
    try:
        G.forward_fixture(load_reference(), 'zinc', [38, 1, 2, 23, 17, 9])
    finally:
        G.OUT = old
    new, fx = np.load(os.path.join(str(tmp_path), 'fwd2d_zinc.npz')), load_fixture('fwd2d_zinc.npz')
    assert sorted(new.files) == sorted(fx)
    for k in fx:
        assert np.array_equal(new[k], fx[k]), k


def _replay(fx):
    return lambda i, kind, like: torch.from_numpy(fx['node_noise' if kind == 'node' else 'edge_noise'][i])


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_sampler_2d_reproduces_trajectory_on_cpu(which):
    fx = load_fixture('traj2d_%s_anc5.npz' % which)
    cfg, om = _oracle_model(str(fx['cfg_name']), int(fx['seed']), head_gain=float(fx['head_gain']))
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    steps = int(fx['steps'])
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond, noise_fn=_replay(fx))
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    x_mean, e_mean = sampler.sampling(om, torch.from_numpy(fx['z']), nm, em, torch.from_numpy(fx['edge_z']), None)
    ex, ee = (x_mean - torch.from_numpy(fx['x_mean'])).abs().max().item(), (e_mean - torch.from_numpy(fx['edge_x_mean'])).abs().max().item()
    print(which, 'end state err', ex, ee)
    assert ex < 1e-3 and ee < 1e-3
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_mean.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_mean.clone(), em,
                                        cfg.data.compress_edge)
    bad, excluded = O2.decode_agrees(fx, one_hot.argmax(2).numpy(), fc.numpy(), et.numpy(), n_nodes)
    assert bad == 0 and excluded <= float(fx['margin_cap'])
    assert float(fx['margin_shares'].max()) <= 0.05


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_post_process_2d_reproduces_recorded_decodes(which):
    fx = load_fixture('traj2d_%s_anc5.npz' % which)
    cfg = make_config(str(fx['cfg_name']))
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(torch.from_numpy(fx['x_mean']).clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv,
                                        torch.from_numpy(fx['edge_x_mean']).clone(), em, cfg.data.compress_edge)
    assert np.array_equal(one_hot.argmax(2).numpy(), fx['atom_type'])
    assert np.array_equal(fc.numpy(), fx['fc']) and np.array_equal(et.numpy(), fx['edge_type'])
    assert len(np.unique(fx['atom_type'][nm[..., 0].numpy() > 0])) >= 2 and len(np.unique(fx['edge_type'])) >= 2
    mols = S.mol_process_2D(one_hot, fc, n_nodes, et)
    assert len(mols) == len(n_nodes)
    for (pos, at, bt, q), n, b in zip(mols, n_nodes, range(len(n_nodes))):
        assert pos is None and at.shape == (n,) and bt.shape == (n, n) and tuple(q.shape) == ((n,) if cfg.model.include_fc_charge else (n, 0))
        assert np.array_equal(at.numpy(), fx['atom_type'][b, :n]) and np.array_equal(bt.numpy(), fx['edge_type'][b, :n, :n])


def test_sampling_fn_2d_reproduces_reference_run():
    fx = load_fixture('samplefn2d_zinc.npz')
    cfg, om = _oracle_model(str(fx['cfg_name']), int(fx['model_seed']), head_gain=float(fx['head_gain']))
    cfg.device = torch.device('cpu')
    cfg.sampling.steps = int(fx['steps'])
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    dist = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k'))
    batch = int(fx['batch'])
    fn = S.get_sampling_fn(cfg, ns, dist, batch, batch, get_data_inverse_scaler(cfg), return_raw=True)
    torch.manual_seed(int(fx['seed']))
    random.seed(int(fx['seed']))
    mols = fn(om)
    assert [int(m[1].shape[0]) for m in mols] == fx['n_nodes'].tolist()
    N = fx['atom_type'].shape[1]
    at, fc, et = np.zeros_like(fx['atom_type']), np.zeros_like(fx['fc']), np.zeros_like(fx['edge_type'])
    for b, (pos, a, e, q) in enumerate(mols):
        n = a.shape[0]
        assert pos is None
        at[b, :n], et[b, :n, :n], fc[b, :n, 0] = a.numpy(), e.numpy(), q.numpy()
    bad, excluded = O2.decode_agrees(fx, at, fc, et, fx['n_nodes'].tolist())
    assert bad == 0 and excluded <= 0.05
    # the shuffled form returns the same molecules in the order of random.shuffle
    torch.manual_seed(int(fx['seed']))
    random.seed(int(fx['seed']))
    fn2 = S.get_sampling_fn(cfg, ns, dist, batch, batch, get_data_inverse_scaler(cfg))
    shuffled = fn2(om)
    order = list(range(batch))
    random.seed(int(fx['seed']))
    random.shuffle(order)
    assert [int(m[1].shape[0]) for m in shuffled] == [int(mols[i][1].shape[0]) for i in order]


def test_sampling_fn_2d_rejects_what_is_not_built():
    cfg = make_config(CFGS[0])
    cfg.device = torch.device('cpu')
    ns = NoiseScheduleVP('cosine')
    dist = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k'))
    inv = get_data_inverse_scaler(cfg)
    for kw in (dict(shard=(0, 2)), dict(hip_graph=True), dict(device_noise=True)):
        with pytest.raises(NotImplementedError):
            S.get_sampling_fn(cfg, ns, dist, 4, 4, inv, **kw)
    cfg.sampling.method = 'fast'
    with pytest.raises(NotImplementedError):
        S.get_sampling_fn(cfg, ns, dist, 4, 4, inv)
    cfg = make_config(CFGS[0])
    cfg.pred_edge = False
    with pytest.raises(NotImplementedError):
        S.get_sampling_fn(cfg, ns, dist, 4, 4, inv)
    cfg3 = make_config('vpsde_qm9_uncond_jodo')
    with pytest.raises(ValueError):
        S.get_sampling_fn(cfg3, ns, dist, 4, 4, inv, cpu_noise=True)


def _header_enum(name):
    import re
    text = open(os.path.join(ROOT, 'include', 'jodo_hip.h')).read()
    m = re.search(r'enum %s \{(.*?)\};' % name, text, re.S)
    return [t.strip().split('=')[0].strip() for t in m.group(1).replace('\n', ' ').split(',') if t.strip()]


def test_slot_enums_match_python_packer_2d():
    g, b = _header_enum('jodo2d_wslot_global'), _header_enum('jodo2d_wslot_block')
    assert g[-1] == 'J2_GLOBAL_COUNT' and b[-1] == 'J2B_BLOCK_COUNT'
    assert [n[3:] for n in g[:-1]] == P2.GLOBAL_SLOTS and [n[4:] for n in b[:-1]] == P2.BLOCK_SLOTS


@pytest.mark.parametrize('name', CFGS)
def test_c_packer_matches_python_packer(name):
    cfg = make_config(name)
    model = make_model(cfg, seed=11)
    sd = state_dict_cpu(model)
    blob, woff, n_woff = capi.pack_weights_2d(model._cfg_struct, {'module.' + k: v for k, v in sd.items()})     # DataParallel keys accepted
    want, want_off = P2.pack({k: v.numpy() for k, v in sd.items()}, cfg.model.nf, cfg.model.n_layers, model.in_node_dim, cfg.model.edge_ch)
    assert n_woff == len(P2.GLOBAL_SLOTS) + cfg.model.n_layers * len(P2.BLOCK_SLOTS) == len(want_off)
    assert list(woff) == want_off
    assert blob.numel() == want.size
    assert np.array_equal(blob.numpy(), want)


def test_c_packer_names_missing_and_missized_tensors():
    cfg = make_config(CFGS[0])
    model = make_model(cfg, seed=11)
    sd = state_dict_cpu(model)
    miss = {k: v for k, v in sd.items() if k != 'e_block_3.attn_mpnn.lin_edge0.weight'}
    with pytest.raises(capi.JodoHipError, match=r'\(-1\).*e_block_3\.attn_mpnn\.lin_edge0\.weight'):
        capi.pack_weights_2d(model._cfg_struct, miss)
    bad = dict(sd)
    bad['node_5.bias'] = torch.zeros(63)
    with pytest.raises(capi.JodoHipError, match=r'\(-1\).*node_5\.bias'):
        capi.pack_weights_2d(model._cfg_struct, bad)
    # the C side refuses unsupported settings by itself
    from jodo_amd.models.dgt2d import _Cfg2D
    for c in (_Cfg2D(128, 8, 16, 1, 2, 10, 2, 0.0), _Cfg2D(256, 8, 16, 2, 2, 10, 2, 0.0), _Cfg2D(256, 8, 16, 1, 4, 10, 2, 0.0)):
        assert capi.lib().jodo_dgt2d_check_cfg(ctypes.byref(c)) == -3


def test_layout_and_descriptor():
    cfg = make_config(CFGS[0])
    model = get_model_class('DGT_concat_2D')(cfg)
    n = np.array([3, 1, 5], dtype=np.int32)
    lay = (ctypes.c_int64 * 8)()
    L = capi.lib()
    assert L.jodo_dgt2d_layout(ctypes.byref(model._cfg_struct), 3, 5, n.ctypes.data_as(ctypes.c_void_p), lay) == 0
    assert lay[2] == 9 and lay[3] == 35 and lay[6] == 13 and lay[1] > 0
    desc = np.zeros(lay[0], dtype=np.int32)
    assert L.jodo_dgt2d_fill_desc(ctypes.byref(model._cfg_struct), 3, 5, n.ctypes.data_as(ctypes.c_void_p), desc.ctypes.data_as(ctypes.c_void_p),
                                  ctypes.c_int64(len(desc))) == 0
    assert desc[:9].tolist() == [3, 1, 5, 0, 3, 4, 0, 9, 10]
    assert desc[9:18].tolist() == [0, 1, 2, 256, 512, 513, 514, 515, 516]
    assert desc[18:21].tolist() == [(0 << 6) | 1, (0 << 6) | 2, (1 << 6) | 2] and desc[21] == (2 << 12) | 1
    bad = np.array([3, 0, 5], dtype=np.int32)
    assert L.jodo_dgt2d_layout(ctypes.byref(model._cfg_struct), 3, 5, bad.ctypes.data_as(ctypes.c_void_p), lay) == -1
    big = np.array([70], dtype=np.int32)
    assert L.jodo_dgt2d_layout(ctypes.byref(model._cfg_struct), 1, 70, big.ctypes.data_as(ctypes.c_void_p), lay) == -3


def test_unsupported_2d_settings_fail_loudly():
    for key, val in (('n_extra_heads', 2), ('nf', 128), ('pred_data', False), ('mlp_ratio', 4), ('n_layers', 10), ('cond_time', False),
                     ('softmax_inf', False), ('trans_name', 'Trans_Layer'), ('time_dim', 512)):
        cfg = make_config(CFGS[0])
        cfg.model[key] = val
        with pytest.raises(NotImplementedError, match=key):
            get_model_class('DGT_concat_2D')(cfg)


def test_forward_refuses_cpu_gradients_and_split():
    cfg = make_config(CFGS[0])
    model = make_model(cfg, seed=3)
    nm, em = masks([3, 2])
    xh, ex, nl = torch.zeros(2, 3, 10), torch.zeros(2, 3, 3, 2), torch.zeros(2)
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
        model(None, xh, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)

    class _Cuda(torch.Tensor):                     # a CPU tensor that claims to live on the GPU: reaches the checks behind the device test
        is_cuda = True
    xc = xh.as_subclass(_Cuda)
    with pytest.raises(NotImplementedError, match='inference only'):
        model(None, xc, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)
    model.split_bf16 = True
    with torch.no_grad(), pytest.raises(NotImplementedError, match='split_bf16'):
        model(None, xc, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)


def test_dgt_concat_still_rejects_its_unsupported_settings():
    for key, val in (('dist_gbf', False), ('cond_time', False), ('pred_data', False), ('nf', 512), ('n_layers', 3), ('n_extra_heads', 1)):
        cfg = configs.get('vpsde_qm9_uncond_jodo')
        cfg.model[key] = val
        with pytest.raises(NotImplementedError):
            get_model_class('DGT_concat')(cfg)

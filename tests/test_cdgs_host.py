"""Host-side tests of the CDGS model: registry and configs, parameter tree, strict loading, the C packer against an independent Python
packer, the float32 oracle against the reference's fixtures, refused settings, and the bytes of deterministic_init_ on an existing model."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from jodo_amd import capi, configs
from jodo_amd.models import get_model_class, deterministic_init_
from helpers import load_fixture, make_config, masks, GOLDEN
import oracle_cdgs as OC
import py_packing_cdgs as PP

CFGS = ('vpsde_qm9_2d_cdgs', 'vpsde_geom_2d_cdgs')


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _plain(v):
    if hasattr(v, 'items'):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


@pytest.mark.parametrize('name', CFGS)
def test_registry_and_config_fields(name):
    cfg = configs.get(name)
    assert cfg.model.name == 'CDGS' and get_model_class('CDGS').__name__ == 'CDGS'
    want = _json('cfg_cdgs.json')[name]
    got = _plain(cfg.to_dict() if hasattr(cfg, 'to_dict') else cfg)
    got.pop('device', None)
    assert json.loads(json.dumps(got, sort_keys=True)) == want


@pytest.mark.parametrize('name', CFGS)
def test_state_dict_manifest(name):
    model = get_model_class('CDGS')(configs.get(name))
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == _json('sd_cdgs_manifest.json')[name]
    assert len(got) == (334 if 'qm9' in name else 260)
    eps = [k for k, _ in got if k.endswith('local_model.eps')]
    assert len(eps) == model.n_layers and all(k in dict(model.named_buffers()) for k in eps)
    assert model.state_dict()['all_modules.2.weight'].dim() == 4


@pytest.mark.parametrize('name', CFGS)
def test_strict_load_of_a_reference_ordered_state_dict(name):
    man = _json('sd_cdgs_manifest.json')[name]
    g = torch.Generator().manual_seed(3)
    sd = {k: torch.randn(shape, generator=g) for k, shape in man}
    model = get_model_class('CDGS')(configs.get(name))
    model.load_state_dict(sd, strict=True)
    assert all(torch.equal(model.state_dict()[k], v) for k, v in sd.items())
    from jodo_amd.models.utils import _ModulePrefix
    wrapped = _ModulePrefix(get_model_class('CDGS')(configs.get(name)))
    wrapped.load_state_dict({'module.' + k: v for k, v in sd.items()}, strict=True)
    assert all(torch.equal(wrapped.module.state_dict()[k], v) for k, v in sd.items())


@pytest.mark.parametrize('name', CFGS)
def test_c_packer_matches_python_packer(name):
    cfg = configs.get(name)
    model = deterministic_init_(get_model_class('CDGS')(cfg), seed=5)
    sd = dict(model.state_dict())
    sd['time_freq'] = model._time_freq()
    blob, woff, n_woff = capi.pack_weights_cdgs(model._cfg_struct, sd)
    want, G, blocks = PP.pack({k: v.numpy() for k, v in model.state_dict().items()}, model.nf, model.n_layers, model.atom_ch,
                              model.edge_ch, model.rw_depth, model._time_freq().numpy())
    assert n_woff == len(PP.GLOBAL) + model.n_layers * len(PP.BLOCK)
    offs = [G[k] for k in PP.GLOBAL] + [b[k] for b in blocks for k in PP.BLOCK]
    assert list(woff) == offs
    assert blob.numel() == want.size and np.array_equal(blob.numpy(), want)
    # the `module.` prefix of a DataParallel checkpoint is accepted by name
    blob2, _, _ = capi.pack_weights_cdgs(model._cfg_struct, {('module.' + k if k != 'time_freq' else k): v for k, v in sd.items()})
    assert torch.equal(blob, blob2)
    # a missing tensor is a named error
    bad = dict(sd)
    del bad['all_modules.10.local_model.eps']
    with pytest.raises(capi.JodoHipError, match='local_model.eps'):
        capi.pack_weights_cdgs(model._cfg_struct, bad)


def _fixture_model(fx):
    cfg = make_config(str(fx['cfg_name']))
    model = deterministic_init_(get_model_class('CDGS')(cfg), seed=int(fx['seed'])).eval()
    return cfg, {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize('which', ['qm9', 'geom'])
def test_oracle_reproduces_the_forward_fixtures(which):
    fx = load_fixture('fwd_cdgs_%s.npz' % which)
    cfg, sd = _fixture_model(fx)
    nm, em = masks(fx['n_nodes'].tolist())
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        ox, oe = OC.forward(sd, OC.hparams(cfg), t('t'), t('x'), nm, em, t('edge_x'))
    assert float((ox - t('out_x')).abs().max()) < 1e-5 and float((oe - t('out_e')).abs().max()) < 1e-5
    assert float(t('out_x').abs().max()) > 1e-2 and float(t('out_e').abs().max()) > 1e-2


def test_oracle_reproduces_the_block_fixture():
    fx = load_fixture('blocks_cdgs_qm9.npz')
    cfg, sd = _fixture_model(fx)
    n_nodes = fx['n_nodes'].tolist()
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        states = OC.forward(sd, OC.hparams(cfg), t('t'), t('x'), nm, em, t('edge_x'), return_blocks=True)[2]
    real, emk = nm.reshape(-1) > 0, em.reshape(B, N, N) > 0
    for l in range(cfg.model.n_layers):
        h, e = states[l + 1]
        assert float((h.reshape(B * N, -1)[real] - torch.from_numpy(fx['h'][l])).abs().max()) < 1e-5
        assert float((e[emk] - torch.from_numpy(fx['e'][l])).abs().max()) < 1e-5


def test_distance_code_is_a_count_of_zero_powers_not_a_distance():
    """A chain is bipartite: walks of the wrong parity do not exist, so the code differs from the breadth-first distance."""
    n, K = 6, 4
    adj = torch.zeros(1, n, n)
    for i in range(n - 1):
        adj[0, i, i + 1] = adj[0, i + 1, i] = 1
    land, code = OC.rw_features(K, adj)
    # powers 2..5 between the chain's ends (distance 5): only the 5-step walk exists -> 3 empty powers; neighbours (distance 1): walks
    # of length 3 and 5 only -> 2 empty powers, although their distance is 1
    assert int(code[0, 0, 5]) == 3 and int(code[0, 0, 1]) == 2 and int(code[0, 0, 0]) == 2
    assert land.shape == (1, n, K) and float(land[0, 0, 0]) == 0.5 and float(land[0, 0, 1]) == 0.0


def test_unsupported_settings_raise_naming_the_key():
    cls = get_model_class('CDGS')
    for section, key, val in (('model', 'nf', 128), ('model', 'n_heads', 8), ('model', 'cond_time', False), ('data', 'centered', False),
                              ('model', 'edge_ch', 4), ('data', 'atom_types', 17), ('model', 'rw_depth', 17), ('model', 'rw_depth', 0),
                              ('model', 'n_layers', 17)):
        cfg = configs.get(CFGS[0])
        cfg[section][key] = val
        with pytest.raises(NotImplementedError, match=key):
            cls(cfg)
    # other depths that the width arithmetic allows do construct
    for L in (1, 3, 6):
        cfg = configs.get(CFGS[0])
        cfg.model.n_layers = L
        assert len(cls(cfg).state_dict()) == 4 + 16 + 18 + 37 * L
    # the C side refuses the same settings by name
    bad = type(cls(configs.get(CFGS[0]))._cfg_struct)(128, 8, 16, 5, 2, 8)
    assert capi.lib().jodo_cdgs_check_cfg(ctypes.byref(bad)) != 0 and b'nf' in capi.lib().jodo_last_error()
    # CPU tensors: no fallback
    model = cls(configs.get(CFGS[0]))
    nm, em = masks([3, 2])
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
        model(torch.ones(2), torch.zeros(2, 3, 5), nm, em, edge_x=torch.zeros(2, 3, 3, 2))
    # the layout refuses a padded width above the limit, naming it
    lay = (ctypes.c_int64 * 8)()
    n = np.array([182], dtype=np.int32)
    assert capi.lib().jodo_cdgs_layout(ctypes.byref(model._cfg_struct), 1, 182, n.ctypes.data_as(ctypes.c_void_p), lay) != 0
    assert b'181' in capi.lib().jodo_last_error()


def test_deterministic_init_keeps_the_bytes_of_existing_models_and_moves_the_new_kinds():
    cfg = configs.get('vpsde_zinc_2d_jodo')
    m = deterministic_init_(get_model_class(cfg.model.name)(cfg), seed=7)
    h = hashlib.sha256()
    for k, v in m.state_dict().items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    assert h.hexdigest() == 'cdd143ac8490efbe4749cabf44443e5b992993f8607a5a47a673748f9ee08fbd'
    sd = deterministic_init_(get_model_class('CDGS')(configs.get(CFGS[0])), seed=7).state_dict()
    gw, gb, eps = sd['all_modules.10.norm2_edge.weight'], sd['all_modules.10.norm2_edge.bias'], sd['all_modules.10.local_model.eps']
    assert 0.5 <= float(gw.min()) and float(gw.max()) <= 1.5 and float(gw.std()) > 0.1
    assert float(gb.abs().max()) <= 0.3 and float(gb.std()) > 0.05
    assert eps.shape == (1,) and float(eps.abs()) > 0

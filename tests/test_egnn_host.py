"""CPU: the property classifier's host side (jodo_amd.cond_gen) — the checker oracle against the reference's fixtures, the parameter
tree, the C packer, input checks, checkpoint loading — and the two-property evaluation loop, its config and its context normalisation."""
import argparse
import ctypes
import pickle

import numpy as np
import pytest
import torch

import oracle_egnn as OE
import py_packing_egnn as PP
from helpers import OracleModel, grad_fixture_batch, load_fixture, make_config, make_model, state_dict_cpu
from jodo_amd import capi
from jodo_amd.cond_gen import EGNN, get_classifier, get_model
from jodo_amd.cond_gen.model import _CfgEGNN

FIXTURES = ['nf128_l7_a1_n0', 'nf64_l2_a0_n1', 'nf256_l1_a1_n1', 'nf192_l3_a1_n0', 'nf64_l1_a0_n0']
COMBOS = ['nf128_l7_a1_n0', 'nf64_l2_a0_n1', 'nf256_l1_a1_n1', 'nf64_l1_a0_n0']          # attention on / off x node_attr 0 / 1


@pytest.mark.parametrize("tag", FIXTURES)
def test_oracle_matches_the_reference_fixture(tag):
    """tests/oracle_egnn.py against what the reference's module computed: 1e-6 relative (to the tensor's largest value) in fp32,
    1e-12 in float64, hidden states included."""
    fx, fh = load_fixture('egnn_%s.npz' % tag), load_fixture('egnn_%s_h64.npz' % tag)
    st = OE.settings_of(fx)
    _, sd = OE.init_state_dict(st, int(fx['seed']))
    h0, x, n = torch.from_numpy(fx['h0']), torch.from_numpy(fx['x']), fx['n_nodes']
    o32, h32 = OE.forward(sd, st, h0, x, n)
    o64, h64 = OE.forward(sd, st, h0, x, n, torch.float64)
    rel = lambda got, want: float((got - torch.from_numpy(want)).abs().max()) / float(np.abs(want).max())
    assert rel(o32, fx['out32']) <= 1e-6 and rel(torch.stack(h32), fx['hid32']) <= 1e-6
    assert rel(o64, fx['out64']) <= 1e-12 and rel(h64[0], fh['first']) <= 1e-12
    assert rel(h64[-1], fh['last'] if st['n_layers'] > 1 else fh['first']) <= 1e-12
    e32 = (torch.stack(h32).double() - torch.stack(h64)).abs().amax(dim=(1, 2))
    assert np.allclose(e32.numpy(), fx['hid_e32'], rtol=0.5, atol=1e-7)      # the recorded fp32 distance is an fp32 evaluation's


@pytest.mark.parametrize("tag", COMBOS)
def test_state_dict_has_the_reference_keys_order_and_shapes(tag):
    fx = load_fixture('egnn_%s.npz' % tag)
    st = OE.settings_of(fx)
    sd = EGNN(st['in_node_nf'], 0, st['hidden_nf'], n_layers=st['n_layers'], attention=bool(st['attention']), node_attr=st['node_attr']).state_dict()
    assert list(sd) == fx['keys'].tolist()
    for k, shape in zip(fx['keys'].tolist(), fx['shapes']):
        assert list(sd[k].shape) == shape[:sd[k].dim()].tolist(), k
    if tag == FIXTURES[0]:                                    # the published classifier
        assert len(sd) == 80 and sum(v.numel() for v in sd.values()) == 743944


def test_strict_load_with_and_without_the_module_prefix():
    st = dict(hidden_nf=64, n_layers=2, attention=1, node_attr=1, in_node_nf=5)
    src, sd = OE.init_state_dict(st, 3)
    for prefix in ('', 'module.'):
        dst = EGNN(5, 0, 64, n_layers=2, attention=True, node_attr=1)
        dst._packed = 'stale'
        dst.load_state_dict({prefix + k: v for k, v in sd.items()}, strict=True)
        assert dst._packed is None                            # a load drops the packed weights
        assert all(torch.equal(a, b) for a, b in zip(dst.state_dict().values(), sd.values()))
    with pytest.raises(RuntimeError):
        dst.load_state_dict({k: v for k, v in list(sd.items())[:-1]}, strict=True)


@pytest.mark.parametrize("tag", COMBOS + ['nf192_l3_a1_n0'])
def test_c_packer_matches_the_python_packer(tag):
    fx = load_fixture('egnn_%s.npz' % tag)
    st = OE.settings_of(fx)
    model, sd = OE.init_state_dict(st, int(fx['seed']))
    want, woff = PP.pack({k: v.numpy() for k, v in sd.items()}, st['hidden_nf'], st['n_layers'], st['in_node_nf'], st['attention'], st['node_attr'])
    blob, woff_c, n_woff = capi.pack_weights_egnn(model._cfg_struct, {'module.' + k: v for k, v in sd.items()})
    assert n_woff == PP.GLOBAL_SLOTS + st['n_layers'] * PP.LAYER_SLOTS and list(woff_c) == woff
    assert np.array_equal(blob.numpy(), want)


def test_c_packer_names_a_missing_or_mis_sized_tensor():
    st = dict(hidden_nf=64, n_layers=1, attention=1, node_attr=0, in_node_nf=5)
    model, sd = OE.init_state_dict(st, 1)
    missing = {k: v for k, v in sd.items() if k != 'gcl_0.att_mlp.0.bias'}
    with pytest.raises(capi.JodoHipError, match="gcl_0.att_mlp.0.bias"):
        capi.pack_weights_egnn(model._cfg_struct, missing)
    wrong = dict(sd)
    wrong['gcl_0.edge_mlp.0.weight'] = torch.zeros(64, 128)
    with pytest.raises(capi.JodoHipError, match="gcl_0.edge_mlp.0.weight"):
        capi.pack_weights_egnn(model._cfg_struct, wrong)


def test_unsupported_settings_raise_and_name_the_setting():
    for kw, name in ((dict(hidden_nf=96), 'hidden_nf'), (dict(hidden_nf=320), 'hidden_nf'), (dict(n_layers=17), 'n_layers'),
                     (dict(in_node_nf=17), 'in_node_nf'), (dict(in_edge_nf=2), 'in_edge_nf'), (dict(act_fn=torch.nn.ReLU()), 'act_fn')):
        args = dict(in_node_nf=5, in_edge_nf=0, hidden_nf=128, n_layers=2)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=name):
            EGNN(**args)
    L = capi.lib()
    good = (128, 7, 5, 1, 0)
    assert L.jodo_egnn_check_cfg(ctypes.byref(_CfgEGNN(*good))) == 0
    for idx, val, name in ((0, 96, 'hidden_nf'), (0, 512, 'hidden_nf'), (1, 0, 'n_layers'), (2, 0, 'in_node_nf'), (3, 2, 'attention'), (4, 3, 'node_attr')):
        bad = list(good)
        bad[idx] = val
        assert L.jodo_egnn_check_cfg(ctypes.byref(_CfgEGNN(*bad))) == -3                  # JODO_ERR_UNSUPPORTED
        assert name in L.jodo_last_error().decode()
    lay = (ctypes.c_int64 * 8)()
    n = np.array([3, 300], dtype=np.int32)
    assert L.jodo_egnn_layout(ctypes.byref(_CfgEGNN(*good)), 2, 300, n.ctypes.data_as(ctypes.c_void_p), lay) == -3
    assert 'padded width' in L.jodo_last_error().decode()


def test_descriptor_words_at_the_widest_layout_and_its_refusals():
    """jodo_egnn_layout + jodo_egnn_fill_desc at B = 5000, N = 255 (molecule index 4999 and atom slot 254 share one word as
    (b << 8) | i): counts, exclusive prefix sums and every atom word against a numpy restatement; then what the layout refuses."""
    L = capi.lib()
    cfg = ctypes.byref(_CfgEGNN(128, 7, 5, 1, 0))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    B, N = 5000, 255
    n = np.array([[255, 1, 181, 2, 224][b % 5] for b in range(B)], dtype=np.int32)
    Nn = int(n.sum())
    lay = (ctypes.c_int64 * 8)()
    assert L.jodo_egnn_layout(cfg, B, N, ptr(n), lay) == 0
    assert lay[2] == Nn == 1000 * 663 and lay[0] == 2 * B + Nn
    desc = np.full(int(lay[0]) + 1, -7, dtype=np.int32)
    assert L.jodo_egnn_fill_desc(cfg, B, N, ptr(n), ptr(desc), ctypes.c_int64(int(lay[0]))) == 0
    assert desc[-1] == -7                                     # nothing behind the words asked for
    noff = np.concatenate([[0], np.cumsum(n)[:-1]])
    assert np.array_equal(desc[:B], n) and np.array_equal(desc[B:2 * B], noff)
    words = desc[2 * B:-1]
    mol = np.repeat(np.arange(B), n)
    assert np.array_equal(words >> 8, mol) and np.array_equal(words & 255, np.arange(Nn) - noff[mol])
    assert int((words & 255).max()) == 254 and int((words >> 8).max()) == B - 1
    # refusals
    assert L.jodo_egnn_fill_desc(cfg, B, N, ptr(n), ptr(desc), ctypes.c_int64(int(lay[0]) - 1)) == -1      # JODO_ERR_ARG
    assert 'words' in L.jodo_last_error().decode()
    for idx, bad in ((3, 0), (4998, N + 1)):
        m = n.copy()
        m[idx] = bad
        assert L.jodo_egnn_layout(cfg, B, N, ptr(m), lay) == -1                                         # JODO_ERR_ARG
        assert 'n_nodes[%d]=%d' % (idx, bad) in L.jodo_last_error().decode()
    small = np.array([255, 3], dtype=np.int32)
    assert L.jodo_egnn_layout(cfg, 2, 256, ptr(small), lay) == -3                                       # JODO_ERR_UNSUPPORTED
    assert 'padded width' in L.jodo_last_error().decode()
    assert L.jodo_egnn_layout(cfg, 2, 255, ptr(small), lay) == 0 and lay[2] == 258


def test_cpu_grad_enabled_and_sparse_calls_raise_with_directions():
    from jodo_amd.sampling import build_masks, full_edge_index
    m = EGNN(5, 0, 64, n_layers=1).eval()
    nm, em = build_masks([2, 3], 3, 'cpu')
    args = dict(h0=torch.zeros(6, 5), x=torch.zeros(6, 3), edge_attr=None, node_mask=nm.reshape(6, 1), edge_mask=em, n_nodes=3)
    with pytest.raises(NotImplementedError, match="no_grad"):
        m(edges=full_edge_index(3, 2, 'cpu'), **args)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            m(edges=full_edge_index(3, 2, 'cpu'), **args)
        with pytest.raises(NotImplementedError, match="edge_attr"):
            m(edges=None, **dict(args, edge_attr=torch.zeros(18, 1)))
        sparse = [e[:-3] for e in full_edge_index(3, 2, 'cpu')]
        with pytest.raises(NotImplementedError, match="fully connected"):
            m(edges=sparse, **args)
    with pytest.raises(RuntimeError, match="DataParallel"):
        m._replicate_for_data_parallel()


def test_get_classifier_round_trips_the_published_layout(tmp_path):
    st = dict(hidden_nf=128, n_layers=7, attention=1, node_attr=0, in_node_nf=5)
    _, sd = OE.init_state_dict(st, 9)
    args = argparse.Namespace(nf=128, n_layers=7, attention=True, node_attr=0, device='cuda', model_name='egnn', lr=1e-3)
    with open(tmp_path / 'args.pickle', 'wb') as f:
        pickle.dump(args, f)
    torch.save({'module.' + k: v for k, v in sd.items()}, tmp_path / 'best_checkpoint.npy')
    clf = get_classifier(str(tmp_path / 'best_checkpoint.npy'), str(tmp_path / 'args.pickle'))
    assert isinstance(clf, EGNN) and clf.hidden_nf == 128 and clf.n_layers == 7 and clf.attention and not clf.node_attr
    got = clf.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) and got[k].device.type == 'cpu' for k in sd)
    with pytest.raises(Exception, match="Wrong model name"):
        get_model(argparse.Namespace(model_name='other'))


# ---- the two-property evaluation --------------------------------------------------------------------------------------------------------
class _Scaled(torch.nn.Module):
    """oracle.stubs.StubClassifier times a factor: two different stand-in classifiers."""

    def __init__(self, factor):
        super().__init__()
        from oracle.stubs import StubClassifier
        self.stub, self.factor = StubClassifier(), factor

    def forward(self, **kw):
        return self.factor * self.stub(**kw)


class _Ctx:
    def __init__(self, cols):
        self.cols, self.seen = cols, []

    def sample_batch(self, n_nodes):
        c = torch.randn(len(n_nodes), self.cols)
        self.seen.append(c.clone())
        return c


def test_multi_config_builds_the_two_column_conditional_model():
    from jodo_amd import configs
    cfg = configs.get('vpsde_qm9_cond_multi_jodo')
    assert cfg.exp_type == 'vpsde_edge_cond_multi' and (cfg.cond_property1, cfg.cond_property2) == ('alpha', 'mu')
    assert cfg.model.name == 'cond_DGT_concat' and cfg.model.cond_ch == 2 and cfg.data.transform == 'EdgeComCondMulti'
    from jodo_amd.models import get_model_class
    model = get_model_class(cfg.model.name)(cfg)
    assert model.conditional and model.dims.cond_ch == 2 and model.cond_lin.in_features == 2 * cfg.model.nf


def test_cond_multi_sampling_eval_fn_on_the_oracle_model():
    """get_cond_multi_sampling_eval_fn driven like the single-property test of tests/test_oracle_golden.py: the CPU oracle model, two
    stand-in classifiers, a [B, 2] context.  Same molecules as get_sampling_fn from the same generator state; both scores recomputed
    from the returned molecules and the drawn contexts; a one-column context is refused."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import get_cond_multi_sampling_eval_fn, get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    from oracle import dgt_oracle as O
    from oracle.stubs import FixedNodes
    cfg = make_config('vpsde_qm9_cond_multi_jodo')
    cfg.device = 'cpu'
    cfg.sampling.steps, cfg.sampling.method = 3, 'ancestral'
    om = OracleModel(state_dict_cpu(make_model(cfg, 12, head_gain=10.0)), O.Hyper.from_config(cfg), faithful=True)
    ns, inv = NoiseScheduleVP(cfg.sde.schedule), get_data_inverse_scaler(cfg)
    n_nodes = [4, 7, 3, 5, 2, 6]
    norm = {'alpha': {'mean': 75.3, 'mad': 6.3}, 'mu': {'mean': 2.7, 'mad': 1.2}}
    ctx = _Ctx(2)
    torch.manual_seed(8)
    fn = get_cond_multi_sampling_eval_fn(cfg, ns, FixedNodes(n_nodes), 3, 5, inv, prop_dist=ctx, prop_norm=norm)
    mols, s1, s2 = fn(om, _Scaled(1.0), _Scaled(-0.5))
    assert len(mols) == 5 and [int(m[0].shape[0]) for m in mols] == n_nodes[:5]
    torch.manual_seed(8)
    plain = get_sampling_fn(cfg, ns, FixedNodes(n_nodes), 3, 6, inv, prop_dist=_Ctx(2), return_raw=True)(om)
    for got, want in zip(mols, plain):
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    targets = torch.cat(ctx.seen)
    for k, (score, factor, prop) in enumerate(((s1, 1.0, 'alpha'), (s2, -0.5, 'mu'))):
        mean, mad = norm[prop]['mean'], norm[prop]['mad']
        errs = []
        for i, (pos, at, et, fc) in enumerate(mols):
            h0 = torch.nn.functional.one_hot(at, cfg.data.atom_types).float()
            w = torch.arange(1, h0.shape[1] + 1, dtype=torch.float32)
            pred = factor * ((h0 * w).sum(1) * 0.1 + pos.square().sum(1)).mean()
            errs.append(abs(float(pred) * mad + mean - (float(targets[i, k]) * mad + mean)))
        assert abs(score - sum(errs) / len(errs)) < 1e-3 * max(1.0, score)              # outputNorm of alpha and mu = 1
    torch.manual_seed(8)
    one = get_cond_multi_sampling_eval_fn(cfg, ns, FixedNodes(n_nodes), 3, 5, inv, prop_dist=_Ctx(1), prop_norm=norm)
    with pytest.raises(ValueError, match="two-column context"):
        one(om, _Scaled(1.0), _Scaled(1.0))


def test_process_edge_batch_normalises_a_two_column_context():
    from jodo_amd.losses import process_edge_batch
    from jodo_amd.utils import get_data_scaler
    cfg = make_config('vpsde_qm9_cond_multi_jodo')
    batch, _ = grad_fixture_batch(cfg, [4, 6, 3], 5)
    raw = torch.tensor([[70.0, 1.5], [80.1, 3.25], [75.3, 2.7]])
    batch['context'] = raw.clone()
    norm = {'alpha': {'mean': 75.3, 'mad': 6.3}, 'mu': {'mean': 2.7, 'mad': 1.2}}
    context = process_edge_batch(batch, 'cpu', cfg.model.include_fc_charge, get_data_scaler(cfg), norm)[4]
    assert context.shape == (3, 2)
    assert torch.allclose(context[:, 0], (raw[:, 0] - 75.3) / 6.3) and torch.allclose(context[:, 1], (raw[:, 1] - 2.7) / 1.2)

"""DGT_concat_sim (the 3-D score network without extra attention heads) on the host: parameter tree against the reference's recorded
manifest, the seeded default initialisation, the config keys the class must ignore, tests/oracle_sim.py against the reference's
recorded outputs (tools/make_golden_sim.py), the packed weights against the Python packer, and the errors of what is not built."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from jodo_amd import capi
from jodo_amd.models import get_model_class
import oracle_sim as OS
import py_packing as P
from helpers import GOLDEN, load_fixture, make_config, make_model, masks, reference_blocks_dense

NAME = 'DGT_concat_sim'
CFGS = ('vpsde_qm9_uncond_jodo', 'vpsde_geom_uncond_jodo')


def sim_config(cfg_name, **over):
    return make_config(cfg_name, name=NAME, **over)


def manifest():
    with open(os.path.join(GOLDEN, 'sd_sim_manifest.json')) as f:
        return json.load(f)


@pytest.mark.parametrize("cfg_name", CFGS)
def test_parameter_tree_matches_the_reference_manifest(cfg_name):
    want = manifest()[cfg_name]
    model = get_model_class(NAME)(sim_config(cfg_name))
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == want                                              # names, shapes AND order (positional EMA lists)
    assert len(want) == (351 if 'qm9' in cfg_name else 431)
    nf = 256
    shapes = dict((k, s) for k, s in want)
    assert shapes['e_block_0.attn_mpnn.lin_query.weight'] == [nf, nf] and shapes['e_block_0.attn_mpnn.lin_key.bias'] == [nf]
    assert shapes['e_block_3.attn_mpnn.lin_edge0.weight'] == [nf, nf // 4] and shapes['e_block_7.equi_update.coord_mlp.2.weight'] == [1, nf]
    # a checkpoint with exactly the reference's keys loads strictly; DGT_concat's does not (other shapes)
    model.load_state_dict({k: torch.zeros(s) for k, s in want}, strict=True)
    with pytest.raises(RuntimeError, match='size mismatch'):
        model.load_state_dict(get_model_class('DGT_concat')(make_config(cfg_name)).state_dict(), strict=True)


def test_seeded_default_initialisation_is_the_references():
    """torch.manual_seed(s); Model(config): the tree is built from stock torch containers in the reference's construction order, so
    the default initialisation draws the same numbers (sha256 over the state_dict recorded from the reference's class)."""
    rec = manifest()['default_init']
    if rec['torch'] != torch.__version__.split('+')[0]:
        pytest.fail("fixture recorded with torch %s, running %s: regenerate with tools/make_golden_sim.py sd_sim_manifest"
                    % (rec['torch'], torch.__version__))
    torch.manual_seed(int(rec['seed']))
    model = get_model_class(NAME)(sim_config(rec['cfg_name']))
    h = hashlib.sha256()
    for v in model.state_dict().values():
        h.update(v.detach().contiguous().numpy().tobytes())
    assert h.hexdigest() == rec['sha256']


def test_ignored_config_keys_have_no_effect():
    """The reference's constructor never reads n_extra_heads / trans_name, passes softmax_inf on without effect, and edge_quan_th /
    spatial_cut_off only feed an adjacency nobody reads: same tree, same C configuration whatever they hold."""
    base = get_model_class(NAME)(sim_config(CFGS[0]))
    shapes = [(k, tuple(v.shape)) for k, v in base.state_dict().items()]
    for over in (dict(n_extra_heads=0), dict(n_extra_heads=5), dict(softmax_inf=False), dict(trans_name='Trans_Layer'),
                 dict(edge_quan_th=0.3), dict(spatial_cut_off=7.5)):
        m = get_model_class(NAME)(sim_config(CFGS[0], **over))
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == shapes, over
        assert bytes(m._cfg()) == bytes(base._cfg()), over
    assert base._cfg().n_extra == 0 and base.dims.XH == 0 and base.dims.SH == 16 and base.dims.SC == 16 and base.dims.QKP == 256
    # ... while the mixed model still insists on its two adjacency heads
    with pytest.raises(NotImplementedError):
        get_model_class('DGT_concat')(make_config(CFGS[0], n_extra_heads=0))


@pytest.mark.parametrize("over,word", [(dict(nf=128, n_layers=6), 'nf=128'), (dict(nf=384), 'nf=384'), (dict(kernel_layout='wide'), 'wide')])
def test_widths_that_are_not_built_say_so(over, word):
    with pytest.raises(NotImplementedError, match=word):
        get_model_class(NAME)(sim_config(CFGS[1], **over))


def test_split_bf16_and_training_are_refused():
    model = make_model(sim_config(CFGS[0]), 3)
    nm, em = masks([3, 2])
    xh, ex, nl = torch.zeros(2, 3, 9), torch.zeros(2, 3, 3, 2), torch.zeros(2)
    call = lambda: model(nl, xh, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)
    with pytest.raises(NotImplementedError, match='inference'):     # grad-enabled call = training
        call()
    with torch.no_grad():
        model.split_bf16 = True
        with pytest.raises(NotImplementedError, match='split-bf16'):
            call()
        model.split_bf16 = False
        model.train()                                               # dropout 0.1 under train(): the training path as well
        with pytest.raises(NotImplementedError, match='inference'):
            call()
        model.eval()
        with pytest.raises(RuntimeError, match='no CPU fallback'):  # and then the same input checks as the other classes
            call()


# ---- the oracle against the reference's recorded outputs ---------------------------------------------------------------------
@pytest.mark.parametrize("fname", ['fwd_sim_qm9.npz', 'fwd_sim_geom.npz'])
def test_oracle_matches_reference_fixture(fname):
    fx = load_fixture(fname)
    assert str(fx['model_name']) == NAME
    cfg = sim_config(str(fx['cfg_name']))
    hp = OS.HyperSim.from_config(cfg)
    sd = {k: v.detach() for k, v in make_model(cfg, int(fx['seed'])).state_dict().items()}
    nm, em = masks(fx['n_nodes'].tolist())
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        for ex, cx, cex, want in ((t('edge_x'), None, None, 'out1'), (t('edge_x'), t('out1_x'), t('out1_e'), 'out2'),
                                  (t('asym_edge_x'), t('out1_x'), t('out1_e'), 'out_asym')):
            got = OS.forward_dense(sd, hp, t('xh'), nm, em, ex, cx, cex, t('noise_level'))
            assert (got[0] - t(want + '_x')).abs().max() < 1e-5 and (got[1] - t(want + '_e')).abs().max() < 1e-5, want
    # float64 evaluation of the same formulas: the yardstick of the GPU tests
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        g64 = OS.forward_dense(sd64, hp, t('xh').double(), nm.double(), em.double(), t('edge_x').double(), t('out1_x').double(),
                               t('out1_e').double(), t('noise_level').double())
    assert g64[0].dtype == torch.float64 and (g64[0] - t('out2_x')).abs().max() < 1e-5


def test_oracle_blocks_match_reference_fixture():
    fx = load_fixture('blocks_sim_qm9.npz')
    cfg = sim_config(str(fx['cfg_name']))
    hp = OS.HyperSim.from_config(cfg)
    sd = {k: v.detach() for k, v in make_model(cfg, int(fx['seed'])).state_dict().items()}
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        _, _, inter = OS.forward_dense(sd, hp, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'),
                                       return_intermediates=True)
    for l in range(hp.n_layers):
        for b, (rh, re, rp) in enumerate(reference_blocks_dense(fx, l)):
            offd = ~torch.eye(n_nodes[b], dtype=torch.bool)
            blk = inter[b][l]
            assert (blk['h'] - rh).abs().max() < 2e-5 and (blk['pos'] - rp).abs().max() < 2e-5
            assert n_nodes[b] == 1 or (blk['e'][offd] - re[offd]).abs().max() < 2e-5
            if n_nodes[b] > 1:                                       # softmax over the real incoming edges of every head: sums to one
                assert (blk['alpha'].sum(0) - 1).abs().max() < 1e-5 and blk['alpha'].shape[-1] == 16


def test_oracle_follows_the_recorded_trajectory_step():
    """One recorded step of each trajectory (inputs, self-conditioning from the step before) through the oracle."""
    for fname in ('traj_sim_qm9_anc5.npz', 'traj_sim_qm9_dpm_single2.npz'):
        fx = load_fixture(fname)
        cfg = sim_config(str(fx['cfg_name']))
        hp = OS.HyperSim.from_config(cfg)
        sd = {k: v.detach() for k, v in make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain'])).state_dict().items()}
        nm, em = masks(fx['n_nodes'].tolist())
        t = lambda k, i: torch.from_numpy(fx[k][i])
        with torch.no_grad():
            got = OS.forward_dense(sd, hp, t('step_x', 2), nm, em, t('step_edge_x', 2), t('step_pred', 1), t('step_edge_pred', 1),
                                   t('step_noise_level', 2))
        assert (got[0] - t('step_pred', 2)).abs().max() < 5e-5 and (got[1] - t('step_edge_pred', 2)).abs().max() < 5e-5
        assert float(fx['margin_shares'].max()) <= float(fx['margin_cap']) == 0.05


# ---- packing ------------------------------------------------------------------------------------------------------------------
def test_qk_arrangement_without_a_tail_block():
    """SH = 16, SC = 16: eight full 32-row blocks, half h of block b = the 16 channels of head 2b + h, no tail block — the natural
    order, a bijection; and a packed projection emulated on it gives every head's score as a register-local sum."""
    m = P.qk_out_map(16, 16)
    assert m.shape == (8, 2, 16)
    assert np.array_equal(m.reshape(-1), np.arange(256))
    assert np.array_equal(m, P.natural_out_map(256))
    for b in range(8):
        for h in (0, 1):
            assert set((m[b, h] // 16).tolist()) == {2 * b + h}
    rng = np.random.default_rng(0)
    Wq, Wk = (rng.standard_normal((256, 256)).astype(np.float32) / 16 for _ in range(2))
    W0 = rng.standard_normal((256, 64)).astype(np.float32) / 8
    ht, et = rng.standard_normal((32, 256)).astype(np.float32), rng.standard_normal((32, 64)).astype(np.float32)   # [items, features]
    proj = lambda W, x: P.emulate_projection(P.pack_projection(W, P.natural_in_map(W.shape[1]), m), P.to_slots(x, P.natural_in_map(W.shape[1])))
    aq, ak, a0 = proj(Wq, ht), proj(Wk, ht), proj(W0, et)            # accumulators [block, register, half, item]
    assert np.allclose(P.from_slots(aq, m, 256), ht @ Wq.T, atol=1e-4)
    # the kernel's score of item j with itself as partner: slot k of half h = head 2k + h = the sum over block k's 16 registers
    got = (aq * ak * np.tanh(a0)).sum(1) / 4.0                        # [block, half, item]
    q, k, t0 = (ht @ Wq.T).reshape(32, 16, 16), (ht @ Wk.T).reshape(32, 16, 16), np.tanh(et @ W0.T).reshape(32, 16, 16)
    want = (q * k * t0).sum(-1) / np.sqrt(16.0)                       # [item, head]
    for b in range(8):
        for h in (0, 1):
            assert np.allclose(got[b, h], want[:, 2 * b + h], atol=1e-4)


@pytest.mark.parametrize("cfg_name", CFGS)
def test_c_packer_equals_python_packer(cfg_name):
    from py_packing_model import BLOCK_SLOTS, GLOBAL_SLOTS, pack_model
    model = make_model(sim_config(cfg_name), 3)
    sd = model.state_dict()
    blob_py, woff_py = pack_model({k: v.detach().float().cpu() for k, v in sd.items()}, model.dims)
    blob_c, woff_c, n = capi.pack_weights(model._cfg(), sd)
    assert n == len(woff_py) and list(woff_c) == woff_py.tolist() and blob_c.numel() == blob_py.size
    bc, bp = blob_c.numpy(), blob_py
    exact = np.ones(bc.size, bool)                                  # (the composed slots: see tests/test_packing.py)
    lo, hi = woff_py[GLOBAL_SLOTS.index('MOD_W')], woff_py[GLOBAL_SLOTS.index('MOD_B') + 1]
    exact[lo:hi] = False
    assert np.allclose(bc[lo:hi], bp[lo:hi], rtol=1e-6, atol=1e-9)
    nb, ng = len(BLOCK_SLOTS), len(GLOBAL_SLOTS)
    D = model.dims.D
    for l in range(model.dims.L):
        lo = woff_py[ng + l * nb + BLOCK_SLOTS.index('ROWQ_W')]
        hi = woff_py[ng + (l + 1) * nb] if l + 1 < model.dims.L else bc.size
        exact[lo:hi] = False
        assert np.allclose(bc[lo:hi], bp[lo:hi], rtol=1e-5, atol=2e-6)
        # the coordinate head: ONE row of D weights, then the next slot
        c2 = woff_py[ng + l * nb + BLOCK_SLOTS.index('C2_W')]
        assert woff_py[ng + l * nb + BLOCK_SLOTS.index('C2_W') + 1] - c2 == D
        assert np.array_equal(bc[c2:c2 + D], sd['e_block_%d.equi_update.coord_mlp.2.weight' % l].numpy().reshape(-1))
    assert np.array_equal(bc[exact].view(np.uint32), bp[exact].view(np.uint32))


def test_c_library_validates_the_new_shapes():
    model = make_model(sim_config(CFGS[0]), 3)
    mixed = make_model(make_config(CFGS[0]), 3)
    # the mixed model's tensors under the new configuration (and the other way round): a named error, never a mis-packed blob
    with pytest.raises(capi.JodoHipError, match='lin_query'):
        capi.pack_weights(model._cfg(), mixed.state_dict())
    with pytest.raises(capi.JodoHipError, match='lin_query'):
        capi.pack_weights(mixed._cfg(), model.state_dict())
    lib = capi.lib()
    Cfg = type(model._cfg())
    n = np.asarray([5, 6], dtype=np.int32)

    def plan(cfg):
        h = ctypes.c_void_p()
        return lib.jodo_plan_create(ctypes.byref(cfg), 2, 6, n.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(h)), h

    rc, h = plan(Cfg(256, 8, 16, 0, 2, 6, 2, 0, 0.0, 0.0, 0))
    assert rc == 0
    assert lib.jodo_plan_set_option(h, 13, 1) < 0 and b'without extra heads' in lib.jodo_last_error()      # split-bf16
    assert lib.jodo_plan_set_option(h, 3, 1) < 0                                                            # attention variants
    assert lib.jodo_plan_set_option(h, 13, 0) == 0 and lib.jodo_plan_set_option(h, 4, 1) == 0               # pins work as ever
    lib.jodo_plan_destroy(h)
    for bad, word in ((Cfg(384, 10, 16, 0, 4, 17, 3, 0, 0.0, 0.0, 0), b'nf=384'), (Cfg(128, 6, 16, 0, 4, 17, 3, 0, 0.0, 0.0, 0), b'nf=128'),
                      (Cfg(256, 8, 16, 0, 2, 6, 2, 0, 0.0, 0.0, 1), b'layout'), (Cfg(256, 8, 16, 0, 2, 6, 2, 1, 0.0, 0.0, 0), b'cond_ch'),
                      (Cfg(256, 8, 16, 1, 2, 6, 2, 0, 0.0, 0.0, 0), b'n_extra_heads=1')):
        rc, _ = plan(bad)
        assert rc < 0 and word in lib.jodo_last_error(), (word, lib.jodo_last_error())
    tot = [ctypes.c_size_t() for _ in range(4)]
    assert lib.jodo_dgt_split_size(ctypes.byref(model._cfg()), *[ctypes.byref(t) for t in tot]) < 0
    assert b'split-bf16' in lib.jodo_last_error()

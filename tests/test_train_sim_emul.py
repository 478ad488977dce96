"""CPU checks of the training path of DGT_concat_sim (the 3-D score network without extra attention heads): the SAME kernel sources
that libjodo_hip.so runs on the GPU (jodo_amd/csrc/dgt_train.hip + train_ops.h with n_extra = 0: 16 learned heads, one coordinate
head), compiled for the host by tests/emul/Makefile exactly as tests/test_train_emul.py builds them and run on the op-by-op path,
against the reference's own loss.backward() (tests/golden/grad_sim_qm9.npz, tools/make_golden_sim_train.py) and against float64
autograd through tests/oracle_sim.py.  nf 256 is the only width the module builds, so every case runs the full-width network (8 or 10
blocks) on a handful of small molecules.  tests/test_train_sim_gpu.py repeats the cases on the device."""
import ctypes
import os
import subprocess

import pytest
import torch

from oracle import train_ref as T

import oracle_sim as OS
import train_sim_common as C
from helpers import compare_grads, load_fixture, make_config, make_model, masks, random_inputs

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')
NAME = 'DGT_concat_sim'
QM9, GEOM = 'vpsde_qm9_uncond_jodo', 'vpsde_geom_uncond_jodo'


@pytest.fixture(scope='module')
def emul():
    subprocess.run(['make', '-C', EMUL_DIR], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_train_emul.so'))


def engine_for(emul, model, n_nodes):
    from jodo_amd.train import TrainEngine
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    return TrainEngine(model._cfg(), n_nodes, max(n_nodes), named, 'cpu', lib=emul, stream_ptr=lambda: ctypes.c_void_p(0)), [k for k, _ in named]


def test_training_step_reproduces_the_reference_backward(emul):
    """The reference's recorded training step of DGT_concat_sim (grad_sim_qm9: QM9 config, self-conditioning branch, eval-mode dropout):
    forward == the reference's prediction, loss == its loss to 2e-5 relative, the 17 recorded parameter gradients == the reference's to
    2e-4 relative, and all 351 gradients == float64 autograd through the oracle by the gradient rule."""
    fx = load_fixture('grad_sim_qm9.npz')
    cfg = make_config(str(fx['cfg_name']), name=str(fx['model_name']))
    model = make_model(cfg, int(fx['seed']))
    hp = OS.HyperSim.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    eng, names = engine_for(emul, model, n_nodes)
    assert len(names) == 351
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    out_x, out_e = eng.forward(params, t('z_t'), t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), None, 0.0, 0)
    assert eng.flags.tolist()[0] == 0 and eng.flags.tolist()[3] == 1
    C.forward_close(out_x, t('pred'), 'pred vs the reference')
    C.forward_close(out_e, t('edge_pred'), 'edge_pred vs the reference')
    px, pe = out_x.clone().requires_grad_(True), out_e.clone().requires_grad_(True)
    lw = [float(w) for w in cfg.model.loss_weights.split(',')]
    loss = T.sde_graph_loss(px, pe, t('xh'), t('edge_x'), t('align_pos'), nm, em, t('alpha_t'), t('sigma_t'), lw, cfg.training.reduce_mean)
    print('loss %.9g, the reference %.9g' % (loss.item(), float(fx['loss'])))
    assert abs(loss.item() - float(fx['loss'])) < 2e-5 * float(fx['loss'])
    loss.backward()
    grads = eng.backward(params, t('noise_level'), px.grad.contiguous(), pe.grad.contiguous(), 0.0, 0)
    by_name = dict(zip(names, grads))
    recorded = fx['grad_names'].tolist()
    for k in ('e_block_7.equi_update.coord_mlp.2.weight', 'dist_layer.means.weight'):
        assert k in recorded
    for i, k in enumerate(recorded):
        want = t('grad_%d' % i)
        rel = (by_name[k] - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        print('%s: %.3e of the reference' % (k, rel))
        assert rel < 2e-4, "%s: %g" % (k, rel)
    args = (model, hp, t('z_t'), nm, em, t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), px.grad, pe.grad)
    want = C.oracle_param_grads(*args)[2]
    want32 = C.oracle_param_grads(*args, dtype=torch.float32)[2]
    compare_grads(zip(names, grads), want, C.GRAD_REL, want32, C.K32, what='grad_sim_qm9')


CASES = [
    # first step; a one-atom molecule (empty softmax, alpha = 0), a two-atom one; 346 edge rows: no multiple of 32
    (QM9, {}, [4, 1, 2, 6, 17], False),
    # GEOM: 10 blocks, mlp_ratio 4, edge_ch 3, self-conditioned
    (GEOM, {}, [7, 3, 12], True),
]


@pytest.mark.parametrize("cfg_name,over,n_nodes,selfcond", CASES)
def test_all_parameter_gradients_match_autograd_through_the_oracle(emul, cfg_name, over, n_nodes, selfcond):
    cfg = make_config(cfg_name, name=NAME, **over)
    model = make_model(cfg, 3, gain=1.5, coord_scale=0.05)
    hp = OS.HyperSim.from_config(cfg)
    xh, ex, nl, _, nm, em = random_inputs(hp, n_nodes, seed=5)
    cx, cex, d_x, d_e = C.selfcond_inputs(xh, ex, nm, em, selfcond)
    eng, names = engine_for(emul, model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    out_x, out_e = eng.forward(params, xh, ex, cx, cex, nl, None, 0.0, 0)
    px, pe, want = C.oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e)
    want32 = C.oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e, dtype=torch.float32)[2]
    C.forward_close(out_x, px, 'out_x vs float64')
    C.forward_close(out_e, pe, 'out_edge vs float64')
    assert eng.flags.tolist()[0] == 0 and eng.flags.tolist()[3] == (1 if selfcond else 0)
    grads = eng.backward(params, nl, d_x, d_e, 0.0, 0)
    assert float(dict(zip(names, grads))['e_block_0.equi_update.coord_mlp.2.weight'].abs().max()) > 0
    compare_grads(zip(names, grads), want, C.GRAD_REL, want32, C.K32, what='%s %s' % (cfg_name, n_nodes))


def test_masked_restatement_with_all_ones_masks_is_the_oracle():
    """train_sim_common.forward_dense_masked with every multiplier 1 == oracle_sim.forward_dense, bit for bit (float64)."""
    cfg = make_config(QM9, name=NAME)
    model = make_model(cfg, 3, gain=1.5, coord_scale=0.05)
    hp = OS.HyperSim.from_config(cfg)
    n_nodes = [4, 1, 3]
    xh, ex, nl, _, nm, em = random_inputs(hp, n_nodes, seed=5)
    cx, cex, _, _ = C.selfcond_inputs(xh, ex, nm, em, True)
    ones = C.drop_masks_for(hp, n_nodes, 0.0, C.DROP_SEED)
    sd = {k: v.double() for k, v in model.state_dict().items()}
    d = lambda v: None if v is None else v.double()
    with torch.no_grad():
        for c_, ce_ in ((None, None), (cx, cex)):
            a = OS.forward_dense(sd, hp, d(xh), d(nm), d(em), d(ex), d(c_), d(ce_), d(nl))
            b = C.forward_dense_masked(sd, hp, d(xh), d(nm), d(em), d(ex), d(c_), d(ce_), d(nl), ones)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_dropout_on_matches_autograd_through_the_masked_oracle(emul):
    """Training-mode dropout (p = 0.1, a seed above 2^32) through the emulation build against float64 autograd through the masked
    restatement with the restated masks: outputs at the forward tolerance, every parameter's gradient by the gradient rule.  Pins the four
    live sites (the two feed-forwards) and that the softmax weights are not dropped."""
    cfg = make_config(QM9, name=NAME)
    model = make_model(cfg, 3, gain=1.5, coord_scale=0.05)
    hp = OS.HyperSim.from_config(cfg)
    n_nodes = [5, 1, 3, 7]
    xh, ex, nl, _, nm, em = random_inputs(hp, n_nodes, seed=5)
    cx, cex, d_x, d_e = C.selfcond_inputs(xh, ex, nm, em, True)
    p = 0.1
    drop = C.drop_masks_for(hp, n_nodes, p, C.DROP_SEED)
    eng, names = engine_for(emul, model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    eng.forward(params, xh, ex, cx, cex, nl, None, 0.0, C.DROP_SEED)
    alpha0 = eng.debug_fetch(1, 0)
    out_x, out_e = eng.forward(params, xh, ex, cx, cex, nl, None, p, C.DROP_SEED)
    assert torch.equal(eng.debug_fetch(1, 0), alpha0) and float(alpha0.abs().max()) > 0      # block 0's attention precedes every live site
    px, pe, want = C.oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e, drop=drop)
    want32 = C.oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e, dtype=torch.float32, drop=drop)[2]
    C.forward_close(out_x, px, 'out_x vs the masked float64 oracle')
    C.forward_close(out_e, pe, 'out_edge vs the masked float64 oracle')
    ev = C.oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e)[0]
    assert (ev - px).abs().max() > 1e-3                          # the masks matter at this size: eval mode is far away
    grads = eng.backward(params, nl, d_x, d_e, p, C.DROP_SEED)
    compare_grads(zip(names, grads), want, C.GRAD_REL, want32, C.K32, what='dropout 0.1')


def test_create_refuses_other_head_layouts_by_name(emul):
    """jodo_train_create takes n_extra 0 only as the module builds it: every other value, and n_extra 0 at another width, head count,
    depth, layout or with a context, is refused with the values in the message."""
    from jodo_amd import capi
    from jodo_amd.train import TrainEngine
    cfg = make_config(QM9, name=NAME)
    model = make_model(cfg, 3)
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    base = model._cfg()
    for field, value, word in (('n_extra', 1, 'n_extra_heads 1'), ('n_extra', 3, 'n_extra_heads 3'), ('nf', 128, 'nf 128'),
                               ('n_layers', 6, 'n_layers 6'), ('layout', 1, 'layout 1'), ('cond_ch', 1, 'cond_ch 1'), ('n_heads', 8, 'n_heads 8')):
        c = type(base)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(base), ctypes.sizeof(base))
        setattr(c, field, value)
        with pytest.raises(capi.JodoHipError, match=word):
            TrainEngine(c, [3, 2], 3, named, 'cpu', lib=emul, stream_ptr=lambda: ctypes.c_void_p(0))

"""CPU checks of the 2-D training path: the SAME kernel sources libjodo_hip.so runs on the GPU (jodo_amd/csrc/dgt2d_train.hip +
train_ops.h), compiled for the host by tests/emul2d/Makefile against the sequential stand-in for the HIP runtime of tests/emul/, driven
through jodo_amd.train.TrainEngine2D with host pointers, and compared with two independent yardsticks: the reference's own recorded
training steps (tests/golden/grad2d_*.npz, train_drop2d_zinc.npz) and float64 autograd through the dense oracle (tests/oracle2d.py,
tests/oracle2d_train.py), with and without dropout.  tests/test_train2d_gpu.py repeats it on the device.  Shapes and tolerances:
tests/train2d_common.py."""
import ctypes
import os
import subprocess

import pytest
import torch

import oracle2d as O2
import oracle2d_train as O2T
from oracle import philox_ref as PR

import train2d_common as C
from helpers import load_fixture, make_config, make_model, masks

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul2d')


@pytest.fixture(scope='module')
def emul():
    subprocess.run(['make', '-C', EMUL_DIR], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_train2d_emul.so'))


def engine_for(emul, model, n_nodes, pool=None):
    from jodo_amd.train import TrainEngine2D
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    eng = TrainEngine2D(model._cfg_struct, n_nodes, max(n_nodes), named, 'cpu', lib=emul, stream_ptr=lambda: ctypes.c_void_p(0), pool=pool)
    return eng, [k for k, _ in named]


def params_of(model):
    return [v.detach().float().contiguous() for v in model.state_dict().values()]


def test_masked_oracle_without_masks_is_the_dense_oracle():
    c = C.random_case('moses', seed=11, n_nodes=[2, 5, 1])
    _, model = C.model_for('moses', 3)
    sd = model.state_dict()
    for cx, cex in ((None, None), (c['cx'], c['cex'])):
        with torch.no_grad():
            a = O2.forward_dense(sd, c['hp'], c['xh'], c['nm'], c['em'], c['ex'], cx, cex, c['nl'], return_blocks=True)
            b = O2T.forward_dense_drop(sd, c['hp'], c['xh'], c['nm'], c['em'], c['ex'], cx, cex, c['nl'], return_blocks=True, drop=None)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a[2], b[2]))


def test_235_parameters_and_option_refusals(emul):
    _, model = C.model_for('zinc', 3)
    eng, names = engine_for(emul, model, [3, 2])
    assert len(names) == 235 == len(list(model.parameters()))
    assert emul.jodo_train2d_set_option(eng.handle, 0, 0) == 0
    assert emul.jodo_train2d_set_option(eng.handle, 0, 1) != 0          # no matrix instructions on the host: an error, never a quiet fall-back
    assert emul.jodo_train2d_set_option(eng.handle, 7, 0) != 0


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_training_step_reproduces_the_reference_backward(emul, which):
    """(a) The reference's recorded 2-D training step (eval-mode dropout, self-conditioned branch): forward == its prediction, loss ==
    its loss, the recorded gradients == the reference's (2e-4), every parameter == float64 autograd through the oracle."""
    fx = load_fixture('grad2d_%s.npz' % which)
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), gain=float(fx['gain']), head_gain=float(fx['head_gain']))
    hp = O2.Hyper2D.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    assert n_nodes == C.TRAIN_NODES[which]
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    eng, names = engine_for(emul, model, n_nodes)
    params = params_of(model)
    out_x, out_e = eng.forward(params, t('z_t'), t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), None, 0.0, 0)
    C.fwd_close(out_x, t('pred'), 'pred vs reference')
    C.fwd_close(out_e, t('edge_pred'), 'edge_pred vs reference')
    px, pe = out_x.clone().requires_grad_(True), out_e.clone().requires_grad_(True)
    loss = C.loss2d_from_outputs(cfg, px, pe, t('xh'), t('edge_x'), nm, em, t('alpha_t'), t('sigma_t'))
    assert abs(loss.item() - float(fx['loss'])) < 1e-5 * float(fx['loss'])
    loss.backward()
    grads = eng.backward(params, t('noise_level'), px.grad.contiguous(), pe.grad.contiguous(), 0.0, 0)
    by_name = dict(zip(names, grads))
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (by_name[k] - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < C.GRAD_REF_REL, "%s: %g" % (k, rel)
    sd = model.state_dict()
    args = (sd, hp, nm, em, t('z_t'), t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), px.grad, pe.grad)
    _, _, want = C.oracle_grads(*args)
    _, _, want32 = C.oracle_grads(*args, dtype=torch.float32)
    C.assert_all_nonzero(want)
    C.compare_grads(zip(names, grads), want, want32=want32, what='grad2d_%s' % which)


@pytest.mark.parametrize('which,selfcond', [('zinc', False), ('zinc', True), ('moses', False), ('moses', True), ('zinc_chunks', False), ('zinc_chunks', True)])
def test_all_parameter_gradients_match_autograd_through_the_oracle(emul, which, selfcond):
    """(b) First-step call (no conditioning input: all-ones adjacency head) and self-conditioned call, all 235 gradients."""
    c, sd, (px, pe, want), (_, _, want32) = C.random_case_yardsticks(which, selfcond)
    _, model = C.model_for(which, 3)
    eng, names = engine_for(emul, model, c['n_nodes'])
    params = params_of(model)
    cx, cex = (c['cx'], c['cex']) if selfcond else (None, None)
    out_x, out_e = eng.forward(params, c['xh'], c['ex'], cx, cex, c['nl'], None, 0.0, 0)
    C.fwd_close(out_x, px, 'atom_pred')
    C.fwd_close(out_e, pe, 'edge_pred')
    assert float(out_e.abs().max()) > 0 and torch.equal(out_e, out_e.transpose(1, 2))
    grads = eng.backward(params, c['nl'], c['d_x'], c['d_e'], 0.0, 0)
    C.assert_all_nonzero(want)
    C.compare_grads(zip(names, grads), want, want32=want32, what='%s selfcond=%s' % (which, selfcond))


def test_training_mode_dropout_reproduces_the_reference(emul):
    """(c) train_drop2d_zinc replayed with its seeds: both calls' outputs and the recorded gradients against the reference under
    model.train() with the same masks injected; every other gradient against the masked dense oracle with philox_ref's masks."""
    fx = load_fixture('train_drop2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), gain=float(fx['gain']), head_gain=float(fx['head_gain']))
    hp = O2.Hyper2D.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    p, s1, s2 = float(fx['p']), int(fx['seed1']), int(fx['seed2'])
    assert p == pytest.approx(cfg.model.dropout)
    eng, names = engine_for(emul, model, n_nodes)
    params = params_of(model)
    o1 = eng.forward(params, t('xh'), t('edge_x'), None, None, t('noise_level'), None, p, s1, save_activations=False)
    C.fwd_close(o1[0], t('out1_x'), 'no-grad call, atoms')
    C.fwd_close(o1[1], t('out1_e'), 'no-grad call, edges')
    o2 = eng.forward(params, t('xh'), t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), None, p, s2)
    C.fwd_close(o2[0], t('out2_x'), 'grad-enabled call, atoms')
    C.fwd_close(o2[1], t('out2_e'), 'grad-enabled call, edges')
    grads = eng.backward(params, t('noise_level'), t('d_out_x'), t('d_out_e'), p, s2)
    by_name = dict(zip(names, grads))
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (by_name[k] - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < C.GRAD_REF_REL, "%s: %g" % (k, rel)
    m2 = PR.dropout_masks(s2, p, n_nodes, hp.L, hp.D, hp.De, hp.r)
    args = (model.state_dict(), hp, nm, em, t('xh'), t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), t('d_out_x'), t('d_out_e'))
    _, _, want = C.oracle_grads(*args, drop=m2)
    _, _, want32 = C.oracle_grads(*args, dtype=torch.float32, drop=m2)
    C.compare_grads(zip(names, grads), want, want32=want32, what='train_drop2d_zinc')


def test_backward_is_linear_and_two_forwards_use_two_slots(emul):
    """(d) Backward is linear in the output gradient; two forwards before two backwards keep both sets of activations."""
    from jodo_amd.train import TrainEngine2D
    c = C.random_case('moses', seed=21, n_nodes=[2, 5, 9])
    _, model = C.model_for('moses', 4)
    pool = TrainEngine2D.new_pool()
    eng, names = engine_for(emul, model, c['n_nodes'], pool=pool)
    params = params_of(model)
    p, seed = 0.1, 77
    eng.forward(params, c['xh'], c['ex'], None, None, c['nl'], None, p, seed, keep=True)
    st1 = eng.stamp
    eng.forward(params, c['xh'], c['ex'], c['cx'], c['cex'], c['nl'], None, p, seed + 1, keep=True)
    st2 = eng.stamp
    assert st1 != st2 and eng.slot_of(st1) is not eng.slot_of(st2) and eng.slot_of(st1) is not None
    g2 = eng.backward(params, c['nl'], c['d_x'], c['d_e'], p, seed + 1, stamp=st2)
    g1 = eng.backward(params, c['nl'], c['d_x'], c['d_e'], p, seed, stamp=st1)
    assert any(not torch.equal(a, b) for a, b in zip(g1, g2))
    # the first forward again, alone: the same gradients bit for bit (nothing of the second forward leaked into its slot)
    eng.forward(params, c['xh'], c['ex'], None, None, c['nl'], None, p, seed)
    g1b = eng.backward(params, c['nl'], c['d_x'], c['d_e'], p, seed)
    assert all(torch.equal(a, b) for a, b in zip(g1, g1b))
    gs = eng.backward(params, c['nl'], (2.0 * c['d_x']).contiguous(), (2.0 * c['d_e']).contiguous(), p, seed)     # x 2: exact in binary
    assert all(torch.equal(2.0 * a, b) for a, b in zip(g1b, gs))
    gz = eng.backward(params, c['nl'], torch.zeros_like(c['d_x']), torch.zeros_like(c['d_e']), p, seed)
    assert all(float(g.abs().max()) == 0.0 for g in gz)

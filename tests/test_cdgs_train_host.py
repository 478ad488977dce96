"""CPU checks of the CDGS training path: the SAME kernel source libjodo_hip.so runs on the GPU (jodo_amd/csrc/cdgs_train.hip +
train_ops.h), compiled for the host by tests/emulcdgs/Makefile against the sequential stand-in for the HIP runtime of tests/emul/, driven
through jodo_amd.train.TrainEngineCDGS with host pointers, and compared with float64 / float32 autograd through the dense oracle
(tests/oracle_cdgs.py, tests/oracle_cdgs_train.py), with and without dropout, and with the reference's recorded forward
(tests/golden/fwd_cdgs_qm9.npz).  tests/test_cdgs_train_gpu.py repeats it on the device.  Cases and tolerances: tests/cdgs_train_common.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cdgs_train_common as C
import oracle_cdgs as OC
import oracle_cdgs_train as OCT
from helpers import FWD_ATOL, FWD_RTOL, close64, load_fixture
from jodo_amd.sampling import build_masks
from oracle import philox_ref as PR

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emulcdgs')


@pytest.fixture(scope='module')
def emul():
    subprocess.run(['make', '-C', EMUL_DIR, 'libjodo_cdgs_train_emul.so'], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_cdgs_train_emul.so'))


def engine_for(emul, model, n_nodes, N):
    from jodo_amd.train import TrainEngineCDGS
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    return TrainEngineCDGS(model._cfg_struct, n_nodes, N, named, 'cpu', lib=emul, stream_ptr=lambda: ctypes.c_void_p(0))


def tensors_of(model):
    return [v.detach().float().contiguous() for v in model.state_dict().values()]


def run(emul, c, p=0.0, seed=0, model=None, backward=True):
    model = C.model_for(c['which'])[1] if model is None else model
    eng = engine_for(emul, model, c['n_nodes'], c['N'])
    ts = tensors_of(model)
    out = eng.forward(ts, model._time_freq(), c['t'], c['x'], c['ex'], p, seed)
    grads = eng.backward(ts, c['x'], c['ex'], c['d_x'], c['d_e'], p, seed) if backward else None
    return eng, out, (None if grads is None else list(zip(C.param_names(model)[1], grads)))


def test_tensor_counts_and_option_refusals(emul):
    for which, n_tensors, n_params in (('qm9', 334, 326), ('geom', 260, 254)):
        _, model, _ = C.model_for(which)
        keys, params = C.param_names(model)
        assert (len(keys), len(params)) == (n_tensors, n_params) and len(list(model.parameters())) == n_params
    eng = engine_for(emul, C.model_for('qm9')[1], [3, 2], 4)
    assert sum(eng.is_buffer) == 8
    assert emul.jodo_cdgs_train_set_option(eng.handle, 2, 0) == 0
    assert emul.jodo_cdgs_train_set_option(eng.handle, 0, 1) != 0
    assert emul.jodo_cdgs_train_set_option(eng.handle, 7, 0) != 0


def test_masked_oracle_with_unit_masks_is_the_dense_oracle():
    c = C.random_case('w12')
    _, _, sd = C.model_for('qm9')
    sd64 = {k: v.double() for k, v in sd.items()}
    hp = c['hp']
    args = (sd64, hp, c['t'], c['x'], c['nm'], c['em'], c['ex'])
    with torch.no_grad():
        a = OC.forward(*args, return_blocks=True)
        for drop in (None, OCT.ones_masks(c['B'], c['N'], hp.n_layers, hp.nf)):
            b = OCT.forward_drop(*args, drop=drop, return_blocks=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(a[2], b[2]))


def test_padded_positions_of_the_masks_move_the_outputs():
    """With dropout, forcing the multipliers of the padded and diagonal edge positions to 1 moves the outputs by more than 100 x the
    forward bound: a kernel that skipped those positions could not pass the dropout tests."""
    c = C.random_case('w12')
    _, _, sd = C.model_for('qm9')
    sd64 = {k: v.double() for k, v in sd.items()}
    hp = c['hp']
    masks = OCT.drop_masks(77, 0.1, c['B'], c['N'], hp.n_layers, hp.nf)
    live = c['em'].reshape(c['B'], c['N'], c['N'], 1).double()
    forced = {k: (m * live + (1 - live) if k[1] in (5, 6) else m) for k, m in masks.items()}
    args = (sd64, hp, c['t'], c['x'], c['nm'], c['em'], c['ex'])
    with torch.no_grad():
        a, b = OCT.forward_drop(*args, drop=masks), OCT.forward_drop(*args, drop=forced)
    for u, v in zip(a, b):
        ratio = ((u - v).abs() / (FWD_ATOL + FWD_RTOL * u.abs())).max().item()
        print('padded multipliers forced to 1: %.1f x the forward bound' % ratio)
        assert ratio > 100


def test_mask_builder_is_drop_mul_element_by_element():
    B, N, L, Cw = 2, 3, 2, 8
    masks = OCT.drop_masks(2 ** 40 + 5, 0.5, B, N, L, Cw, dtype=torch.float32)
    shapes = OCT.site_shapes(B, N, Cw)
    for (l, s), m in masks.items():
        assert tuple(m.shape) == shapes[s]
        flat = PR.drop_mul(2 ** 40 + 5, 8 * l + s, 0.5, m.numel())
        for idx in range(m.numel()):
            assert float(m.reshape(-1)[idx]) == float(flat[idx])
        assert set(np.unique(flat).tolist()) == {0.0, 2.0}


def test_mask_builder_and_kernel_index_across_2_to_the_34(emul):
    """The windowed builder equals philox_ref.drop_mul element by element from element 0, and equals the kernels' own drop_mul (host
    build, element = row * width + f formed as the kernels form it) on windows of an edge site's [B N^2, 512] tile that begin at element
    0, straddle 2^32 (the first counter word's carry) and straddle 2^34 (where idx >> 34, the second counter word, becomes 1), and far
    beyond (2^38)."""
    from jodo_amd import capi
    capi.bind_cdgs_train(emul)
    seed, p, layer, site, W = 2 ** 40 + 5, 0.5, 3, 5, 512
    flat = PR.drop_mul(seed, 8 * layer + site, p, 4 * W + 3)
    win = OCT.drop_mul_window(seed, 8 * layer + site, p, 0, 4 * W + 3)
    for idx in range(flat.size):
        assert float(flat[idx]) == float(win[idx])
    assert np.array_equal(OCT.drop_mul_window(seed, 8 * layer + site, p, 1029, 777), flat[1029:1029 + 777])
    seen = set()
    for row0 in (0, 2 ** 32 // W - 2, 2 ** 34 // W - 3, 2 ** 38 // W + 1):
        rows = 6
        out = torch.empty(rows, W)
        assert emul.jodo_cdgs_train_debug_drop(p, seed, 8 * layer + site, row0, rows, W, ctypes.c_void_p(out.data_ptr()), None) == 0
        want = OCT.drop_mask_rows(seed, p, layer, site, row0, rows, W)
        if row0 * W < 2 ** 34:
            assert (row0 + rows) * W > 2 ** 34 or row0 * W < 2 ** 33
        for r in range(rows):
            for f in range(W):
                assert float(out[r, f]) == float(want[r, f]), (row0, r, f)
        seen.add(want.tobytes())
    assert len(seen) == 4                                        # the windows differ: the high index bits reach the counter


def test_forward_matches_the_reference_fixture(emul):
    fx = load_fixture('fwd_cdgs_qm9.npz')
    _, model = C.fresh_model('qm9', int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    eng = engine_for(emul, model, n_nodes, max(n_nodes))
    out_x, out_e = eng.forward(tensors_of(model), model._time_freq(), t('t'), t('x'), t('edge_x'), 0.0, 0)
    for got, want, what in ((out_x, t('out_x'), 'x'), (out_e, t('out_e'), 'e')):
        err = (got.double() - want.double()).abs()
        bound = FWD_ATOL + FWD_RTOL * want.double().abs()
        print('%s: worst err / bound %.3f' % (what, (err / bound).max().item()))
        assert bool((err <= bound).all())


@pytest.mark.parametrize('fixture', ['grad_cdgs_qm9.npz', 'train_drop_cdgs_qm9.npz'])
def test_recorded_reference_gradients(emul, fixture):
    """One call of the reference's own 2-D loss on its own module: with dropout off (grad_cdgs_qm9.npz), and under model.train() with
    every block's dropout module replaced by an object that applies the restated masks in the reference's call order
    (train_drop_cdgs_qm9.npz: this is what pins the site order 1 .. 6 and the placement of the masks).  The engine's outputs equal the
    recorded ones at the forward bound; every recorded gradient entry, and every tensor's max-abs and sum, equal the reference's within
    2e-4 of the tensor's largest entry — and so do the (masked) oracle's float64 gradients, which pins the yardstick of the other tests."""
    fx = load_fixture(fixture)
    p_drop, drop_seed = float(fx['p']) if 'p' in fx else 0.0, int(fx['drop_seed']) if 'drop_seed' in fx else 0
    assert (p_drop > 0) == fixture.startswith('train_drop')
    _, model = C.fresh_model('qm9', int(fx['seed']))
    n_nodes = fx['n_nodes'].tolist()
    N = max(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    eng = engine_for(emul, model, n_nodes, N)
    ts = tensors_of(model)
    out_x, out_e = eng.forward(ts, model._time_freq(), t('t'), t('z_t'), t('edge_z_t'), p_drop, drop_seed)
    for got, want, what in ((out_x, t('out_x'), 'x'), (out_e, t('out_e'), 'e')):
        err = (got.double() - want.double()).abs()
        assert bool((err <= FWD_ATOL + FWD_RTOL * want.double().abs()).all()), what
    grads = dict(zip(C.param_names(model)[1], eng.backward(ts, t('z_t'), t('edge_z_t'), t('d_out_x'), t('d_out_e'), p_drop, drop_seed)))
    nm, em = build_masks(n_nodes, N, 'cpu')
    case = dict(hp=OC.hparams(C.model_for('qm9')[0]), t=t('t'), x=t('z_t'), ex=t('edge_z_t'), nm=nm, em=em, d_x=t('d_out_x'), d_e=t('d_out_e'))
    hp = case['hp']
    masks_ = OCT.drop_masks(drop_seed, p_drop, len(n_nodes), N, hp.n_layers, hp.nf) if p_drop > 0 else None
    _, _, oracle = C.oracle_grads(model.state_dict(), case, torch.float64, drop=masks_)
    names = fx['grad_names'].tolist()
    assert sorted(names) == sorted(grads) and len(names) == 326
    worst = 0.0
    for i, k in enumerate(names):
        scale, want = float(fx['grad_maxabs'][i]), torch.from_numpy(fx['grad_%d' % i]).double()
        for what, g in (('engine', grads[k].double().reshape(-1)), ('oracle', oracle[k].reshape(-1))):
            part = g[torch.from_numpy(fx['idx_%d' % i])] if 'idx_%d' % i in fx else g
            rel = max(float((part - want).abs().max()), abs(float(g.abs().max()) - scale), abs(float(g.sum()) - float(fx['grad_sum'][i])) / g.numel()) / scale
            worst = max(worst, rel)
            assert rel < C.GRAD_REF_REL, "%s %s: %g" % (what, k, rel)
    print(fixture + ': recorded reference gradients: worst relative distance %.2e (bound %.0e)' % (worst, C.GRAD_REF_REL))


@pytest.mark.parametrize('name', ['mixed', 'w12', 'w9', 'geom', 'b65'])
def test_all_parameter_gradients_match_autograd_through_the_oracle(emul, name):
    c, (px, pe, want), (px32, pe32, want32) = C.yardsticks(name)
    _, out, grads = run(emul, c)
    close64(out[0], px32, px, name + ' x')
    close64(out[1], pe32, pe, name + ' e')
    B, N = c['B'], c['N']
    assert float((out[0] * (1 - c['nm'])).abs().max()) == 0.0 and float((out[1] * (1 - c['em'].reshape(B, N, N, 1))).abs().max()) == 0.0
    assert torch.equal(out[1], out[1].transpose(1, 2))
    C.assert_all_nonzero(want)
    assert len(grads) == len(want) == (254 if name == 'geom' else 326)
    C.compare_grads(grads, want, want32=want32, what=name)


@pytest.mark.parametrize('name,p', [('mixed', 0.0), ('mixed', 0.1), ('geom', 0.0), ('geom', 0.1)])
def test_kept_activations_match_the_oracle(emul, name, p):
    """After a training-mode forward: h and e after every block, alpha and the xhat of norm2_edge of every block (debug_fetch selectors
    0 - 3) against the oracle's per-block tensors."""
    c, yard = C.kept_yardsticks(name, p, 12345)
    eng, out, _ = run(emul, c, p, 12345, backward=False)
    close64(out[0], yard[torch.float32][0], yard[torch.float64][0], '%s dropout %g x' % (name, p))
    close64(out[1], yard[torch.float32][1], yard[torch.float64][1], '%s dropout %g e' % (name, p))
    C.check_kept(eng.debug_fetch, c, yard, '%s dropout %g' % (name, p))


def test_unconditioned_inputs_are_reported(emul):
    """REPORTED, not asserted on the gradients: `mixed` at input seed 5, which the conditioning rule of cdgs_train_common rejects (a ReLU
    argument of the float64 yardstick 4.5e-7 from zero in block 1).  Shows what one ReLU taking the other branch in a float32
    evaluation does to the gradient comparison, and whether the widening rule of compare_grads copes with it (it does not: the float32
    yardstick takes the float64 branch there).  The forward comparison is asserted as everywhere."""
    c = C.random_case('mixed', 5)
    _, _, sd = C.model_for(c['which'])
    margin = C.relu_margin(c, sd)
    (px, pe, want), (px32, pe32, want32) = C.oracle_grads(sd, c, torch.float64), C.oracle_grads(sd, c, torch.float32)
    _, out, grads = run(emul, c)
    close64(out[0], px32, px, 'unconditioned x')
    close64(out[1], pe32, pe, 'unconditioned e')
    assert all(bool(torch.isfinite(g).all()) for _, g in grads)
    try:
        C.compare_grads(grads, want, want32=want32, what='unconditioned mixed, seed 5')
        verdict = 'inside the bound'
    except AssertionError as e:
        verdict = str(e).split('\n')[0]
    print('unconditioned mixed, seed 5: smallest |ReLU argument| %.2e (rule %.0e); gradient comparison: %s' % (margin, C.RELU_MARGIN, verdict))
    assert margin <= C.RELU_MARGIN                               # still the case the rule exists for


def test_one_atom_molecules_have_exactly_zero_edge_embedding_gradients(emul):
    c, (px, pe, want), (px32, pe32, want32) = C.yardsticks('single')
    _, out, grads = run(emul, c)
    close64(out[0], px32, px, 'single x')
    assert float(out[1].abs().max()) == 0.0
    C.compare_grads(grads, want, want32=want32, what='single')
    got = dict(grads)
    for i in (2, 3, 4, 5):
        for leaf in ('weight', 'bias'):
            k = 'all_modules.%d.%s' % (i, leaf)
            assert float(want[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, k


def test_gradients_depend_on_the_padded_width(emul):
    """The same molecules at N = 9 and N = 12: both pass, and the engine's own gradients differ by more than 100 x the bound on every
    ff_linear3, ff_linear4 and norm2_edge tensor (the yardstick alone: >= 569)."""
    g9, g12 = dict(run(emul, C.yardsticks('w9')[0])[2]), dict(run(emul, C.yardsticks('w12')[0])[2])
    keys = [k for k in g9 if any(s in k for s in ('ff_linear3', 'ff_linear4', 'norm2_edge'))]
    assert len(keys) == 8 * 6
    for k in keys:
        ratio = (g9[k] - g12[k]).abs().max().item() / (C.GRAD_REL * g12[k].abs().max().item())
        assert ratio > 100, (k, ratio)


@pytest.mark.parametrize('name,p,seed', [('w12', 0.1, 12345), ('w9', 0.5, 2 ** 32 + 11)])
def test_training_mode_dropout_matches_the_masked_oracle(emul, name, p, seed):
    c, (px, pe, want), (px32, pe32, want32) = C.drop_yardsticks(name, p, seed)
    _, out, grads = run(emul, c, p, seed)
    close64(out[0], px32, px, name + ' dropout x')
    close64(out[1], pe32, pe, name + ' dropout e')
    C.compare_grads(grads, want, want32=want32, what='%s dropout %g' % (name, p))
    _, out2, _ = run(emul, c, p, seed, backward=False)
    assert torch.equal(out[0], out2[0]) and torch.equal(out[1], out2[1])


def test_backward_is_deterministic_and_linear(emul):
    c = C.random_case('w9')
    model = C.model_for('qm9')[1]
    eng = engine_for(emul, model, c['n_nodes'], c['N'])
    ts = tensors_of(model)
    eng.forward(ts, model._time_freq(), c['t'], c['x'], c['ex'], 0.1, 9)
    g1 = eng.backward(ts, c['x'], c['ex'], c['d_x'], c['d_e'], 0.1, 9)
    g2 = eng.backward(ts, c['x'], c['ex'], c['d_x'], c['d_e'], 0.1, 9)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    gs = eng.backward(ts, c['x'], c['ex'], (2.0 * c['d_x']).contiguous(), (2.0 * c['d_e']).contiguous(), 0.1, 9)     # x 2: exact in binary
    assert all(torch.equal(2.0 * a, b) for a, b in zip(g1, gs))
    gz = eng.backward(ts, c['x'], c['ex'], torch.zeros_like(c['d_x']), torch.zeros_like(c['d_e']), 0.1, 9)
    assert all(float(g.abs().max()) == 0.0 for g in gz)

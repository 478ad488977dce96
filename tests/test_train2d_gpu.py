"""The 2-D training path on the device (csrc/dgt2d_train.hip through jodo_amd.train.TrainEngine2D and the registered module with
`hip_training`): the checks of tests/test_train2d_emul.py repeated on an MI355X, `loss.backward()` on the module under the
dataparallel_keys wrapper, training steps through get_step_fn, the inference path after an optimiser step, and one B = 128 batch drawn
from the dataset's atom-count histogram.  Shapes, yardsticks and tolerances: tests/train2d_common.py.

(a) to (c) below ask for the fused form (train_fused.hip: k2d_chain_a / k2d_bwd_a, chain B / B', the node LayerNorm kernels;
options 0 and 1 of jodo_train2d_set_option); test_fused_matches_op_by_op compares it with the op-by-op reference form, which the
get_step_fn test runs (a module's default).  The fused chains
take LayerNorm's row sums in another order than the op-by-op kernels (a lane pair per row instead of eight partial sums), by design:
that comparison therefore uses the forward tolerance on the saved activations and the gradient rule on the gradients, not torch.equal."""
import os
import random

import numpy as np
import pytest
import torch

import oracle2d as O2
from oracle import philox_ref as PR

import train2d_common as C
from helpers import GOLDEN, load_fixture, make_config, make_model, masks

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def d(x):
    return None if x is None else x.to(DEV)


FUSED = {0: 1, 1: 1}            # jodo_train2d_set_option: fused forward and backward chains


def engine_for(model, n_nodes, options=FUSED):
    from jodo_amd.train import TrainEngine2D
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    return TrainEngine2D(model._cfg_struct, n_nodes, max(n_nodes), named, DEV, options=options), [k for k, _ in named]


def params_of(model):
    return [v.detach().float().contiguous() for v in model.state_dict().values()]


def test_loss_backward_on_the_wrapped_module_reproduces_the_reference_gradients():
    """(a) grad2d_zinc through `loss.backward()` on the registered module under the dataparallel_keys wrapper: prediction, loss, the
    reference's recorded gradients (2e-4) and all 235 gradients against float64 autograd through the oracle."""
    from jodo_amd.models import deterministic_init_
    from jodo_amd.models.utils import create_model
    fx = load_fixture('grad2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.device = DEV
    ref_model = make_model(cfg, int(fx['seed']), gain=float(fx['gain']), head_gain=float(fx['head_gain']))
    model = create_model(cfg)                                   # wrap = 'dataparallel_keys'
    model.module.load_state_dict(ref_model.state_dict())
    assert all(k.startswith('module.') for k in model.state_dict())
    model.module.hip_training = True
    model.module.train_options = dict(FUSED)
    model.eval()
    hp = O2.Hyper2D.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    pred, edge_pred = model(d(t('t')), d(t('z_t')), d(nm), d(em), edge_x=d(t('edge_z_t')), cond_x=d(t('cond_x')), cond_edge_x=d(t('cond_edge_x')),
                            noise_level=d(t('noise_level')))
    C.fwd_close(pred, t('pred'), 'pred vs reference')
    C.fwd_close(edge_pred, t('edge_pred'), 'edge_pred vs reference')
    loss = C.loss2d_from_outputs(cfg, pred, edge_pred, d(t('xh')), d(t('edge_x')), d(nm), d(em), d(t('alpha_t')), d(t('sigma_t')))
    assert abs(loss.item() - float(fx['loss'])) < 1e-5 * float(fx['loss'])
    pred.retain_grad(); edge_pred.retain_grad()
    loss.backward()
    got = {k[len('module.'):]: p.grad for k, p in model.named_parameters()}
    assert len(got) == 235 and all(g is not None for g in got.values())
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (got[k].cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < C.GRAD_REF_REL, "%s: %g" % (k, rel)
    args = (ref_model.state_dict(), hp, nm, em, t('z_t'), t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), pred.grad.cpu(), edge_pred.grad.cpu())
    _, _, want = C.oracle_grads(*args)
    _, _, want32 = C.oracle_grads(*args, dtype=torch.float32)
    C.compare_grads(got.items(), want, want32=want32, what='grad2d_zinc on the module')


# jodo_train2d_debug_locate selectors: hhat, alpha, f1, a1, f2, f3, a3, f4, xhat / rstd of the edges' LayerNorm1, et, t0, t1
SAVED = ('hhat', 'alpha', 'f1', 'a1', 'f2', 'f3', 'a3', 'f4', 'xh_e1', 'rs_e1', 'et', 't0', 't1')


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_fused_matches_op_by_op(which):
    """Self-conditioned call with dropout 0.1: every saved activation of every block found through jodo_train2d_debug_locate within the
    forward tolerance of the op-by-op form's (reduction order of the LayerNorm sums differs by design, see the module docstring), the
    outputs too, and every gradient within the gradient rule (rel_tol 3e-4 of the op-by-op gradient's scale).  The no-grad form of the
    fused forward (option 2 = 0: backward-only stores skipped) gives bit-identical outputs."""
    c = C.random_case(which, seed=5)
    _, model = C.model_for(which, 3)
    params = [d(q) for q in params_of(model)]
    p, seed = 0.1, 1234
    res = {}
    for form, opts in (('op', {0: 0, 1: 0}), ('fused', {0: 1, 1: 1})):
        eng, names = engine_for(model, c['n_nodes'], opts)
        out = eng.forward(params, d(c['xh']), d(c['ex']), d(c['cx']), d(c['cex']), d(c['nl']), None, p, seed)
        acts = {(w, l): eng.debug_fetch(i, l).cpu() for l in range(c['hp'].L) for i, w in enumerate(SAVED)}
        grads = [g.cpu() for g in eng.backward(params, d(c['nl']), d(c['d_x']), d(c['d_e']), p, seed)]
        res[form] = (out[0].cpu(), out[1].cpu(), acts, grads)
        if form == 'fused':
            o2 = eng.forward(params, d(c['xh']), d(c['ex']), d(c['cx']), d(c['cex']), d(c['nl']), None, p, seed, save_activations=False)
            assert torch.equal(o2[0].cpu(), out[0].cpu()) and torch.equal(o2[1].cpu(), out[1].cpu())
    C.fwd_close(res['fused'][0], res['op'][0], 'atom_pred, fused vs op-by-op')
    C.fwd_close(res['fused'][1], res['op'][1], 'edge_pred, fused vs op-by-op')
    worst = 0.0
    for key, a in res['op'][2].items():
        b = res['fused'][2][key]
        assert a.shape == b.shape and float(a.abs().max()) > 0
        err = (a.double() - b.double()).abs()
        ratio = float((err / (C.ATOL + C.RTOL * a.double().abs())).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s of block %d: worst err / bound %g" % (key[0], key[1], ratio)
    print('saved activations, fused vs op-by-op: worst err / bound %.3f' % worst)
    C.compare_grads(zip(names, res['fused'][3]), dict(zip(names, res['op'][3])), what='%s fused vs op-by-op' % which)


def test_recorded_moses_step_through_the_engine():
    """(a) grad2d_moses (nd = 7, ch = 3) through TrainEngine2D."""
    fx = load_fixture('grad2d_moses.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), gain=float(fx['gain']), head_gain=float(fx['head_gain']))
    hp = O2.Hyper2D.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    eng, names = engine_for(model, n_nodes)
    params = [d(q) for q in params_of(model)]
    out_x, out_e = eng.forward(params, d(t('z_t')), d(t('edge_z_t')), d(t('cond_x')), d(t('cond_edge_x')), d(t('noise_level')), None, 0.0, 0)
    C.fwd_close(out_x, t('pred'), 'pred vs reference')
    C.fwd_close(out_e, t('edge_pred'), 'edge_pred vs reference')
    px, pe = out_x.cpu().requires_grad_(True), out_e.cpu().requires_grad_(True)
    loss = C.loss2d_from_outputs(cfg, px, pe, t('xh'), t('edge_x'), nm, em, t('alpha_t'), t('sigma_t'))
    assert abs(loss.item() - float(fx['loss'])) < 1e-5 * float(fx['loss'])
    loss.backward()
    grads = eng.backward(params, d(t('noise_level')), d(px.grad.contiguous()), d(pe.grad.contiguous()), 0.0, 0)
    by_name = dict(zip(names, grads))
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (by_name[k].cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < C.GRAD_REF_REL, "%s: %g" % (k, rel)
    args = (model.state_dict(), hp, nm, em, t('z_t'), t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), px.grad, pe.grad)
    _, _, want = C.oracle_grads(*args)
    _, _, want32 = C.oracle_grads(*args, dtype=torch.float32)
    C.compare_grads(zip(names, grads), want, want32=want32, what='grad2d_moses')


@pytest.mark.parametrize('which,selfcond', [('zinc', False), ('zinc', True), ('moses', False), ('moses', True), ('zinc_chunks', False), ('zinc_chunks', True)])
def test_all_parameter_gradients_match_autograd_through_the_oracle(which, selfcond):
    """(b) First-step and self-conditioned call through the module (eval mode: no dropout), all 235 gradients; a no-grad call of the
    same module in eval mode goes to the inference kernels and agrees."""
    c, sd, (px, pe, want), (_, _, want32) = C.random_case_yardsticks(which, selfcond)
    _, model = C.model_for(which, 3, DEV)
    model.hip_training = True
    model.train_options = dict(FUSED)
    cx, cex = (c['cx'], c['cex']) if selfcond else (None, None)
    kw = dict(edge_x=d(c['ex']), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(c['nl']))
    nmd, emd = d(c['nm']), d(c['em'])
    ox, oe = model(d(c['nl']), d(c['xh']), nmd, emd, **kw)
    assert ox.requires_grad and oe.requires_grad
    C.fwd_close(ox, px, 'atom_pred')
    C.fwd_close(oe, pe, 'edge_pred')
    ((ox * d(c['d_x'])).sum() + (oe * d(c['d_e'])).sum()).backward()
    C.assert_all_nonzero(want)
    C.compare_grads([(k, p.grad) for k, p in model.named_parameters()], want, want32=want32, what='%s selfcond=%s' % (which, selfcond))
    with torch.no_grad():
        ix, ie = model(d(c['nl']), d(c['xh']), nmd, emd, **kw)
    assert model._last_plan is not None                          # the inference kernels ran
    C.fwd_close(ix, px, 'atom_pred, inference kernels')
    C.fwd_close(ie, pe, 'edge_pred, inference kernels')


def test_training_mode_dropout_reproduces_the_reference():
    """(c) train_drop2d_zinc replayed with its seeds on the device."""
    fx = load_fixture('train_drop2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), gain=float(fx['gain']), head_gain=float(fx['head_gain']))
    hp = O2.Hyper2D.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    p, s1, s2 = float(fx['p']), int(fx['seed1']), int(fx['seed2'])
    eng, names = engine_for(model, n_nodes)
    params = [d(q) for q in params_of(model)]
    o1 = eng.forward(params, d(t('xh')), d(t('edge_x')), None, None, d(t('noise_level')), None, p, s1, save_activations=False)
    C.fwd_close(o1[0], t('out1_x'), 'no-grad call, atoms')
    C.fwd_close(o1[1], t('out1_e'), 'no-grad call, edges')
    o2 = eng.forward(params, d(t('xh')), d(t('edge_x')), d(t('out1_x')), d(t('out1_e')), d(t('noise_level')), None, p, s2)
    C.fwd_close(o2[0], t('out2_x'), 'grad-enabled call, atoms')
    C.fwd_close(o2[1], t('out2_e'), 'grad-enabled call, edges')
    grads = eng.backward(params, d(t('noise_level')), d(t('d_out_x')), d(t('d_out_e')), p, s2)
    by_name = dict(zip(names, grads))
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (by_name[k].cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < C.GRAD_REF_REL, "%s: %g" % (k, rel)
    m2 = PR.dropout_masks(s2, p, n_nodes, hp.L, hp.D, hp.De, hp.r)
    args = (model.state_dict(), hp, nm, em, t('xh'), t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), t('d_out_x'), t('d_out_e'))
    _, _, want = C.oracle_grads(*args, drop=m2)
    _, _, want32 = C.oracle_grads(*args, dtype=torch.float32, drop=m2)
    C.compare_grads(zip(names, grads), want, want32=want32, what='train_drop2d_zinc')


def _loader_batch(cfg, n_nodes, seed):
    """A loader-shaped CPU batch of 2-D graphs."""
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    g = torch.Generator().manual_seed(seed)
    at = torch.randint(0, cfg.data.atom_types, (B, N), generator=g)
    bond = torch.triu(torch.randint(0, 4, (B, N, N), generator=g), 1)
    bond = bond + bond.transpose(1, 2)
    chans = [(bond > 0).float(), bond.float() / 3.] + ([(bond == 3).float()] if cfg.model.edge_ch == 3 else [])
    return dict(atom_mask=nm[..., 0], edge_mask=em, atom_one_hot=torch.nn.functional.one_hot(at, cfg.data.atom_types).float() * nm,
                edge_one_hot=torch.stack(chans, -1) * em.reshape(B, N, N, 1),
                formal_charges=torch.randint(-1, 2, (B, N, 1), generator=g).float() * nm)


def test_training_steps_through_get_step_fn():
    """Three steps through get_step_fn under model.train() with dropout 0.1, AdamW, warm-up and clipping: asking for a training step
    is the opt-in; the loss is finite, every parameter moves, the same seeds give bit-identical parameters; afterwards a no-grad
    inference forward equals the float64 oracle on the UPDATED weights, and the eval step_fn restores the live weights."""
    from jodo_amd import losses as L
    from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
    from jodo_amd.models.ema import ExponentialMovingAverage
    from jodo_amd.utils import get_data_scaler
    cfg = make_config('vpsde_zinc_2d_jodo')
    cfg.device = DEV
    cfg.optim.warmup = 10
    assert cfg.optim.optimizer == 'AdamW' and cfg.optim.grad_clip >= 0 and cfg.model.dropout == pytest.approx(0.1)
    batch = _loader_batch(cfg, [5, 9, 1, 12, 3, 2, 19, 33], 4)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)

    def run(n_steps):
        model = make_model(cfg, 6, DEV)
        assert model.hip_training is False
        opt = L.get_optimizer(cfg, model.parameters())
        state = dict(model=model, optimizer=opt, ema=ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_decay), step=1)
        step_fn = L.get_step_fn(ns, True, L.optimization_manager(cfg), get_data_scaler(cfg), cfg)
        random.seed(3)
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)
        losses = [float(step_fn(state, batch)) for _ in range(n_steps)]
        return model, state, losses

    before = make_model(cfg, 6, DEV).state_dict()
    model, state, losses = run(3)
    assert model.hip_training is True and model.training and all(np.isfinite(losses)) and state['step'] == 4
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v, before[k])]
    assert len(moved) == len(before) == 235
    model2, _, losses2 = run(3)
    assert losses == losses2 and all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), model2.state_dict().values()))
    # the evaluation step runs under the EMA weights and puts the live ones back
    live = [p.detach().clone() for p in model.parameters()]
    eval_fn = L.get_step_fn(ns, False, None, get_data_scaler(cfg), cfg)
    random.seed(3)
    assert np.isfinite(float(eval_fn(state, batch)))
    assert all(torch.equal(a, b.detach()) for a, b in zip(live, model.parameters()))
    # inference on the trained weights == float64 oracle on the same weights
    model.eval()
    c = C.random_case('zinc', seed=2, n_nodes=[6, 11, 3])
    sd64 = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    with torch.no_grad():
        got = model(d(c['nl']), d(c['xh']), d(c['nm']), d(c['em']), edge_x=d(c['ex']), cond_x=None, cond_edge_x=None, noise_level=d(c['nl']))
        want = O2.forward_dense(sd64, c['hp'], c['xh'].double(), c['nm'], c['em'], c['ex'].double(), None, None, c['nl'].double())
        stale = O2.forward_dense({k: v.cpu().double() for k, v in before.items()}, c['hp'], c['xh'].double(), c['nm'], c['em'], c['ex'].double(),
                                 None, None, c['nl'].double())
    C.fwd_close(got[0], want[0], 'atoms after three steps')
    C.fwd_close(got[1], want[1], 'edges after three steps')
    assert float((want[1] - stale[1]).abs().max()) > 1e-3         # the check can tell the updated weights from the initial ones


def test_full_training_batch_backward_is_linear_and_matches_the_oracle_on_a_slice():
    """One B = 128 batch drawn from ZINC250k's atom-count histogram, dropout on: the backward is linear in the output gradient and a
    replay is bit-identical; the forward of the full batch equals the forward of its first 8 molecules alone (molecules do not
    interact), whose gradients float64 autograd through the oracle then checks."""
    cfg, model = C.model_for('zinc', 8)
    hp = O2.Hyper2D.from_config(cfg)
    hist = O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k')['train_n_nodes']
    g = torch.Generator().manual_seed(5)
    sizes = torch.tensor(list(hist.keys()))
    n_nodes = sizes[torch.multinomial(torch.tensor(list(hist.values()), dtype=torch.float64), 128, replacement=True, generator=g)].tolist()
    c = C.random_case('zinc', seed=3, n_nodes=n_nodes)
    eng, names = engine_for(model, n_nodes)
    params = [d(q) for q in params_of(model)]
    p, seed = 0.1, 77
    ox, oe = eng.forward(params, d(c['xh']), d(c['ex']), None, None, d(c['nl']), None, p, seed)
    assert torch.isfinite(ox).all() and torch.isfinite(oe).all()
    gg = torch.Generator().manual_seed(1)
    d1x, d1e, d2x, d2e = (torch.randn(s, generator=gg).to(DEV) for s in (c['xh'].shape, c['ex'].shape, c['xh'].shape, c['ex'].shape))
    g1 = [t.clone() for t in eng.backward(params, d(c['nl']), d1x, d1e, p, seed)]
    g2 = [t.clone() for t in eng.backward(params, d(c['nl']), d2x, d2e, p, seed)]
    g3 = eng.backward(params, d(c['nl']), 0.5 * d1x - 2.0 * d2x, 0.5 * d1e - 2.0 * d2e, p, seed)
    bad = []
    for name, a, b, cc in zip(names, g1, g2, g3):
        want = 0.5 * a.double() - 2.0 * b.double()
        scale = max(float(a.abs().max()), float(b.abs().max()), 1e-12)
        err = float((cc.double() - want).abs().max())
        if err > 2e-4 * scale:
            bad.append('%s: %.3e of %.3e' % (name, err, scale))
    assert not bad, bad[:10]
    assert all(torch.equal(a, b) for a, b in zip(g1, eng.backward(params, d(c['nl']), d1x, d1e, p, seed)))
    ox0, oe0 = eng.forward(params, d(c['xh']), d(c['ex']), None, None, d(c['nl']), None, 0.0, 0)
    k = 8
    sub = n_nodes[:k]
    Ns = max(sub)
    nm_s, em_s = masks(sub)
    xs = (c['xh'][:k, :Ns] * nm_s).contiguous()
    es = (c['ex'][:k, :Ns, :Ns] * em_s.reshape(k, Ns, Ns, 1)).contiguous()
    nls = c['nl'][:k].contiguous()
    eng_s, _ = engine_for(model, sub)
    oxs, oes = eng_s.forward(params, d(xs), d(es), None, None, d(nls), None, 0.0, 0)
    C.fwd_close(ox0[:k, :Ns].cpu() * nm_s, oxs, 'slice of the full batch vs the slice alone, atoms')
    C.fwd_close(oe0[:k, :Ns, :Ns].cpu() * em_s.reshape(k, Ns, Ns, 1), oes, 'slice of the full batch vs the slice alone, edges')
    dxs, des = d1x[:k, :Ns].contiguous(), d1e[:k, :Ns, :Ns].contiguous()
    gs = eng_s.backward(params, d(nls), dxs, des, 0.0, 0)
    args = (model.state_dict(), hp, nm_s, em_s, xs, es, None, None, nls, dxs.cpu(), des.cpu())
    px, pe, want = C.oracle_grads(*args)
    _, _, want32 = C.oracle_grads(*args, dtype=torch.float32)
    C.fwd_close(oxs, px, 'slice, atoms vs float64 oracle')
    C.fwd_close(oes, pe, 'slice, edges vs float64 oracle')
    C.compare_grads(zip(names, gs), want, want32=want32, what='slice of 8 molecules')

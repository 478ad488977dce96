"""GPU parity of the training path of DGT_concat_sim (the 3-D score network without extra attention heads): the registered module with
`hip_training = True` under autograd (csrc/dgt_train.hip with n_extra = 0: 16 learned heads, one coordinate head; the fused chains
k_chain_c / k_bwd_c at one coordinate head) against the reference's recorded loss.backward() (tests/golden/grad_sim_qm9.npz) and
against autograd through tests/oracle_sim.py.  nf 256 is the only width the module builds.  tests/test_train_sim_emul.py runs the same
kernel sources on the host."""
import numpy as np
import pytest
import torch

from oracle import train_ref as T

import oracle_sim as OS
import train_sim_common as C
from helpers import compare_grads, load_fixture, make_config, make_model, random_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAME = 'DGT_concat_sim'
QM9, GEOM = 'vpsde_qm9_uncond_jodo', 'vpsde_geom_uncond_jodo'


def sim_model(cfg_name, seed, training=True, **kw):
    cfg = make_config(cfg_name, name=NAME)
    cfg.device = torch.device(DEV)
    model = make_model(cfg, seed, DEV, **kw)
    model.hip_training = bool(training)
    return cfg, model, OS.HyperSim.from_config(cfg)


def d(x):
    return None if x is None else x.to(DEV)


def call(model, xh, nm, em, ex, cx, cex, nl):
    return model(d(nl), d(xh), d(nm), d(em), edge_x=d(ex), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(nl))


def module_grads(model):
    return [(k, p.grad) for k, p in model.named_parameters()]


def test_loss_backward_on_the_module_reproduces_the_reference_gradients():
    """`loss.backward()` on the registered module with hip_training = True, driven by jodo_amd.losses' loss function on the reference's
    recorded training batch and seeds, reproduces tests/golden/grad_sim_qm9.npz: the reference's own diffused inputs (bit for bit),
    prediction, loss (2e-5 relative) and the gradients of its 17 recorded parameters (2e-4 relative); all 351 gradients equal float64
    autograd through the oracle by the gradient rule."""
    import random
    from jodo_amd import losses as L
    from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
    from jodo_amd.utils import get_data_scaler
    from helpers import grad_fixture_batch
    fx = load_fixture('grad_sim_qm9.npz')
    assert str(fx['model_name']) == NAME
    seed = int(fx['seed'])
    cfg, model, hp = sim_model(str(fx['cfg_name']), seed)
    batch, pyseed = grad_fixture_batch(cfg, fx['n_nodes'].tolist(), seed)
    assert pyseed == int(fx['py_seed'])
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    t = lambda k: torch.from_numpy(fx[k])
    cfg_cpu = make_config(str(fx['cfg_name']), name=NAME)
    cfg_cpu.device = torch.device('cpu')
    probe = []

    class Probe:
        def eval(self): pass
        def train(self): pass
        def __call__(self, t_, xh, node_mask, edge_mask, context=None, **kw):
            probe.append((t_, xh, node_mask, edge_mask, kw))
            return torch.zeros_like(xh), torch.zeros_like(kw['edge_x'])

    # The fixture was recorded on the CPU (the reference's noise samplers draw on the tensors' device): the diffusion inputs are rebuilt
    # by a CPU pass of the same loss_fn up to its first model call and must equal the recorded ones bit for bit.
    random.seed(pyseed)
    torch.manual_seed(seed)
    L.get_sde_graph_loss_fn(ns, False, get_data_scaler(cfg_cpu), cfg_cpu)(Probe(), batch)
    t_, z_t, nm, em, kw = probe[0]
    assert torch.equal(z_t, t('z_t')) and torch.equal(kw['edge_x'], t('edge_z_t')) and torch.equal(kw['noise_level'], t('noise_level'))
    with torch.no_grad():
        cx, cex = model(d(t_), d(z_t), d(nm), d(em), edge_x=d(kw['edge_x']), noise_level=d(kw['noise_level']), cond_x=None, cond_edge_x=None)
    C.forward_close(cx, t('cond_x'), 'self-conditioning prediction vs the reference')
    C.forward_close(cex, t('cond_edge_x'), 'self-conditioning edge prediction vs the reference')
    model.zero_grad()
    pred, edge_pred = model(d(t_), d(z_t), d(nm), d(em), edge_x=d(kw['edge_x']), noise_level=d(kw['noise_level']), cond_x=d(t('cond_x')),
                            cond_edge_x=d(t('cond_edge_x')))
    assert pred.requires_grad and edge_pred.requires_grad
    C.forward_close(pred, t('pred'), 'pred vs the reference')
    C.forward_close(edge_pred, t('edge_pred'), 'edge_pred vs the reference')
    lw = [float(w) for w in cfg.model.loss_weights.split(',')]
    loss = T.sde_graph_loss(pred, edge_pred, d(t('xh')), d(t('edge_x')), d(t('align_pos')), d(nm), d(em), d(t('alpha_t')), d(t('sigma_t')), lw,
                            cfg.training.reduce_mean)
    print('loss %.9g, the reference %.9g' % (loss.item(), float(fx['loss'])))
    assert abs(loss.item() - float(fx['loss'])) < 2e-5 * float(fx['loss'])
    loss.backward()
    grads = dict(model.named_parameters())
    assert len(grads) == 351
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (grads[k].grad.cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        print('%s: %.3e of the reference' % (k, rel))
        assert rel < 2e-4, "%s: %g" % (k, rel)
    px, pe = pred.detach().clone().requires_grad_(True), edge_pred.detach().clone().requires_grad_(True)
    T.sde_graph_loss(px, pe, d(t('xh')), d(t('edge_x')), d(t('align_pos')), d(nm), d(em), d(t('alpha_t')), d(t('sigma_t')), lw,
                     cfg.training.reduce_mean).backward()
    args = (model, hp, z_t, nm, em, kw['edge_x'], t('cond_x'), t('cond_edge_x'), kw['noise_level'], px.grad, pe.grad)
    want = C.oracle_param_grads(*args)[2]
    want32 = C.oracle_param_grads(*args, dtype=torch.float32)[2]
    compare_grads(module_grads(model), want, C.GRAD_REL, want32, C.K32, what='grad_sim_qm9')
    # the loss function itself on the module, self-conditioning forward included (on the device the noise samplers draw from another
    # generator than the recorded one: the loss and every gradient are finite)
    model.zero_grad()
    random.seed(pyseed)
    torch.manual_seed(seed)
    loss2 = L.get_sde_graph_loss_fn(ns, False, get_data_scaler(cfg), cfg)(model, batch)
    loss2.backward()
    assert np.isfinite(float(loss2.detach())) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


CASES = [
    (QM9, {}, [4, 1, 2, 6, 29, 17], False),          # first step; one- and two-atom molecules
    (GEOM, {}, [7, 3, 44], True),                    # 10 blocks, mlp_ratio 4, edge_ch 3, self-conditioned
    # 65 atoms next to the smallest molecule: one target's source column past a 64-lane pass of the inference attention kernels (the
    # training attention kernels walk the sources 16 per pass, four waves per atom: 65 = four full passes and one source), and 4 225 edge
    # rows = 64 chunks of 67 rows in the per-molecule two-level sums
    (QM9, {}, [65, 2], True),
]


@pytest.mark.parametrize("cfg_name,over,n_nodes,selfcond", CASES)
def test_parameter_gradients_match_autograd_through_the_oracle(cfg_name, over, n_nodes, selfcond):
    """Fused forms on (the default): outputs against float64 at the forward tolerance, every gradient against float64 autograd by the
    gradient rule (widened by float32 autograd), the training forward against the inference kernels, and a second forward + backward
    bit for bit."""
    cfg, model, hp = sim_model(cfg_name, 3, gain=1.5, coord_scale=0.05)
    xh, ex, nl, _, nm, em = random_inputs(hp, n_nodes, seed=5)
    cx, cex, d_x, d_e = C.selfcond_inputs(xh, ex, nm, em, selfcond)
    model.zero_grad()
    out_x, out_e = call(model, xh, nm, em, ex, cx, cex, nl)
    assert out_x.requires_grad
    px, pe, want = C.oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e)
    want32 = C.oracle_param_grads(model, hp, xh, nm, em, ex, cx, cex, nl, d_x, d_e, dtype=torch.float32)[2]
    C.forward_close(out_x, px, 'training forward, nodes vs float64')
    C.forward_close(out_e, pe, 'training forward, edges vs float64')
    ((out_x * d(d_x)).sum() + (out_e * d(d_e)).sum()).backward()
    assert int(model.last_flags[0]) == 0 and int(model.last_flags[3]) == (1 if selfcond else 0)
    compare_grads(module_grads(model), want, C.GRAD_REL, want32, C.K32, what='%s %s' % (cfg_name, n_nodes))
    with torch.no_grad():                                         # the inference kernels: an independent implementation
        ix, ie = call(model, xh, nm, em, ex, cx, cex, nl)
    C.forward_close(out_x, ix, 'training forward vs inference kernels, nodes')
    C.forward_close(out_e, ie, 'training forward vs inference kernels, edges')
    g1 = [p.grad.clone() for p in model.parameters()]
    model.zero_grad()
    o2 = call(model, xh, nm, em, ex, cx, cex, nl)
    ((o2[0] * d(d_x)).sum() + (o2[1] * d(d_e)).sum()).backward()
    assert torch.equal(o2[0], out_x) and torch.equal(o2[1], out_e)
    assert all(torch.equal(a, p.grad) for a, p in zip(g1, model.parameters()))      # fixed-order sums, no atomics


def test_fused_chains_equal_the_op_by_op_engine():
    """The fused forward and backward chains (k_chain_c / k_bwd_c with one coordinate head among them) against the op-by-op engine
    (train_options) under model.train() with dropout 0.1 and one seed: outputs at the forward tolerance, gradients by the rule of
    tests/test_train_gpu.py test_fused_forward_chains_equal_the_op_by_op_forward (2e-4 of the tensor's scale; 1e-3 on the Gaussian-layer
    and time-path parameters)."""
    cfg, model, hp = sim_model(QM9, 6, gain=1.2, coord_scale=0.05)
    n_nodes = [9, 29, 4, 1, 17]
    xh, ex, nl, _, nm, em = random_inputs(hp, n_nodes, seed=4)
    cx, cex, d_x, d_e = C.selfcond_inputs(xh, ex, nm, em, True, seed=3)
    model.train()
    assert model.dropout_p > 0
    res = {}
    for fused in ((1, 1), (1, 0), (0, 0)):
        model.train_options = {0: fused[0], 1: fused[1]}
        model.zero_grad()
        torch.manual_seed(77)
        ox, oe = call(model, xh, nm, em, ex, cx, cex, nl)
        ((ox * d(d_x)).sum() + (oe * d(d_e)).sum()).backward()
        res[fused] = (ox.detach().cpu(), oe.detach().cpu(), [p.grad.detach().cpu().clone() for p in model.parameters()])
    ref = res[(0, 0)]
    C.forward_close(res[(1, 1)][0], ref[0], 'fused vs op-by-op, nodes')
    C.forward_close(res[(1, 1)][1], ref[1], 'fused vs op-by-op, edges')
    assert not torch.equal(res[(1, 1)][0], ref[0])                     # different arithmetic: not the same code twice
    assert torch.equal(res[(1, 1)][0], res[(1, 0)][0])                 # the backward option does not touch the forward
    for key in ((1, 1), (1, 0)):
        bad = []
        for (name, _), a, b in zip(model.named_parameters(), res[key][2], ref[2]):
            scale, err = float(b.abs().max()), float((a - b).abs().max())
            tol = 1e-3 if ('dist_layer' in name or 'time_mlp' in name) else 2e-4
            if not err <= tol * max(scale, 1e-12) + 1e-9:
                bad.append("%s: %.3e of %.3e" % (name, err, scale))
        assert not bad, "fused %s vs op-by-op gradients differ:\n  " % (key,) + "\n  ".join(bad[:30])
    assert any(not torch.equal(a, b) for a, b in zip(res[(1, 1)][2], res[(1, 0)][2]))       # the fused backward really ran
    i2 = [k for k, _ in model.named_parameters()].index('e_block_3.equi_update.coord_mlp.2.weight')
    assert res[(1, 1)][2][i2].shape == (1, 256) and float(res[(1, 1)][2][i2].abs().max()) > 0


def test_training_steps_through_get_step_fn():
    """Two optimiser steps through get_step_fn on the 3-D sim config (FlatAdam, clipping, EMA run unmodified): the step function sets the
    switch, the losses are finite, every parameter moves, the inference forward after the steps follows the new weights (bit for bit the
    forward of a freshly built module loaded with them, and the oracle on them at the forward tolerance), and a DGT_concat module stepped
    beside it has no `hip_training` attribute afterwards."""
    import random
    from jodo_amd import losses as L
    from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
    from jodo_amd.models.ema import ExponentialMovingAverage
    from jodo_amd.utils import get_data_scaler
    from helpers import grad_fixture_batch
    cfg, model, hp = sim_model(QM9, 6, training=False)
    cfg.optim.warmup = 10
    assert model.hip_training is False
    batch, pyseed = grad_fixture_batch(cfg, [5, 9, 7, 12, 3, 1, 2, 19], 4)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    xh, ex, nl, _, nm, em = random_inputs(hp, [6, 11, 3], seed=2)
    model.eval()
    with torch.no_grad():
        stale = call(model, xh, nm, em, ex, None, None, nl)       # packs the blob and builds the plan the later call must not reuse stale
    before = {k: v.clone() for k, v in model.state_dict().items()}
    state = dict(model=model, optimizer=L.get_optimizer(cfg, model.parameters()),
                 ema=ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_decay), step=1)
    step_fn = L.get_step_fn(ns, True, L.optimization_manager(cfg), get_data_scaler(cfg), cfg)
    random.seed(pyseed)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    losses = [float(step_fn(state, batch)) for _ in range(2)]
    assert model.hip_training is True and model.training
    assert all(np.isfinite(losses)) and state['step'] == 3
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v, before[k])]
    assert len(moved) == len(before)
    model.eval()
    with torch.no_grad():
        got = call(model, xh, nm, em, ex, None, None, nl)
        fresh = make_model(cfg, 1, DEV)
        fresh.load_state_dict(model.state_dict())
        want = call(fresh, xh, nm, em, ex, None, None, nl)
        ora = OS.forward_dense({k: v.cpu() for k, v in model.state_dict().items()}, hp, xh, nm, em, ex, None, None, nl)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], stale[0])
    C.forward_close(got[0], ora[0], 'inference after the steps vs the oracle on the new weights, nodes')
    C.forward_close(got[1], ora[1], 'inference after the steps vs the oracle on the new weights, edges')
    # DGT_concat beside it: the step function gives it no switch
    cfg3 = make_config(QM9)
    cfg3.device = torch.device(DEV)
    cfg3.optim.warmup = 10
    m3 = make_model(cfg3, 6, DEV)
    st3 = dict(model=m3, optimizer=L.get_optimizer(cfg3, m3.parameters()), ema=ExponentialMovingAverage(m3.parameters(), decay=cfg3.model.ema_decay), step=1)
    random.seed(pyseed)
    assert np.isfinite(float(L.get_step_fn(ns, True, L.optimization_manager(cfg3), get_data_scaler(cfg3), cfg3)(st3, batch)))
    assert not hasattr(m3, 'hip_training')


def test_dropout_is_seeded_and_refusals_stay():
    """model.train() with dropout 0.1: two calls under one seed agree bit for bit (outputs and gradients), differ from p = 0, and the NaN
    guard stays down (flags[0] == 0).  Without the switch the module refuses as before; split_bf16 keeps raising with it."""
    cfg, model, hp = sim_model(QM9, 4, gain=1.5, coord_scale=0.05)
    n_nodes = [5, 1, 12, 3]
    xh, ex, nl, _, nm, em = random_inputs(hp, n_nodes, seed=8)
    cx, cex, d_x, d_e = C.selfcond_inputs(xh, ex, nm, em, True, seed=2)
    o0 = call(model, xh, nm, em, ex, cx, cex, nl)                 # eval mode: p = 0
    model.train()
    assert model.dropout_p == pytest.approx(0.1)
    runs = []
    for _ in range(2):
        model.zero_grad()
        torch.manual_seed(1234)
        ox, oe = call(model, xh, nm, em, ex, cx, cex, nl)
        ((ox * d(d_x)).sum() + (oe * d(d_e)).sum()).backward()
        assert int(model.last_flags[0]) == 0
        runs.append((ox.detach().clone(), oe.detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    assert not torch.equal(runs[0][0], o0[0].detach()) and not torch.equal(runs[0][1], o0[1].detach())
    with torch.no_grad():                                         # the no-grad self-conditioning call of a training step: same masks
        torch.manual_seed(1234)
        nx, ne = call(model, xh, nm, em, ex, cx, cex, nl)
    assert torch.equal(nx, runs[0][0]) and torch.equal(ne, runs[0][1])
    model.split_bf16 = True
    with pytest.raises(NotImplementedError, match='split-bf16'):
        call(model, xh, nm, em, ex, cx, cex, nl)
    model.split_bf16 = False
    model.hip_training = False
    with pytest.raises(NotImplementedError, match='inference'):
        call(model, xh, nm, em, ex, cx, cex, nl)
    x_req = xh.clone().to(DEV).requires_grad_(True)
    model.hip_training = True
    with pytest.raises(RuntimeError, match='parameter gradients only'):
        model(d(nl), x_req, d(nm), d(em), edge_x=d(ex), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(nl))

"""Host checks of the 2-D training step's Python side (jodo_amd/losses.py): get_sde_2D_loss_fn against the reference's own loss_fn
call (tests/golden/loss2d_zinc.npz: the recorded batch, seeds, draws, coin and loss) through a differentiable oracle-backed
stand-in for the module, the dispatch of get_step_fn, and the opt-in: a default DGT_concat_2D still refuses grad-enabled calls."""
import random

import pytest
import torch

import oracle2d as O2

from helpers import load_fixture, make_config, make_model, masks


class _OracleModule2D:
    """Differentiable CPU stand-in with the score-network call signature: forward_dense on leaf copies of the weights."""

    def __init__(self, sd, hp):
        self.sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        self.hp, self.calls, self.modes = hp, [], []

    def train(self):
        self.modes.append('train')
        return self

    def eval(self):
        self.modes.append('eval')
        return self

    def __call__(self, t, xh, node_mask, edge_mask, context=None, **kw):
        self.calls.append(dict(t=t.clone(), grad=torch.is_grad_enabled(), noise_level=kw['noise_level'].clone(), z_t=xh.clone(),
                               edge_z_t=kw['edge_x'].clone(), cond=kw.get('cond_x') is not None))
        return O2.forward_dense(self.sd, self.hp, xh, node_mask, edge_mask, kw['edge_x'], kw.get('cond_x'), kw.get('cond_edge_x'),
                                kw['noise_level'])


def _setup():
    from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
    from jodo_amd.utils import get_data_scaler
    fx = load_fixture('loss2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.device = 'cpu'
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    batch = {k[len('batch_'):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith('batch_')}
    model = make_model(cfg, int(fx['seed']), gain=float(fx['gain']), head_gain=float(fx['head_gain']))
    return fx, cfg, ns, get_data_scaler(cfg), batch, model


def test_2d_loss_fn_reproduces_the_reference_loss():
    from jodo_amd import losses as L
    fx, cfg, ns, scaler, batch, model = _setup()
    stand_in = _OracleModule2D(model.state_dict(), O2.Hyper2D.from_config(cfg))
    loss_fn = L.get_sde_2D_loss_fn(ns, False, scaler, cfg)
    torch.manual_seed(int(fx['seed']))
    random.seed(int(fx['py_seed']))
    loss = loss_fn(stand_in, batch)
    # the draws in the reference's order: t, node noise, edge noise from torch's generator, then the coin from python's
    assert stand_in.modes == ['eval'] and len(stand_in.calls) == 2 and float(fx['coin']) < 0.5
    first, second = stand_in.calls
    assert not first['grad'] and not first['cond'] and second['grad'] and second['cond']
    t = torch.from_numpy(fx['t'])
    assert torch.equal(second['t'], t)
    alpha_t, sigma_t = ns.marginal_prob(t)
    xh, edge_x, nm, em = L.process_batch_2D(batch, 'cpu', cfg.model.include_fc_charge, scaler)
    assert nm._jodo_counts.tolist() == fx['n_nodes'].tolist()
    e = lambda v, d: v.reshape((-1,) + (1,) * (d - 1))
    assert torch.equal(second['z_t'], e(alpha_t, 3) * xh + e(sigma_t, 3) * torch.from_numpy(fx['noise']))
    assert torch.equal(second['edge_z_t'], e(alpha_t, 4) * edge_x + e(sigma_t, 4) * torch.from_numpy(fx['edge_noise']))
    assert torch.equal(second['noise_level'], torch.log(alpha_t ** 2 / sigma_t ** 2))
    assert abs(loss.item() - float(fx['loss'])) < 1e-5 * float(fx['loss'])
    loss.backward()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in stand_in.sd.values())


def test_2d_loss_fn_noise_prediction_branch_and_reduce_mean():
    """Both pred_data branches of the loss arithmetic and reduce_mean, against the formulas written out."""
    from jodo_amd import losses as L
    fx, cfg, ns, scaler, batch, model = _setup()
    B = batch['atom_mask'].shape[0]
    for pred_data, reduce_mean in ((False, False), (False, True), (True, False)):
        cfg.model.pred_data, cfg.model.self_cond, cfg.training.reduce_mean = pred_data, False, reduce_mean
        seen = {}

        class _Const:
            def train(self):
                return self

            def eval(self):
                return self

            def __call__(self, t, xh, node_mask, edge_mask, **kw):
                seen.update(t=t, z=xh, ez=kw['edge_x'])
                return torch.zeros_like(xh), torch.zeros_like(kw['edge_x'])

        torch.manual_seed(5)
        loss = L.get_sde_2D_loss_fn(ns, True, scaler, cfg)(_Const(), batch)
        xh, edge_x, nm, em = L.process_batch_2D(batch, 'cpu', cfg.model.include_fc_charge, scaler)
        alpha_t, sigma_t = ns.marginal_prob(seen['t'])
        if pred_data:
            tar_x, tar_e = xh, edge_x
        else:       # z = alpha x + sigma noise
            tar_x = (seen['z'] - alpha_t.reshape(B, 1, 1) * xh) / sigma_t.reshape(B, 1, 1)
            tar_e = (seen['ez'] - alpha_t.reshape(B, 1, 1, 1) * edge_x) / sigma_t.reshape(B, 1, 1, 1)
        la = tar_x.square().mean(-1).sum(-1)
        le = tar_e.square().mean(-1).reshape(B, -1).sum(-1)
        if reduce_mean:
            la, le = la / nm.squeeze(-1).sum(-1), le / (em.reshape(B, -1).sum(-1) + 1e-8)
        _, wa, we = (float(w) for w in cfg.model.loss_weights.split(','))
        want = wa * la + we * le
        if pred_data:
            want = torch.sqrt(alpha_t / sigma_t) * want
        assert loss.item() == pytest.approx(want.mean().item(), rel=1e-4)


def test_get_step_fn_dispatches_for_2d_and_refuses_models_without_edges():
    from jodo_amd import losses as L
    fx, cfg, ns, scaler, batch, model = _setup()
    assert cfg.only_2D and cfg.pred_edge
    step_fn = L.get_step_fn(ns, True, L.optimization_manager(cfg), scaler, cfg)
    assert callable(step_fn)
    cfg.pred_edge = False
    with pytest.raises(NotImplementedError, match='pred_edge'):
        L.get_step_fn(ns, True, L.optimization_manager(cfg), scaler, cfg)
    cfg3 = make_config('vpsde_qm9_uncond_jodo')
    cfg3.pred_edge = False
    with pytest.raises(NotImplementedError, match='pred_edge'):
        L.get_step_fn(ns, True, L.optimization_manager(cfg3), scaler, cfg3)


def test_training_is_opt_in():
    """A default module keeps the refusal with its text; the attribute exists and defaults to False; with it set, inputs that want a
    gradient are refused and split_bf16 still raises."""
    cfg = make_config('vpsde_zinc_2d_jodo')
    model = make_model(cfg, seed=3)
    assert model.hip_training is False
    nm, em = masks([3, 2])
    xh, ex, nl = torch.zeros(2, 3, 10), torch.zeros(2, 3, 3, 2), torch.zeros(2)

    class _Cuda(torch.Tensor):                     # a CPU tensor that claims to live on the GPU: reaches the checks behind the device test
        is_cuda = True
    xc = xh.as_subclass(_Cuda)
    with pytest.raises(NotImplementedError, match='DGT_concat_2D is inference only: call it under torch.no_grad'):
        model(None, xc, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)
    model.hip_training = True
    with pytest.raises(RuntimeError, match='parameter gradients only'):
        model(None, xc, nm, em, edge_x=ex.clone().requires_grad_(True), cond_x=None, cond_edge_x=None, noise_level=nl)
    model.split_bf16 = True
    with pytest.raises(NotImplementedError, match='split_bf16'):
        model(None, xc, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)


def test_engine_classes_share_their_plumbing():
    from jodo_amd.train import TrainEngine, TrainEngine2D, dgt2d_autograd
    assert issubclass(TrainEngine2D, TrainEngine) and TrainEngine2D._abi == 'jodo_train2d' and TrainEngine._abi == 'jodo_train'
    for name in ('forward', 'backward', '_take_slot', '_upload_tables', 'new_pool', 'named_table'):
        assert getattr(TrainEngine2D, name) is getattr(TrainEngine, name)
    assert callable(dgt2d_autograd)

"""GPU: training-mode dropout against an independent statement of it.  The masks of the training path
(csrc/train_common.h drop_mul, applied by the element-wise kernels, the training GEMM's epilogue and the fused chains, and regenerated
by the backward) are restated in numpy (oracle/philox_ref.dropout_masks) and fed to the float64 oracle; the oracle with those masks
reproduces the reference under model.train() (tests/golden/train_drop_qm9.npz, tests/test_oracle_golden.py)."""
import pytest
import torch

from oracle import dgt_oracle as O
from oracle import philox_ref as PR
from oracle import train_ref as T

from helpers import load_fixture, make_config, make_model, masks, random_inputs
from test_train_emul import DROP_SEED, check_ffn_masks
from test_train_gpu import _compare_grads, close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _engine(model, n_nodes, options=None):
    from jodo_amd.train import TrainEngine
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    return TrainEngine(model._cfg(), n_nodes, max(n_nodes), named, DEV, options=options), [k for k, _ in named]


def _masked_oracle(model, hp, xh, nm, em, ex, cx, cex, nl, ctx, d_x, d_e, drop, dtype=torch.float64):
    sd = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model.state_dict().items()}
    c = lambda t: None if t is None else t.detach().cpu().to(dtype)
    px, pe = O.forward_dense(sd, hp, c(xh), c(nm), c(em), c(ex), c(cx), c(cex), c(nl), c(ctx), drop=drop)
    ((px * c(d_x)).sum() + (pe * c(d_e)).sum()).backward()
    return px.detach(), pe.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}


def _set_grads(model, names, grads):
    by_name = dict(zip(names, grads))
    for k, p in model.named_parameters():
        p.grad = by_name[k].detach().clone()


def test_reference_dropout_fixture_replayed_through_the_engine():
    """tests/golden/train_drop_qm9.npz through TrainEngine with the recorded seeds: the no-grad self-conditioning call (seed 1) and
    the grad-enabled call on its outputs (seed 2) reproduce the reference's outputs; the backward of the recorded output gradients
    reproduces its recorded gradients (every block's FFN biases among them) and every other gradient equals autograd through the
    float64 oracle with the restated masks."""
    fx = load_fixture('train_drop_qm9.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV, gain=float(fx['gain']))
    hp = O.Hyper.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    p, s1, s2 = float(fx['p']), int(fx['seed1']), int(fx['seed2'])
    assert s2 >= 2 ** 32
    t = lambda k: torch.from_numpy(fx[k])
    d = lambda x: x.to(DEV)
    eng, names = _engine(model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    o1 = eng.forward(params, d(t('xh')), d(t('edge_x')), None, None, d(t('noise_level')), None, p, s1)
    close(o1[0], t('out1_x'), atol=2e-5)
    close(o1[1], t('out1_e'), atol=2e-5)
    o2 = eng.forward(params, d(t('xh')), d(t('edge_x')), d(t('out1_x')), d(t('out1_e')), d(t('noise_level')), None, p, s2)
    assert eng.flags.tolist()[3] == 1
    close(o2[0], t('out2_x'), atol=2e-5)
    close(o2[1], t('out2_e'), atol=2e-5)
    grads = eng.backward(params, d(t('noise_level')), d(t('d_out_x')), d(t('d_out_e')), p, s2)
    by_name = dict(zip(names, grads))
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (by_name[k].cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < 2e-4, "%s: %g" % (k, rel)
    drop = PR.dropout_masks(s2, p, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio)
    args = (model, hp, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), None, t('d_out_x'), t('d_out_e'), drop)
    _, _, want = _masked_oracle(*args)
    _, _, want32 = _masked_oracle(*args, dtype=torch.float32)
    _set_grads(model, names, grads)
    _compare_grads(model, want, 3e-4, want32)


OPTION_SETS = [None, {0: 0, 1: 0, 3: 0, 4: 0}, {4: 2, 5: 2}]


@pytest.mark.parametrize("cfg_name,n_nodes,over,selfcond", [
    ('vpsde_qm9_uncond_jodo', [4, 1, 2, 6, 29, 17], {}, False),
    ('vpsde_geom_uncond_jodo', [5, 23], dict(nf=384), True),                   # mlp_ratio 4, edge_ch 3
    ('vpsde_qm9_cond_jodo', [3, 5, 18, 27], {}, True),                         # context
    ('vpsde_geom_uncond_jodo', [181, 2], dict(nf=128, n_layers=2), True),
])
def test_dropout_on_matches_the_masked_float64_oracle(cfg_name, n_nodes, over, selfcond):
    """p = 0.1 and a seed above 2^32 through the fused default path, the op-by-op path (forward, backward, one launch per weight
    gradient, op-by-op attention) and the one-wave attention / chunked Gaussian backward: outputs and every parameter's gradient
    against float64 autograd through the oracle with the restated masks (computed once per shape); plus a no-grad forward that skips
    the backward-only stores (the self-conditioning call of a training step)."""
    cfg = make_config(cfg_name, **over)
    model = make_model(cfg, 3, DEV, gain=1.5, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=5)
    g = torch.Generator().manual_seed(9)
    cx = cex = None
    if selfcond:
        cx = torch.randn(xh.shape, generator=g) * nm
        cex = torch.randn(ex.shape, generator=g)
        cex = (cex + cex.transpose(1, 2)) * em.reshape(ex.shape[0], ex.shape[1], ex.shape[1], 1)
    d_x, d_e = torch.randn(xh.shape, generator=g), torch.randn(ex.shape, generator=g)
    p, seed = 0.1, DROP_SEED
    drop = PR.dropout_masks(seed, p, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio)
    args = (model, hp, xh, nm, em, ex, cx, cex, nl, ctx, d_x, d_e, drop)
    px, pe, want = _masked_oracle(*args)
    _, _, want32 = _masked_oracle(*args, dtype=torch.float32)
    d = lambda x: None if x is None else x.to(DEV)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    for opts in OPTION_SETS:
        eng, names = _engine(model, n_nodes, opts)
        ox, oe = eng.forward(params, d(xh), d(ex), d(cx), d(cex), d(nl), d(ctx), p, seed)
        close(ox, px, atol=2e-5)
        close(oe, pe, atol=2e-5)
        grads = eng.backward(params, d(nl), d(d_x), d(d_e), p, seed)
        _set_grads(model, names, grads)
        print("options", opts)
        _compare_grads(model, want, 3e-4, want32)
    eng, _ = _engine(model, n_nodes)
    ox, oe = eng.forward(params, d(xh), d(ex), d(cx), d(cex), d(nl), d(ctx), p, seed, save_activations=False)
    close(ox, px, atol=2e-5)
    close(oe, pe, atol=2e-5)


def test_dropout_masks_of_the_kernels_on_the_config_training_batch():
    """The config's training batch (128 QM9 molecules, ~43 000 edge rows): the zero pattern of a1 = SiLU(f1) x dropout (the training
    GEMM's epilogue) and a3 (the fused edge chain, or the GEMM epilogue op by op) equals the restatement's, element for element, and
    kept values are SiLU(f) x 1 / (1 - p) to a few ulps; first and last block, fused and op-by-op forwards, p 0.1 and 0.5, seeds
    above 2^32."""
    from jodo_amd.models import load_dataset_info, get_node_dist
    cfg = make_config('vpsde_qm9_uncond_jodo')
    model = make_model(cfg, 8, DEV)
    hp = O.Hyper.from_config(cfg)
    torch.manual_seed(5)
    n_nodes = get_node_dist(load_dataset_info('qm9_with_h')).sample(int(cfg.training.batch_size)).tolist()
    assert sum(n * n for n in n_nodes) > 30000
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=3)
    d = lambda x: x.to(DEV)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    for opts in (None, {0: 0}):
        eng, _ = _engine(model, n_nodes, opts)
        for p, seed in ((0.1, DROP_SEED), (0.5, DROP_SEED + (3 << 32))):
            eng.forward(params, d(xh), d(ex), None, None, d(nl), None, p, seed)
            for l in (0, hp.n_layers - 1):
                print("options", opts, "p", p, "block", l)
                check_ffn_masks(eng, hp, n_nodes, p, seed, l, PR)


def test_a_training_step_under_model_train_matches_the_masked_oracle():
    """One step of jodo_amd.losses' loss function on the registered module under model.train() (self-conditioning branch taken):
    the module draws one dropout seed per call from torch's generator; with those two seeds' masks the float64 oracle reproduces the
    self-conditioning output, the prediction, the loss (train_ref.sde_graph_loss) and every parameter's gradient."""
    import random
    from jodo_amd import losses as L
    from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
    from jodo_amd.utils import get_data_scaler
    from helpers import grad_fixture_batch
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = DEV
    seed = 41
    n_nodes = [5, 9, 7]
    batch, pyseed = grad_fixture_batch(cfg, n_nodes, seed)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    model = make_model(cfg, seed, DEV, gain=1.5, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    p = float(cfg.model.dropout)
    assert p > 0
    calls = []
    hk = model.register_forward_hook(lambda m, a, kw, out: calls.append((a, dict(kw), [o.detach().clone() for o in out])), with_kwargs=True)
    random.seed(pyseed)
    torch.manual_seed(seed)
    cpu_state = torch.get_rng_state()
    model.zero_grad()
    try:
        loss = L.get_sde_graph_loss_fn(ns, True, get_data_scaler(cfg), cfg)(model, batch)
        assert model.training
        loss.backward()
    finally:
        hk.remove()
    torch.set_rng_state(cpu_state)
    s1, s2 = (int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2))
    assert len(calls) == 2 and calls[0][1]['cond_x'] is None and calls[1][1]['cond_x'] is not None
    (t_, z_t, nm, em), kw = calls[1][0][:4], calls[1][1]
    cpu = lambda x: None if x is None else x.detach().cpu()
    m1 = PR.dropout_masks(s1, p, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio)
    m2 = PR.dropout_masks(s2, p, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    c = lambda x: None if x is None else x.detach().cpu().double()
    with torch.no_grad():
        q1 = O.forward_dense(sd, hp, c(z_t), c(nm), c(em), c(kw['edge_x']), None, None, c(kw['noise_level']), None, drop=m1)
    close(calls[0][2][0], q1[0], atol=2e-5)
    close(calls[0][2][1], q1[1], atol=2e-5)
    pred, edge_pred = calls[1][2]
    xh, edge_x = L.process_edge_batch(batch, DEV, cfg.model.include_fc_charge, get_data_scaler(cfg), None)[:2]
    alpha_t, sigma_t = ns.marginal_prob(t_)
    align_pos = L.get_align_position(z_t, xh)
    lw = [float(w) for w in cfg.model.loss_weights.split(',')]
    px = pred.clone().requires_grad_(True)
    pe = edge_pred.clone().requires_grad_(True)
    ol = T.sde_graph_loss(px, pe, xh, edge_x, align_pos, nm, em, alpha_t, sigma_t, lw, cfg.training.reduce_mean)
    assert abs(ol.item() - loss.item()) <= 1e-5 * abs(loss.item())
    ol.backward()
    args = (model, hp, z_t, nm, em, kw['edge_x'], kw['cond_x'], kw['cond_edge_x'], kw['noise_level'], None, px.grad, pe.grad, m2)
    qx, qe, want = _masked_oracle(*args)
    close(pred, qx, atol=2e-5)
    close(edge_pred, qe, atol=2e-5)
    ql = T.sde_graph_loss(qx, qe, c(xh), c(edge_x), c(align_pos), c(nm), c(em), c(alpha_t), c(sigma_t), lw, cfg.training.reduce_mean)
    assert abs(ql.item() - loss.item()) <= 1e-4 * abs(loss.item()), (ql.item(), loss.item())
    _, _, want32 = _masked_oracle(*args, dtype=torch.float32)
    _compare_grads(model, want, 3e-4, want32)

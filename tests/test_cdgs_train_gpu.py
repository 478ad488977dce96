"""GPU: the CDGS training path (jodo_amd/models/cdgs.py hip_training, jodo_amd/train.py TrainEngineCDGS, csrc/cdgs_train.hip) against
float64 / float32 autograd through the dense oracle (tests/oracle_cdgs.py, tests/oracle_cdgs_train.py): forward under helpers.close64,
all 326 (QM9) / 254 (GEOM) parameter gradients under train2d_common.compare_grads, with and without dropout, reached through
loss.backward() on the registered module and through jodo_amd.losses.get_step_fn.  Cases and tolerances: tests/cdgs_train_common.py;
tests/test_cdgs_train_host.py runs the same kernels on the CPU."""
import random

import numpy as np
import pytest
import torch

import cdgs_train_common as C
import oracle_cdgs as OC
from helpers import FWD_ATOL, FWD_RTOL, close64, make_config

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_MODELS = {}


def d(v):
    return None if v is None else v.to(DEV)


def shared_model(which):
    """One device model per config with hip_training on, for the tests that do not touch the weights."""
    if which not in _MODELS:
        _MODELS[which] = C.fresh_model(which, device=DEV)[1]
        _MODELS[which].hip_training = True
    return _MODELS[which]


def module_grads(model, c):
    """Outputs and d <d_out, outputs> / d parameter through the registered module: a grad-enabled call and loss.backward()."""
    model.zero_grad(set_to_none=True)
    out_x, out_e = model(d(c['t']), d(c['x']), d(c['nm']), d(c['em']), edge_x=d(c['ex']))
    ((out_x * d(c['d_x'])).sum() + (out_e * d(c['d_e'])).sum()).backward()
    return (out_x.detach(), out_e.detach()), [(k, p.grad.detach().clone()) for k, p in model.named_parameters()]


def engine_run(model, c, p, seed, backward=True):
    """The engine of the case driven directly (a chosen dropout seed)."""
    eng = model._train_engine(d(c['nm']), d(c['em']), torch.device(DEV))
    ts = [v.detach().contiguous() for v in model.state_dict().values()]
    freq = model._time_freq().to(DEV)
    x, ex = d(c['x']).contiguous(), d(c['ex']).contiguous()
    out = eng.forward(ts, freq, d(c['t']), x, ex, p, seed)
    grads = [g.clone() for g in eng.backward(ts, x, ex, d(c['d_x']).contiguous(), d(c['d_e']).contiguous(), p, seed)] if backward else None
    return eng, ts, out, (None if grads is None else list(zip(C.param_names(model)[1], grads)))


@pytest.mark.parametrize('name', ['mixed', 'w12', 'w9', 'geom', 'b65'])
def test_forward_and_all_gradients_match_the_oracle(name):
    c, (px, pe, want), (px32, pe32, want32) = C.yardsticks(name)
    assert c['relu_margin'] > C.RELU_MARGIN
    model = shared_model(c['which'])
    with torch.no_grad():
        inf_x, inf_e = model(d(c['t']), d(c['x']), d(c['nm']), d(c['em']), edge_x=d(c['ex']))          # the inference kernels
    (out_x, out_e), grads = module_grads(model, c)
    close64(out_x, px32, px, name + ' train x')
    close64(out_e, pe32, pe, name + ' train e')
    close64(out_x, px32, inf_x.cpu().double(), name + ' train x vs inference')
    close64(out_e, pe32, inf_e.cpu().double(), name + ' train e vs inference')
    B, N = c['B'], c['N']
    assert float((out_x.cpu() * (1 - c['nm'])).abs().max()) == 0.0 and float((out_e.cpu() * (1 - c['em'].reshape(B, N, N, 1))).abs().max()) == 0.0
    assert torch.equal(out_e, out_e.transpose(1, 2))
    C.assert_all_nonzero(want)
    assert len(grads) == len(want) == (254 if name == 'geom' else 326)
    C.compare_grads(grads, want, want32=want32, what=name)


def test_wide_case_forward_and_all_gradients_match_the_oracle():
    """GEOM with one block at [100, 65, 1], N = 100: the first run of the engine above N = 44 and above 64 (30 000 tile rows)."""
    c, (px, pe, want), (px32, pe32, want32) = C.yardsticks('wide')
    assert c['relu_margin'] > C.RELU_MARGIN
    (out_x, out_e), grads = module_grads(shared_model(c['which']), c)
    close64(out_x, px32, px, 'wide train x')
    close64(out_e, pe32, pe, 'wide train e')
    B, N = c['B'], c['N']
    assert float((out_x.cpu() * (1 - c['nm'])).abs().max()) == 0.0 and float((out_e.cpu() * (1 - c['em'].reshape(B, N, N, 1))).abs().max()) == 0.0
    assert torch.equal(out_e, out_e.transpose(1, 2))
    C.assert_all_nonzero(want)
    assert len(grads) == len(want) == 74
    C.compare_grads(grads, want, want32=want32, what='wide')


@pytest.mark.parametrize('name,p', [('mixed', 0.0), ('mixed', 0.1), ('geom', 0.0), ('geom', 0.1), ('full', 0.0)])
def test_kept_activations_match_the_oracle(name, p):
    """After a training-mode forward: h and e after every block, alpha and the xhat of norm2_edge of every block (debug_fetch selectors
    0 - 3) against the oracle's per-block tensors; `full` is the GEOM config's own width, [181, 2] at N = 181, one block, forward only."""
    c, yard = C.kept_yardsticks(name, p, 12345)
    eng, _, out, _ = engine_run(shared_model(c['which']), c, p, 12345, backward=False)
    close64(out[0], yard[torch.float32][0], yard[torch.float64][0], '%s dropout %g x' % (name, p))
    close64(out[1], yard[torch.float32][1], yard[torch.float64][1], '%s dropout %g e' % (name, p))
    C.check_kept(eng.debug_fetch, c, yard, '%s dropout %g' % (name, p))


def test_one_atom_molecules_have_exactly_zero_edge_embedding_gradients():
    c, (px, pe, want), (px32, pe32, want32) = C.yardsticks('single')
    (out_x, out_e), grads = module_grads(shared_model('qm9'), c)
    close64(out_x, px32, px, 'single x')
    assert float(out_e.abs().max()) == 0.0
    C.compare_grads(grads, want, want32=want32, what='single')
    got = dict(grads)
    for i in (2, 3, 4, 5):
        for leaf in ('weight', 'bias'):
            k = 'all_modules.%d.%s' % (i, leaf)
            assert float(want[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, k


def test_gradients_depend_on_the_padded_width():
    """The same molecules and output gradients at N = 9 and N = 12 (both checked against the oracle above): the engine's own gradients
    differ by more than 100 x the bound on every ff_linear3, ff_linear4 and norm2_edge tensor (the yardstick alone: >= 569)."""
    model = shared_model('qm9')
    g9, g12 = dict(module_grads(model, C.yardsticks('w9')[0])[1]), dict(module_grads(model, C.yardsticks('w12')[0])[1])
    keys = [k for k in g9 if any(s in k for s in ('ff_linear3', 'ff_linear4', 'norm2_edge'))]
    assert len(keys) == 8 * 6
    for k in keys:
        ratio = (g9[k] - g12[k]).abs().max().item() / (C.GRAD_REL * g12[k].abs().max().item())
        assert ratio > 100, (k, ratio)


@pytest.mark.parametrize('name,p,seed', [('w12', 0.1, 12345), ('w9', 0.5, 2 ** 32 + 11)])
def test_training_mode_dropout_matches_the_masked_oracle(name, p, seed):
    c, (px, pe, want), (px32, pe32, want32) = C.drop_yardsticks(name, p, seed)
    model = shared_model(c['which'])
    _, _, out, grads = engine_run(model, c, p, seed)
    out = (out[0].clone(), out[1].clone())
    close64(out[0], px32, px, name + ' dropout x')
    close64(out[1], pe32, pe, name + ' dropout e')
    C.compare_grads(grads, want, want32=want32, what='%s dropout %g' % (name, p))
    _, _, out2, _ = engine_run(model, c, p, seed, backward=False)
    assert torch.equal(out[0], out2[0]) and torch.equal(out[1], out2[1])
    _, _, out3, _ = engine_run(model, c, p, seed + 1, backward=False)
    assert not torch.equal(out[1], out3[1])


def test_two_backward_calls_give_the_same_bits():
    c = C.random_case('mixed')
    model = shared_model('qm9')
    eng, ts, _, g1 = engine_run(model, c, 0.1, 9)
    x, ex = d(c['x']).contiguous(), d(c['ex']).contiguous()
    g2 = eng.backward(ts, x, ex, d(c['d_x']).contiguous(), d(c['d_e']).contiguous(), 0.1, 9)
    assert all(torch.equal(a[1], b) for a, b in zip(g1, g2))


def test_a_weight_update_reaches_the_next_forward_and_gradient():
    c = C.random_case('w9')
    _, model = C.fresh_model('qm9', device=DEV)
    model.hip_training = True
    out_a, g_a = module_grads(model, c)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith('ff_linear3.weight') or k == 'all_modules.5.weight':
                p.add_(0.05 * torch.randn_like(p))
    out_b, g_b = module_grads(model, c)
    assert not torch.equal(out_a[0], out_b[0]) and not torch.equal(out_a[1], out_b[1])
    same = [a[0] for a, b in zip(g_a, g_b) if torch.equal(a[1], b[1])]
    h0 = 10 + 3 * 8                                              # the heads' last biases: their gradient is the masked output gradient's sum
    assert same == ['all_modules.%d.bias' % (h0 + i) for i in (2, 5, 8)]
    sd = model.state_dict()
    (px, pe, want), (px32, pe32, want32) = C.oracle_grads(sd, c, torch.float64), C.oracle_grads(sd, c, torch.float32)
    close64(out_b[0], px32, px, 'updated x')
    close64(out_b[1], pe32, pe, 'updated e')
    margin = C.relu_margin(c, sd)
    if margin > C.RELU_MARGIN:                                   # (the conditioning rule of cdgs_train_common, on the updated weights)
        C.compare_grads(g_b, want, want32=want32, what='after a weight update')
    else:
        print('after a weight update: a ReLU argument of the float64 yardstick lies %.2e from zero (rule: %.0e): the gradient comparison '
              'is NOT made on these weights; forward and inference comparisons are' % (margin, C.RELU_MARGIN))
    with torch.no_grad():                                        # the packed inference weights follow too
        inf = model(d(c['t']), d(c['x']), d(c['nm']), d(c['em']), edge_x=d(c['ex']))
    close64(inf[1], pe32, pe, 'updated e, inference')


def _loader_batch(cfg, n_nodes, seed):
    """A loader-shaped CPU batch of 2-D graphs."""
    from jodo_amd.sampling import build_masks
    B, N = len(n_nodes), max(n_nodes)
    nm, em = build_masks(list(n_nodes), N, 'cpu')
    g = torch.Generator().manual_seed(seed)
    at = torch.randint(0, cfg.data.atom_types, (B, N), generator=g)
    bond = torch.triu(torch.randint(0, 4, (B, N, N), generator=g), 1)
    bond = bond + bond.transpose(1, 2)
    chans = [(bond > 0).float(), bond.float() / 3.] + ([(bond == 3).float()] if cfg.model.edge_ch == 3 else [])
    return dict(atom_mask=nm[..., 0], edge_mask=em, atom_one_hot=torch.nn.functional.one_hot(at, cfg.data.atom_types).float() * nm,
                edge_one_hot=torch.stack(chans, -1) * em.reshape(B, N, N, 1),
                formal_charges=torch.randint(-1, 2, (B, N, 1), generator=g).float() * nm)


class _OracleModule(torch.nn.Module):
    """The dense torch oracle as a module with the model's call: the same parameters in the same order, float32 on the device."""

    def __init__(self, model, cfg):
        super().__init__()
        self.names = list(model.state_dict().keys())
        self.is_param = [not k.endswith('local_model.eps') for k in self.names]
        sd = model.state_dict()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(sd[k].detach().clone()) for k, p in zip(self.names, self.is_param) if p])
        self.bufs = [sd[k].detach().clone() for k, p in zip(self.names, self.is_param) if not p]
        self.hp = OC.hparams(cfg)

    def forward(self, t, x, node_mask, edge_mask, **kw):
        ps, bufs = iter(self.ps), iter(self.bufs)
        sd = {k: (next(ps) if p else next(bufs)) for k, p in zip(self.names, self.is_param)}
        return OC.forward(sd, self.hp, t, x, node_mask, edge_mask, kw['edge_x'])


def _steps(cfg, model, batch, n_steps):
    from jodo_amd import losses as L
    from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
    from jodo_amd.models.ema import ExponentialMovingAverage
    from jodo_amd.utils import get_data_scaler
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    opt = L.get_optimizer(cfg, model.parameters())
    state = dict(model=model, optimizer=opt, ema=ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_decay), step=1)
    step_fn = L.get_step_fn(ns, True, L.optimization_manager(cfg), get_data_scaler(cfg), cfg)
    random.seed(3)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    losses = [float(step_fn(state, batch)) for _ in range(n_steps)]
    eval_fn = L.get_step_fn(ns, False, None, get_data_scaler(cfg), cfg)
    return state, losses, eval_fn


def test_training_steps_through_get_step_fn():
    """get_step_fn on vpsde_qm9_2d_cdgs, batch [1, 2, 5, 17, 29, 9].  Asking for a training step is the opt-in.
    (a) Dropout off: three AdamW steps equal three steps of the dense torch oracle (float32, same device) under the same loss, optimiser
    and draws, compared as tests/test_train2d_gpu.py::test_training_steps_through_get_step_fn compares: after the steps a no-grad
    inference forward on the UPDATED weights equals the float64 oracle on the same weights under helpers.close64 (and the check can tell
    them from the initial weights).  On top of it, from the project's own bounds: every step's loss within 2 x FWD_RTOL = 2e-4 relative
    (the loss is a mean of squares of outputs that agree to 1e-4 relative, and a parameter entry can differ after a step only where its
    gradient is below the gradient bound, i.e. where the loss does not feel it); and the direction of the whole three-step update: AdamW's
    first steps move every entry by about lr x sign(g), so the two updates differ where the sign of an entry can differ — entries with
    |g| <= K32 x GRAD_REL x max |g| of their tensor, a share f measured on the ORACLE's own gradients — which bounds the cosine by 1 - 2 f.
    (b) Dropout on (the config's 0.1): one step runs, the loss is finite, every parameter moves, the same seeds give the same bits.
    (c) The evaluation branch (train=False) returns a loss through the inference path and leaves the live weights in place."""
    cfg = make_config('vpsde_qm9_2d_cdgs')
    cfg.device = DEV
    cfg.optim.warmup = 10
    assert cfg.optim.optimizer == 'AdamW' and cfg.model.dropout == pytest.approx(0.1) and not cfg.model.pred_data
    batch = _loader_batch(cfg, [1, 2, 5, 17, 29, 9], 4)
    # (a)
    cfg.model.dropout = 0.0
    _, model = C.fresh_model('qm9', device=DEV)
    model.dropout_p = 0.0
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    oracle = _OracleModule(model, cfg).to(DEV)
    assert model.hip_training is False
    state, losses, _ = _steps(cfg, model, batch, 3)
    assert model.hip_training is True and model.training and state['step'] == 4 and all(np.isfinite(losses))
    _, losses_o, _ = _steps(cfg, oracle, batch, 3)
    print('losses HIP %s oracle %s' % (losses, losses_o))
    for a, b in zip(losses, losses_o):
        assert abs(a - b) <= 2 * FWD_RTOL * abs(b), (losses, losses_o)
    names = [k for k in before if not k.endswith('local_model.eps')]
    up = torch.cat([(model.state_dict()[k] - before[k]).reshape(-1) for k in names]).double()
    up_o = torch.cat([(p.detach() - before[k]).reshape(-1) for k, p in zip(names, oracle.ps)]).double()
    cos = float((up * up_o).sum() / (up.norm() * up_o.norm()))
    small = sum(int((p.grad.abs() <= C.K32 * C.GRAD_REL * p.grad.abs().max()).sum()) for p in oracle.ps)
    f = small / float(sum(p.numel() for p in oracle.ps))
    print('three-step update: cosine %.5f; share of entries whose sign the gradient bound does not fix %.4f -> bound %.4f' % (cos, f, 1 - 2 * f))
    assert cos >= 1 - 2 * f
    model.eval()
    c = C.random_case('w9')
    sd_new = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        got = model(d(c['t']), d(c['x']), d(c['nm']), d(c['em']), edge_x=d(c['ex']))
        args = (c['hp'], c['t'], c['x'], c['nm'], c['em'], c['ex'])
        r32 = OC.forward(sd_new, *args)
        r64 = OC.forward({k: v.double() for k, v in sd_new.items()}, *args)
        stale = OC.forward({k: v.cpu().double() for k, v in before.items()}, *args)
    close64(got[0], r32[0], r64[0], 'atoms after three steps')
    close64(got[1], r32[1], r64[1], 'edges after three steps')
    moved_by = float((r64[1] - stale[1]).abs().max())
    print('three steps move the edge output by %.3e' % moved_by)
    assert moved_by > 100 * FWD_ATOL                              # the check can tell the updated weights from the initial ones
    # (b)
    def run_drop():
        cfg_d = make_config('vpsde_qm9_2d_cdgs')
        cfg_d.device = DEV
        cfg_d.optim.warmup = 10
        m = C.fresh_model('qm9', device=DEV)[1]
        st, ls, ev = _steps(cfg_d, m, batch, 1)
        return cfg_d, m, st, ls, ev
    cfg_d, m1, state1, l1, eval_fn = run_drop()
    assert np.isfinite(l1[0]) and m1.training and m1.dropout_p == pytest.approx(0.1)
    moved = [k for k, v in m1.state_dict().items() if not torch.equal(v, before[k])]
    assert len(moved) == 326
    _, m2, _, l2, _ = run_drop()
    assert l1 == l2 and all(torch.equal(a, b) for a, b in zip(m1.state_dict().values(), m2.state_dict().values()))
    # (c)
    live = [p.detach().clone() for p in m1.parameters()]
    random.seed(3)
    assert np.isfinite(float(eval_fn(state1, batch)))
    assert not m1.training and all(torch.equal(a, b.detach()) for a, b in zip(live, m1.parameters()))


def test_dropout_index_across_2_to_the_34_on_the_device():
    """The kernels' dropout multipliers at element = row * 512 + f for rows around 2^32 / 512 and 2^34 / 512 (where the second Philox
    counter word, idx >> 34, becomes 1) and far beyond, against the windowed restatement of oracle.philox_ref.drop_mul."""
    import oracle_cdgs_train as OCT
    from jodo_amd import capi
    seed, p, layer, site, W, rows = 2 ** 40 + 5, 0.5, 3, 5, 512, 6
    for row0 in (0, 2 ** 32 // W - 2, 2 ** 34 // W - 3, 2 ** 38 // W + 1):
        out = torch.empty(rows, W, device=DEV)
        capi.check(capi.lib().jodo_cdgs_train_debug_drop(p, seed, 8 * layer + site, row0, rows, W, capi.ptr(out), capi.current_stream_ptr()),
                   'jodo_cdgs_train_debug_drop')
        want = torch.from_numpy(OCT.drop_mask_rows(seed, p, layer, site, row0, rows, W))
        assert torch.equal(out.cpu(), want), row0


def test_refusals():
    c = C.random_case('w9')
    _, model = C.fresh_model('qm9', device=DEV)
    args = lambda: (d(c['t']), d(c['x']), d(c['nm']), d(c['em']))
    with pytest.raises(NotImplementedError, match='inference only'):                 # hip_training unset: as before
        model(*args(), edge_x=d(c['ex']))
    model.hip_training = True
    with pytest.raises(RuntimeError, match='parameter gradients only'):
        model(*args(), edge_x=d(c['ex']).requires_grad_(True))
    with pytest.raises(RuntimeError, match='parameter gradients only'):
        model(d(c['t']), d(c['x']).requires_grad_(True), d(c['nm']), d(c['em']), edge_x=d(c['ex']))
    model.split_bf16 = True
    with pytest.raises(NotImplementedError, match='split_bf16'):
        model(*args(), edge_x=d(c['ex']))
    model.split_bf16 = False
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        model(c['t'], c['x'], c['nm'], c['em'], edge_x=c['ex'])


def test_workspace_larger_than_the_device_is_refused_before_allocating():
    """A batch whose dense tile cannot fit: the error names bytes wanted and bytes free, and nothing was allocated."""
    model = shared_model('qm9')
    B, N = 4096, 181                                             # 134 million tile rows: terabytes of kept activations
    nm = torch.ones(B, N, 1, device=DEV)
    nm._jodo_counts = np.full(B, N, np.int32)                    # (the counts the loss leaves: the masks are not read)
    used = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=r'needs \d+ bytes, the device has \d+ bytes free'):
        model._train_engine(nm, torch.zeros(1, N, N, device=DEV), torch.device(DEV))
    assert torch.cuda.memory_allocated() <= used + (1 << 20)

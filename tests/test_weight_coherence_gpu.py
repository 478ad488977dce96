"""GPU: the forward paths follow weight updates.  The module keeps derived device copies of its parameters — the packed fp32 blob, the
opt-in split-bf16 weight tape and the tape handed to each pinned plan — and every way a caller changes the weights must reach every
kernel of the next evaluation.  Stale weights give plausible outputs, so a tolerance test cannot see them; the oracle here is exact
instead: the kernels are deterministic, so a model whose weights were changed in place must give BIT-IDENTICAL outputs to a freshly
built model loaded with the same weights and run through the same calls.  One float64-oracle comparison per weight set and
configuration guards against both models sharing a bug.  (The CPU side of the bookkeeping: tests/test_weight_coherence_host.py.)"""
import pytest
import torch

from jodo_amd.models import get_model_class
from oracle import dgt_oracle as O

from forms_common import assert_pinned_call
from helpers import K64, close64, make_config, make_model, masks, oracle_32_64, random_inputs, state_dict_cpu

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

QM9_N = [3, 9, 17, 29, 12, 5, 1, 2, 28, 29, 18, 7, 23]          # several node strips, idle waves, n = 1 and 2
GEOM_N = [29, 7, 1, 2, 18, 25]
COND_N = [12, 29, 3, 17, 1, 8]

# path id -> (config, model overrides, split_bf16, n_streams, atom counts)
PATHS = {
    'exact-s1': ('vpsde_qm9_uncond_jodo', {}, False, 1, QM9_N),
    'exact-s2': ('vpsde_qm9_uncond_jodo', {}, False, 2, QM9_N),
    'split-s1': ('vpsde_qm9_uncond_jodo', {}, True, 1, QM9_N),             # pair update + node kernel
    'split-s2': ('vpsde_qm9_uncond_jodo', {}, True, 2, QM9_N),
    'split384-s1': ('vpsde_geom_uncond_jodo', dict(nf=384), True, 1, GEOM_N),   # pair update only
    'cond-s1': ('vpsde_qm9_cond_jodo', {}, False, 1, COND_N),               # the conditional model has no split form
}
ROUTES = ['data+invalidate', 'data+new-round', 'reference-ema', 'version-bump', 'load_state_dict']


def build(cfg, sd, split, streams):
    """A new model of `cfg` loaded with the CPU state_dict `sd` (the same construction for the model under test and `fresh`)."""
    model = get_model_class(cfg.model.name)(cfg)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    model.split_bf16, model.n_streams = split, streams
    return model


def settle(model, inp, nm, em, unpin=True):
    """A sampler's sequence on fixed inputs: first evaluation (no self-conditioning input), self-conditioned evaluation, pin_paths(),
    the self-conditioned evaluation again (under the pins: the split kernels where they are on), then the round's unpin.
    -> the three evaluations' outputs on the CPU [x1, e1, x2, e2, x3, e3]."""
    xh, ex, nl, ctx = inp
    inner = getattr(model, 'module', model)

    def ev(cx, cex):
        with torch.no_grad():
            return model(nl, xh, nm, em, edge_x=ex, cond_x=cx, cond_edge_x=cex, noise_level=nl, context=ctx)

    o1 = ev(None, None)
    o2 = ev(*o1)
    inner.pin_paths()
    pinned = list(inner._last_plans)
    o3 = ev(*o1)
    assert_pinned_call(inner, pinned)                            # AFTER the call: it ran on the plan(s) that were pinned
    assert inner.take_nan_count() == 0
    if unpin:
        inner.unpin_paths()
    torch.cuda.synchronize()
    return [t.cpu() for o in (o1, o2, o3) for t in o]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def assert_split_ran(model, split):
    plans = getattr(model, 'module', model)._last_plans
    assert all(('split_tape' in p) == split for p in plans), "the split kernels did not run where they should (or ran where they should not)"


class RefStyleEma:
    """Store / copy_to / restore that write through `param.data.copy_`, as the reference's EMA does: no version bump, no address
    change — only the content fingerprint of a new round (or an explicit invalidate) can notice."""

    def __init__(self, shadow):
        self.shadow = shadow

    def store(self, params):
        self.kept = [p.detach().clone() for p in params]

    def copy_to(self, params):
        for s, p in zip(self.shadow, params):
            p.data.copy_(s.data)

    def restore(self, params):
        for c, p in zip(self.kept, params):
            p.data.copy_(c.data)


_CFG, _CASE = {}, {}


@pytest.fixture(scope='module')
def cases():
    yield _case
    _CFG.clear()
    _CASE.clear()


def _config_data(cfg_name, over, n_nodes):
    """Per configuration: the two weight sets W and W' (CPU state_dicts) and the fixed inputs (device)."""
    key = (cfg_name, tuple(sorted(over.items())))
    if key not in _CFG:
        cfg = make_config(cfg_name, **over)
        hp = O.Hyper.from_config(cfg)
        W = state_dict_cpu(make_model(cfg, 11, 'cpu', coord_scale=0.05))
        Wp = state_dict_cpu(make_model(cfg, 12, 'cpu', gain=1.2, coord_scale=0.05))
        xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=5)
        nl = torch.full_like(nl, 0.3)                    # one noise level per batch, as in sampling: the pinned split kernels engage
        _CFG[key] = dict(cfg=cfg, hp=hp, W=W, Wp=Wp, cpu=(xh, ex, nl, ctx, nm, em),
                         inp=tuple(None if t is None else t.to(DEV) for t in (xh, ex, nl, ctx)), nm=nm.to(DEV), em=em.to(DEV))
    return _CFG[key]


def _case(path):
    """Per path: fresh(W') — a new model loaded with W', settled on the same masks — checked once against the float64 oracle."""
    if path not in _CASE:
        cfg_name, over, split, streams, n_nodes = PATHS[path]
        c = dict(_config_data(cfg_name, over, n_nodes), split=split, streams=streams)
        fresh = build(c['cfg'], c['Wp'], split, streams)
        want = settle(fresh, c['inp'], c['nm'], c['em'])
        assert_split_ran(fresh, split)
        del fresh
        xh, ex, nl, ctx, nm, em = c['cpu']
        r32, r64 = oracle_32_64(c['Wp'], c['hp'], xh, nm, em, ex, want[0], want[1], nl, ctx)
        close64(want[4], r32[0], r64[0], "%s: fresh(W') pinned self-conditioned nodes" % path, k=K64)
        close64(want[5], r32[1], r64[1], "%s: fresh(W') pinned self-conditioned edges" % path, k=K64)
        c['want_b'] = want
        _CASE[path] = c
    return _CASE[path]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("path", list(PATHS))
def test_weight_switch_reaches_every_kernel(cases, path, route):
    """A/B/A: settle on W (a), switch to W' through `route` and settle (b), switch back through the same route and settle (a2).
    b is bit-equal to fresh(W') and differs from a; a2 is bit-equal to a."""
    c = cases(path)
    model = build(c['cfg'], c['W'], c['split'], c['streams'])
    nm, em = c['nm'], c['em']
    a = settle(model, c['inp'], nm, em)
    names = [n for n, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    dev = lambda sd: [sd[n].to(DEV) for n in names]
    ema = RefStyleEma(dev(c['Wp']))

    def switch(sd, forward):
        if route in ('data+invalidate', 'data+new-round'):
            for p, q in zip(params, dev(sd)):
                p.data.copy_(q)
            if route == 'data+invalidate':                 # what jodo_amd.losses does around an evaluation under the EMA weights
                model.invalidate_packed_weights()
                return nm, em
            return nm.clone(), em.clone()                  # a new round: new mask tensors, same content
        if route == 'reference-ema':
            if forward:
                ema.store(params)
                ema.copy_to(params)
            else:
                ema.restore(params)
            return nm.clone(), em.clone()
        if route == 'version-bump':
            with torch.no_grad():
                for p, q in zip(params, dev(sd)):
                    p.copy_(q)
            return nm, em
        model.load_state_dict(sd)
        return nm, em

    b = settle(model, c['inp'], *switch(c['Wp'], True))
    assert_split_ran(model, c['split'])
    assert all(not torch.equal(x, y) for x, y in zip(a, b)), "the two weight sets give the same outputs: the test is vacuous"
    assert same(b, c['want_b']), "%s via %s: outputs differ from a fresh model loaded with the new weights" % (path, route)
    a2 = settle(model, c['inp'], *switch(c['W'], False))
    assert same(a2, a), "%s via %s: switching back does not give the first weights' outputs" % (path, route)


@pytest.mark.parametrize("route", ['version-bump', 'data+invalidate'])
@pytest.mark.parametrize("streams", [1, 2])
def test_weight_change_under_pinned_plans(cases, streams, route):
    """Weights changed between two calls on the same masks while the plans stay pinned (an optimiser step inside a round, or an
    explicit invalidate after a `.data` write): the next call's split kernels read the new tape — on every sub-batch plan when
    n_streams > 1."""
    c = cases('split-s%d' % streams)
    model = build(c['cfg'], c['W'], True, streams)
    settle(model, c['inp'], c['nm'], c['em'], unpin=False)
    assert all(p.get('pinned') for p in model._last_plans) and len(model._last_plans) == streams
    with torch.no_grad():
        for n, p in model.named_parameters():
            if route == 'version-bump':
                p.copy_(c['Wp'][n].to(DEV))
            else:
                p.data.copy_(c['Wp'][n].to(DEV))
    if route == 'data+invalidate':
        model.invalidate_packed_weights()
    want = c['want_b']
    xh, ex, nl, ctx = c['inp']
    with torch.no_grad():
        got = model(nl, xh, c['nm'], c['em'], edge_x=ex, cond_x=want[0].to(DEV), cond_edge_x=want[1].to(DEV), noise_level=nl)
    assert_split_ran(model, True)
    assert model.take_nan_count() == 0
    assert torch.equal(got[0].cpu(), want[4]) and torch.equal(got[1].cpu(), want[5]), \
        "n_streams=%d via %s: a pinned plan kept the old split tape" % (streams, route)


@pytest.mark.parametrize("hip_graph", [False, True])
def test_sampling_rounds_around_a_reference_style_ema_swap(cases, hip_graph):
    """Whole sampling rounds with the split kernels, eager and graph-replayed: round 1 on W, a reference-style copy_to of W' and round 2,
    restore and round 3.  One seed per call redraws the same atom counts, initial noise and in-kernel Philox draws, so round 2 equals a
    fresh model's round on W' and round 3 equals round 1, bit for bit."""
    from jodo_amd import fused
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models import get_node_dist, load_dataset_info
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    c = cases('split-s1')
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = torch.device(DEV)
    cfg.sampling.steps = 8
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    nodes_dist, inv = get_node_dist(load_dataset_info(cfg.data.info_name)), get_data_inverse_scaler(cfg)
    raw = []
    decode = fused.decode

    def recording_decode(config, x, e, nd):                # the round's end state as it reaches the decode
        raw.append((x.cpu(), e.cpu()))
        return decode(config, x, e, nd)

    def one_round(m):
        del raw[:]
        fn = get_sampling_fn(cfg, ns, nodes_dist, 16, 16, inv, shard=(0, 1), shard_mode='perf', seed=31, device_noise=True,
                             hip_graph=hip_graph)
        fused.decode = recording_decode
        try:
            fn(m)
        finally:
            fused.decode = decode
        assert len(raw) == 1 and not bool(torch.isnan(raw[0][0]).any())
        assert_split_ran(m, True)
        return list(raw[0])

    model = build(cfg, c['W'], True, 1)
    params = list(model.parameters())
    ema = RefStyleEma([c['Wp'][n].to(DEV) for n, _ in model.named_parameters()])
    r1 = one_round(model)
    ema.store(params)
    ema.copy_to(params)
    r2 = one_round(model)
    ema.restore(params)
    r3 = one_round(model)
    want2 = one_round(build(cfg, c['Wp'], True, 1))
    assert not same(r1, r2)
    assert same(r2, want2), "round 2 did not sample with the EMA weights in every kernel"
    assert same(r3, r1), "round 3 did not sample with the restored weights in every kernel"


def test_training_step_then_pinned_split_evaluation(cases):
    """One optimiser step through get_step_fn (FlatAdam: the parameters become views of one flat buffer, written through raw pointers,
    versions bumped explicitly) after the blob and tape of the pre-step weights were built: the next pinned split evaluation equals
    a fresh model loaded with the post-step weights, bit for bit."""
    import random
    from jodo_amd import losses as L
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models.ema import ExponentialMovingAverage
    from jodo_amd.optim import FlatAdam
    from jodo_amd.utils import get_data_scaler
    from tools.train_bench import synthetic_batch
    c = cases('split-s1')
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = torch.device(DEV)
    cfg.optim.warmup = 10
    model = build(cfg, c['W'], True, 1)
    before = settle(model, c['inp'], c['nm'], c['em'])
    pre = [p.detach().clone() for p in model.parameters()]
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    model.train()
    state = dict(model=model, optimizer=L.get_optimizer(cfg, model.parameters()), ema=ExponentialMovingAverage(model.parameters(), decay=0.999),
                 step=1)
    assert isinstance(state['optimizer'], FlatAdam)
    step_fn = L.get_step_fn(ns, True, L.optimization_manager(cfg), get_data_scaler(cfg), cfg)
    random.seed(3)
    torch.manual_seed(3)
    loss = step_fn(state, synthetic_batch(cfg, [5, 9, 4, 12, 7, 9], 60))
    assert bool(torch.isfinite(loss))
    model.eval()
    assert any(not torch.equal(a, p) for a, p in zip(pre, model.parameters())), "the step moved no parameter"
    got = settle(model, c['inp'], c['nm'], c['em'])
    assert_split_ran(model, True)
    want = settle(build(cfg, state_dict_cpu(model), True, 1), c['inp'], c['nm'], c['em'])
    assert same(got, want)
    assert not same(got, before)


def test_dataparallel_wrap_with_streams(cases):
    """torch.nn.DataParallel over one device hands the module a fresh view of the masks on every call: with n_streams = 2 a 5-step
    eager round keeps ONE cached split and the two sub-batch plans, and samples what the unwrapped model samples, bit for bit."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models.utils import sample_combined_position_feature_noise, sample_symmetric_edge_feature_noise
    from jodo_amd.sampling import AncestralSampler
    from jodo_amd.utils import get_self_cond_fn
    c = cases('split-s2')
    cfg = c['cfg']
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    smp = AncestralSampler(ns, torch.linspace(ns.T, 1e-3, 5), True, True, True, get_self_cond_fn(cfg))
    nm, em = masks(QM9_N, DEV)
    B, N = nm.shape[0], nm.shape[1]

    def sample(m):
        torch.manual_seed(9)
        z = sample_combined_position_feature_noise(B, N, c['hp'].in_node_dim, nm)
        edge_z = sample_symmetric_edge_feature_noise(B, N, c['hp'].edge_ch, em)
        with torch.no_grad():
            x, e = smp.sampling(m, z, nm, em, edge_z)
        torch.cuda.synchronize()
        return [x.cpu(), e.cpu()]

    model = build(cfg, c['W'], True, 2)
    got = sample(torch.nn.DataParallel(model, device_ids=[0]))
    assert len(model._splits) == 1, "the sub-batch split was recomputed for fresh views of the same masks"
    assert len(model._plans) == 2 and len(model._last_plans) == 2
    assert_split_ran(model, True)
    want = sample(build(cfg, c['W'], True, 2))
    assert same(got, want)

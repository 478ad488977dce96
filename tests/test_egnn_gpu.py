"""GPU tests of the property classifier (jodo_amd.cond_gen.EGNN, csrc/egnn_forward.hip) against the fixtures the reference's own module
produced (tools/make_egnn_golden.py; weights regenerated from the seed), its layout invariants, weight coherence, mask validation, and
the two conditional evaluation loops (one and two properties) on the HIP score network with the HIP classifier.

One batch hits every edge of the kernel: n_nodes = [1, 2, 5, 29, 31, 32, 33, 64, 65] at padded width 65 — no sources, one source, the
32-source chunk boundary from both sides, two full chunks, two chunks plus one source, and 32-row strips cut inside molecules."""
import functools

import numpy as np
import pytest
import torch

import oracle_egnn as OE
from helpers import close64, load_fixture, make_config, make_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = ['nf128_l7_a1_n0', 'nf64_l2_a0_n1', 'nf256_l1_a1_n1', 'nf192_l3_a1_n0']


@functools.lru_cache(maxsize=None)
def _case(tag):
    fx, fh = load_fixture('egnn_%s.npz' % tag), load_fixture('egnn_%s_h64.npz' % tag)
    st = OE.settings_of(fx)
    model, sd = OE.init_state_dict(st, int(fx['seed']))
    return fx, fh, st, model.to(DEV).eval(), sd


def _call(model, h0, x, n_nodes, edges=True):
    """h0 [B, N, nf_in], x [B, N, 3] (CPU) -> the classifier's result, called as the evaluation loops call it."""
    from jodo_amd.sampling import build_masks, full_edge_index
    B, N = h0.shape[0], h0.shape[1]
    nm, em = build_masks(list(n_nodes), N, DEV)
    with torch.no_grad():
        out = model(h0=h0.reshape(B * N, -1).to(DEV), x=x.reshape(B * N, 3).to(DEV), edges=full_edge_index(N, B, DEV) if edges else None,
                    edge_attr=None, node_mask=nm.reshape(B * N, 1), edge_mask=em, n_nodes=N)
    torch.cuda.synchronize()
    return out.cpu()


def _inputs(fx):
    return torch.from_numpy(fx['h0']), torch.from_numpy(fx['x']), fx['n_nodes'].tolist()


@pytest.mark.parametrize("tag", CASES)
def test_output_and_hidden_states_match_the_reference(tag):
    """Output and the hidden state after the first and the last layer against the reference's float64 values; the bound is
    max(2e-5 + 1e-4 |x|, 4 e32) with e32 the reference's own fp32 distance from float64 (helpers.close64)."""
    fx, fh, st, model, _ = _case(tag)
    h0, x, n_nodes = _inputs(fx)
    L = st['n_layers']
    t = torch.from_numpy
    out = _call(model, h0, x, n_nodes)
    print("%s output: err %.3e, reference fp32 %.3e" % ((tag,) + close64(out, t(fx['out32']), t(fx['out64']), 'egnn %s output' % tag)))
    try:
        for layers, r32, r64 in ((1, fx['hid32'][0], fh['first']), (L, fx['hid32'][L - 1], fh['last'] if L > 1 else fh['first'])):
            model.max_layers = layers
            hid = _call(model, h0, x, n_nodes)
            assert hid.shape == r64.shape
            print("%s hidden after %d: err %.3e, reference fp32 %.3e" % ((tag, layers) + close64(hid, t(r32), t(r64), 'egnn %s hidden %d' % (tag, layers))))
    finally:
        model.max_layers = -1


def test_result_does_not_depend_on_padding_batch_order_or_neighbours():
    fx, _, st, model, _ = _case(CASES[0])
    h0, x, n_nodes = _inputs(fx)
    B, N = h0.shape[0], h0.shape[1]
    base = _call(model, h0, x, n_nodes)
    # the same molecules at width 80, junk on the padding atoms
    g = torch.Generator().manual_seed(5)
    h0w, xw = torch.zeros(B, 80, h0.shape[2]), 3.0 * torch.randn(B, 80, 3, generator=g)
    h0w[:, :, 1] = 1.0
    for b, n in enumerate(n_nodes):
        h0w[b, :n], xw[b, :n] = h0[b, :n], x[b, :n]
    assert torch.equal(_call(model, h0w, xw, n_nodes), base)
    # reversed batch order: the sums are per atom and per molecule
    assert torch.equal(_call(model, h0.flip(0), x.flip(0), n_nodes[::-1]), base.flip(0))
    # every molecule alone
    for b, n in enumerate(n_nodes):
        assert torch.equal(_call(model, h0[b:b + 1], x[b:b + 1], [n], edges=False), base[b:b + 1]), "molecule %d alone" % b


def test_output_follows_weight_updates():
    fx, _, st, _, _ = _case(CASES[1])
    h0, x, n_nodes = _inputs(fx)
    model, _ = OE.init_state_dict(st, int(fx['seed']))
    model = model.to(DEV).eval()

    def check(what):
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        r32, _ = OE.forward(sd, st, h0, x, n_nodes)
        r64, _ = OE.forward(sd, st, h0, x, n_nodes, torch.float64)
        close64(_call(model, h0, x, n_nodes), r32, r64, what)
        return r64

    first = check('initial weights')
    p = model.gcl_1.node_mlp[2].weight
    p.data.mul_(1.5)                                         # no version bump: needs the explicit call
    model.invalidate_packed_weights()
    second = check('after .data.mul_ + invalidate_packed_weights')
    assert float((second - first).abs().max()) > 1e-2
    with torch.no_grad():
        model.embedding.weight.mul_(0.5)                     # bumps the version: followed without the call
    third = check('after an in-place update')
    assert float((third - second).abs().max()) > 1e-2


def test_invalid_masks_raise():
    from jodo_amd.sampling import build_masks
    fx, _, st, model, _ = _case(CASES[1])
    h0, x, n_nodes = _inputs(fx)
    B, N = h0.shape[0], h0.shape[1]
    nm, em = build_masks(n_nodes, N, DEV)
    args = dict(h0=h0.reshape(B * N, -1).to(DEV), x=x.reshape(B * N, 3).to(DEV), edges=None, edge_attr=None, n_nodes=N)
    assert model.validate_masks
    bad_nm = nm.clone()
    bad_nm[2, 0], bad_nm[2, 6] = 0.0, 1.0                    # 5 atoms, not a prefix
    bad_em = em.clone().reshape(B, N, N)
    bad_em[3, 4, 4] = 1.0                                    # a live diagonal entry
    with torch.no_grad():
        with pytest.raises(ValueError, match="prefix"):
            model(node_mask=bad_nm.reshape(B * N, 1), edge_mask=em, **args)
        with pytest.raises(ValueError, match="diagonal"):
            model(node_mask=nm.reshape(B * N, 1), edge_mask=bad_em.reshape(B * N * N, 1), **args)
        model(node_mask=nm.reshape(B * N, 1), edge_mask=em, **args)


# ---- the evaluation loops on the HIP score network with the HIP classifier -------------------------------------------------------------
class _FixedNodes:
    def __init__(self, rounds):
        self.rounds, self.calls = rounds, 0

    def sample(self, n):
        out = torch.tensor(self.rounds[self.calls])
        self.calls += 1
        assert len(out) == n
        return out


class _Ctx:
    def __init__(self, cols):
        self.cols, self.seen = cols, []

    def sample_batch(self, n_nodes):
        c = torch.randn(len(n_nodes), self.cols)
        self.seen.append(c.clone())
        return c


LISTS = [[27, 5, 9, 14], [8, 27, 2, 20]]


def _classifier(seed):
    st = dict(hidden_nf=128, n_layers=7, attention=1, node_attr=0, in_node_nf=5)      # the published classifier's settings
    model, sd = OE.init_state_dict(st, seed)
    return st, model.to(DEV).eval(), sd


def _oracle_mae(mols, st, sd, targets, mean, mad, atom_types):
    errs = []
    for k, (pos, at, et, fc) in enumerate(mols):
        h0 = torch.nn.functional.one_hot(at, atom_types).double().unsqueeze(0)
        pred, _ = OE.forward(sd, st, h0, pos.unsqueeze(0), [pos.shape[0]], torch.float64)
        errs.append(abs(float(pred[0]) * mad + mean - (float(targets[k]) * mad + mean)))
    return sum(errs) / len(errs)


def test_single_property_loop_with_the_hip_classifier():
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import get_cond_sampling_eval_fn
    from jodo_amd.utils import get_data_inverse_scaler
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.device = torch.device(DEV)
    cfg.sampling.steps, cfg.sampling.method = 5, 'ancestral'
    model = make_model(cfg, 12, DEV, head_gain=10.0)
    st, clf, sd = _classifier(21)
    mean, mad = 75.3, 6.3
    ctx = _Ctx(1)
    torch.manual_seed(41)
    fn = get_cond_sampling_eval_fn(cfg, NoiseScheduleVP(cfg.sde.schedule), _FixedNodes([sum(LISTS, [])]), 4, 7, get_data_inverse_scaler(cfg),
                                   prop_dist=ctx, prop_norm={cfg.cond_property: {'mean': mean, 'mad': mad}})
    mols, score = fn(model, clf)
    assert len(mols) == 7 and [int(m[0].shape[0]) for m in mols] == sum(LISTS, [])[:7]
    want = _oracle_mae(mols, st, sd, torch.cat(ctx.seen).squeeze(-1), mean, mad, cfg.data.atom_types)
    print("score %.6f, float64 oracle %.6f" % (score, want))
    assert abs(score - want) < 1e-3 * max(1.0, score)        # outputNorm['alpha'] = 1


def test_two_property_loop_with_hip_classifiers_under_data_parallel():
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import get_cond_multi_sampling_eval_fn, get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    cfg = make_config('vpsde_qm9_cond_multi_jodo')
    assert cfg.model.cond_ch == 2
    cfg.device = torch.device(DEV)
    cfg.sampling.steps, cfg.sampling.method = 5, 'ancestral'
    model = make_model(cfg, 12, DEV, head_gain=10.0)
    ns, inv = NoiseScheduleVP(cfg.sde.schedule), get_data_inverse_scaler(cfg)
    (st, clf1, sd1), (_, clf2, sd2) = _classifier(21), _classifier(22)
    norm = {cfg.cond_property1: {'mean': 75.3, 'mad': 6.3}, cfg.cond_property2: {'mean': 2.7, 'mad': 1.2}}
    ctx = _Ctx(2)
    torch.manual_seed(41)
    fn = get_cond_multi_sampling_eval_fn(cfg, ns, _FixedNodes([sum(LISTS, [])]), 4, 7, inv, prop_dist=ctx, prop_norm=norm)
    wrap = lambda m: torch.nn.DataParallel(m, device_ids=[0])
    mols, score1, score2 = fn(model, wrap(clf1), wrap(clf2))
    assert len(mols) == 7 and [int(m[0].shape[0]) for m in mols] == sum(LISTS, [])[:7]
    torch.manual_seed(41)
    plain = get_sampling_fn(cfg, ns, _FixedNodes([sum(LISTS, [])]), 4, 8, inv, prop_dist=_Ctx(2), return_raw=True, fused_decode=False,
                            device_noise=False)(model)
    for got, want in zip(mols, plain):
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    targets = torch.cat(ctx.seen)
    for k, (score, sd, prop) in enumerate(((score1, sd1, cfg.cond_property1), (score2, sd2, cfg.cond_property2))):
        want = _oracle_mae(mols, st, sd, targets[:, k], norm[prop]['mean'], norm[prop]['mad'], cfg.data.atom_types)
        print("property %d (%s): score %.6f, float64 oracle %.6f" % (k + 1, prop, score, want))
        assert abs(score - want) < 1e-3 * max(1.0, score)    # outputNorm of alpha and mu = 1
    assert abs(score1 - score2) > 1e-6
    with pytest.raises(RuntimeError, match="DataParallel"):
        clf1._replicate_for_data_parallel()

"""GPU tests of the property classifier's training path (EGNN.hip_training, csrc/egnn_train.hip, jodo_amd.cond_gen.train): every
parameter gradient against float64 autograd through tests/oracle_egnn_train.py, the training forward against the inference forward and
the fixtures, determinism, layout invariance, every instantiation of the edge backward kernel past one trip of its persistent loop, live
weights, the refusals, and the optimiser step.  Cases, shapes and the bound: tests/egnn_train_common.py."""
import functools

import pytest
import torch

import egnn_scale_common as S
import egnn_train_common as C
import oracle_egnn as OE
import oracle_egnn_train as OET
from helpers import close64
from train2d_common import compare_grads

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _args(h0, x, n_nodes):
    from jodo_amd.sampling import build_masks, full_edge_index
    B, N = h0.shape[0], h0.shape[1]
    nm, em = build_masks(list(n_nodes), N, DEV)
    return dict(h0=h0.reshape(B * N, -1).to(DEV), x=x.reshape(B * N, 3).to(DEV), edges=full_edge_index(N, B, DEV), edge_attr=None,
                node_mask=nm.reshape(B * N, 1), edge_mask=em, n_nodes=N)


def _train_call(model, h0, x, n_nodes):
    """The grad-enabled call of a module with hip_training set: out [B] on the device, attached to the graph."""
    return model(**_args(h0, x, n_nodes))


def _infer(model, h0, x, n_nodes):
    with torch.no_grad():
        out = model(**_args(h0, x, n_nodes))
    torch.cuda.synchronize()
    return out.cpu()


def _grads(model, h0, x, n_nodes, d_out):
    """(out [B] on the CPU, [(name, gradient on the CPU)]) of <d_out, out> through the HIP training path."""
    model.zero_grad(set_to_none=True)
    out = _train_call(model, h0, x, n_nodes)
    out.backward(d_out.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), [(k, p.grad.detach().cpu().clone()) for k, p in model.named_parameters()]


def _fresh(tag):
    fx, st, sd, h0, x, n_nodes, d_out = C.case(tag)
    model, _ = OE.init_state_dict(st, int(fx['seed']))
    model = model.to(DEV)
    model.hip_training = True
    return model


@functools.lru_cache(maxsize=None)
def _model(tag):
    return _fresh(tag)


@functools.lru_cache(maxsize=None)
def _base(tag):
    """The HIP result of a case, computed once: (out, [(name, grad)])."""
    _, _, _, h0, x, n_nodes, d_out = C.case(tag)
    return _grads(_model(tag), h0, x, n_nodes, d_out)


@pytest.mark.parametrize("tag", C.CASES)
def test_every_parameter_gradient_matches_float64_autograd(tag):
    (out64, g64), (out32, g32) = C.yardsticks(tag)
    out, grads = _base(tag)
    assert [k for k, _ in grads] == list(g64)
    worst = compare_grads(grads, g64, want32=g32, what='egnn train %s' % tag)
    print("%s: worst gradient error / bound %.4f" % (tag, worst))


@pytest.mark.parametrize("tag", C.CASES)
def test_training_forward_is_the_inference_forward(tag):
    fx, _, _, h0, x, n_nodes, _ = C.case(tag)
    out, _ = _base(tag)
    assert torch.equal(out, _infer(_model(tag), h0, x, n_nodes))
    close64(out, torch.from_numpy(fx['out32']), torch.from_numpy(fx['out64']), 'egnn train %s output' % tag)


@pytest.mark.parametrize("tag", C.CASES)
def test_two_backward_calls_give_the_same_bits(tag):
    _, _, _, h0, x, n_nodes, d_out = C.case(tag)
    _, first = _base(tag)
    _, again = _grads(_model(tag), h0, x, n_nodes, d_out)
    for (k, a), (_, b) in zip(first, again):
        assert torch.equal(a, b), k


def test_gradients_do_not_depend_on_padding_and_are_linear_in_the_batch():
    tag = C.CASES[0]
    _, _, _, h0, x, n_nodes, d_out = C.case(tag)
    model = _model(tag)
    B = h0.shape[0]
    _, base = _base(tag)
    want = dict(base)
    # the same molecules at width 80, junk on the padding atoms
    g = torch.Generator().manual_seed(5)
    h0w, xw = torch.zeros(B, 80, h0.shape[2]), 3.0 * torch.randn(B, 80, 3, generator=g)
    h0w[:, :, 1] = 1.0
    for b, n in enumerate(n_nodes):
        h0w[b, :n], xw[b, :n] = h0[b, :n], x[b, :n]
    _, wide = _grads(model, h0w, xw, n_nodes, d_out)
    for (k, a), (_, b_) in zip(base, wide):
        assert torch.equal(a, b_), k
    # reversed batch order: the sums over atoms and edges run in another order
    _, rev = _grads(model, h0.flip(0), x.flip(0), n_nodes[::-1], d_out.flip(0))
    compare_grads(rev, want, what='reversed batch')
    # every molecule alone: the batch's gradient is the sum
    total = {k: torch.zeros_like(v) for k, v in base}
    for b, n in enumerate(n_nodes):
        _, one = _grads(model, h0[b:b + 1], x[b:b + 1], [n], d_out[b:b + 1])
        for k, v in one:
            total[k] += v
    compare_grads(list(total.items()), want, what='sum over molecules')


@pytest.mark.parametrize("tag", list(S.TRIP_CASES))
def test_each_edge_backward_instantiation_past_one_trip(tag):
    """4 986 atoms: three trips of the persistent edge backward kernel (the forward's grid cap), 1 - 2 layers; float64 and float32 autograd
    through the oracle in chunks of 32 molecules, gradients summed over chunks."""
    st, model, sd, h0, x, n_nodes, _, (out64, _) = S.trip_case(tag)
    assert sum(n_nodes) > 2 * S.TRIP
    d_out = torch.randn(len(n_nodes), generator=torch.Generator().manual_seed(23))
    o64, g64 = OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float64, chunk=32)
    _, g32 = OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float32, chunk=32)
    assert float((o64 - out64).abs().max()) < 1e-9
    model.hip_training = True
    try:
        model.requires_grad_(True)
        out, grads = _grads(model, h0, x, n_nodes, d_out)
    finally:
        model.hip_training = False
        model.zero_grad(set_to_none=True)
    assert torch.equal(out, S.call(model, h0, x, n_nodes, 33))
    worst = compare_grads(grads, g64, want32=g32, what='egnn train trips %s' % tag)
    print("%s: worst gradient error / bound %.4f" % (tag, worst))


@pytest.mark.parametrize("nf", [64, 192])
def test_wide_molecules_gradients(nf):
    """The training path at the forward's size edges (test_egnn_scale_gpu.test_wide_molecules): n = 255 (eight source chunks, the last
    with 31 sources; compact edge rows up to 64 770 per molecule) and 181 beside 1 and 2 at padded width 255, 16 real-valued input
    channels, node_attr and attention, one layer; W2 in LDS (nf 64) and streamed (nf 192).  97 352 edge rows: the workspace sizing and
    the capped split-K of the edge_mlp.2 weight gradient at that many rows."""
    n_nodes, N = [255, 1, 2, 181], 255
    assert sum(n * (n - 1) for n in n_nodes) == 97352
    st = S.settings(nf, 1, 1, 1, in_nf=16)
    model, sd = S.make_model(st, 37)
    h0, x = S.batch(n_nodes, N, 41, 16, False)
    d_out = torch.randn(len(n_nodes), generator=torch.Generator().manual_seed(29))
    _, g64 = OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float64, chunk=1)
    _, g32 = OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float32, chunk=1)
    assert min(float(v.abs().max()) for v in g64.values()) > 1e-3              # no gradient tensor vanishes
    reference = S.call(model, h0, x, n_nodes, N)
    model.hip_training = True
    try:
        model.requires_grad_(True)
        out, grads = _grads(model, h0, x, n_nodes, d_out)
    finally:
        model.hip_training = False
        model.zero_grad(set_to_none=True)
    assert torch.equal(out, reference)
    worst = compare_grads(grads, g64, want32=g32, what='egnn train wide nf%d' % nf)
    print("wide nf %d: worst gradient error / bound %.4f" % (nf, worst))


def test_forward_and_gradients_follow_the_live_weights():
    tag = C.CASES[1]
    _, st, _, h0, x, n_nodes, d_out = C.case(tag)
    model = _fresh(tag)
    before, _ = _grads(model, h0, x, n_nodes, d_out)
    model.gcl_1.node_mlp[2].weight.data.mul_(1.5)             # no version bump, no invalidate_packed_weights()
    model.gcl_0.edge_mlp[2].weight.data.mul_(1.5)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    out, grads = _grads(model, h0, x, n_nodes, d_out)
    o64, g64 = OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float64)
    o32, g32 = OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float32)
    assert float((out - before).abs().max()) > 1e-2
    close64(out, o32, o64, 'training forward after .data.mul_')
    compare_grads(grads, g64, want32=g32, what='after .data.mul_')
    # after an optimiser step the inference forward follows too
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.step()
    stepped = _infer(model, h0, x, n_nodes)
    assert float((stepped - out).abs().max()) > 1e-3
    again, _ = _grads(model, h0, x, n_nodes, d_out)
    assert torch.equal(again, stepped)


def test_opt_in_and_refusals():
    tag = C.CASES[1]
    _, st, _, h0, x, n_nodes, d_out = C.case(tag)
    model = _fresh(tag)
    model.hip_training = False
    with pytest.raises(NotImplementedError, match="no_grad"):
        _train_call(model, h0, x, n_nodes)
    model.hip_training = True
    args = _args(h0, x, n_nodes)
    args['h0'].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="input gradients"):
        model(**args)
    # two workspaces per module: a third pending forward takes the oldest one's, whose backward then raises
    outs = [_train_call(model, h0, x, n_nodes) for _ in range(3)]
    with pytest.raises(RuntimeError, match="overwritten"):
        outs[0].sum().backward()
    outs[2].sum().backward()
    torch.cuda.synchronize()


def test_step_function_with_adam_and_flat_adam():
    from jodo_amd.cond_gen import get_classifier_step_fn
    from jodo_amd.optim import FlatAdam
    tag = C.CASES[1]
    _, _, _, h0, x, n_nodes, _ = C.case(tag)
    B = len(n_nodes)
    mean, mad = 0.3, 1.7
    probe = _fresh(tag)
    pred0 = _infer(probe, h0, x, n_nodes)
    sign = torch.tensor([1.0 if b % 2 else -1.0 for b in range(B)])
    label = (pred0 - 1.5 * sign) * mad + mean                 # normalised labels 1.5 from the initial predictions: a stable L1 sign
    _, want = _grads(probe, h0, x, n_nodes, sign / B)
    losses = {}
    for name in ('adam', 'flat'):
        model = _fresh(tag)
        # the seeded weights are steep: sum |d loss / d p| is 2.7e3 here, and an Adam step moves every parameter by about lr, so the
        # loss falls by about lr x 2.7e3 per step while the step stays in the linear range (5e-3 at lr 2e-6; lr 1e-4 overshoots)
        lr = 2e-6
        opt = torch.optim.Adam(model.parameters(), lr=lr) if name == 'adam' else FlatAdam(model.parameters(), lr=lr, decoupled=False)
        step_fn = get_classifier_step_fn(opt, mean, mad)
        losses[name] = []
        for it in range(4):
            losses[name].append(float(step_fn(model, h0.to(DEV), x.to(DEV), n_nodes, label)))
            if it == 0:
                for (k, w), (_, p) in zip(want, model.named_parameters()):
                    print("first step %s %s: max |diff| %.3e" % (name, k, float((p.grad.cpu() - w).abs().max())))
                    assert torch.equal(p.grad.cpu(), w), k
        assert abs(losses[name][0] - 1.5) < 1e-4
        assert losses[name][-1] < losses[name][0]
        assert all(b < a for a, b in zip(losses[name], losses[name][1:]))
    print("losses", losses)
    for a, b in zip(losses['adam'], losses['flat']):
        assert abs(a - b) <= 2e-5 + 1e-4 * abs(a)


def test_gradient_accumulation_over_two_micro_batches():
    tag = C.CASES[3]
    _, _, _, h0, x, n_nodes, d_out = C.case(tag)
    model = _fresh(tag)
    parts = [(h0[:5], x[:5], n_nodes[:5], d_out[:5]), (h0[5:], x[5:], n_nodes[5:], d_out[5:])]
    alone = [_grads(model, *p)[1] for p in parts]
    model.zero_grad(set_to_none=True)
    outs = [_train_call(model, *p[:3]) for p in parts]        # two forwards, then two backwards
    for o, p in zip(outs, parts):
        o.backward(p[3].to(DEV))
    torch.cuda.synchronize()
    for (k, p), (_, a), (_, b) in zip(model.named_parameters(), alone[0], alone[1]):
        assert torch.equal(p.grad.cpu(), a + b), k

"""Shared by tests/test_egnn_scale_gpu.py: the batches at which the property classifier (csrc/egnn_forward.hip) runs at evaluation size
and at its size edges, and the float32 / float64 yardsticks through tests/oracle_egnn.py (computed once per case, never modified).

The dense oracle holds a [B, N, N, 2 nf + 1] tensor per layer, so a large batch is evaluated in slices of `chunk` molecules
(oracle_chunked); every molecule's result depends on that molecule alone, so slicing changes nothing.

The persistent edge kernel: edge_launch caps the grid at EDGE_GRID_MAX workgroups of EDGE_WAVES waves and wave w walks the compact
atoms w, w + 2048, ...: atom t is handled on trip t // 2048 of its wave.  cycle_batch(272, 33, ...) has 4 986 atoms: three trips."""
import functools

import torch

import oracle_egnn as OE

DEV = 'cuda:0'
EDGE_GRID_MAX, EDGE_WAVES = 512, 4             # csrc/egnn_forward.hip edge_launch: grid cap; kegnn_edge: waves per workgroup
TRIP = EDGE_GRID_MAX * EDGE_WAVES              # atoms per trip of the persistent loop at the capped grid
CYCLE = [1, 2, 5, 29, 31, 32, 33] * 3 + list(range(3, 34))


def oracle_chunked(sd, st, h0, x, n_nodes, dtype, chunk):
    """oracle_egnn.forward on slices of `chunk` molecules: (out [B], [hidden state after layer l, [sum n, nf]]) in atom order."""
    n_nodes = list(n_nodes)
    outs, hids = [], [[] for _ in range(st['n_layers'])]
    with torch.no_grad():
        for b0 in range(0, len(n_nodes), chunk):
            o, hid = OE.forward(sd, st, h0[b0:b0 + chunk], x[b0:b0 + chunk], n_nodes[b0:b0 + chunk], dtype)
            outs.append(o)
            for l, v in enumerate(hid):
                hids[l].append(v)
    return torch.cat(outs), [torch.cat(v) for v in hids]


def batch(n_nodes, N, seed, in_nf, one_hot, scale=1.5):
    """(h0 [B, N, in_nf], x [B, N, 3]) on the CPU for the atom counts given: positions scale * randn, h0 one-hot or randn; padding
    atoms hold draws like any other."""
    B = len(n_nodes)
    g = torch.Generator().manual_seed(seed)
    x = scale * torch.randn(B, N, 3, generator=g)
    if one_hot:
        h0 = torch.nn.functional.one_hot(torch.randint(0, in_nf, (B, N), generator=g), in_nf).float()
    else:
        h0 = torch.randn(B, N, in_nf, generator=g)
    return h0, x


def cycle_batch(B, N, seed, in_nf, one_hot):
    """(h0, x, n_nodes): atom counts cycling through CYCLE, positions 1.5 randn, h0 one-hot or real-valued."""
    n_nodes = [CYCLE[b % len(CYCLE)] for b in range(B)]
    assert max(n_nodes) <= N
    return batch(n_nodes, N, seed, in_nf, one_hot) + (n_nodes,)


def call(model, h0, x, n_nodes, N, edges=True):
    """The classifier's result on h0 [B, N, in_nf], x [B, N, 3] (CPU), called as the evaluation loops call it (test_egnn_gpu._call)."""
    from test_egnn_gpu import _call
    assert h0.shape[1] == N and x.shape[1] == N
    return _call(model, h0, x, n_nodes, edges=edges)


def hidden(model, h0, x, n_nodes, N, layers=1):
    """The hidden state [sum n, nf] after `layers` layers, as the kernels left it."""
    model.max_layers = layers
    try:
        return call(model, h0, x, n_nodes, N)
    finally:
        model.max_layers = -1


def settings(nf, layers, attention, node_attr, in_nf=5):
    return dict(hidden_nf=nf, n_layers=layers, attention=attention, node_attr=node_attr, in_node_nf=in_nf)


def make_model(st, seed, att_gain=1.0):
    """(module on the GPU, CPU state dict): deterministic_init_ at gain 1.0 as OE.init_state_dict; att_gain multiplies every layer's
    att_mlp.0.weight (a saturating gate)."""
    model, sd = OE.init_state_dict(st, seed)
    if att_gain != 1.0:
        with torch.no_grad():
            for l in range(st['n_layers']):
                getattr(model, 'gcl_%d' % l).att_mlp[0].weight.mul_(att_gain)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.to(DEV).eval(), sd


def yardsticks(sd, st, h0, x, n_nodes, chunk):
    """((out32, hidden32), (out64, hidden64)) through the chunked oracle."""
    return oracle_chunked(sd, st, h0, x, n_nodes, torch.float32, chunk), oracle_chunked(sd, st, h0, x, n_nodes, torch.float64, chunk)


def per_trip_errors(got, r64, trip=TRIP):
    """Worst |got - r64| over the atoms of each trip of the persistent edge loop: rows [Nn, nf] in atom order."""
    err = (got.double() - r64.double()).abs().amax(dim=1)
    return [float(err[t0:t0 + trip].max()) for t0 in range(0, err.shape[0], trip)]


TRIP_CASES = {          # the four instantiations of kegnn_edge: tag -> (nf, layers, attention, node_attr)
    'nb2_lds': (64, 2, 0, 1), 'nb4_lds': (128, 2, 1, 0), 'nb6_streamed': (192, 1, 1, 0), 'nb8_streamed': (256, 1, 1, 1)}


@functools.lru_cache(maxsize=None)
def trip_case(tag):
    """(st, model, sd, h0, x, n_nodes, (out32, hid32), (out64, hid64)) of the three-trip batch for one instantiation."""
    nf, layers, att, na = TRIP_CASES[tag]
    st = settings(nf, layers, att, na)
    model, sd = make_model(st, 31)
    h0, x, n_nodes = cycle_batch(272, 33, 17, 5, True)
    r32, r64 = yardsticks(sd, st, h0, x, n_nodes, 32)
    return st, model, sd, h0, x, n_nodes, r32, r64

"""Shared by tests/test_egnn_train_host.py and tests/test_egnn_train_gpu.py: the cases of the classifier's training path, their random
output gradients and the float64 / float32 autograd yardsticks through tests/oracle_egnn_train.py (computed once per case, shared,
never modified).

Cases: the four fixtures of the forward (tests/golden/egnn_*.npz), weights regenerated from the seed.  Their batch n_nodes = [1, 2, 5,
29, 31, 32, 33, 64, 65] at N = 65: a molecule with no sources, one with one source, the 32-source chunk boundary from both sides, two
chunks and two chunks plus one; 262 atoms (no multiple of 32, nor of the 64-row chunks of the column sums) and 12 036 edges (23 slices
of 512 rows of the split-K weight gradient plus 260: no multiple of 32).

The persistent edge backward kernel uses the forward's grid cap (jegnn::EDGE_GRID_MAX workgroups of EDGE_WAVES waves), so the
three-trip batch of tests/egnn_scale_common.py (cycle_batch(272, 33, ...): 4 986 atoms) is three trips of it as well.

Gradient bound: the project's own rule (train2d_common.compare_grads): per tensor |err| <= 3e-4 max|want|, widened to 16 x the
float32-autograd distance where that is larger."""
import functools

import torch

import oracle_egnn as OE
import oracle_egnn_train as OET
from helpers import load_fixture

CASES = ['nf128_l7_a1_n0', 'nf64_l2_a0_n1', 'nf256_l1_a1_n1', 'nf192_l3_a1_n0']


@functools.lru_cache(maxsize=None)
def case(tag):
    """(fx, st, sd (CPU float32), h0, x, n_nodes, d_out) of a fixture case; d_out is seeded, not from a loss."""
    fx = load_fixture('egnn_%s.npz' % tag)
    st = OE.settings_of(fx)
    _, sd = OE.init_state_dict(st, int(fx['seed']))
    h0, x, n_nodes = torch.from_numpy(fx['h0']), torch.from_numpy(fx['x']), fx['n_nodes'].tolist()
    d_out = torch.randn(len(n_nodes), generator=torch.Generator().manual_seed(11))
    return fx, st, sd, h0, x, n_nodes, d_out


@functools.lru_cache(maxsize=None)
def yardsticks(tag):
    """((out64, grads64), (out32, grads32)) of a case."""
    _, st, sd, h0, x, n_nodes, d_out = case(tag)
    return OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float64), OET.grads(sd, st, h0, x, n_nodes, d_out, torch.float32)

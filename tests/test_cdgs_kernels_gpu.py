"""The launch sequences of the CDGS training step (csrc/cdgs_train.hip: 39 kernels, about 150 launches per block) one by one on the
device against float64, through the test entry jodo_cdgs_train_debug_op.  The network-level tests (test_cdgs_train_gpu.py) see these
kernels only through two outputs and the parameter gradients, each compared at 3e-4 of its tensor's largest entry; here EVERY element
of EVERY array an op stores is compared with the restatement of tests/cdgs_kernels_common.py (anchored to the oracle and to autograd
by tests/test_cdgs_kernels_host.py, which also runs this file's small shapes through the host emulation build of the same kernels).

Around every call: outputs start as NaN, every array sits between two guard bands of 512 floats that are compared bit for bit
afterwards, inputs must come back unchanged (but for the documented in-place arrays: alpha in ATTN_FWD, d alpha in ATTN_BWD, x turned
into xhat in EGN_FWD), and the call is repeated and must give the same bits.  Tolerances are the project's two rules, unchanged:
helpers.close64 for activation-type arrays, train2d_common.compare_grads for gradient-type arrays, both yardsticks from the restatement
alone; adj, cnt, onehot, masked zeros, the diagonal, padded rows of masked ops and the dropout multipliers are compared bit for bit.

Shapes: the smallest at which each op can still go wrong: n_nodes, N = [1], 1; [2, 1], 2; [9, 4, 7, 2], 12 (no molecule reaches the
width); [12, 1, 5], 12 for every tiled op; [64, 1], 64; [65, 2], 65; [181, 2], 181 (the GEOM config's width, ch = 3, K = 16) for
attention, GINE, the edge GroupNorm, the pair ops, the sums and the random-walk prologue; column sums over 1 .. 2 113 rows (32 and 33
chunks, a ragged tail) and 6 209 rows (three groups and a ragged one), dense and with dy on ONE live row."""
import pytest
import torch

import cdgs_kernels_common as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hs():
    h = K.Harness('cuda:0')
    yield h
    print('worst err / bound per op (device): ' + ', '.join('%s %.3f' % kv for kv in sorted(h.ratios.items())))


@pytest.mark.parametrize('shape', range(len(K.SMALL)))
@pytest.mark.parametrize('op', K.TILED)
def test_every_op_at_the_small_widths(hs, op, shape):
    n_nodes, N = K.SMALL[shape]
    K.run_variants(hs, op, n_nodes, N)


@pytest.mark.parametrize('shape', range(len(K.WIDE)))
@pytest.mark.parametrize('op', K.WIDE_OPS)
def test_wide_tiles(hs, op, shape):
    """N = 64, 65 and 181: benign values (the first variant of every op; RW: a random graph and a path), and the hard softmax at 65"""
    n_nodes, N = K.WIDE[shape]
    variants = K.VARIANTS[op][:1]
    if op == 'RW':
        variants = K.VARIANTS[op][:2]
    if op in ('ATTN_FWD', 'ATTN_BWD') and N == 65:
        variants = K.VARIANTS[op]
    K.run_variants(hs, op, n_nodes, N, variants)


@pytest.mark.parametrize('rows,mode,one_row', K.norm_grads_cases())
def test_column_sums(hs, rows, mode, one_row):
    K.run_norm_grads(hs, rows, mode, one_row)


@pytest.mark.parametrize('op', ['ATTN_FWD', 'EGN_FWD', 'GINE'])
def test_each_molecule_alone(hs, op):
    K.molecule_alone(hs, op, [9, 4, 7, 2], 12, 31)
    K.molecule_alone(hs, op, [65, 2], 65, 32)


def test_hard_sets_end_where_they_must(hs):
    """n = 1: alpha exactly 0; n = 2: 1 / (1 + 1e-16) = 1 in float32; equal channels / a constant tile: xhat exactly 0, rstd 1 / sqrt(1e-6);
    EGN with an n = 1 molecule: nothing live, e_out and d pre exactly 0 there whatever the padded rows hold"""
    (_, d, got, _), = K.run_variants(hs, 'ATTN_FWD', [2, 1], 2, [('hard', True, {})])
    assert K.is_zero(got['ALPHA'][1]) and K.is_zero(got['ATT'][1]) and bool((got['ALPHA'][0, 1, 0] == 1.0).all()) and bool((got['ALPHA'][0, 0, 1] == 1.0).all())
    (_, d, got, _), = K.run_variants(hs, 'GN_FWD', [12, 1, 5], 12, [('hard', True, {})])
    assert K.is_zero(got['XHAT'][:, :, 0:8]) and float((got['RSTD'][:, :, 0] - 1000).abs().max()) < 1e-3
    (_, d, got, _), = K.run_variants(hs, 'EGN_FWD', [12, 1, 5], 12, [('constant', 'constant', {})])
    assert K.is_zero(got['XHAT'][0]) and float((got['RSTD'][0] - 1000).abs().max()) < 1e-3 and K.is_zero(got['Y'][1])
    (_, d, got, _), = K.run_variants(hs, 'EGN_BWD', [12, 1, 5], 12, [('benign', None, {})])
    assert K.is_zero(got['DX'][1]) and not K.is_zero(got['DX'][2][5:])          # n = 1: nothing live; n = 5: the padded rows carry gradient


def test_entry_refusals(hs):
    """Raised only through arguments the host rejects; no kernel runs and every poisoned output keeps its NaN."""
    K.refusals(hs)

"""forms_common.strip_order / seam_batch / seams against the plan builder itself (csrc/dgt_plan.cpp through jodo_plan_stats), on the
CPU: the GPU tests of test_forms_gpu.py name node strips, so the Python restatement of the strip layout and the batches built to sit
on a seam must follow the plan — a change of the plan cannot quietly move a case off its seam."""
import ctypes

import numpy as np
import pytest

from jodo_amd import capi

from forms_common import LIVE_LAST, ROUND, SEAM_SIZES, SPLIT_GATE_PATTERN, align32, seam_batch, seams, straddler, strip_order


class _Cfg(ctypes.Structure):
    _fields_ = [('nf', ctypes.c_int32), ('n_layers', ctypes.c_int32), ('n_heads', ctypes.c_int32),
                ('n_extra', ctypes.c_int32), ('mlp_ratio', ctypes.c_int32), ('in_node_dim', ctypes.c_int32),
                ('edge_ch', ctypes.c_int32), ('cond_ch', ctypes.c_int32),
                ('spatial_cut_off', ctypes.c_float), ('edge_quan_th', ctypes.c_float), ('layout', ctypes.c_int32)]


def _plan_stats(n_nodes):
    lib = capi.lib()
    cfg = _Cfg(256, 8, 16, 2, 2, 6, 2, 0, 2.0, 0.0)
    n = np.asarray(n_nodes, dtype=np.int32)
    h = ctypes.c_void_p()
    assert lib.jodo_plan_create(ctypes.byref(cfg), len(n), int(n.max()), n.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(h)) == 0
    st = (ctypes.c_int64 * 6)()
    assert lib.jodo_plan_stats(h, st) == 0
    lib.jodo_plan_destroy(h)
    return list(st)


@pytest.mark.parametrize("n_nodes", [[3, 29, 18, 18, 1], [32], [1], [29, 3], [29, 4], list(range(1, 30)) * 3, SPLIT_GATE_PATTERN * 7,
                                     [5] * 20 + [19] * 14])
def test_strip_order_restates_the_plan(n_nodes):
    so = strip_order(n_nodes)
    st = _plan_stats(n_nodes)
    assert so['Nn'] == st[0] == sum(n_nodes) and so['n_strips'] == st[3] and so['Nn_pad'] == align32(sum(n_nodes)) == 32 * st[3]
    # stable descending order, molecules back to back
    sizes = [n_nodes[b] for b in so['order']]
    assert sizes == sorted(n_nodes, reverse=True)
    for a, b in zip(so['order'], so['order'][1:]):
        assert n_nodes[a] > n_nodes[b] or (n_nodes[a] == n_nodes[b] and a < b)
        assert so['first'][b] == so['first'][a] + n_nodes[a]
    # every atom has a strip, every strip's owners are exactly the molecules with a row in it
    assert len(so['atom_strip']) == so['Nn'] and so['atom_strip'] == [v // 32 for v in range(so['Nn'])]
    for s, own in enumerate(so['owners']):
        want = [b for b in so['order'] if so['first'][b] < 32 * (s + 1) and so['first'][b] + n_nodes[b] > 32 * s]
        assert own == want and own


@pytest.mark.parametrize("S", SEAM_SIZES)
def test_seam_batches_sit_on_their_seams(S):
    n_nodes = seam_batch(S, LIVE_LAST)
    assert 1 <= min(n_nodes) and max(n_nodes) <= 29                                   # QM9-sized
    st = _plan_stats(n_nodes)
    assert st[3] == S, "the plan gives %d strips where the case needs %d" % (st[3], S)
    assert st[0] == (S - 1) * 32 + LIVE_LAST                                          # live rows of the last strip: padded lanes exist
    so = strip_order(n_nodes)
    assert so['n_strips'] == S
    b = straddler(n_nodes)
    if S > ROUND:
        assert b is not None and so['first'][b] < 32 * ROUND < so['first'][b] + n_nodes[b]
        assert b in so['owners'][ROUND - 1] and b in so['owners'][ROUND]
    else:
        assert b is None
    pick = seams(n_nodes)
    assert len(pick) <= 16 and len(set(pick)) == len(pick)
    for s in (0, ROUND - 1, ROUND, S - 1):
        if s < S:
            assert set(so['owners'][s]) <= set(pick)
    if b is not None:
        assert b in pick
    # the smallest and the largest size are among them (first and last strip of a descending order)
    assert max(n_nodes[i] for i in pick) == 29 and min(n_nodes[i] for i in pick) == 1
    # chunks of 400 molecules stay below one full round, so the chunk model never takes a >= 1024-strip form
    assert all(strip_order(n_nodes[lo:lo + 400])['n_strips'] < ROUND for lo in range(0, len(n_nodes), 400))


def test_seam_batch_other_fill():
    # (S = 1025 with ONE live row cannot straddle: the last row is the size-1 molecule, so the boundary falls between molecules)
    for S, live in ((2, 1), (40, 32), (1025, 2), (1100, 16)):
        n_nodes = seam_batch(S, live)
        st = _plan_stats(n_nodes)
        assert st[3] == S and st[0] == (S - 1) * 32 + live
        assert (straddler(n_nodes) is not None) == (S > ROUND)

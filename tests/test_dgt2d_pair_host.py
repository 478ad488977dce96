"""CPU: the host side of the pair-symmetric attention walk of DGT_concat_2D — groups of whole molecules in 128 atom slots
(jodo_dgt2d_pair_layout / jodo_dgt2d_pair_fill_desc, include/jodo_hip.h).  The walk is replayed here from the descriptor alone and must
visit every unordered pair of every molecule exactly once; the directed plan's layout and descriptor functions are unchanged."""
import ctypes
import os

import numpy as np
import pytest
import torch

from jodo_amd import capi
from jodo_amd.models import get_model_class, get_node_dist
from helpers import make_config, GOLDEN
import oracle2d as O2

SLOTS = 128


@pytest.fixture(scope='module')
def cfg_struct():
    return get_model_class('DGT_concat_2D')(make_config('vpsde_zinc_2d_jodo'))._cfg_struct


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pair_desc(cfg_struct, n_nodes, N=None):
    n = np.ascontiguousarray(n_nodes, dtype=np.int32)
    N = int(n.max()) if N is None else N
    L = capi.lib()
    lay = (ctypes.c_int64 * 8)()
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), len(n), N, _ptr(n), lay) == 0
    words, groups, items, off_items, off_slots, slots, item_words = (int(v) for v in lay[:7])
    assert slots == SLOTS and item_words == 4 and words == off_slots + groups * SLOTS and off_slots >= off_items + 4 * items
    desc = np.full(words + 3, -77, dtype=np.int32)                       # three guard words behind the descriptor
    assert L.jodo_dgt2d_pair_fill_desc(ctypes.byref(cfg_struct), len(n), N, _ptr(n), _ptr(desc), ctypes.c_int64(words)) == 0
    assert desc[words:].tolist() == [-77] * 3
    return desc[off_items:off_items + 4 * items].reshape(items, 4), desc[off_slots:off_slots + groups * SLOTS].reshape(groups, SLOTS)


def check_walk(n_nodes, items, slots):
    """Every molecule in one group in consecutive slots, no group above 128 slots, and the walk (atom i meets (i + d) mod n at every
    offset d <= n / 2 of its group's item; at d = n / 2 of an even n both atoms of a pair meet it as targets only) covers every
    directed edge exactly once and evaluates every unordered pair once — twice, as two targets, at the half offset only."""
    B = len(n_nodes)
    where = {}
    for g in range(slots.shape[0]):
        used = slots[g][slots[g] >= 0]
        assert len(used) >= 1 and (slots[g][:len(used)] >= 0).all() and (slots[g][len(used):] == -1).all()
        assert len(used) <= SLOTS
        at = 0
        while at < len(used):
            b, i = int(used[at]) >> 8, int(used[at]) & 255
            assert i == 0 and b not in where and 0 <= b < B
            n = int(n_nodes[b])
            assert used[at:at + n].tolist() == [(b << 8) | k for k in range(n)]
            where[b] = (g, at)
            at += n
    assert sorted(where) == list(range(B))
    # items: one range of offsets per group, together 1 .. max n / 2 of the group, longest first
    spans = {}
    for g, d0, d1, pad in items.tolist():
        assert pad == 0 and 0 <= g < slots.shape[0]
        spans.setdefault(g, []).append((d0, d1))
    assert sorted(spans) == list(range(slots.shape[0]))
    lengths = [d1 - d0 + 1 for _, d0, d1, _ in items.tolist()]
    assert lengths == sorted(lengths, reverse=True)
    edges, evaluations = {}, {}
    for g, rng in spans.items():
        offsets = sorted(d for d0, d1 in rng for d in range(d0, d1 + 1))
        mols = sorted({int(c) >> 8 for c in slots[g] if c >= 0})
        dmax = max(int(n_nodes[b]) // 2 for b in mols)
        assert offsets == list(range(1, dmax + 1))
        for d in offsets:
            for s in range(SLOTS):
                c = int(slots[g, s])
                if c < 0:
                    continue
                b, i = c >> 8, c & 255
                n = int(n_nodes[b])
                if 2 * d > n:
                    continue
                p = (i + d) % n
                assert where[b][0] == g and slots[g, s - i + p] == ((b << 8) | p)         # the partner's slot is in this group
                key = (b, min(i, p), max(i, p))
                evaluations[key] = evaluations.get(key, 0) + 1
                edges[(b, p, i)] = edges.get((b, p, i), 0) + 1                            # source p -> target i: own
                if 2 * d < n:
                    edges[(b, i, p)] = edges.get((b, i, p), 0) + 1                        # source i -> target p: handed over
    want_edges = {(b, r, c) for b in range(B) for r in range(int(n_nodes[b])) for c in range(int(n_nodes[b])) if r != c}
    assert set(edges) == want_edges and set(edges.values()) <= {1}
    want_pairs = {(b, r, c) for b, r, c in want_edges if r < c}
    assert set(evaluations) == want_pairs
    for (b, r, c), cnt in evaluations.items():
        assert cnt == (2 if 2 * (c - r) == int(n_nodes[b]) else 1)
    return len(spans)


@pytest.mark.parametrize('n', list(range(1, 65)))
def test_single_molecule(cfg_struct, n):
    items, slots = pair_desc(cfg_struct, [n])
    assert check_walk([n], items, slots) == 1
    assert items.tolist() == [[0, 1, n // 2, 0]]


@pytest.mark.parametrize('n_nodes', [[1, 2, 3, 9, 33, 38], [2, 5, 27]])
def test_small_batches(cfg_struct, n_nodes):
    items, slots = pair_desc(cfg_struct, n_nodes)
    assert check_walk(n_nodes, items, slots) == 1                        # 86 and 34 atoms: one group each
    order = [int(c) >> 8 for c in slots[0] if c >= 0 and (int(c) & 255) == 0]
    assert [n_nodes[b] for b in order] == sorted(n_nodes, reverse=True)  # largest first


def test_fills_gaps_with_the_largest_that_fits(cfg_struct):
    n_nodes = [60, 60, 60, 8, 7, 5, 3]                                   # 60 + 60 + 8 = 128, then 60 + 7 + 5 + 3
    items, slots = pair_desc(cfg_struct, n_nodes)
    assert check_walk(n_nodes, items, slots) == 2
    first = lambda g: [int(c) >> 8 for c in slots[g] if c >= 0 and (int(c) & 255) == 0]
    assert first(0) == [0, 1, 3] and first(1) == [2, 4, 5, 6]
    assert (slots[0] >= 0).all() and int((slots[1] >= 0).sum()) == 75


def test_zinc_batch_of_2000(cfg_struct):
    torch.manual_seed(5)
    n_nodes = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k')).sample(2000).tolist()
    items, slots = pair_desc(cfg_struct, n_nodes)
    groups = check_walk(n_nodes, items, slots)
    # the filling rule: a group is closed only when no molecule that is still unplaced fits its unused slots
    room = [int((slots[g] < 0).sum()) for g in range(groups)]
    smallest = [min(n_nodes[int(c) >> 8] for c in slots[g] if c >= 0) for g in range(groups)]
    for g in range(groups - 1):
        assert room[g] < min(smallest[g + 1:])
    assert groups > 256                                                  # more groups than the persistent grid has workgroups


def test_bad_arguments(cfg_struct):
    L = capi.lib()
    lay = (ctypes.c_int64 * 8)()
    ok = np.array([3, 1, 5], dtype=np.int32)
    desc = np.zeros(4096, dtype=np.int32)
    err = lambda: L.jodo_last_error().decode()
    bad = np.array([3, 0, 5], dtype=np.int32)
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), 3, 5, _ptr(bad), lay) == -1 and 'n_nodes[1]=0' in err()
    assert L.jodo_dgt2d_pair_fill_desc(ctypes.byref(cfg_struct), 3, 5, _ptr(bad), _ptr(desc), ctypes.c_int64(4096)) == -1 and 'n_nodes[1]' in err()
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), 3, 4, _ptr(ok), lay) == -1 and 'n_nodes[2]=5' in err()       # above the width
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), 0, 5, _ptr(ok), lay) == -1 and 'bad batch' in err()
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), 3, 5, None, lay) == -1 and 'bad batch' in err()
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), 3, 5, _ptr(ok), None) == -1 and 'null' in err()
    assert L.jodo_dgt2d_pair_fill_desc(ctypes.byref(cfg_struct), 3, 5, _ptr(ok), None, ctypes.c_int64(4096)) == -1 and 'null' in err()
    big = np.array([70], dtype=np.int32)
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), 1, 70, _ptr(big), lay) == -3 and 'above 64' in err()
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(cfg_struct), 3, 5, _ptr(ok), lay) == 0
    assert L.jodo_dgt2d_pair_fill_desc(ctypes.byref(cfg_struct), 3, 5, _ptr(ok), _ptr(desc), ctypes.c_int64(int(lay[0]) - 1)) == -1 and 'need' in err()
    from jodo_amd.models.dgt2d import _Cfg2D
    wrong = _Cfg2D(128, 8, 16, 1, 2, 10, 2, 0.0)
    assert L.jodo_dgt2d_pair_layout(ctypes.byref(wrong), 3, 5, _ptr(ok), lay) == -3
    # the walk selector of the forward entry is checked before anything touches a device
    assert L.jodo_dgt2d_forward_walk(ctypes.byref(cfg_struct), 3, 5, _ptr(ok), None, None, 2, *([None] * 2), 0, *([None] * 9), 0, -1, None) == -1
    assert 'walk 2' in err()
    assert L.jodo_dgt2d_forward_walk(ctypes.byref(cfg_struct), 3, 5, _ptr(ok), None, None, 1, *([None] * 2), 0, *([None] * 9), 0, -1, None) == -1
    assert 'group descriptor' in err()


def _directed_plan(n_nodes, N):
    """jodo_dgt2d_layout / jodo_dgt2d_fill_desc as include/jodo_hip.h and csrc/dgt2d_forward.hip document them."""
    D, De, T, L, = 256, 64, 1024, 8
    MODW, EHW, NHW = L * (6 * D + 6 * De), De + L * 16, D + L * 64
    B = len(n_nodes)
    Nn, R, P = sum(n_nodes), sum(n * n for n in n_nodes), sum(n * (n - 1) // 2 for n in n_nodes)
    up = lambda v: (v + 63) // 64 * 64
    Bp, Np, Rp = up(B), up(Nn), up(R)
    at, offs = 0, {}
    for name, cnt in (('hid1', Bp * T), ('tembs', Bp * T), ('mods', Bp * MODW), ('h', Np * D), ('hm', Np * D), ('qkv', Np * 3 * D),
                      ('hn', Np * D), ('u', Np * De), ('f1', Np * 2 * D), ('ahid', Np * NHW), ('nh1', Np * D), ('nh2', Np * (D // 2)),
                      ('nh3', Np * 32), ('e', Rp * De), ('ehid', Rp * EHW)):
        offs[name] = at
        at += up(cnt)
    lay = [3 * B + Nn + P + 1, at * 4, Nn, R, offs['h'] * 4, offs['e'] * 4, P, 0]
    desc, noff, eoff = list(n_nodes), [], []
    a = e = 0
    for n in n_nodes:
        noff.append(a); eoff.append(e)
        a += n; e += n * n
    desc += noff + eoff
    desc += [(b << 8) | i for b, n in enumerate(n_nodes) for i in range(n)]
    desc += [(b << 12) | (r << 6) | c for b, n in enumerate(n_nodes) for r in range(n) for c in range(r + 1, n)]
    return lay, desc + [0]


@pytest.mark.parametrize('n_nodes', [[3, 1, 5], [1, 2, 3, 9, 33, 38], [64], [1]])
def test_directed_layout_and_descriptor_are_unchanged(cfg_struct, n_nodes):
    L = capi.lib()
    n = np.array(n_nodes, dtype=np.int32)
    N = max(n_nodes)
    want_lay, want_desc = _directed_plan(n_nodes, N)
    lay = (ctypes.c_int64 * 8)()
    assert L.jodo_dgt2d_layout(ctypes.byref(cfg_struct), len(n), N, _ptr(n), lay) == 0
    assert list(lay) == want_lay
    desc = np.full(lay[0] + 2, -77, dtype=np.int32)
    assert L.jodo_dgt2d_fill_desc(ctypes.byref(cfg_struct), len(n), N, _ptr(n), _ptr(desc), ctypes.c_int64(int(lay[0]))) == 0
    assert desc.tolist() == want_desc + [-77, -77]


def test_switch_is_runtime_state():
    model = get_model_class('DGT_concat_2D')(make_config('vpsde_zinc_2d_jodo'))
    assert model.pair_attention is False
    model.pair_attention = True
    assert not any('pair' in k for k in model.state_dict())


def test_exports_are_declared_in_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'jodo_hip.h')).read()
    for name in ('jodo_dgt2d_pair_layout', 'jodo_dgt2d_pair_fill_desc', 'jodo_dgt2d_forward_walk'):
        assert ('int %s(' % name) in text and getattr(capi.lib(), name) is not None

"""CPU: the split-bf16 ("bf16x3") weight tape of DGT_concat_2D (jodo_dgt2d_split_size / jodo_dgt2d_pack_split_host) against the packed
blob it is derived from, and the switch's defaults.  The tape re-reads every covered tiled matrix float [nb][nk][8 quads][64 lanes][4] as
bf16 [nb][nk * 4 K16 steps][hi, mid, lo][64 lanes][8]: element j of lane l in K16 step G of a chunk is the chunk's f32 k-step 8 G + j of
the same lane — the relation tests/test_split_gate.py pins for the 3-D packer."""
import ctypes

import numpy as np
import pytest
import torch

from jodo_amd import capi
from helpers import make_config, make_model, masks, state_dict_cpu

CFG = 'vpsde_zinc_2d_jodo'
# (slot name, index inside its table, output blocks, K chunks) — include/jodo_hip.h enum jodo2d_wslot_global / jodo2d_wslot_block
GLOBAL_COUNT, BLOCK_COUNT = 23, 17
BLOCK_SLOTS = (('QKV', 0, 24, 4), ('N2E', 3, 2, 4), ('FF1', 5, 16, 4), ('FF2', 7, 8, 8), ('NRO', 13, 2, 4), ('FF3', 9, 4, 1),
               ('FF4', 11, 2, 2), ('ERO', 15, 1, 1))
GLOBAL_SLOTS = (('NH1', 11, 8, 12), ('NH2', 13, 4, 4), ('NH3', 15, 1, 2))


def _covered(n_layers):
    out = [('%s[%d]' % (nm, l), GLOBAL_COUNT + l * BLOCK_COUNT + i, nb, nk) for l in range(n_layers) for nm, i, nb, nk in BLOCK_SLOTS]
    return out + [(nm, i, nb, nk) for nm, i, nb, nk in GLOBAL_SLOTS]


@pytest.fixture(scope='module')
def packed():
    cfg = make_config(CFG)
    model = make_model(cfg, seed=7)
    blob, woff, n_woff = capi.pack_weights_2d(model._cfg_struct, state_dict_cpu(model))
    return cfg, model, blob, woff, n_woff


def test_tape_is_the_exact_split_of_the_blob_in_the_k16_permutation(packed):
    cfg, model, blob, woff, n_woff = packed
    assert n_woff == GLOBAL_COUNT + cfg.model.n_layers * BLOCK_COUNT
    tape, toff = capi.split_tape_2d(model._cfg_struct, blob, woff, n_woff)
    total = ctypes.c_size_t()
    toff2 = (ctypes.c_int64 * n_woff)()
    capi.check(capi.lib().jodo_dgt2d_split_size(ctypes.byref(model._cfg_struct), ctypes.byref(total), toff2, n_woff), 'split_size')
    assert list(toff2) == list(toff) and total.value == tape.numel()
    covered = _covered(cfg.model.n_layers)
    assert sorted(i for i in range(n_woff) if toff[i] >= 0) == sorted(s for _, s, _, _ in covered)     # one entry per covered slot, -1 elsewhere
    assert all(toff[i] == -1 for i in range(n_woff) if i not in {s for _, s, _, _ in covered})
    # 16-byte aligned, non-overlapping, and the size query is the end of the last slot
    spans = sorted((toff[s], toff[s] + nb * nk * 4 * 3072) for _, s, nb, nk in covered)
    assert all(a % 16 == 0 for a, _ in spans)
    assert spans[0][0] == 0 and all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
    assert spans[-1][1] == total.value == sum(nb * nk for _, _, nb, nk in covered) * 4 * 3072
    t16 = tape.numpy().view(np.uint16)
    b2f = lambda u: (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    f = blob.numpy()
    G, J = np.meshgrid(np.arange(4), np.arange(8), indexing='ij')
    K = 8 * G + J                                              # f32 k-step of (K16 step, element)
    nonzero = 0
    for name, s, nb, nk in covered:
        tiles = nb * nk
        t = t16[toff[s] // 2:toff[s] // 2 + tiles * 4 * 1536].reshape(tiles, 4, 3, 64, 8)          # [tile][K16 step][term][lane][j]
        rec = b2f(t[:, :, 0]) + b2f(t[:, :, 1]) + b2f(t[:, :, 2])                                 # hi + mid + lo in float64: exact
        f4 = f[woff[s]:woff[s] + tiles * 2048].reshape(tiles, 8, 64, 4)                             # [tile][quad][lane][i]
        want = np.ascontiguousarray(f4[:, K // 4, :, K % 4].transpose(2, 0, 3, 1))                 # [G][j][tile][lane] -> [tile][G][lane][j]
        assert np.array_equal(rec, want.astype(np.float64)), name
        # every term is the round-to-nearest-even bf16 of what the terms before it left
        hi = torch.from_numpy(want).to(torch.bfloat16)
        assert np.array_equal(b2f(t[:, :, 0]), hi.double().numpy()), name
        r1 = torch.from_numpy(want) - hi.float()
        assert np.array_equal(b2f(t[:, :, 1]), r1.to(torch.bfloat16).double().numpy()), name
        nonzero += int(np.count_nonzero(rec))
    assert nonzero > 1000000                                   # the comparison is not one of zeros


def test_tape_entries_refuse_bad_arguments(packed):
    cfg, model, blob, woff, n_woff = packed
    L = capi.lib()
    c = ctypes.byref(model._cfg_struct)
    total = ctypes.c_size_t()
    toff = (ctypes.c_int64 * (n_woff + 1))()
    assert L.jodo_dgt2d_split_size(c, ctypes.byref(total), toff, n_woff) == 0
    for bad in (n_woff - 1, n_woff + 1, 0):
        assert L.jodo_dgt2d_split_size(c, ctypes.byref(total), toff, bad) == -1                    # JODO_ERR_ARG
    assert L.jodo_dgt2d_split_size(c, None, toff, n_woff) == -1
    assert L.jodo_dgt2d_split_size(c, ctypes.byref(total), None, n_woff) == -1
    tape = np.zeros(total.value, dtype=np.uint8)
    tp, bp = tape.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(blob.data_ptr())
    assert L.jodo_dgt2d_pack_split_host(c, bp, woff, n_woff, tp, ctypes.c_size_t(total.value)) == 0
    assert L.jodo_dgt2d_pack_split_host(c, bp, woff, n_woff - 1, tp, ctypes.c_size_t(total.value)) == -1
    assert L.jodo_dgt2d_pack_split_host(c, None, woff, n_woff, tp, ctypes.c_size_t(total.value)) == -1
    assert L.jodo_dgt2d_pack_split_host(c, bp, None, n_woff, tp, ctypes.c_size_t(total.value)) == -1
    assert L.jodo_dgt2d_pack_split_host(c, bp, woff, n_woff, None, ctypes.c_size_t(total.value)) == -1
    assert L.jodo_dgt2d_pack_split_host(c, bp, woff, n_woff, tp, ctypes.c_size_t(total.value - 16)) == -1      # buffer too small
    assert b'need' in L.jodo_last_error()


def test_switch_defaults_and_the_3d_switch_still_raises():
    cfg = make_config(CFG)
    model = make_model(cfg, seed=3)
    assert model.bf16x3 is False and model._tape is None
    assert 'bf16x3' not in model.state_dict() and not any('tape' in k for k in model.state_dict())
    nm, em = masks([3, 2])
    xh, ex, nl = torch.zeros(2, 3, 10), torch.zeros(2, 3, 3, 2), torch.zeros(2)

    class _Cuda(torch.Tensor):                     # a CPU tensor that claims to live on the GPU: reaches the checks behind the device test
        is_cuda = True
    model.split_bf16 = True
    model.bf16x3 = True                            # the new switch does not soften the old one's refusal
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r'split_bf16 is not implemented for DGT_concat_2D \(exact fp32 only\)'):
        model(None, xh.as_subclass(_Cuda), nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)

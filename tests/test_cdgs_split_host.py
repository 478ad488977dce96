"""CPU: the split-bf16 ("bf16x3") weight tape of CDGS (jodo_cdgs_split_size / jodo_cdgs_pack_split_host) against the packed blob it is
derived from, for both configs, and the switch's default.  The tape re-reads every covered tiled matrix float [nb][nk][8 quads][64 lanes][4]
as bf16 [nb][nk * 4 K16 steps][hi, mid, lo][64 lanes][8]: element j of lane l in K16 step G of a chunk is the chunk's f32 k-step 8 G + j of
the same lane.  The conversion is one routine shared with the 2-D model (csrc/split_tape.h); the 2-D tape of a seeded model is pinned by
its sha256, recorded from the build before the routine was shared."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from jodo_amd import capi
from jodo_amd.models import get_model_class, deterministic_init_
from helpers import make_config, make_model, state_dict_cpu

CFG = {'qm9': 'vpsde_qm9_2d_cdgs', 'geom': 'vpsde_geom_2d_cdgs'}
SHAPE = {'qm9': dict(L=8, catp=64, K=704), 'geom': dict(L=6, catp=96, K=768)}      # K = KA = KE: the padded head input widths
# include/jodo_hip.h enum jodo_cdgs_wslot_global / jodo_cdgs_wslot_block: (name, index in its table, output rows, K)
GLOBAL_COUNT, BLOCK_COUNT, D = 35, 28, 256
T_SLOTS = (1, 3, 5)                                           # T1_W, T2_W, TMOD_W: tiled, and exact fp32 in both forms


def _covered(which):
    s = SHAPE[which]
    block = (('GIN1', 1, D, D), ('GIN2', 3, D, D), ('QKV', 5, 3 * D, D), ('E01', 7, 2 * D, D), ('FF1', 12, 2 * D, D), ('FF2', 14, D, 2 * D),
             ('FF3', 18, 2 * D, D), ('FF4', 20, D, 2 * D), ('RN', 24, s['catp'], D), ('RE', 26, s['catp'], D))
    glob = (('EEMB', 13, D, D), ('NEMB', 21, D, D), ('AH1', 23, D, s['K']), ('AH2', 25, D // 2, D), ('AH3', 27, 32, D // 2),
            ('EH1', 29, 2 * D, s['K']), ('EH2', 31, D, 2 * D), ('EH3', 33, 32, D))
    out = [('%s[%d]' % (nm, l), GLOBAL_COUNT + l * BLOCK_COUNT + i, r // 32, k // 64) for l in range(s['L']) for nm, i, r, k in block]
    return out + [(nm, i, r // 32, k // 64) for nm, i, r, k in glob]


_PACKED = {}


def packed(which):
    if which not in _PACKED:
        cfg = make_config(CFG[which])
        model = deterministic_init_(get_model_class('CDGS')(cfg), seed=7)
        sd = state_dict_cpu(model)
        sd['time_freq'] = model._time_freq()
        blob, woff, n_woff = capi.pack_weights_cdgs(model._cfg_struct, sd)
        _PACKED[which] = (cfg, model, blob, woff, n_woff)
    return _PACKED[which]


@pytest.mark.parametrize('which', ['qm9', 'geom'])
def test_tape_is_the_exact_split_of_the_blob_in_the_k16_permutation(which):
    cfg, model, blob, woff, n_woff = packed(which)
    assert cfg.model.n_layers == SHAPE[which]['L'] and n_woff == GLOBAL_COUNT + cfg.model.n_layers * BLOCK_COUNT
    tape, toff = capi.split_tape_cdgs(model._cfg_struct, blob, woff, n_woff)
    total = ctypes.c_size_t()
    toff2 = (ctypes.c_int64 * n_woff)()
    capi.check(capi.lib().jodo_cdgs_split_size(ctypes.byref(model._cfg_struct), ctypes.byref(total), toff2, n_woff), 'split_size')
    assert list(toff2) == list(toff) and total.value == tape.numel()
    covered = _covered(which)
    slots = {s for _, s, _, _ in covered}
    assert len(slots) == len(covered)
    assert sorted(i for i in range(n_woff) if toff[i] >= 0) == sorted(slots)             # one entry per covered slot ...
    assert all(toff[i] == -1 for i in range(n_woff) if i not in slots)                   # ... and -1 for biases, norms, small vectors
    assert all(toff[i] == -1 for i in T_SLOTS)                                           # the time GEMMs stay fp32
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
        mid = r1.to(torch.bfloat16)
        assert np.array_equal(b2f(t[:, :, 1]), mid.double().numpy()), name
        r2 = r1 - mid.float()
        assert np.array_equal(b2f(t[:, :, 2]), r2.to(torch.bfloat16).double().numpy()), name
        nonzero += int(np.count_nonzero(rec))
    assert nonzero > 1000000                                   # the comparison is not one of zeros


def test_tape_entries_refuse_bad_arguments():
    cfg, model, blob, woff, n_woff = packed('qm9')
    L = capi.lib()
    c = ctypes.byref(model._cfg_struct)
    total = ctypes.c_size_t()
    toff = (ctypes.c_int64 * (n_woff + 1))()
    assert L.jodo_cdgs_split_size(c, ctypes.byref(total), toff, n_woff) == 0
    for bad in (n_woff - 1, n_woff + 1, 0):
        assert L.jodo_cdgs_split_size(c, ctypes.byref(total), toff, bad) == -1                     # JODO_ERR_ARG
    assert L.jodo_cdgs_split_size(c, None, toff, n_woff) == -1
    assert L.jodo_cdgs_split_size(c, ctypes.byref(total), None, n_woff) == -1
    tape = np.zeros(total.value, dtype=np.uint8)
    tp, bp, cap = tape.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(blob.data_ptr()), ctypes.c_size_t(total.value)
    assert L.jodo_cdgs_pack_split_host(c, bp, woff, n_woff, tp, cap) == 0
    assert L.jodo_cdgs_pack_split_host(c, bp, woff, n_woff - 1, tp, cap) == -1
    assert L.jodo_cdgs_pack_split_host(c, None, woff, n_woff, tp, cap) == -1
    assert L.jodo_cdgs_pack_split_host(c, bp, None, n_woff, tp, cap) == -1
    assert L.jodo_cdgs_pack_split_host(c, bp, woff, n_woff, None, cap) == -1
    assert L.jodo_cdgs_pack_split_host(c, bp, woff, n_woff, tp, ctypes.c_size_t(total.value - 16)) == -1       # buffer too small
    assert b'need' in L.jodo_last_error()
    for slot, off in ((GLOBAL_COUNT + 5, blob.numel() - 2048), (33, -64)):                         # a covered matrix that leaves the blob
        bad = (ctypes.c_int64 * n_woff)(*woff)
        bad[slot] = off
        assert L.jodo_cdgs_pack_split_host(c, bp, bad, n_woff, tp, cap) == -1
        assert b'outside the packed blob' in L.jodo_last_error()


def test_switch_default_and_runtime_state():
    model = get_model_class('CDGS')(make_config(CFG['qm9']))
    assert model.bf16x3 is False and model._tape is None and model.last_flags is None
    assert 'bf16x3' not in model.state_dict() and not any('tape' in k for k in model.state_dict())


def test_2d_tape_is_byte_identical_to_the_one_before_the_shared_routine():
    cfg = make_config('vpsde_zinc_2d_jodo')
    model = make_model(cfg, seed=7)
    blob, woff, n_woff = capi.pack_weights_2d(model._cfg_struct, state_dict_cpu(model))
    assert hashlib.sha256(blob.numpy().tobytes()).hexdigest() == '229b24ad152b638f61c5c3ec24c0aefa6068db1f6d135dd8ff97a3d5ed271468'
    tape, _ = capi.split_tape_2d(model._cfg_struct, blob, woff, n_woff)
    assert tape.numel() == 25878528
    assert hashlib.sha256(tape.numpy().tobytes()).hexdigest() == '6e1728831411b1ee6dda65d9259842c8f3f21fa052ade59532fafcc41ba44043'

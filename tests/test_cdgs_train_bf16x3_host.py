"""CPU: the switch of the split-bf16 training products (CDGS.train_bf16x3, jodo_amd.train.split_mask) and what the host emulation build
of csrc/cdgs_train.hip (tests/emulcdgs) answers to option 3: it has no matrix instructions, stays exact fp32 and says so."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cdgs_train_common as C

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emulcdgs')
JODO_ERR_ARG, JODO_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def emul():
    subprocess.run(['make', '-C', EMUL_DIR, 'libjodo_cdgs_train_emul.so'], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_cdgs_train_emul.so'))


def engine_for(emul, model, n_nodes, N, **kw):
    from jodo_amd.train import TrainEngineCDGS
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    return TrainEngineCDGS(model._cfg_struct, n_nodes, N, named, 'cpu', lib=emul, stream_ptr=lambda: ctypes.c_void_p(0), **kw)


def test_attribute_default_and_state_dict():
    _, model = C.fresh_model('qm9')
    assert model.train_bf16x3 is False and model.last_train_form is None and model.bf16x3 is False
    keys = set(model.state_dict().keys())
    model.train_bf16x3 = True
    assert set(model.state_dict().keys()) == keys and not any('bf16x3' in k for k in keys)


def test_mask_parsing():
    from jodo_amd.train import TRAIN_BF16X3_ALL, split_mask
    assert TRAIN_BF16X3_ALL == 3                                   # forward products | data gradients: DESIGN.md 4n says why not 7
    assert split_mask(False) == 0 and split_mask(None) == 0 and split_mask(True) == TRAIN_BF16X3_ALL
    for m in range(8):
        assert split_mask(m) == m and split_mask(np.int32(m)) == m
    for bad in (-1, 8, 1.0, 2.5, '7', [1], (1, 2)):
        with pytest.raises(ValueError, match='train_bf16x3'):
            split_mask(bad)


def test_the_host_build_refuses_the_split_form_and_reads_back_zero(emul):
    from jodo_amd import capi
    model = C.model_for('qm9')[1]
    eng = engine_for(emul, model, [3, 2], 4)
    assert eng.form == 0
    assert emul.jodo_cdgs_train_set_option(eng.handle, 3, 0) == 0
    for mask in (1, 2, 4, 7):
        assert emul.jodo_cdgs_train_set_option(eng.handle, 3, mask) == JODO_ERR_UNSUPPORTED
    emul.jodo_last_error.restype = ctypes.c_char_p
    assert b'exact fp32' in emul.jodo_last_error()
    for bad in (-1, 8):
        assert emul.jodo_cdgs_train_set_option(eng.handle, 3, bad) == JODO_ERR_ARG
    assert eng.form == 0
    v = ctypes.c_int(-1)
    assert emul.jodo_cdgs_train_get_option(eng.handle, 3, ctypes.byref(v)) == 0 and v.value == 0
    assert emul.jodo_cdgs_train_get_option(eng.handle, 9, ctypes.byref(v)) == JODO_ERR_ARG
    assert emul.jodo_cdgs_train_get_option(eng.handle, 3, None) == JODO_ERR_ARG
    with pytest.raises(capi.JodoHipError, match='exact fp32'):
        eng.set_form(7)
    with pytest.raises(capi.JodoHipError, match='exact fp32'):                       # the `options` plumbing of the constructor
        engine_for(emul, model, [3, 2], 4, options={3: 1})
    assert engine_for(emul, model, [3, 2], 4, options={3: 0}).form == 0

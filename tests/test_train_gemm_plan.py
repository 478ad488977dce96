"""plan() of tests/test_train_gemm_split_gpu.py — the pure-integer restatement of train_gemm.h gemm_plan by which the split-K tests assert
the slice counts they hit — against gemm_plan itself, exported by the host emulation build (tests/emul/emul_gemm.cpp emul_gemm_plan)."""
import ctypes
import os
import random
import subprocess

import pytest

from test_train_gemm_split_gpu import NT_SHAPES, SLICES, WS_FLOATS, plan

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')


@pytest.fixture(scope='module')
def header_plan():
    subprocess.run(['make', '-C', EMUL_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_train_emul.so'))
    lib.emul_gemm_plan.argtypes = [ctypes.c_int] * 5 + [ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.emul_gemm_plan.restype = None

    def f(tA, M, N, K, have_ws=True, ws_floats=WS_FLOATS):
        a, b = ctypes.c_int(), ctypes.c_int()
        lib.emul_gemm_plan(tA, M, N, K, int(have_ws), ws_floats, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value
    return f


def test_the_restatement_is_the_plan(header_plan):
    """Every shape of the split-K tests and of test_train_gpu.py's GEMM cases, and 20 000 random (tA, M, N, K, scratch) draws."""
    cases = [(1, 64, 64, 64 * s, True, WS_FLOATS) for s in SLICES] + [(1, 64, 64, 64 * s + 5, True, WS_FLOATS) for s in (16, 63)]
    cases += [(1, 64, 64, 300000, True, WS_FLOATS), (1, 64, 64, 2560, True, 5 * 4160 + 7), (1, 64, 64, 2560, True, 2 * 4160 - 1),
              (1, 64, 64, 2560, False, 0)]
    cases += [(0, M, N, K, True, WS_FLOATS) for M, N, K, _, _ in NT_SHAPES]
    cases += [(1, 256, 64, 50000, True, WS_FLOATS), (1, 3, 256, 9000, True, WS_FLOATS), (1, 252, 64, 1187, True, WS_FLOATS),
              (0, 3, 1536, 1024, True, WS_FLOATS), (0, 9001, 256, 256, True, WS_FLOATS), (1, 64, 64, 17, True, WS_FLOATS)]
    rnd = random.Random(4)
    for _ in range(20000):
        M, N = rnd.choice([1, 3, 63, 64, 65, 128, 252, 256, 640, 1536, 9001]), rnd.choice([3, 64, 65, 128, 256, 640, 1536])
        K = rnd.choice([rnd.randint(1, 2000), rnd.randint(1, 70000), rnd.randint(200000, 600000), 64 * rnd.randint(1, 600), 511, 512, 513])
        ws = rnd.choice([WS_FLOATS, 0, (M * N + M) * rnd.randint(0, 600) + rnd.randint(0, 9), rnd.randint(0, 1 << 22)])
        cases.append((rnd.randint(0, 1), M, N, K, rnd.random() < 0.9, ws))
    bad = [(c, plan(*c), header_plan(*c)) for c in cases if plan(*c) != header_plan(*c)]
    assert not bad, bad[:5]


def test_the_slice_counts_the_suite_ran_before(header_plan):
    """The split cases of tests/test_train_gpu.py: 19, 141 and 174 slices and the 8 of the modulation projection — few, and none on an
    edge of k_splitk_sum's loops."""
    assert header_plan(1, 256, 64, 50000) == (174, 288) and header_plan(1, 252, 64, 1187) == (19, 64) and header_plan(1, 64, 64, 1187) == (19, 64)
    assert header_plan(1, 3, 256, 9000) == (141, 64) and header_plan(0, 3, 1536, 1024) == (8, 128) and header_plan(1, 252, 256, 300)[0] == 1

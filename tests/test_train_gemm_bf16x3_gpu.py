"""GPU: the split-bf16 form of the training GEMM (csrc/train_gemm.hip k_gemm_s) through jodo_train_gemm_s.

1. Exactness, zero tolerance: products in which one factor of every output is a pure bf16 number (a signed power of two, a small
   integer) are exact in the three-term form — a missing or misplaced term, a wrong lane map or an unzeroed K tail shows as wrong bits.
2. Edges: ragged M / N / K, unaligned operands (element-wise loads), wide output rows, column ranges of a wider weight, NaN-filled C.
3. Split-K: the slices of train_gemm.h gemm_plan (asserted through tests/test_train_gemm_split_gpu.plan), dbias, no scratch, capped scratch.
4. Epilogues: tanh, SiLU x dropout with the fp32 form's element numbering.
5. Accuracy gate: error against float64 at most 2.0 x the fp32 form's on the same inputs (the project's gate, tests/test_cdgs_split_gpu.py).
6. Determinism and refusals.
Tolerances against float64 are those of tests/test_train_gemm_split_gpu.py (close, 2e-6 sqrt(K) 4 absolute + 2e-5 relative)."""
import ctypes

import pytest
import torch

from test_train_gemm_split_gpu import close, plan

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
JODO_ERR_ARG = -1


def stored(X, t):
    """op(A) [M, K] as A is stored (tA: [K, M]), op(B) [K, N] as B is stored (tB: [N, K])."""
    return X.t().contiguous() if t else X.contiguous()


def raw(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, bias=None, acc=0, act=0, out2=None, dbias=None, p=0.0, seed=0, site=0, ws=None, ws_floats=None):
    from jodo_amd import capi
    as_ptr = lambda v: v if isinstance(v, ctypes.c_void_p) else capi.ptr(v)
    return capi.lib().jodo_train_gemm_s(tA, tB, M, N, K, as_ptr(A), lda, as_ptr(B), ldb, as_ptr(C), ldc, capi.ptr(bias), acc, act, capi.ptr(out2),
                                        capi.ptr(dbias), p, seed, site, capi.ptr(ws), (ws.numel() if ws is not None else 0) if ws_floats is None else ws_floats,
                                        capi.current_stream_ptr())


def product_s(tA, tB, A, B, **kw):
    """op(A) [M, K] x op(B) [K, N] (CPU float32, logical orientation) -> C [M, N] on the CPU, dense operands, C pre-filled with NaN."""
    from jodo_amd import capi
    M, K = A.shape
    N = B.shape[1]
    Ad, Bd = stored(A, tA).to(DEV), stored(B, tB).to(DEV)
    C = torch.full((M, N), float('nan'), device=DEV)
    capi.check(raw(tA, tB, M, N, K, Ad, Ad.shape[1], Bd, Bd.shape[1], C, N, **kw), 'jodo_train_gemm_s')
    torch.cuda.synchronize()
    return C.cpu()


def wide_exponents(g, *shape):
    """Random float32 with full 24-bit significands and exponents spread over 2^-20 .. 2^20."""
    return torch.randn(*shape, generator=g) * torch.pow(2.0, torch.randint(-20, 21, shape, generator=g).float())


def partial_permutation(g, rows, cols):
    """[rows, cols] with one non-zero in min(rows, cols) distinct rows and columns, each +-2^e, e in [-3, 3]."""
    S = torch.zeros(rows, cols)
    n = min(rows, cols)
    r, c = torch.randperm(rows, generator=g)[:n], torch.randperm(cols, generator=g)[:n]
    S[r, c] = torch.pow(2.0, torch.randint(-3, 4, (n,), generator=g).float()) * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)
    return S


# ---- 1. exactness ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tA,tB', LAYOUTS)
def test_products_with_a_pure_bf16_factor_are_exact(tA, tB):
    """A S (S: one +-2^e per used row and column: pins h*h, m*h, l*h and their k positions) and S B (h*h, h*m, h*l): every output is one
    product — or an exact zero — so the result is the permuted, scaled operand BIT FOR BIT."""
    g = torch.Generator().manual_seed(10 * tA + tB)
    for K in (1, 7, 16, 17, 33, 77):
        for M in (1, 3, 65):
            for N in (3, 51, 64):
                A, S = wide_exponents(g, M, K), partial_permutation(g, K, N)
                want = (A.double() @ S.double()).float()
                assert torch.equal(want.double(), A.double() @ S.double())                  # the yardstick itself is exact
                got = product_s(tA, tB, A, S)
                assert torch.equal(got, want), ('A S', K, M, N, float((got - want).abs().max()))
                S, B = partial_permutation(g, M, K), wide_exponents(g, K, N)
                want = (S.double() @ B.double()).float()
                got = product_s(tA, tB, S, B)
                assert torch.equal(got, want), ('S B', K, M, N, float((got - want).abs().max()))


@pytest.mark.parametrize('tA,tB', LAYOUTS)
def test_small_integer_products_are_exact(tA, tB):
    g = torch.Generator().manual_seed(20 + 10 * tA + tB)
    for M, N in ((1, 3), (65, 51), (3, 64)):
        A, B = torch.randint(-8, 9, (M, 77), generator=g).float(), torch.randint(-8, 9, (77, N), generator=g).float()
        assert torch.equal(product_s(tA, tB, A, B).double(), A.double() @ B.double())


# ---- 2. edges --------------------------------------------------------------------------------------------------------------------------
def edge_case(tA, tB, M, N, K, g, pad_a=0, pad_b=0, off=0, acc=0):
    """One product with ldc = N + 4 (sentinel columns), leading dimensions padded by pad_a / pad_b floats, base pointers `off` floats into
    their buffers; C holds NaN where it is overwritten (acc = 0), random numbers where it is accumulated into."""
    from jodo_amd import capi
    A, B, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(N, generator=g)

    def place(X, pad):
        buf = torch.full((X.shape[0] * (X.shape[1] + pad) + off,), 3.5)
        buf[off:].view(X.shape[0], X.shape[1] + pad)[:, :X.shape[1]] = X
        return buf.to(DEV), X.shape[1] + pad
    (Ad, lda), (Bd, ldb) = place(stored(A, tA), pad_a), place(stored(B, tB), pad_b)
    C0 = torch.randn(M, N + 4, generator=g)
    if not acc:
        C0[:, :N] = float('nan')
    Cd = C0.clone().to(DEV)
    at = lambda t_: ctypes.c_void_p(t_.data_ptr() + 4 * off)
    capi.check(raw(tA, tB, M, N, K, at(Ad), lda, at(Bd), ldb, Cd, N + 4, bias=bias.to(DEV), acc=acc), 'jodo_train_gemm_s')
    torch.cuda.synchronize()
    got = Cd.cpu()
    assert torch.equal(got[:, N:], C0[:, N:]), (M, N, K)                                        # the sentinel columns are untouched
    want = A.double() @ B.double() + bias.double() + (C0[:, :N].double() if acc else 0)
    close(got[:, :N], want, atol=2e-6 * (K ** 0.5) * 4, rtol=2e-5)


@pytest.mark.parametrize('tA,tB', LAYOUTS)
def test_ragged_sizes(tA, tB):
    g = torch.Generator().manual_seed(30 + 10 * tA + tB)
    for M in (63, 64, 65, 130):
        for N in (3, 77, 154, 256):
            for K in (8, 15, 31, 32, 48):
                edge_case(tA, tB, M, N, K, g, acc=(M + N + K) & 1)


@pytest.mark.parametrize('tA,tB', LAYOUTS)
def test_unaligned_operands_take_the_element_wise_path(tA, tB):
    """Leading dimensions that are no multiple of 4, and base pointers one float off a 16-byte boundary."""
    g = torch.Generator().manual_seed(40 + 10 * tA + tB)
    for M, N, K in ((65, 77, 31), (63, 3, 48), (130, 154, 32)):
        edge_case(tA, tB, M, N, K, g, pad_a=1, pad_b=3)
        edge_case(tA, tB, M, N, K, g, off=1, acc=1)
        edge_case(tA, tB, M, N, K, g, pad_a=2, pad_b=1, off=1)


@pytest.mark.parametrize('ranges', [(51, 154, 51), (77, 77, 102)])
def test_column_ranges_of_a_wider_weight_accumulate(ranges):
    """Y = sum over column ranges of X[:, range] W[:, range]^T (the heads' input of several column ranges: lda = ldb = the full width, base
    pointers at the range's first column, acc = 1 from the second range on)."""
    from jodo_amd import capi
    g = torch.Generator().manual_seed(sum(ranges) + ranges[0])
    M, N, K0 = 130, 77, sum(ranges)
    X, W, bias = torch.randn(M, K0, generator=g), torch.randn(N, K0, generator=g) / 8, torch.randn(N, generator=g)
    Xd, Wd, Y = X.to(DEV), W.to(DEV), torch.full((M, N), float('nan'), device=DEV)
    c0 = 0
    for i, w in enumerate(ranges):
        at = lambda t_: ctypes.c_void_p(t_.data_ptr() + 4 * c0)
        capi.check(raw(0, 1, M, N, w, at(Xd), K0, at(Wd), K0, Y, N, bias=bias.to(DEV) if i == 0 else None, acc=int(i > 0)), 'jodo_train_gemm_s')
        c0 += w
    torch.cuda.synchronize()
    close(Y, X.double() @ W.double().t() + bias.double(), atol=2e-6 * (K0 ** 0.5) * 4, rtol=2e-5)


# ---- 3. split-K ------------------------------------------------------------------------------------------------------------------------
WS_FLOATS = 8 << 20
SPLIT_CASES = [(511, 1), (512, 8), (513, 9), (1025, 17), (4097, 65)]


def run_dw_s(M, N, K, dbias, ws_floats=WS_FLOATS, have_ws=True):
    """tests/test_train_gemm_split_gpu.run_dw for the split form: dW[M, N] += dY[K, M]^T X[K, N], db[M] += column sums of dY."""
    from jodo_amd import capi
    g = torch.Generator().manual_seed(K + M + (1 if dbias else 0))
    dY, X = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    dW0, db0 = torch.randn(M, N + 4, generator=g), torch.randn(M, generator=g)
    dW, db = dW0.clone().to(DEV), db0.clone().to(DEV)
    guard = 4096
    ws = torch.full((ws_floats + guard,), 7.25, device=DEV) if have_ws else None
    capi.check(raw(1, 0, M, N, K, dY.to(DEV), M, X.to(DEV), N, dW, N + 4, acc=1, dbias=db if dbias else None, ws=ws, ws_floats=ws_floats if have_ws else 0),
               'jodo_train_gemm_s')
    torch.cuda.synchronize()
    got = dW.cpu()
    assert torch.equal(got[:, N:], dW0[:, N:])
    if have_ws:
        assert bool((ws[ws_floats:] == 7.25).all())                                        # nothing behind the scratch the call was given
    close(got[:, :N], dW0[:, :N].double() + dY.double().t() @ X.double(), atol=2e-6 * (K ** 0.5) * 4, rtol=2e-5)
    if dbias:
        close(db, db0.double() + dY.double().sum(0), atol=2e-6 * (K ** 0.5), rtol=2e-5)
    else:
        assert torch.equal(db.cpu(), db0)
    return got


@pytest.mark.parametrize('dbias', [False, True])
@pytest.mark.parametrize('M,N', [(64, 64), (3, 256)])
def test_weight_gradient_slices(M, N, dbias):
    for K, slices in SPLIT_CASES:
        assert plan(1, M, N, K)[0] == slices
        run_dw_s(M, N, K, dbias)


@pytest.mark.parametrize('dbias', [False, True])
def test_weight_gradient_without_scratch_and_under_a_scratch_cap(dbias):
    M, N, per = 64, 64, 64 * 64 + 64
    for K, chunk in ((513, 192), (4097, 1376)):
        assert plan(1, M, N, K, have_ws=False, ws_floats=0)[0] == 1
        run_dw_s(M, N, K, dbias, have_ws=False)
        assert plan(1, M, N, K, ws_floats=3 * per + 5) == (3, chunk)                         # the cap lowers the slice count
        run_dw_s(M, N, K, dbias, ws_floats=3 * per + 5)


# ---- 4. epilogues ----------------------------------------------------------------------------------------------------------------------
def test_tanh_epilogue():
    g = torch.Generator().manual_seed(50)
    M, N, K = 65, 77, 64
    X, W = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / 8
    bias = torch.randn(N, generator=g)
    got = product_s(0, 1, X, W, bias=bias.to(DEV), act=1)
    close(got, torch.tanh(X.double() @ W.double() + bias.double()), atol=2e-6, rtol=1e-4)           # tests/test_train_gpu.py's K = 64 number


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_silu_dropout_epilogue_uses_the_fp32_forms_element_numbering(p):
    """act 2: C keeps the pre-activation, out2 = SiLU(pre) x the dropout multiplier of element m N + n — the multipliers the fp32 training
    kernels draw for the same seed and site (jodo_cdgs_train_debug_drop), so the zero pattern is identical."""
    from jodo_amd import capi
    g = torch.Generator().manual_seed(51)
    M, N, K, seed, site = 130, 77, 64, 2 ** 40 + 9, 13
    X, W, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / 8, torch.randn(N, generator=g)
    out2 = torch.full((M, N), float('nan'), device=DEV)
    pre = product_s(0, 1, X, W, bias=bias.to(DEV), act=2, out2=out2, p=p, seed=seed, site=site)
    out2 = out2.cpu()
    mult = torch.empty(M, N, device=DEV)
    capi.check(capi.lib().jodo_cdgs_train_debug_drop(p, seed, site, 0, M, N, capi.ptr(mult), capi.current_stream_ptr()), 'jodo_cdgs_train_debug_drop')
    mult = mult.cpu()
    want = X.double() @ W.double() + bias.double()
    close(pre, want, atol=1e-5, rtol=1e-4)                                                            # the pre-activation is kept
    assert torch.equal(out2 == 0, (mult == 0) | (pre == 0))
    if p > 0:
        vals = mult.unique().tolist()
        assert 0.05 < float((mult == 0).float().mean()) < 0.15 and len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1 / (1 - p)) < 1e-6
    else:
        assert bool((mult == 1).all())
    close(out2, torch.nn.functional.silu(want) * mult.double(), atol=1e-5 * float(mult.max()), rtol=1e-4)


# ---- 5. accuracy gate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,K,tA,tB', [(2048, 256, 256, 0, 1), (2048, 512, 256, 0, 0), (256, 256, 8192, 1, 0)])
def test_error_against_float64_is_within_twice_the_fp32_forms(M, N, K, tA, tB):
    from jodo_amd import capi
    g = torch.Generator().manual_seed(M + N + K)
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    want = A.double() @ B.double()
    Ad, Bd = stored(A, tA).to(DEV), stored(B, tB).to(DEV)
    ws = torch.empty(WS_FLOATS, device=DEV)
    err = {}
    for form in ('fp32', 'split'):
        C = torch.full((M, N), float('nan'), device=DEV)
        if form == 'fp32':
            capi.check(capi.lib().jodo_train_gemm(tA, tB, M, N, K, capi.ptr(Ad), Ad.shape[1], capi.ptr(Bd), Bd.shape[1], capi.ptr(C), N, None, 0,
                                                  capi.ptr(ws), ctypes.c_size_t(ws.numel()), capi.current_stream_ptr()), 'jodo_train_gemm')
        else:
            capi.check(raw(tA, tB, M, N, K, Ad, Ad.shape[1], Bd, Bd.shape[1], C, N, ws=ws), 'jodo_train_gemm_s')
        torch.cuda.synchronize()
        err[form] = float((C.cpu().double() - want).abs().max())
        close(C, want, atol=2e-6 * (K ** 0.5) * 4, rtol=2e-5)
    print('[%d x %d x %d] (%d, %d): err fp32 form %.3e, split form %.3e, ratio %.2f' % (M, N, K, tA, tB, err['fp32'], err['split'],
                                                                                      err['split'] / max(err['fp32'], 1e-30)))
    assert err['split'] <= 2.0 * err['fp32'], err


# ---- 6. determinism and refusals -------------------------------------------------------------------------------------------------------
def test_two_runs_give_equal_bits():
    g = torch.Generator().manual_seed(60)
    ws = torch.empty(WS_FLOATS, device=DEV)
    for tA, tB, M, N, K in ((1, 0, 64, 154, 4097), (0, 1, 130, 77, 48), (0, 0, 3, 256, 1100)):
        A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
        assert torch.equal(product_s(tA, tB, A, B, ws=ws), product_s(tA, tB, A, B, ws=ws))


def test_bad_arguments_are_refused():
    from jodo_amd import capi
    A, B, C = (torch.zeros(64, 64, device=DEV) for _ in range(3))
    ok = dict(tA=0, tB=1, M=64, N=64, K=64, A=A, lda=64, B=B, ldb=64, C=C, ldc=64)
    assert raw(**ok) == 0
    for bad in (dict(M=-1), dict(N=-1), dict(K=-1), dict(act=1, acc=1), dict(act=2, out2=C, acc=1), dict(act=2), dict(act=3), dict(dbias=C),
                dict(tA=1, act=1, dbias=C), dict(p=1.0), dict(p=-0.5), dict(site=-1), dict(A=None)):
        assert raw(**dict(ok, **bad)) == JODO_ERR_ARG, bad
    assert b'jodo_train_gemm_s' in capi.lib().jodo_last_error()
    torch.cuda.synchronize()

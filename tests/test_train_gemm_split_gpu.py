"""Split-K edges of the training path's fp32 GEMM (csrc/train_gemm.hip jt::gemm, train_gemm.h gemm_plan) that the shapes of
tests/test_train_gpu.py do not reach: slice counts on both sides of k_splitk_sum's 64-wide and 8-wide loops, the 512-slice clamp
(K > 262144: a GEOM batch's edge rows), the workspace cap, no workspace, the non-transposed rule at its 256 / tiles limit, and split-K
with the tanh / SiLU epilogues (the modulation and time projections: K = 4 nf >= 512 on a few rows).  Every case states the slice count
it is meant to hit and asserts it through plan(), a restatement of gemm_plan (held against the header itself by
tests/test_train_gemm_plan.py): a change of the plan cannot quietly move a case off its edge.
Against float64 on the CPU at the tolerances of tests/test_train_gpu.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WS_FLOATS = 8 << 20


def plan(tA, M, N, K, have_ws=True, ws_floats=WS_FLOATS):
    """train_gemm.h gemm_plan in integers: (nsplit, kchunk), nsplit = ceil(K / kchunk) the number of slices that run."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    nsplit = 1
    if have_ws and K >= 512 and (tA or tiles < 128):
        if tA:
            nsplit = (K + 511) // 512
            if tiles * nsplit < 512:
                nsplit = max(nsplit, min(768 // tiles, (K + 63) // 64))
        else:
            nsplit = min((K + 127) // 128, 256 // tiles)
        nsplit = max(1, min(nsplit, ws_floats // (M * N + M), 512))
    kchunk = max(32, ((K + nsplit - 1) // nsplit + 31) // 32 * 32)
    return ((K + kchunk - 1) // kchunk if K > 0 else 1), kchunk


def close(got, want, atol, rtol=1e-4):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    assert bool((err <= atol + rtol * want.abs()).all()), "max err %.3e (max |want| %.3e)" % (err.max().item(), want.abs().max().item())


def run_dw(M, N, K, dbias, ws_floats=WS_FLOATS, have_ws=True, seed=0):
    """dW[M, N] += dY[K, M]^T X[K, N] (tA = 1, tB = 0, accumulating), with db[M] += column sums of dY when dbias: jodo_train_gemm_ex, or
    jodo_train_gemm without dbias.  The workspace is allocated with a guard behind the ws_floats the call is told of.  Checked against
    float64 at the tolerances of test_train_gemm_matches_float64 / ..._bias_gradient_rides_on_the_weight_gradient."""
    from jodo_amd import capi
    g = torch.Generator().manual_seed(1000 * seed + K + (1 if dbias else 0))
    dY, X = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    dW0, db0 = torch.randn(M, N + 4, generator=g), torch.randn(M, generator=g)
    dW, db = dW0.clone().to(DEV), db0.clone().to(DEV)
    guard = 4096
    ws = torch.full((ws_floats + guard,), 7.25, device=DEV) if have_ws else None
    dYd, Xd = dY.to(DEV), X.to(DEV)
    L = capi.lib()
    if dbias:
        capi.check(L.jodo_train_gemm_ex(1, 0, M, N, K, capi.ptr(dYd), M, capi.ptr(Xd), N, capi.ptr(dW), N + 4, None, 0, None, capi.ptr(db), capi.ptr(ws),
                                        ctypes.c_size_t(ws_floats if have_ws else 0), capi.current_stream_ptr()), 'jodo_train_gemm_ex')
    else:
        capi.check(L.jodo_train_gemm(1, 0, M, N, K, capi.ptr(dYd), M, capi.ptr(Xd), N, capi.ptr(dW), N + 4, None, 1, capi.ptr(ws),
                                     ctypes.c_size_t(ws_floats if have_ws else 0), capi.current_stream_ptr()), 'jodo_train_gemm')
    torch.cuda.synchronize()
    got = dW.cpu()
    assert torch.equal(got[:, N:], dW0[:, N:])                                             # nothing written beyond the N columns
    if have_ws:
        assert bool((ws[ws_floats:] == 7.25).all())                                        # ... nor behind the scratch the call was given
    close(got[:, :N], dW0[:, :N].double() + dY.double().t() @ X.double(), atol=2e-6 * (K ** 0.5) * 4, rtol=2e-5)
    if dbias:
        close(db, db0.double() + dY.double().sum(0), atol=2e-6 * (K ** 0.5), rtol=2e-5)
    else:
        assert torch.equal(db.cpu(), db0)


SLICES = [8, 9, 15, 16, 17, 56, 57, 63, 64, 65, 72, 73, 120, 121, 128, 129, 511, 512]


@pytest.mark.parametrize("dbias", [False, True])
@pytest.mark.parametrize("s", SLICES)
def test_weight_gradient_slice_counts(s, dbias):
    """One output tile (M = N = 64), K = 64 s: exactly s slices of 64 rows, s on both sides of the multiples of 8 (the tail loop of
    k_splitk_sum: lanes g < s mod 8 take one slice more) and of 64 (its unrolled loop runs while z + 56 < s: s = 57 is the first slice
    count at which lane group 0 enters it, 64 the first at which all eight do, 121 / 128 the same for the second round)."""
    K = 64 * s
    assert plan(1, 64, 64, K) == (s, 64)
    run_dw(64, 64, K, dbias)


@pytest.mark.parametrize("dbias", [False, True])
@pytest.mark.parametrize("s,want", [(16, 17), (63, 64)])
def test_weight_gradient_ragged_last_slice(s, want, dbias):
    """K = 64 s + 5: s + 1 slices, the last one of five rows (a partial K tile, a partial quad of rows)."""
    K = 64 * s + 5
    assert plan(1, 64, 64, K) == (want, 64) and K - (want - 1) * 64 == 5
    run_dw(64, 64, K, dbias)


@pytest.mark.parametrize("dbias", [False, True])
def test_weight_gradient_at_the_512_slice_clamp(dbias):
    """K = 300000 rows (a GEOM batch: 16 molecules of up to 181 atoms are up to 524 000 edge rows): 586 slices of 512 rows are clamped
    to 512, which rounds the slice to 608 rows and leaves 494 — the last one of 256 rows.  Operands of 77 MB each."""
    assert plan(1, 64, 64, 300000) == (494, 608)
    run_dw(64, 64, 300000, dbias)


@pytest.mark.parametrize("dbias", [False, True])
def test_weight_gradient_under_the_workspace_cap(dbias):
    """K = 2560 wants 40 slices; scratch for 5 partial tiles and their bias sums (+ 7 floats) gives 5 slices of 512 rows, scratch just
    below two gives none, as does no scratch at all — and nothing is written behind the scratch."""
    M = N = 64
    K = 2560
    per = M * N + M
    assert plan(1, M, N, K) == (40, 64)
    assert plan(1, M, N, K, ws_floats=5 * per + 7) == (5, 512)
    run_dw(M, N, K, dbias, ws_floats=5 * per + 7, seed=1)
    assert plan(1, M, N, K, ws_floats=2 * per - 1) == (1, 2560)
    run_dw(M, N, K, dbias, ws_floats=2 * per - 1, seed=2)
    assert plan(1, M, N, K, have_ws=False, ws_floats=0) == (1, 2560)
    run_dw(M, N, K, dbias, have_ws=False, seed=3)


# tA = 0 (forward products of few rows: the per-molecule modulation and time projections): slices of 128, at most 256 / tiles of them.
# M = 128, N = 1536 is 48 tiles -> 5 slices at most: K = 512 stays below the limit (4), K = 1024 and 1100 want 8 and 9 and get 5.
NT_SHAPES = [
    # M, N, K, slices, kchunk
    (3, 256, 512, 4, 128), (3, 256, 1024, 8, 128), (3, 256, 1100, 9, 128),                 # 4 tiles: limit 64
    (128, 256, 512, 4, 128), (128, 256, 1024, 8, 128), (128, 256, 1100, 9, 128),           # 8 tiles: limit 32
    (3, 1536, 512, 4, 128), (3, 1536, 1024, 8, 128), (3, 1536, 1100, 9, 128),              # 24 tiles: limit 10
    (128, 1536, 512, 4, 128), (128, 1536, 1024, 5, 224), (128, 1536, 1100, 5, 224),        # 48 tiles: limit 5
]


def nt_inputs(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    X, W, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / 8, torch.randn(N, generator=g)
    C0 = torch.randn(M, N + 8, generator=g)
    return X, W, bias, C0


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("M,N,K,slices,kchunk", NT_SHAPES)
def test_non_transposed_split(M, N, K, slices, kchunk, acc):
    """Y (+)= X W^T + b, split over K, with bias, overwriting and accumulating."""
    from jodo_amd import capi
    assert plan(0, M, N, K) == (slices, kchunk)
    X, W, bias, C0 = nt_inputs(M, N, K)
    Xd, Wd, bd, Cd = X.to(DEV), W.to(DEV), bias.to(DEV), C0.clone().to(DEV)
    ws = torch.empty(WS_FLOATS, device=DEV)
    capi.check(capi.lib().jodo_train_gemm(0, 1, M, N, K, capi.ptr(Xd), K, capi.ptr(Wd), K, capi.ptr(Cd), N + 8, capi.ptr(bd), acc, capi.ptr(ws),
                                          ctypes.c_size_t(ws.numel()), capi.current_stream_ptr()), 'jodo_train_gemm')
    torch.cuda.synchronize()
    got = Cd.cpu()
    assert torch.equal(got[:, N:], C0[:, N:])
    want = X.double() @ W.double().t() + bias.double() + (C0[:, :N].double() if acc else 0)
    close(got[:, :N], want, atol=2e-6 * (K ** 0.5) * 4, rtol=2e-5)


@pytest.mark.parametrize("M,N,K,slices,kchunk", [(128, 640, 1024, 8, 128), (128, 1536, 1100, 5, 224), (3, 256, 1100, 9, 128)])
def test_non_transposed_split_of_a_plain_b(M, N, K, slices, kchunk):
    """The same rule with B stored [K, N] (the input-gradient layout), accumulating."""
    from jodo_amd import capi
    assert plan(0, M, N, K) == (slices, kchunk)
    g = torch.Generator().manual_seed(M + N + K + 1)
    A, B, C0 = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(M, N + 4, generator=g)
    Ad, Bd, Cd = A.to(DEV), B.to(DEV), C0.clone().to(DEV)
    ws = torch.empty(WS_FLOATS, device=DEV)
    capi.check(capi.lib().jodo_train_gemm(0, 0, M, N, K, capi.ptr(Ad), K, capi.ptr(Bd), N, capi.ptr(Cd), N + 4, None, 1, capi.ptr(ws),
                                          ctypes.c_size_t(ws.numel()), capi.current_stream_ptr()), 'jodo_train_gemm')
    torch.cuda.synchronize()
    got = Cd.cpu()
    assert torch.equal(got[:, N:], C0[:, N:])
    close(got[:, :N], C0[:, :N].double() + A.double() @ B.double(), atol=2e-6 * (K ** 0.5) * 4, rtol=2e-5)


# Activated outputs of the split products.  The suite's numbers (test_train_gemm_fused_activations, K = 64, W / 8): tanh 2e-6, the
# pre-activation and SiLU 1e-5.  At K >= 512 the float32 sum behind the activation carries sqrt(K) more rounding (|v| reaches 21 here), so
# the yardstick was measured first: the distance of a float32 CPU evaluation of the same expression, torch.tanh((X @ W.t() + b).float()),
# from its float64 value — worst over the four shapes of NT_SHAPES at that K (8 threads).  Four times that distance (the suite's K64
# convention) replaces a number above where it exceeds it, which it does everywhere.  On top of these absolute parts: rtol 2e-5, the
# plain products', in place of the 1e-4 the K = 64 tests allow.
#                K:  (tanh, pre-activation, SiLU)  float32-CPU distance from float64, measured
ACT_F32_DISTANCE = {512: (4.70e-6, 6.82e-6, 7.02e-6), 1024: (5.24e-6, 7.87e-6, 7.75e-6), 1100: (5.79e-6, 7.93e-6, 7.99e-6)}


def act_atol(K):
    d = ACT_F32_DISTANCE[K]
    return max(2e-6, 4 * d[0]), max(1e-5, 4 * d[1]), max(1e-5, 4 * d[2])


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("M,N,K,slices,kchunk", NT_SHAPES)
def test_split_with_the_activation_epilogues(M, N, K, slices, kchunk, act):
    """tanh(X W^T + b) (act 1) and the pre-activation with SiLU (act 2) behind a split product: k_splitk_sum applies the epilogue after
    the sum.  C and out2 have rows wider than N (ldc = N + 8): nothing is written beyond column N of either.

    Float32 yardstick (ACT_F32_DISTANCE: a float32 CPU evaluation against float64, worst over the four shapes at each K):
        K = 512:  tanh 4.70e-6, pre-activation 6.82e-6, SiLU 7.02e-6  -> atol 1.88e-5, 2.73e-5, 2.81e-5
        K = 1024: tanh 5.24e-6, pre-activation 7.87e-6, SiLU 7.75e-6  -> atol 2.10e-5, 3.15e-5, 3.10e-5
        K = 1100: tanh 5.79e-6, pre-activation 7.93e-6, SiLU 7.99e-6  -> atol 2.32e-5, 3.17e-5, 3.20e-5
    (four times the distance; each exceeds the suite's K = 64 numbers 2e-6 / 1e-5 / 1e-5), with rtol 2e-5."""
    from jodo_amd import capi
    assert plan(0, M, N, K) == (slices, kchunk)
    X, W, bias, C0 = nt_inputs(M, N, K)
    g = torch.Generator().manual_seed(act)
    O0 = torch.randn(M, N + 8, generator=g)
    Xd, Wd, bd, Cd, Od = X.to(DEV), W.to(DEV), bias.to(DEV), C0.clone().to(DEV), O0.clone().to(DEV)
    ws = torch.empty(WS_FLOATS, device=DEV)
    capi.check(capi.lib().jodo_train_gemm_ex(0, 1, M, N, K, capi.ptr(Xd), K, capi.ptr(Wd), K, capi.ptr(Cd), N + 8, capi.ptr(bd), act, capi.ptr(Od), None,
                                             capi.ptr(ws), ctypes.c_size_t(ws.numel()), capi.current_stream_ptr()), 'jodo_train_gemm_ex')
    torch.cuda.synchronize()
    C, out2 = Cd.cpu(), Od.cpu()
    assert torch.equal(C[:, N:], C0[:, N:]) and torch.equal(out2[:, N:], O0[:, N:])
    pre = X.double() @ W.double().t() + bias.double()
    tol_tanh, tol_pre, tol_silu = act_atol(K)
    if act == 1:
        close(C[:, :N], torch.tanh(pre), atol=tol_tanh, rtol=2e-5)
        assert torch.equal(out2, O0)                                                       # act 1 has no second output
    else:
        close(C[:, :N], pre, atol=tol_pre, rtol=2e-5)
        close(out2[:, :N], torch.nn.functional.silu(pre), atol=tol_silu, rtol=2e-5)

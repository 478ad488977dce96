"""CPU checks of the training step's small kernels (jodo_amd/csrc/train_step.hip: Kabsch rotations, Adam update, clipping decision): the
SAME source that libjodo_hip.so runs on the GPU, compiled for the host by tests/emul_step/Makefile against the sequential stand-in for
the HIP runtime (tests/emul/hip/hip_runtime.h; every kernel of that file is one thread per element or per molecule, without
cooperation), driven with host pointers and compared with float64 restatements.  tests/test_optim_gpu.py repeats the Kabsch batch on the
device.  The emulated library is test infrastructure: nothing under jodo_amd/ loads it."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import kabsch_cases as KC

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul_step')
NULL = ctypes.c_void_p(0)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def emul():
    subprocess.run(['make', '-C', EMUL_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_step_emul.so'))
    lib.jodo_kabsch_rotations.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.jodo_adam_step.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_double] * 5 + [ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                                                                     ctypes.c_void_p]
    lib.jodo_gradnorm_clip.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope='module')
def batch():
    b = KC.build_batch()
    b['want'] = KC.reference_aligned(b)
    return b


def rotations(emul, z, x):
    A = KC.covariance(z, x).contiguous()
    R = torch.full_like(A, math.nan)
    assert emul.jodo_kabsch_rotations(A.shape[0], ptr(A), ptr(R), NULL) == 0
    return A, R


def test_the_batch_holds_every_rank(batch):
    KC.assert_ranks(batch)


def test_kabsch_on_degenerate_molecules(emul, batch, capsys):
    """The batch of tests/kabsch_cases.py (1 to 4 atoms, collinear, planar in a tilted plane and in the xy-plane, thickness 1e-3 to 1e-7,
    regular tetrahedra, scales 1e-6 and 1e6: rank 0 to 3) through k_kabsch on the host: the aligned positions R xh are the float64 SVD
    form's within 2e-5 max(1, max |xh|), R is a proper rotation to 1e-6 wherever det A != 0, and finite where the third term is dropped.
    R itself is not compared: on rank-deficient A it is not unique (up to 1.98 from the SVD form's, measured below).

    Worst aligned-position error per case, in units of max(1, max |xh|) (measured; bound 2e-5):
        planar_tilted 1.2e-7  planar_xy 8.9e-8  n3 1.4e-7  square_rotated 1.1e-7  collinear 1.3e-7  collinear_axis 9.9e-8  n2 8.0e-8
        n1 0  n4 1.2e-7  tetra_exact 0  tetra_rotated 1.2e-7  tetra_perturbed 1.6e-7  thick_1e-3 6.8e-7  thick_1e-5 2.1e-7
        thick_1e-7 2.2e-7  x1e6: planar_tilted 3.2e-7  collinear 1.1e-7  n4 1.3e-7
        x1e-6: planar_tilted 6.1e-13  collinear 1.9e-13  n4 1.8e-13 (2.4e-7, 1.0e-7, 8e-8 of max |xh|: these are also held to 2e-5 max |xh|).
    Every branch of the kernel runs on this batch (gcov on the host build): the Jacobi early exit and the skipped zero pivot, the
    n1 == 0 fallback, the rank-one cross product, det == 0."""
    A, R = rotations(emul, batch['z'], batch['x'])
    aligned = torch.einsum('...ki,...ji->...jk', R, batch['x'])
    with capsys.disabled():
        KC.check_batch(batch, A, R, aligned, batch['want'], report=lambda w: print("\nkabsch (host build) worst |aligned - f64| per case:",
                                                                                  {k: "%.1e" % v for k, v in w.items()}))
    # R against the SVD form's: close where A has full rank, far where it has not (why R is not what the batch is judged by)
    from jodo_amd import losses as L
    Rsvd = L.kabsch_batch(batch['z'].double(), batch['x'].double())
    dist = (R.double() - Rsvd).abs().amax((1, 2))
    full = [b for b, c in enumerate(batch['case']) if c in KC.FULL or c.startswith('n4')]
    flat = [b for b, c in enumerate(batch['case']) if c in KC.PLANAR or c in KC.LINEAR]
    assert float(dist[full].max()) < 5e-6 and float(dist[flat].max()) > 1.0


def test_kabsch_is_deterministic_and_contains_a_nan(emul, batch):
    """The same batch twice gives bit-identical R; a NaN in one molecule's covariance comes back (twelve sweeps, no convergence loop) and
    leaves every other molecule's R bit for bit."""
    _, R1 = rotations(emul, batch['z'], batch['x'])
    _, R2 = rotations(emul, batch['z'], batch['x'])
    assert torch.equal(R1, R2)
    at = batch['case'].index('planar_tilted') + 3
    A, Rn = rotations(emul, KC.with_nan(batch, at), batch['x'])
    assert bool(torch.isnan(A[at]).any())
    keep = torch.ones(R1.shape[0], dtype=torch.bool)
    keep[at] = False
    assert torch.equal(Rn[keep], R1[keep])


def adam64(p, g, m, v, vmax, lr, beta1, beta2, eps, wd, step, decoupled, amsgrad):
    """torch's single-tensor formulas (torch/optim/adam.py, adamw.py _single_tensor_adam) in float64"""
    p, g, m, v, vmax = (t.double().clone() for t in (p, g, m, v, vmax))
    if decoupled:
        p.mul_(1 - lr * wd)
    else:
        g = g.add(p, alpha=wd)
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    if amsgrad:
        vmax = torch.maximum(vmax, v)
        denom = (vmax.sqrt() / math.sqrt(bc2)).add_(eps)
    else:
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
    return p, m, v, vmax


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("decoupled,amsgrad", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_adam_step_follows_the_single_tensor_formulas(emul, n, decoupled, amsgrad):
    """jodo_adam_step on n floats (whole quads and the element-wise tail: n = 1, 3, 4, 5, 1027) at steps 1, 2 and 1000, every
    (decoupled, amsgrad) pair, against the float64 formulas within one step's float32 rounding (bounds derived below), nothing written behind
    the n floats."""
    g_ = torch.Generator().manual_seed(100 * n + 2 * decoupled + amsgrad)
    pad = 8
    lr, beta1, beta2, eps, wd = 2e-4, 0.8, 0.999, 1e-6, 0.01
    for step in (1, 2, 1000):
        p = torch.randn(n + pad, generator=g_) * 0.3
        g = torch.randn(n + pad, generator=g_) * (10.0 ** float(torch.randint(-3, 2, (1,), generator=g_)))
        m = torch.randn(n + pad, generator=g_) * 0.1 if step > 1 else torch.zeros(n + pad)
        v = torch.rand(n + pad, generator=g_) * 0.01 if step > 1 else torch.zeros(n + pad)
        vmax = v * (1 + torch.rand(n + pad, generator=g_) * (torch.rand(n + pad, generator=g_) < 0.5)) if step > 1 else torch.zeros(n + pad)
        want = adam64(p[:n], g[:n], m[:n], v[:n], vmax[:n], lr, beta1, beta2, eps, wd, step, decoupled, amsgrad)
        before = [t.clone() for t in (p, m, v, vmax)]
        assert emul.jodo_adam_step(n, ptr(p), ptr(g), ptr(m), ptr(v), ptr(vmax) if amsgrad else NULL, lr, beta1, beta2, eps, wd, step, decoupled,
                                   amsgrad, NULL) == 0
        for got, b in zip((p, m, v, vmax), before):
            assert torch.equal(got[n:], b[n:])                                             # the tail loop stops at n
        # float32 rounding of one step, u = 2^-24 per operation, carried through the formulas.  Adam's g + wd p and m0 + w1 (g - m0) cancel, so
        # their errors scale with their inputs, not with their values: tol_g = 3 u (|g| + wd |p0|) (none for AdamW), tol_m = 4 u (|m0| + |g| +
        # wd |p0|).  v = beta2 v0 + w2 g g: six roundings of non-negative terms, plus tol_g through the square.  p = p0 - step_size m / d:
        # p0's roundings (the decay constant, its product, the final difference: 3, taken as 4), m's absolute error through 1 / d, the
        # quotient's own roundings (the root, bc2_sqrt, the division, eps, the sum, m / d, step_size, the product: 8, with v's six halved by
        # the root taken as 12), and v's cancellation error through |sqrt a - sqrt b| <= |a - b| / sqrt(max(a, b)).
        u = 2.0 ** -24
        p0, m0, g0 = before[0][:n].double(), before[1][:n].double(), g[:n].double()
        bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
        tol_g = torch.zeros(n, dtype=torch.float64) if decoupled else 3 * u * (g0.abs() + wd * p0.abs())
        g_eff = g0 if decoupled else g0 + wd * p0
        tol_m = 4 * u * (m0.abs() + g0.abs() + wd * p0.abs())
        tol_v = 6 * u * want[2] + (1 - beta2) * (2 * g_eff.abs() * tol_g + tol_g ** 2)
        vv = want[3] if amsgrad else want[2]
        d = vv.sqrt() / math.sqrt(bc2) + eps
        tol_d = tol_v / (vv.sqrt() + 1e-300) / math.sqrt(bc2)
        tol_p = 4 * u * p0.abs() + (lr / bc1) * ((tol_m + 12 * u * want[1].abs()) / d + want[1].abs() / d ** 2 * tol_d)
        checks = [('m', m, want[1], tol_m), ('p', p, want[0], tol_p), ('v', v, want[2], tol_v)] + ([('vmax', vmax, want[3], tol_v)] if amsgrad else [])
        for name, got, w, tol in checks:
            ratio = float(((got[:n].double() - w).abs() / (tol + 1e-300)).max())
            assert ratio <= 1.0, "%s at step %d: %.3f of its rounding bound" % (name, step, ratio)
        if not amsgrad:
            assert torch.equal(vmax, before[3])                                            # not touched without amsgrad


def test_adam_step_refuses_bad_arguments(emul):
    t = torch.zeros(8)
    assert emul.jodo_adam_step(0, ptr(t), ptr(t), ptr(t), ptr(t), NULL, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 0, NULL) != 0
    assert emul.jodo_adam_step(4, ptr(t), ptr(t), ptr(t), ptr(t), NULL, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 1, NULL) != 0      # amsgrad without vmax
    assert emul.jodo_adam_step(4, ptr(t), ptr(t), ptr(t), ptr(t), NULL, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, 0, NULL) != 0      # steps count from 1
    assert emul.jodo_adam_step(4, ctypes.c_void_p(t.data_ptr() + 4), ptr(t), ptr(t), ptr(t), NULL, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 0, NULL) != 0


def test_gradnorm_clip_follows_the_host_queue(emul):
    """jodo_gradnorm_clip over 130 norms with spikes (the ring of 50 wraps twice) against a float64 restatement of losses.py' host side:
    Queue (newest first, at most 50; numpy's population std), allowed = min(1.5 mean + 2 std, max_grad), coef = min(1, allowed /
    (norm + 1e-6)), min(norm, allowed) pushed."""
    from jodo_amd import losses as L
    g = torch.Generator().manual_seed(3)
    q = L.Queue(); q.add(3000)
    st = torch.zeros(52, dtype=torch.float64)
    st[0], st[50], st[51] = 3000.0, 1, 1
    coef, allowed_out = torch.full((1,), math.nan), torch.full((1,), math.nan)
    max_grad, clipped = 2000.0, 0
    for step in range(130):
        norm = float(torch.rand((), generator=g)) * 300.0 + 20.0
        if step in (20, 41, 42, 70, 111):
            norm *= 40.0
        if step < 3:
            norm *= 500.0
        nrm = torch.tensor([norm], dtype=torch.float32)
        norm = float(nrm)                                                                   # the float32 norm both sides see
        allowed = min(1.5 * q.mean() + 2 * q.std(), max_grad)
        want_coef = min(1.0, allowed / (norm + 1e-6))
        q.add(float(min(norm, allowed)))
        assert emul.jodo_gradnorm_clip(ptr(nrm), ptr(st), max_grad, ptr(coef), ptr(allowed_out), NULL) == 0
        assert abs(float(coef) - want_coef) <= 2e-7 * want_coef and abs(float(allowed_out) - allowed) <= 1e-7 * allowed
        clipped += int(float(coef) < 1.0)
        cnt, nxt = int(st[50]), int(st[51])
        assert cnt == len(q) and nxt == (step + 2) % 50
        np.testing.assert_allclose([float(st[(nxt - 1 - i) % 50]) for i in range(cnt)], q.items, rtol=1e-12)
    assert 5 <= clipped <= 60 and len(q) == 50

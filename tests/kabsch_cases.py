"""One batch of degenerate and near-degenerate molecules for the Kabsch rotation kernel (csrc/train_step.hip k_kabsch), and the checks
both of its users run on it: tests/test_optim_gpu.py on the device, tests/test_step_emul.py on the host build of the same source.

get_align_position(z_t, xh) rotates the data xh onto the noisy z_t:  A = z_t^T xh = U S V^T,  R = U diag(1, 1, sign det A) V^T,
aligned = R xh.  QM9 holds 1-, 2- and 3-atom molecules, linear and planar ones: xh then spans less than three dimensions and A has
rank 0, 1 or 2.  R is NOT unique there (any rotation about the normal of a planar xh's image, composed with a reflection through its
plane, serves as well: the kernel's R and the float64 SVD form's differ by up to 1.98 in an element, and the SVD form's own det R is
+-1 at random), but R xh is — xh has no component along the directions R is free in.  So the batch is judged by the aligned positions,
and by what the kernel promises about R itself: a proper rotation wherever det A != 0."""
import math

import torch

N_MAX = 12
PER_CASE = 16
TETRA = torch.tensor([[1., 1., 1.], [1., -1., -1.], [-1., 1., -1.], [-1., -1., 1.]])

# case -> what the float64 singular values s1 >= s2 >= s3 of A must show (the rank the case is meant to have)
PLANAR = ('planar_tilted', 'planar_xy', 'n3', 'square_rotated', 'planar_tilted_x1e-6', 'planar_tilted_x1e6')
LINEAR = ('collinear', 'collinear_axis', 'n2', 'collinear_x1e-6', 'collinear_x1e6')
FULL = ('tetra_exact', 'tetra_rotated', 'tetra_perturbed')
THICK = {'thick_1e-3': 1e-3, 'thick_1e-5': 1e-5, 'thick_1e-7': 1e-7}
OTHER = ('n1', 'n4', 'n4_x1e-6', 'n4_x1e6')
ALL_CASES = PLANAR + LINEAR + FULL + tuple(THICK) + OTHER


def _frame(g):
    """a random proper rotation (columns e1, e2, e3)"""
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def _centre(p, n):
    p = p.clone()
    p[n:] = 0
    p[:n] -= p[:n].mean(0, keepdim=True)
    return p


def _one(case, g):
    """(z_t, xh, n): float32 [N_MAX, 3] each, zero beyond the n real atoms, centred over them (as the loss centres positions)."""
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n = int(torch.randint(4, N_MAX + 1, (1,), generator=g))
    e = _frame(g)
    z = rnd(N_MAX, 3)                                                  # the noisy side: generic unless the case says otherwise
    scale = 1.0
    base = case
    for tag, s in (('_x1e-6', 1e-6), ('_x1e6', 1e6)):
        if case.endswith(tag):
            base, scale = case[:-len(tag)], s
    if base == 'planar_tilted':
        x = rnd(N_MAX, 1) * e[:, 0] + rnd(N_MAX, 1) * e[:, 1]
    elif base == 'planar_xy':
        x = torch.cat([rnd(N_MAX, 2), torch.zeros(N_MAX, 1, dtype=torch.float64)], 1)       # an exactly zero column of A, det A == 0
    elif base == 'collinear':
        n = int(torch.randint(3, N_MAX + 1, (1,), generator=g))
        x = rnd(N_MAX, 1) * e[:, 0]
    elif base == 'collinear_axis':
        x = torch.cat([rnd(N_MAX, 1), torch.zeros(N_MAX, 2, dtype=torch.float64)], 1)       # two zero columns
    elif base in ('n1', 'n2', 'n3', 'n4'):
        n = int(base[1])
        x = rnd(N_MAX, 3)                                              # n <= 3 points, centred: both sides span n - 1 dimensions
    elif base in THICK:
        x = rnd(N_MAX, 1) * e[:, 0] + rnd(N_MAX, 1) * e[:, 1] + THICK[base] * rnd(N_MAX, 1) * e[:, 2]
    elif base == 'square_rotated':                                     # x^T x = diag(2, 2, 0) in the plane: a repeated eigenvalue at rank two
        n = 4
        sq = torch.tensor([[1., 1.], [1., -1.], [-1., -1.], [-1., 1.]], dtype=torch.float64)
        x = torch.zeros(N_MAX, 3, dtype=torch.float64)
        x[:4] = sq[:, :1] * e[:, 0] + sq[:, 1:] * e[:, 1]
        z = x @ _frame(g).t() + 1e-3 * rnd(N_MAX, 3)
    elif base.startswith('tetra'):
        n = 4
        x = torch.zeros(N_MAX, 3, dtype=torch.float64)
        x[:4] = TETRA.double()                                         # x^T x = 4 I: A = 4 R0, a triple eigenvalue of A^T A
        if base == 'tetra_exact':
            z = x.clone()                                              # A^T A diagonal from the start: Jacobi leaves at once
        elif base == 'tetra_rotated':
            z = x @ _frame(g).t()
        else:
            x[:4] += 1e-3 * rnd(4, 3)
            z = x @ _frame(g).t() + 1e-3 * rnd(N_MAX, 3)
    else:
        raise KeyError(case)
    z, x = (z * scale).float(), (x * scale).float()
    return _centre(z, n), _centre(x, n), n


def build_batch(seed=17):
    """dict(z=[B, 12, 3], x=[B, 12, 3] float32, case=[B] names, n=[B]): PER_CASE molecules of every case in ALL_CASES."""
    g = torch.Generator().manual_seed(seed)
    zs, xs, names, ns = [], [], [], []
    for case in ALL_CASES:
        for _ in range(PER_CASE):
            z, x, n = _one(case, g)
            zs.append(z); xs.append(x); names.append(case); ns.append(n)
    return dict(z=torch.stack(zs), x=torch.stack(xs), case=names, n=ns)


def covariance(z, x):
    return torch.einsum('...ki,...kj->...ij', z, x)


def reference_aligned(batch):
    """The SVD form in float64 on the CPU (jodo_amd.losses.get_align_position; tests/test_losses_host.py ties it to the reference)."""
    from jodo_amd import losses as L
    return L.get_align_position(batch['z'].double(), batch['x'].double())


def assert_ranks(batch):
    """every case has the rank it is meant to have, by the float64 singular values of A"""
    s = torch.linalg.svdvals(covariance(batch['z'].double(), batch['x'].double()))
    assert sorted(set(batch['case'])) == sorted(ALL_CASES)
    for b, case in enumerate(batch['case']):
        s1, s2, s3 = (float(v) for v in s[b])
        if case == 'n1':
            assert s1 == 0.0
            continue
        if case in PLANAR or case in LINEAR:
            assert s3 / s1 < 1e-6, (case, s1, s2, s3)
        if case in LINEAR:
            assert s2 / s1 < 1e-6, (case, s1, s2, s3)
        if case in PLANAR:
            assert s2 / s1 > 1e-3, (case, s1, s2, s3)
        if case in FULL:
            assert s3 / s1 > 0.5, (case, s1, s2, s3)
        if case in THICK:
            assert s3 / s1 < 10 * THICK[case] and s2 / s1 > 1e-3, (case, s1, s2, s3)


def kernel_det(A32):
    """det A as k_kabsch forms it: in double from the float32 covariance, by the first row"""
    A = A32.double()
    return (A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1]) - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0])
            + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]))


def check_batch(batch, A32, R, aligned, want, report=None):
    """A32 [B, 3, 3]: the float32 covariance the kernel was given; R [B, 3, 3] float32: what it returned; aligned [B, 12, 3] float32 = R x;
    want: reference_aligned(batch).  Returns the worst aligned-position error per case in units of max(1, max |xh|)."""
    A32, R, aligned = A32.cpu(), R.cpu(), aligned.cpu()
    B = R.shape[0]
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(aligned).all())
    # 1. aligned positions: 2e-5 at unit scale (the bound of test_kabsch_rotations_match_the_svd_form), times the size of the molecule
    size = batch['x'].abs().amax((1, 2)).double()
    err = (aligned.double() - want).abs().amax((1, 2))
    unit = torch.clamp(size, min=1.0)
    worst = {}
    for b, case in enumerate(batch['case']):
        worst[case] = max(worst.get(case, 0.0), float(err[b] / unit[b]))
    if report is not None:
        report(worst)
    bad = [(batch['case'][b], float(err[b]), float(size[b])) for b in range(B) if not err[b] <= 2e-5 * unit[b]]
    assert not bad, "aligned positions differ from the float64 SVD form: %s" % bad[:8]
    # ... and relative to the molecule's own size where that is far below one: nothing in the kernel depends on the scale of A (its
    # thresholds are relative, exact zero, or 1e-150), so the unit-scale bound holds there as well
    small = [b for b in range(B) if batch['case'][b].endswith('_x1e-6')]
    bad = [(batch['case'][b], float(err[b]), float(size[b])) for b in small if not err[b] <= 2e-5 * size[b]]
    assert not bad, "aligned positions of the molecules scaled by 1e-6 differ: %s" % bad[:8]
    # 2. / 3. R itself: a proper rotation wherever det A != 0 (formed in double, rounded once to float32: about 2e-7); where A is all zero
    # or has an exactly zero column the third term is dropped like the reference's sign(0) — finite (above), judged by R x alone
    zero_col = (A32 == 0).all(1).any(1)
    det = kernel_det(A32)
    for case in ('planar_xy', 'collinear_axis', 'n1'):
        idx = [b for b in range(B) if batch['case'][b] == case]
        assert bool(zero_col[idx].all()) and bool((det[idx] == 0).all()), case
    # (what is left there is the reference's U diag(1, 1, 0) V^T, a partial isometry of rank two: R^T R is a projector of trace 2)
    G = R.double()[zero_col].transpose(1, 2) @ R.double()[zero_col]
    assert float((G @ G - G).abs().max()) <= 1e-6 and float((G.diagonal(dim1=1, dim2=2).sum(1) - 2).abs().max()) <= 1e-6
    proper = (det != 0) & ~zero_col
    assert int(proper.sum()) >= B - 3 * PER_CASE - 2                                       # (an exact zero among the noise-level determinants is possible, not likely)
    Rd = R.double()[proper]
    eye = torch.eye(3, dtype=torch.float64)
    orth = (Rd.transpose(1, 2) @ Rd - eye).abs().amax((1, 2))
    assert float(orth.max()) <= 1e-6, "R^T R - I: %.3e" % float(orth.max())
    dets = torch.det(Rd)
    assert float((dets - 1).abs().max()) <= 1e-6, "det R - 1: %.3e" % float((dets - 1).abs().max())
    return worst


def with_nan(batch, at):
    """the batch with one NaN coordinate in molecule `at` of the noisy side"""
    z = batch['z'].clone()
    z[at, 0, 1] = math.nan
    return z

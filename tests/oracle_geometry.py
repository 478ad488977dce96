"""A numpy restatement of the sub-structure geometry (jodo_amd/evaluation/geometry.py, csrc/geometry_kernels.hip): the enumeration with its
multiplicities, the three value formulas in a chosen precision, and the MMD in float64.  Written from the rules in DESIGN.md §4m, not
from the reference's code; tests/test_geometry_host.py holds it against the values the reference's own functions recorded
(tests/golden/geometry_cases.npz).
"""
import numpy as np

CODES = {1: 1, 2: 2, 3: 3, 4: 12}


def length(p, i, j, dt=np.float64):
    d = p[i].astype(dt) - p[j].astype(dt)
    return np.sqrt((d * d).sum(dtype=dt))


def angle(p, i, j, k, dt=np.float64):
    a, b = p[i].astype(dt) - p[j].astype(dt), p[k].astype(dt) - p[j].astype(dt)
    if not (a * a).sum() or not (b * b).sum():
        return dt(np.nan)
    c = np.cross(a, b).astype(dt)
    return dt(np.degrees(np.arctan2(np.sqrt((c * c).sum(dtype=dt)), (a * b).sum(dtype=dt))))


def dihedral(p, i, j, k, l, dt=np.float64):
    q = p.astype(dt)
    rij, rjk, rkl = q[j] - q[i], q[k] - q[j], q[l] - q[k]
    nijk, njkl = np.cross(rij, rjk).astype(dt), np.cross(rjk, rkl).astype(dt)
    m = np.cross(nijk, rjk).astype(dt)
    dot = lambda a, b: (a * b).sum(dtype=dt)
    with np.errstate(invalid='ignore', divide='ignore'):
        y = dot(m, njkl) / np.sqrt(dot(m, m) * dot(njkl, njkl))
        x = dot(nijk, njkl) / np.sqrt(dot(nijk, nijk) * dot(njkl, njkl))
    return dt(-np.degrees(np.arctan2(y, x)))


def _find(classes, fwd, rev):
    """(class, reversed?) of the forward tuple if it is listed, else of the reversed one, else None"""
    for t, r in ((fwd, False), (rev, True)):
        for c, row in enumerate(classes):
            if tuple(row) == tuple(t):
                return c, r
    return None


def extract(classes, pos, typ, edge, dt=np.float64):
    """classes: three int arrays [C,3], [C,6], [C,9] -> three lists (per class a list of values, non-finite ones left out) and the three
    numbers of values dropped, for one molecule (pos [n,3], typ [n], edge [n,n]: the upper triangle is read)."""
    n = len(typ)
    pos, typ, edge = np.asarray(pos), np.asarray(typ).astype(int), np.asarray(edge).astype(int)
    out = [[[] for _ in c] for c in classes]
    dropped = [0, 0, 0]
    code = lambda a, b: CODES.get(edge[min(a, b), max(a, b)], -1)
    nbr = [[b for b in range(n) if b != a and edge[min(a, b), max(a, b)]] for a in range(n)]

    def put(g, hit, fwd_value, rev_value):
        if hit is None:
            return
        v = rev_value() if hit[1] else fwd_value()
        if np.isfinite(v):
            out[g][hit[0]].append(float(v))
        else:
            dropped[g] += 1

    for i in range(n):
        for j in range(i + 1, n):
            if not edge[i, j]:
                continue
            cm = code(i, j)
            put(0, _find(classes[0], (typ[i], cm, typ[j]), (typ[j], cm, typ[i])), lambda: length(pos, i, j, dt), lambda: length(pos, j, i, dt))
            for k in nbr[j]:                                  # first bond: the one that ENDS at j; paired with every other bond at j
                if k == i:
                    continue
                c1 = code(j, k)
                put(1, _find(classes[1], (typ[i], cm, typ[j], typ[j], c1, typ[k]), (typ[k], c1, typ[j], typ[j], cm, typ[i])),
                    lambda: angle(pos, i, j, k, dt), lambda: angle(pos, k, j, i, dt))
            for d in nbr[j]:
                if d == i:
                    continue
                cr = code(j, d)
                for a in nbr[i]:
                    if a == j:
                        continue
                    cl = code(i, a)
                    put(2, _find(classes[2], (typ[a], cl, typ[i], typ[i], cm, typ[j], typ[j], cr, typ[d]),
                                 (typ[d], cr, typ[j], typ[j], cm, typ[i], typ[i], cl, typ[a])),
                        lambda: dihedral(pos, a, i, j, d, dt), lambda: dihedral(pos, d, j, i, a, dt))
    return out, dropped


def extract_many(classes, mols, dt=np.float64, keep=None):
    """molecules (dicts with n, pos, type, edge) -> three lists of per-class value arrays in molecule order, and the dropped counts"""
    out = [[[] for _ in c] for c in classes]
    dropped = [0, 0, 0]
    for b, m in enumerate(mols):
        if m['n'] == 0 or (keep is not None and not keep[b]):
            continue
        got, dr = extract(classes, m['pos'], m['type'], m['edge'], dt)
        for g in range(3):
            dropped[g] += dr[g]
            for c, v in enumerate(got[g]):
                out[g][c] += v
    return [[np.asarray(v, np.float64) for v in grp] for grp in out], dropped


def mmd(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """the multi-bandwidth Gaussian MMD in float64, diagonals included: all pairs of the concatenation, dense"""
    s, t = np.asarray(source, np.float64), np.asarray(target, np.float64)
    ns, nt = len(s), len(t)
    z = np.concatenate([s, t])
    n = ns + nt
    with np.errstate(invalid='ignore', divide='ignore'):
        if fix_sigma:
            bw = float(fix_sigma)
        else:
            bw = 2. * n * ((z - z.mean()) ** 2).sum() / (n * n - n) if n else np.nan
        bw /= kernel_mul ** (kernel_num // 2)
        total = [0., 0., 0.]
        for q, (a, b) in enumerate(((s, s), (t, t), (s, t))):
            for r0 in range(0, len(a), 1024):
                d2 = (a[r0:r0 + 1024, None] - b[None, :]) ** 2
                for i in range(kernel_num):
                    total[q] += np.exp(-d2 / (bw * kernel_mul ** i)).sum()
        return float(np.float64(total[0]) / (ns * ns) + np.float64(total[1]) / (nt * nt) - 2. * np.float64(total[2]) / (ns * nt))

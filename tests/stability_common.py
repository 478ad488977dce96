"""Shared by tests/test_stability_host.py and tests/test_stability_gpu.py: the recorded cases of tests/golden/stability_cases.npz
(tools/make_stability_golden.py) cut back into molecules, the rules file, and padded batches in the decode's layout."""
import os

import numpy as np

from helpers import GOLDEN, load_fixture
from jodo_amd.evaluation import StabilityRules

DATASETS = ('QM9', 'GeomDrug')
RULES_FILE = os.path.join(GOLDEN, 'stability_rules.json')
_cache = {}


def rules(name):
    if name not in _cache:
        _cache[name] = StabilityRules.from_file(RULES_FILE, name)
    return _cache[name]


def recorded(rule):
    """'3d' | 'bonds' -> list of dicts, one per recorded molecule: dataset, name, n, the rule's inputs (pos, type | type, fc, edge) and the
    reference's verdicts (stable_atoms, mol_stable, valence)."""
    key = 'cases_' + rule
    if key in _cache:
        return _cache[key]
    fx = load_fixture('stability_cases.npz')
    p = 'd3_' if rule == '3d' else 'b_'
    ns = fx[p + 'n'].astype(np.int64)
    a0 = np.concatenate([[0], np.cumsum(ns)])
    e0 = np.concatenate([[0], np.cumsum(ns * ns)])
    out = []
    for m, n in enumerate(ns):
        c = dict(dataset=DATASETS[int(fx[p + 'dataset'][m])], name=str(fx[p + 'name'][m]), n=int(n), type=fx[p + 'type'][a0[m]:a0[m + 1]],
                 stable_atoms=int(fx[p + 'stable_atoms'][m]), mol_stable=bool(fx[p + 'mol_stable'][m]), valence=fx[p + 'valence'][a0[m]:a0[m + 1]])
        if rule == '3d':
            c['pos'] = fx['d3_pos'][a0[m]:a0[m + 1]]
        else:
            c['fc'] = fx['b_fc'][a0[m]:a0[m + 1]]
            c['edge'] = fx['b_edge'][e0[m]:e0[m + 1]].reshape(n, n)
        out.append(c)
    _cache[key] = out
    return out


def pad_batch(mols, N=None, junk=None):
    """molecules (dicts with n, type and pos | fc, edge) -> pos f32 [B,N,3], at u8 [B,N], fc i8 [B,N], et u8 [B,N,N], n i32 [B]; the padding
    is what the decode leaves (zeros) or, with junk = a numpy Generator, random positions near the molecule, types, charges and bonds."""
    B = len(mols)
    N = N or max(max(m['n'] for m in mols), 1)
    if junk is None:
        pos, at = np.zeros((B, N, 3), np.float32), np.zeros((B, N), np.uint8)
        fc, et = np.zeros((B, N), np.int8), np.zeros((B, N, N), np.uint8)
    else:
        pos, at = junk.normal(0., 1.5, (B, N, 3)).astype(np.float32), junk.integers(0, 256, (B, N)).astype(np.uint8)
        fc, et = junk.integers(-2, 3, (B, N)).astype(np.int8), junk.integers(0, 5, (B, N, N)).astype(np.uint8)
    for b, m in enumerate(mols):
        n = m['n']
        at[b, :n] = m['type']
        pos[b, :n] = m.get('pos', np.zeros((n, 3), np.float32))
        fc[b, :n] = m.get('fc', np.zeros(n, np.int8))
        et[b, :n, :n] = m.get('edge', np.zeros((n, n), np.uint8))
    return pos, at, fc, et, np.array([m['n'] for m in mols], np.int32)


def clear_of_thresholds(r, pos, typ, margin_pm=0.01):
    """every pair's 100 d (float64 on the float32 coordinates) at least margin_pm from each of its thresholds, in either pair ordering:
    more than 10x the float32 rounding of a distance between coordinates below 10 A, so no summation order or fused multiply-add can
    flip an order between the oracle and the kernel"""
    n = len(typ)
    p = np.asarray(pos, np.float64)
    d = 100. * np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    a, b = np.broadcast_to(np.asarray(typ)[:, None], (n, n)), np.broadcast_to(np.asarray(typ)[None, :], (n, n))
    for first, second in ((a, b), (np.minimum(a, b), np.maximum(a, b))):
        t = r.thr[first, second].astype(np.float64)
        gap = np.abs(d[..., None] - t)
        gap[t == 0] = np.inf
        gap[np.eye(n, dtype=bool)] = np.inf
        if n > 1 and gap.min() < margin_pm:
            return False
    return True


def lattice_molecule(rng, r, n, spacing=1.25, jitter=0.22):
    """a seeded molecule for the 3-D rule: n atoms on distinct sites of a sparse cubic lattice, jittered, hydrogen-rich types over all of
    r's types; drawn again until it is clear of every threshold"""
    T = r.n_types
    p = np.full(T, 0.5 / max(T - 1, 1))
    p[0] = 0.5 if T > 1 else 1.
    side = max(2, int(np.ceil((2.2 * n) ** (1. / 3.))))
    while True:
        sites = rng.choice(side ** 3, size=n, replace=False)
        grid = np.stack([sites // (side * side), (sites // side) % side, sites % side], 1).astype(np.float64)
        pos = (spacing * grid + rng.uniform(-jitter, jitter, size=(n, 3))).astype(np.float32)
        pos -= pos.mean(0, keepdims=True).astype(np.float32)
        typ = rng.choice(T, size=n, p=p).astype(np.uint8)
        if np.abs(pos).max() < 10. and clear_of_thresholds(r, pos, typ):
            return dict(n=n, pos=pos, type=typ)


def bond_molecule(rng, r, n, symmetric=True):
    """a seeded molecule for the bond rule: about one bond per atom with orders 1-3 in the upper triangle, the lower triangle its mirror or
    unrelated entries; charges -1 .. +1"""
    up = np.zeros((n, n), dtype=np.int64)
    if n > 1:
        k = int(rng.integers(max(1, n // 2), max(2, int(1.3 * n))))
        i, j = rng.integers(0, n, size=k), rng.integers(0, n, size=k)
        keep = i != j
        up[np.minimum(i, j)[keep], np.maximum(i, j)[keep]] = rng.choice([1, 2, 3], size=int(keep.sum()), p=[0.72, 0.2, 0.08])
    low = up.T if symmetric else np.tril(rng.integers(0, 4, size=(n, n)) * (rng.random((n, n)) < 0.3), -1)
    return dict(n=n, type=rng.integers(0, r.n_types, size=n).astype(np.uint8), fc=rng.integers(-1, 2, size=n).astype(np.int8),
                edge=(up + low).astype(np.uint8))

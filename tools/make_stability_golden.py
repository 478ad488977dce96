"""Fixtures of the stability metrics: tests/golden/stability_rules.json and tests/golden/stability_cases.npz, recorded from the reference's
own check_stability / check_2D_stability on the CPU.

    python tools/make_stability_golden.py       (JODO_REFERENCE_ROOT names the reference checkout, see oracle/ref_import.py)

The reference's evaluation/stability.py and evaluation/bond_analyze.py are imported from their path at run time; nothing of them is kept
here, and the rule tables reach the rules file through StabilityRules.from_tables(...).to_file only.  RDKit is not needed: `rdkit`,
`rdkit.Chem`, `rdkit.Geometry` and `evaluation.rdkit_metric` are throw-away in-process stand-ins — a recording RWMol (AddBond / GetBonds)
and a Kekulize that does nothing, which is exact for molecules without aromatic bonds, the only ones generated.  Build machine only: no
test, smoke() or benchmark imports this file or reads the reference.

stability_cases.npz (ragged arrays, molecules concatenated; dataset 0 = QM9, 1 = GeomDrug):
  d3_dataset [M] u8, d3_n [M] i32, d3_pos [sum n, 3] f32, d3_type [sum n] u8           inputs of the 3-D rule
  d3_stable_atoms [M] i32, d3_mol_stable [M] bool                                       check_stability's verdicts
  d3_valence [sum n] i32                                                               per-atom sum of the orders it gave to AddBond
  b_dataset, b_n, b_type, b_fc [sum n] i8, b_edge [sum n^2] u8 (row-major n x n per molecule)   inputs of the bond rule
  b_stable_atoms, b_mol_stable, b_valence                                              check_2D_stability's verdicts, the same way
  d3_name [M], b_name [M]                                                              what a case is ('lattice', 'CH4', 'asym', ...)
Conditions asserted below (a molecule with a pair too close to a threshold is drawn again; nothing is left out): every pair's 100 d is at
least 0.01 pm from each of its thresholds; orders 0, 1, 2, 3 all occur; under each rule at least 10 % of the atoms are stable and at least
10 % unstable; at least 8 molecules are stable.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from jodo_amd.evaluation.rules import StabilityRules               # noqa: E402
from oracle.ref_import import REFERENCE_ROOT                         # noqa: E402
import oracle_stability as OS                                        # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DATASETS = ('QM9', 'GeomDrug')
MARGIN_PM = 0.01
LATTICE = 1.25


# ---- stand-ins for RDKit, alive for this process only -------------------------------------------------------------------------------------
class _BondType:
    def __init__(self, order):
        self.order = order

    def __deepcopy__(self, memo):                             # an enumeration member: the reference keys a dict with it after a deepcopy
        return self


class _Bond:
    def __init__(self, i, j, kind):
        self.i, self.j, self.kind = int(i), int(j), kind

    def GetBeginAtomIdx(self):
        return self.i

    def GetEndAtomIdx(self):
        return self.j

    def GetBondType(self):
        return self.kind


class _Atom:
    def __init__(self, symbol):
        self.symbol, self.charge = symbol, 0

    def GetSymbol(self):
        return self.symbol

    def SetFormalCharge(self, q):
        self.charge = q


class _RWMol:
    def __init__(self):
        self.atoms, self.bonds = [], []

    def AddAtom(self, a):
        self.atoms.append(a)

    def GetNumAtoms(self):
        return len(self.atoms)

    def GetAtomWithIdx(self, i):
        return self.atoms[i]

    def GetAtoms(self):
        return self.atoms

    def AddConformer(self, conf):
        pass

    def AddBond(self, i, j, kind):
        assert kind is not None
        self.bonds.append(_Bond(i, j, kind))

    def GetBonds(self):
        return self.bonds


class _Conformer:
    def __init__(self, n):
        pass

    def SetAtomPosition(self, i, p):
        pass


def _install_standins():
    rdkit, chem, geometry = types.ModuleType('rdkit'), types.ModuleType('rdkit.Chem'), types.ModuleType('rdkit.Geometry')
    bt = types.SimpleNamespace(SINGLE=_BondType(1), DOUBLE=_BondType(2), TRIPLE=_BondType(3), AROMATIC=_BondType(4))
    chem.rdchem = types.SimpleNamespace(BondType=bt)
    chem.RWMol, chem.Atom, chem.Conformer = _RWMol, _Atom, _Conformer
    chem.Kekulize = lambda mol: None
    geometry.Point3D = lambda x, y, z: (x, y, z)
    rdkit.Chem, rdkit.Geometry = chem, geometry
    metric = types.ModuleType('evaluation.rdkit_metric')
    metric.eval_rdmol = lambda *a, **k: {}
    package = types.ModuleType('evaluation')                  # the package without its __init__ (which imports the RDKit metrics)
    package.__path__ = [os.path.join(REFERENCE_ROOT, 'evaluation')]
    sys.modules.update({'rdkit': rdkit, 'rdkit.Chem': chem, 'rdkit.Geometry': geometry, 'evaluation': package,
                        'evaluation.rdkit_metric': metric})


def load_reference():
    if not os.path.isfile(os.path.join(REFERENCE_ROOT, 'evaluation', 'stability.py')):
        raise SystemExit("reference not present at %s" % REFERENCE_ROOT)
    _install_standins()
    stab = importlib.import_module('evaluation.stability')
    ba = importlib.import_module('evaluation.bond_analyze')
    spec = importlib.util.spec_from_file_location('_ref_datasets_config', os.path.join(REFERENCE_ROOT, 'datasets', 'datasets_config.py'))
    dc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dc)
    infos = {'QM9': dc.qm9_with_h, 'GeomDrug': dc.geom_with_h_1}
    assert all(infos[k]['name'] == k for k in DATASETS)
    return stab, ba, infos


def valence_of(mol, n):
    v = np.zeros(n, dtype=np.int32)
    for b in mol.GetBonds():
        v[b.i] += b.kind.order
        v[b.j] += b.kind.order
    return v


# ---- 3-D cases ------------------------------------------------------------------------------------------------------------------------------
def clear_of_thresholds(rules, pos, typ):
    """every pair's 100 d at least MARGIN_PM from each of its thresholds (float64 on the float32 coordinates)"""
    n = len(typ)
    d = 100. * np.sqrt(((pos[:, None].astype(np.float64) - pos[None].astype(np.float64)) ** 2).sum(-1))
    a, b = np.broadcast_to(typ[:, None], (n, n)), np.broadcast_to(typ[None, :], (n, n))
    for first, second in ((a, b), (np.minimum(a, b), np.maximum(a, b))):          # whichever ordering a rule uses
        t = rules.thr[first, second].astype(np.float64)
        gap = np.abs(d[..., None] - t)
        gap[t == 0] = np.inf
        gap[np.eye(n, dtype=bool)] = np.inf
        if gap.min() < MARGIN_PM:
            return False
    return True


def lattice_molecule(rng, rules, n, type_p):
    """n atoms on distinct sites of a sparse cubic lattice (spacing LATTICE), each coordinate jittered, seeded types"""
    side = max(2, int(np.ceil((2.2 * n) ** (1. / 3.))))
    while True:
        sites = rng.choice(side ** 3, size=n, replace=False)
        grid = np.stack([sites // (side * side), (sites // side) % side, sites % side], 1).astype(np.float64)
        pos = (LATTICE * grid + rng.uniform(-0.22, 0.22, size=(n, 3))).astype(np.float32)
        pos -= pos.mean(0, keepdims=True).astype(np.float32)
        typ = rng.choice(len(type_p), size=n, p=type_p).astype(np.int64)
        if np.abs(pos).max() < 10. and clear_of_thresholds(rules, pos, typ):
            return pos, typ


def hand_placed():
    """Small molecules at textbook geometries (Angstrom); element symbols, decoded per dataset by the caller."""
    t = 1.09 / np.sqrt(3.)
    ch3 = lambda x, s: [(x + s * 0.36, 1.03, 0.), (x + s * 0.36, -0.515, 0.892), (x + s * 0.36, -0.515, -0.892)]
    return [
        ('CH4', 'CHHHH', [(0, 0, 0), (t, t, t), (t, -t, -t), (-t, t, -t), (-t, -t, t)]),
        ('H2O', 'OHH', [(0, 0, 0), (0.96, 0, 0), (-0.24, 0.93, 0)]),
        ('NH3', 'NHHH', [(0, 0, 0), (0.94, 0, -0.37), (-0.47, 0.814, -0.37), (-0.47, -0.814, -0.37)]),
        ('HF', 'HF', [(0, 0, 0), (0.92, 0, 0)]),
        ('C2H6', 'CCHHHHHH', [(-0.77, 0, 0), (0.77, 0, 0)] + ch3(-0.77, -1.) + [(x, -y, z) for x, y, z in ch3(0.77, 1.)]),
        ('C2H4', 'CCHHHH', [(-0.67, 0, 0), (0.67, 0, 0), (-1.24, 0.93, 0), (-1.24, -0.93, 0), (1.24, 0.93, 0), (1.24, -0.93, 0)]),
        ('C2H2', 'HCCH', [(-1.66, 0, 0), (-0.60, 0, 0), (0.60, 0, 0), (1.66, 0, 0)]),
        ('HCN', 'HCN', [(-1.06, 0, 0), (0, 0, 0), (1.16, 0, 0)]),
        ('CO2', 'OCO', [(-1.20, 0, 0), (0, 0, 0), (1.20, 0, 0)]),
    ]


def symbols(formula):
    return [c for c in formula]


def cases_3d(stab, infos, rules):
    rng = np.random.default_rng(20240611)
    out = []
    # seeded types: hydrogen-rich like the data, every type present
    p_qm9 = np.array([0.50, 0.30, 0.07, 0.09, 0.04])
    p_geom = np.full(16, 0.25 / 14.)
    p_geom[0], p_geom[2] = 0.45, 0.30
    p_geom /= p_geom.sum()
    sizes_qm9 = [1 + (k % 29) for k in range(250)]
    sizes_geom = [2, 3, 5, 9, 17, 30, 31, 32, 33, 47, 63, 64, 65, 66, 80, 96, 97, 110, 127, 128, 129, 140, 150, 160, 170, 175, 179, 180, 181, 181]
    for name, sizes, p in (('QM9', sizes_qm9, p_qm9), ('GeomDrug', sizes_geom, p_geom)):
        for n in sizes:
            pos, typ = lattice_molecule(rng, rules[name], n, p)
            out.append((name, 'lattice', pos, typ))
    for name in DATASETS:
        dec = infos[name]['atom_decoder']
        for tag, formula, xyz in hand_placed():
            pos, typ = np.asarray(xyz, dtype=np.float32), np.array([dec.index(s) for s in symbols(formula)], dtype=np.int64)
            assert clear_of_thresholds(rules[name], pos, typ), tag
            out.append((name, tag, pos, typ))
    dec = infos['GeomDrug']['atom_decoder']                   # the ordered lookup: C before S and S before C by atom index
    for tag, pair in (('C,S', 'CS'), ('S,C', 'SC')):
        pos, typ = np.array([(0, 0, 0), (1.55, 0, 0)], dtype=np.float32), np.array([dec.index(s) for s in pair], dtype=np.int64)
        assert clear_of_thresholds(rules['GeomDrug'], pos, typ)
        out.append(('GeomDrug', tag, pos, typ))
    rec = dict(dataset=[], n=[], pos=[], type=[], stable_atoms=[], mol_stable=[], valence=[], name=[])
    for name, tag, pos, typ in out:
        mol_stable, stable_atoms, n, mol = stab.check_stability(pos, typ, infos[name])
        assert n == len(typ)
        val = valence_of(mol, n)
        mine = OS.stability_3d(rules[name], pos, typ)         # the oracle agrees before anything is written
        assert mine['stable_atoms'] == stable_atoms and np.array_equal(mine['valence'], val), (name, tag, n)
        if tag in ('C,S', 'S,C'):
            assert val.tolist() == [2, 2], val
        elif tag != 'lattice':
            assert mol_stable, "%s should be stable under the %s rule" % (tag, name)
        rec['dataset'].append(DATASETS.index(name)); rec['n'].append(n); rec['pos'].append(pos); rec['type'].append(typ)
        rec['stable_atoms'].append(int(stable_atoms)); rec['mol_stable'].append(bool(mol_stable)); rec['valence'].append(val)
        rec['name'].append(tag)
    return rec


# ---- bond-rule cases ------------------------------------------------------------------------------------------------------------------------
def random_bonds(rng, n, symmetric):
    """upper triangle: about one bond per atom, orders 1-3; the lower triangle mirrors it or holds unrelated entries"""
    up = np.zeros((n, n), dtype=np.int64)
    if n > 1:
        k = rng.integers(max(1, n // 2), max(2, int(1.3 * n)))
        i, j = rng.integers(0, n, size=k), rng.integers(0, n, size=k)
        keep = i != j
        up[np.minimum(i, j)[keep], np.maximum(i, j)[keep]] = rng.choice([1, 2, 3], size=int(keep.sum()), p=[0.72, 0.2, 0.08])
    if symmetric:
        return up + up.T
    low = np.tril(rng.integers(0, 4, size=(n, n)) * (rng.random((n, n)) < 0.3), -1)
    return up + low


def cases_bonds(stab, infos, rules):
    rng = np.random.default_rng(20240612)
    p_qm9 = np.array([0.50, 0.30, 0.07, 0.09, 0.04])
    p_geom = np.full(16, 0.25 / 14.)
    p_geom[0], p_geom[2] = 0.45, 0.30
    p_geom /= p_geom.sum()
    plan = [('QM9', 1 + (k % 29), k % 3 != 2, p_qm9) for k in range(150)]
    plan += [('GeomDrug', n, k % 2 == 0, p_geom) for k, n in enumerate([2, 3, 7, 16, 29, 31, 32, 33, 40, 48, 56, 63, 64, 65, 70, 72, 76, 80, 90, 100])]
    drawn = []
    for name, n, symmetric, p in plan:
        typ = rng.choice(len(p), size=n, p=p).astype(np.int64)
        fc = rng.choice([-1, 0, 1], size=n, p=[0.15, 0.7, 0.15]).astype(np.int64)     # charges an element lists and charges that fall back
        drawn.append((name, 'symmetric' if symmetric else 'asym', typ, fc, random_bonds(rng, n, symmetric)))
    for name in DATASETS:                                     # the hand-placed molecules with the bonds the 3-D rule gives them, uncharged
        dec = infos[name]['atom_decoder']
        for tag, formula, xyz in hand_placed():
            typ = np.array([dec.index(s) for s in symbols(formula)], dtype=np.int64)
            drawn.append((name, tag, typ, np.zeros(len(typ), np.int64), OS.orders_3d(rules[name], np.asarray(xyz, np.float32), typ)))
    rec = dict(dataset=[], n=[], type=[], fc=[], edge=[], stable_atoms=[], mol_stable=[], valence=[], name=[])
    for name, tag, typ, fc, et in drawn:
        n = len(typ)
        mol_stable, stable_atoms, n_, mol = stab.check_2D_stability(None, torch.from_numpy(typ), torch.from_numpy(fc),
                                                                    torch.from_numpy(et).float(), infos[name])
        assert n_ == n
        val = valence_of(mol, n)
        mine = OS.stability_bonds(rules[name], typ, fc, et)
        assert mine['stable_atoms'] == stable_atoms and np.array_equal(mine['valence'], val) and mine['needs_kekulize'] == 0, (name, n)
        rec['dataset'].append(DATASETS.index(name)); rec['n'].append(n); rec['type'].append(typ); rec['fc'].append(fc)
        rec['edge'].append(et.reshape(-1)); rec['stable_atoms'].append(int(stable_atoms)); rec['mol_stable'].append(bool(mol_stable))
        rec['valence'].append(val); rec['name'].append(tag)
        assert mol_stable or tag in ('symmetric', 'asym'), "%s should be stable under the %s bond rule" % (tag, name)
    return rec


def check_coverage(what, rec, orders):
    atoms, stable = int(np.sum(rec['n'])), int(np.sum(rec['stable_atoms']))
    assert 0.1 * atoms <= stable <= 0.9 * atoms, "%s: %d of %d atoms stable" % (what, stable, atoms)
    assert int(np.sum(rec['mol_stable'])) >= 8, "%s: %d stable molecules" % (what, int(np.sum(rec['mol_stable'])))
    assert set(orders) >= {0, 1, 2, 3}, "%s: orders %s" % (what, sorted(set(orders)))
    print("%s: %d molecules, %d atoms, %d stable atoms (%.1f %%), %d stable molecules" % (
        what, len(rec['n']), atoms, stable, 100. * stable / atoms, int(np.sum(rec['mol_stable']))))


def main():
    stab, ba, infos = load_reference()
    rules = {name: StabilityRules.from_tables(infos[name]['atom_decoder'], name, ba.bonds1, ba.bonds2, ba.bonds3,
                                              (ba.margin1, ba.margin2, ba.margin3), ba.allowed_bonds, ba.allowed_fc_bonds)
             for name in DATASETS}
    os.makedirs(GOLDEN, exist_ok=True)
    rules_path = os.path.join(GOLDEN, 'stability_rules.json')
    rules['QM9'].to_file(rules_path, also=(rules['GeomDrug'],))
    rules = {name: StabilityRules.from_file(rules_path, name) for name in DATASETS}      # what the tests will load
    d3, bd = cases_3d(stab, infos, rules), cases_bonds(stab, infos, rules)
    seen = set()
    for k, (pos, typ) in enumerate(zip(d3['pos'], d3['type'])):
        seen |= set(np.unique(OS.orders_3d(rules[DATASETS[d3['dataset'][k]]], pos, typ)).tolist())
    check_coverage('3-D rule', d3, seen)
    check_coverage('bond rule', bd, set(np.unique(np.concatenate(bd['edge'])).tolist()))
    cat = lambda xs, dt: np.concatenate([np.asarray(x) for x in xs]).astype(dt)
    cases_path = os.path.join(GOLDEN, 'stability_cases.npz')
    np.savez_compressed(
        cases_path,
        d3_dataset=np.asarray(d3['dataset'], np.uint8), d3_n=np.asarray(d3['n'], np.int32), d3_pos=cat(d3['pos'], np.float32),
        d3_type=cat(d3['type'], np.uint8), d3_stable_atoms=np.asarray(d3['stable_atoms'], np.int32),
        d3_mol_stable=np.asarray(d3['mol_stable'], bool), d3_valence=cat(d3['valence'], np.int32), d3_name=np.asarray(d3['name']),
        b_dataset=np.asarray(bd['dataset'], np.uint8), b_n=np.asarray(bd['n'], np.int32), b_type=cat(bd['type'], np.uint8),
        b_fc=cat(bd['fc'], np.int8), b_edge=cat(bd['edge'], np.uint8), b_stable_atoms=np.asarray(bd['stable_atoms'], np.int32),
        b_mol_stable=np.asarray(bd['mol_stable'], bool), b_valence=cat(bd['valence'], np.int32), b_name=np.asarray(bd['name']))
    size = os.path.getsize(rules_path) + os.path.getsize(cases_path)
    assert size < 300 * 1024, size
    print("wrote %s and %s (%d bytes together)" % (rules_path, cases_path, size))


if __name__ == '__main__':
    main()

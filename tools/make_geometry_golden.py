"""Fixtures of the sub-structure geometry metric: tests/golden/geometry_cases.npz, recorded from the reference's own cal_bond_distance,
cal_bond_angle, cal_dihedral_angle, compute_geo_mmd (evaluation/cal_geometry.py) and compute_mmd (evaluation/mmd.py) on the CPU.

    python tools/make_geometry_golden.py        (JODO_REFERENCE_ROOT names the reference checkout, see oracle/ref_import.py)

The reference's modules are imported from their path at run time, without the package's __init__ (which imports the RDKit metrics);
nothing of them is kept here.  RDKit is not needed: `rdkit`, `rdkit.Chem`, `rdkit.Geometry`, `rdkit.Chem.rdMolTransforms` and
`evaluation.rdkit_metric` are throw-away in-process stand-ins — a recording RWMol / Atom / Bond / Conformer (bonds in the order they
were added; an atom's bonds in that order too) and GetBondLength / GetAngleDeg / GetDihedralDeg as the closed formulas of DESIGN.md
§4m in float64.  The molecules are built by the reference's check_2D_stability.  So parity with the reference's PYTHON (which bonds, in
which roles, how often, under which symbol; the MMD) is pinned; parity with the real RDKit's three accessors is NOT pinned: RDKit is
not on the build machine.  Build machine only: no test, smoke() or benchmark imports this file or reads the reference.

geometry_cases.npz (data only; dataset 0 = QM9, 1 = GeomDrug):
  m_dataset [M] u8, m_n [M] i32, m_name [M], m_pos [sum n, 3] f32, m_type [sum n] u8, m_edge [sum n^2] u8     the molecules
  m_counts [M, 24] i32, m_values [sum counts] f64      per molecule and symbol (the dataset's bond, angle, dihedral lists in order) the
                                                       values the reference's functions return for [that molecule]
  sym_<d> [24]                                         the symbols of dataset d in that order
  mmd_ns, mmd_nt [K] i32, mmd_family [K], mmd_x [sum ns + nt] f32 (source then target per case)    the MMD cases
  mmd_ref64, mmd_ref32 [K] f64                         compute_mmd on float64 and on float32 tensors of those samples (kernel_mul 2)
  mmd3_case [J] i32, mmd3_ref64 [J] f64                the same with kernel_mul = 3 on some of the cases
  e2e_<d>_ref32, e2e_<d>_ref64 [27] f64                compute_geo_mmd's three dicts (24 symbols and the three means, in the order of the
                                                       returned dict) for generated = the dataset's even-numbered molecules, target = the
                                                       values of its odd-numbered ones; float32 as the reference runs, and float64
Conditions asserted below (a molecule that misses one is drawn again): no recorded angle within 1 degree of 0 or 180, no recorded
dihedral within 1 degree of +-180, no two atoms closer than 0.3 A; every symbol is hit at least 3 times by the even-numbered and by the
odd-numbered molecules of its dataset; the named special molecules are present.
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
from oracle.ref_import import REFERENCE_ROOT                         # noqa: E402
import oracle_geometry as OG                                         # noqa: E402
from jodo_amd.evaluation import GeometrySymbols                      # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DATASETS = ('QM9', 'GeomDrug')
GROUP_KEYS = ('top_bond_sym', 'top_angle_sym', 'top_dihedral_sym')
MEANS = ('bond_length_mean', 'bond_angle_mean', 'dihedral_angle_mean')


# ---- stand-ins for RDKit, alive for this process only -------------------------------------------------------------------------------------
class _BondType:
    def __init__(self, code):
        self.code = code

    def __int__(self):
        return self.code


class _Atom:
    def __init__(self, symbol):
        self.symbol, self.bonds = symbol, []

    def GetSymbol(self):
        return self.symbol

    def GetBonds(self):
        return self.bonds

    def SetFormalCharge(self, q):
        pass


class _Bond:
    def __init__(self, mol, idx, i, j, kind):
        self.mol, self.idx, self.i, self.j, self.kind = mol, idx, int(i), int(j), kind

    def GetIdx(self):
        return self.idx

    def GetBeginAtomIdx(self):
        return self.i

    def GetEndAtomIdx(self):
        return self.j

    def GetBeginAtom(self):
        return self.mol.atoms[self.i]

    def GetEndAtom(self):
        return self.mol.atoms[self.j]

    def GetBondType(self):
        return self.kind


class _Conformer:
    def __init__(self, n):
        self.p = np.zeros((n, 3), np.float64)

    def SetAtomPosition(self, i, p):
        self.p[i] = p


class _RWMol:
    def __init__(self):
        self.atoms, self.bonds, self.conf = [], [], None

    def AddAtom(self, a):
        self.atoms.append(a)

    def GetNumAtoms(self):
        return len(self.atoms)

    def GetAtomWithIdx(self, i):
        return self.atoms[i]

    def GetAtoms(self):
        return self.atoms

    def AddConformer(self, conf):
        self.conf = conf

    def GetConformer(self):
        return self.conf

    def AddBond(self, i, j, kind):
        assert kind is not None and i < j
        b = _Bond(self, len(self.bonds), i, j, kind)
        self.bonds.append(b)
        self.atoms[i].bonds.append(b)
        self.atoms[j].bonds.append(b)

    def GetBonds(self):
        return self.bonds


def _install_standins():
    rdkit, chem, geometry = types.ModuleType('rdkit'), types.ModuleType('rdkit.Chem'), types.ModuleType('rdkit.Geometry')
    transforms = types.ModuleType('rdkit.Chem.rdMolTransforms')
    bt = types.SimpleNamespace(SINGLE=_BondType(1), DOUBLE=_BondType(2), TRIPLE=_BondType(3), AROMATIC=_BondType(12))
    chem.rdchem = types.SimpleNamespace(BondType=bt)
    chem.RWMol, chem.Atom, chem.Conformer = _RWMol, _Atom, _Conformer
    chem.Kekulize = lambda mol: None
    chem.rdMolTransforms = transforms
    geometry.Point3D = lambda x, y, z: (x, y, z)
    transforms.GetBondLength = lambda conf, i, j: float(OG.length(conf.p, i, j))
    transforms.GetAngleDeg = lambda conf, i, j, k: float(OG.angle(conf.p, i, j, k))
    transforms.GetDihedralDeg = lambda conf, i, j, k, l: float(OG.dihedral(conf.p, i, j, k, l))
    rdkit.Chem, rdkit.Geometry, rdkit.RDLogger = chem, geometry, types.SimpleNamespace()
    metric = types.ModuleType('evaluation.rdkit_metric')
    metric.eval_rdmol = lambda *a, **k: {}
    package = types.ModuleType('evaluation')                  # the package without its __init__
    package.__path__ = [os.path.join(REFERENCE_ROOT, 'evaluation')]
    sys.modules.update({'rdkit': rdkit, 'rdkit.Chem': chem, 'rdkit.Geometry': geometry, 'rdkit.Chem.rdMolTransforms': transforms,
                        'evaluation': package, 'evaluation.rdkit_metric': metric})
    if importlib.util.find_spec('tqdm') is None:
        sys.modules['tqdm'] = types.SimpleNamespace(tqdm=lambda x, *a, **k: x)


def load_reference():
    if not os.path.isfile(os.path.join(REFERENCE_ROOT, 'evaluation', 'cal_geometry.py')):
        raise SystemExit("reference not present at %s" % REFERENCE_ROOT)
    _install_standins()
    geo = importlib.import_module('evaluation.cal_geometry')
    mmd = importlib.import_module('evaluation.mmd')
    stab = importlib.import_module('evaluation.stability')
    spec = importlib.util.spec_from_file_location('_ref_datasets_config', os.path.join(REFERENCE_ROOT, 'datasets', 'datasets_config.py'))
    dc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dc)
    infos = {'QM9': dc.qm9_with_h, 'GeomDrug': dc.geom_with_h_1}
    assert all(infos[k]['name'] == k for k in DATASETS)
    return geo, mmd, stab, infos


def build_mol(stab, info, m):
    """the reference's own construction; a dataset name it has no stability rule for makes it return right after the bonds"""
    n = m['n']
    _, _, _, mol = stab.check_2D_stability(torch.from_numpy(m['pos'].astype(np.float32)), torch.from_numpy(m['type'].astype(np.int64)),
                                           torch.zeros(n, 0), torch.from_numpy(m['edge'].astype(np.int64)),
                                           {'name': 'fixture', 'atom_decoder': info['atom_decoder']})
    return mol


# ---- molecules ------------------------------------------------------------------------------------------------------------------------------
def place(rng, n):
    """n points, no two closer than 0.3 A, at a density near one atom per 3.4 cubic Angstrom"""
    side = max(1.5, (3.4 * n) ** (1. / 3.))
    while True:
        p = rng.uniform(-side / 2, side / 2, size=(n, 3)).astype(np.float32)
        if n < 2:
            return p
        d = np.sqrt(((p[:, None].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1)) + 10. * np.eye(n)
        if d.min() >= 0.3:
            return p


def random_molecule(rng, n, type_p, code_p, extra=0.25, symmetric=True):
    """a connected seeded graph: every atom bonded to an earlier one (the nearest few preferred), some further bonds; edge_type 1-4"""
    pos = place(rng, n)
    typ = rng.choice(len(type_p), size=n, p=type_p).astype(np.uint8)
    up = np.zeros((n, n), np.uint8)
    draw = lambda: rng.choice([1, 2, 3, 4], p=code_p)
    for a in range(1, n):
        b = int(rng.integers(0, a))
        up[b, a] = draw()
    for _ in range(int(extra * n)):
        a, b = sorted(rng.integers(0, n, size=2).tolist())
        if a != b:
            up[a, b] = draw()
    low = up.T if symmetric else np.tril((rng.integers(0, 5, size=(n, n)) * (rng.random((n, n)) < 0.3)).astype(np.uint8), -1)
    return dict(n=n, pos=pos, type=typ, edge=(up + low).astype(np.uint8))


def hand(dec, name, formula, bonds, rng):
    """a named molecule: element symbols and (i, j, edge_type) bonds, seeded positions"""
    n = len(formula)
    up = np.zeros((n, n), np.uint8)
    for i, j, o in bonds:
        up[min(i, j), max(i, j)] = o
    return dict(n=n, pos=place(rng, n), type=np.array([dec.index(s) for s in formula], np.uint8), edge=(up + up.T).astype(np.uint8), name=name)


def specials(dec, rng):
    C, H, N, O = 'C', 'H', 'N', 'O'
    ring3 = [C, C, C, H, H, H]
    ring4 = [C, C, C, C, H, H]
    hub = [C] + [H, C, H, C, H, C, H]
    return [
        hand(dec, '3-ring', ring3, [(0, 1, 1), (1, 2, 1), (0, 2, 1), (0, 3, 1), (1, 4, 1), (2, 5, 1)], rng),
        hand(dec, '4-ring', ring4, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 3, 1), (0, 4, 1), (2, 5, 1)], rng),
        hand(dec, 'degree-7', hub, [(0, k, 1) for k in range(1, 8)] + [(2, 4, 1)], rng),
        hand(dec, 'aromatic', [C, C, C, N, H, H], [(0, 1, 4), (1, 2, 4), (2, 3, 4), (0, 4, 1), (1, 5, 1)], rng),
        hand(dec, '1-atom', [C], [], rng),
        hand(dec, '2-atom', [C, H], [(0, 1, 1)], rng),
        dict(n=0, pos=np.zeros((0, 3), np.float32), type=np.zeros(0, np.uint8), edge=np.zeros((0, 0), np.uint8), name='empty'),
        hand(dec, 'angle-twice', [H, C, C], [(0, 2, 1), (1, 2, 1)], rng),          # both arms below the centre: recorded twice
        hand(dec, 'angle-never', [C, H, C], [(0, 1, 1), (0, 2, 1)], rng),          # both arms above the centre: never recorded
        hand(dec, 'O-C-N', [O, C, N, C, H], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (0, 4, 1)], rng),
    ]


def well_posed(classes, m):
    """the value conditions of the module docstring, on what the oracle records for m in float64"""
    if m['n'] == 0:
        return True
    got, dropped = OG.extract(classes, m['pos'], m['type'], m['edge'])
    if any(dropped):
        return False
    ang = np.asarray([v for c in got[1] for v in c])
    dih = np.asarray([v for c in got[2] for v in c])
    return (not len(ang) or (ang.min() > 1. and ang.max() < 179.)) and (not len(dih) or np.abs(dih).max() < 179.)


def molecules(name, info, classes):
    rng = np.random.default_rng(20240901 + DATASETS.index(name))
    T = len(info['atom_decoder'])
    p = np.full(T, 0.08 / max(T - 4, 1))
    for s, w in (('H', 0.40), ('C', 0.36), ('N', 0.09), ('O', 0.07)):
        p[info['atom_decoder'].index(s)] = w
    p /= p.sum()
    codes = [0.84, 0.12, 0.04, 0.] if name == 'QM9' else [0.55, 0.08, 0.02, 0.35]
    sizes = [9, 9, 5, 12, 17, 23, 29, 29, 3, 8, 20, 26] if name == 'QM9' else [9, 29, 33, 33, 40, 64, 65, 65, 20, 50]
    plan = [(n, k != 3) for k, n in enumerate(sizes)]
    out = []

    def add(make, tag):
        while True:
            m = make()
            if well_posed(classes, m):
                m.setdefault('name', tag)
                out.append(m)
                return

    for sp in specials(info['atom_decoder'], rng):
        add(lambda: sp if well_posed(classes, sp) else dict(sp, pos=place(rng, sp['n'])), sp['name'])
    for n, symmetric in plan:
        add(lambda: random_molecule(rng, n, p, codes, symmetric=symmetric), 'random' if symmetric else 'random-asym')
    while True:                                               # until both halves hit every symbol three times
        halves = [np.zeros(sum(len(c) for c in classes), np.int64) for _ in range(2)]
        for k, m in enumerate(out):
            got, _ = OG.extract(classes, m['pos'], m['type'], m['edge']) if m['n'] else ([[[]] * len(c) for c in classes], None)
            halves[k % 2] += np.asarray([len(v) for g in got for v in g])
        if min(h.min() for h in halves) >= 3:
            return out
        assert len(out) < 200, (name, halves)
        add(lambda: random_molecule(rng, int(rng.integers(14, 30)), p, codes, extra=0.4), 'random')


# ---- MMD cases ----------------------------------------------------------------------------------------------------------------------------------
def family(rng, kind, n, shift):
    if kind == 'length':
        return (1.10 + shift * 0.01 + 0.03 * rng.standard_normal(n)).astype(np.float32)
    if kind == 'angle':
        return (110. + shift * 2. + 5. * rng.standard_normal(n)).astype(np.float32)
    side = rng.random(n) < 0.5 + 0.1 * shift                  # dihedral: two modes
    return np.where(side, -60. + 12. * rng.standard_normal(n), 175. - 15. * rng.random(n)).astype(np.float32)


def mmd_cases(ref_mmd):
    rng = np.random.default_rng(20240903)
    rec = dict(ns=[], nt=[], family=[], x=[], ref64=[], ref32=[], case3=[], ref3=[])
    sizes = [(1, 1), (63, 257), (256, 256), (1000, 1500), (5000, 3000), (0, 40)]
    for ns, nt in sizes:
        for kind in ('length', 'angle', 'dihedral'):
            s, t = family(rng, kind, ns, 0.), family(rng, kind, nt, 1.)
            r64 = ref_mmd.compute_mmd(torch.from_numpy(s.astype(np.float64)), torch.from_numpy(t.astype(np.float64)), batch_size=1000)
            r32 = ref_mmd.compute_mmd(torch.from_numpy(s), torch.from_numpy(t), batch_size=1000)
            mine = OG.mmd(s, t)
            assert (np.isnan(r64) and np.isnan(mine)) or abs(mine - r64) < 1e-12, (ns, nt, kind, mine, r64)
            assert np.isnan(r64) == (ns == 0)
            if (ns, nt) in ((63, 257), (1000, 1500)):
                rec['case3'].append(len(rec['ns']))
                rec['ref3'].append(ref_mmd.compute_mmd(torch.from_numpy(s.astype(np.float64)), torch.from_numpy(t.astype(np.float64)),
                                                       batch_size=1000, kernel_mul=3.0))
                assert abs(OG.mmd(s, t, kernel_mul=3.0) - rec['ref3'][-1]) < 1e-12
            rec['ns'].append(ns); rec['nt'].append(nt); rec['family'].append(kind); rec['x'] += [s, t]
            rec['ref64'].append(float(r64)); rec['ref32'].append(float(r32))
            print("mmd %-8s (%4d, %4d): float64 %.9f  float32 - float64 %+.2e" % (kind, ns, nt, r64, r32 - r64))
    return rec


def write_npz(path, **arrays):
    """np.savez_compressed with a fixed time stamp on every member, so that the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    geo, ref_mmd, stab, infos = load_reference()
    cal = (geo.cal_bond_distance, geo.cal_bond_angle, geo.cal_dihedral_angle)
    save = {}
    M = dict(dataset=[], n=[], name=[], pos=[], type=[], edge=[], counts=[], values=[])
    for d, name in enumerate(DATASETS):
        info = infos[name]
        sy = GeometrySymbols.from_dataset_info(info)
        assert [len(s) for s in sy.syms] == [8, 8, 8] and sy.syms == [list(info[k]) for k in GROUP_KEYS]
        mols = molecules(name, info, sy.classes)
        rdmols = [build_mol(stab, info, m) for m in mols]
        whole = [fn(rdmols, info[k]) for fn, k in zip(cal, GROUP_KEYS)]
        per_sym = {s: [] for s in sy.all_syms}
        for m, rd in zip(mols, rdmols):
            one = {}
            for fn, k in zip(cal, GROUP_KEYS):
                one.update(fn([rd], info[k]))
            mine, dropped = OG.extract(sy.classes, m['pos'], m['type'], m['edge']) if m['n'] else ([[[]] * 8] * 3, [0, 0, 0])
            flat = [v for g in mine for v in g]
            for s, v in zip(sy.all_syms, flat):               # the oracle agrees before anything is written: same values, same order
                assert len(v) == len(one[s]) and np.allclose(v, one[s], rtol=0, atol=1e-9), (name, m['name'], s)
                per_sym[s] += one[s]
            M['dataset'].append(d); M['n'].append(m['n']); M['name'].append(m['name']); M['pos'].append(m['pos'].reshape(-1, 3))
            M['type'].append(m['type']); M['edge'].append(m['edge'].reshape(-1))
            M['counts'].append([len(one[s]) for s in sy.all_syms]); M['values'] += [np.asarray(one[s], np.float64) for s in sy.all_syms]
        for grp in whole:                                     # a list of molecules gives the molecules' lists, concatenated
            for s, v in grp.items():
                assert v == per_sym[s], (name, s)
        names = [m['name'] for m in mols]
        for tag in ('3-ring', '4-ring', 'degree-7', 'aromatic', '1-atom', '2-atom', 'empty', 'angle-twice', 'angle-never'):
            assert tag in names, tag
        if name == 'QM9':
            k = names.index('angle-twice')
            assert M['counts'][-len(mols) + k][8 + sy.syms[1].index('C1C-C1H')] == 2
            assert sum(M['counts'][-len(mols) + names.index('angle-never')][8:16]) == 0
        # end to end: generated = even-numbered molecules, target = the values of the odd-numbered ones
        gen, tar_mols = rdmols[0::2], rdmols[1::2]
        tar = {}
        for fn, k in zip(cal, GROUP_KEYS):
            tar.update(fn(tar_mols, info[k]))
        assert all(3 <= len(v) <= 20000 for v in tar.values())
        ref32, ref64 = [], []
        for fn, k, mean in zip(cal, GROUP_KEYS, MEANS):
            res = geo.compute_geo_mmd(gen, tar, fn, info[k], mean_name=mean)
            assert list(res) == list(info[k]) + [mean]
            ref32 += [float(v) for v in res.values()]
            vals = fn(gen, info[k])
            r64 = [ref_mmd.compute_mmd(torch.tensor(vals[s], dtype=torch.float64), torch.tensor(tar[s], dtype=torch.float64), batch_size=10000)
                   for s in info[k]]
            ref64 += r64 + [float(np.nanmean(r64))]
        save['sym_%d' % d] = np.asarray(sy.all_syms)
        save['e2e_%d_ref32' % d], save['e2e_%d_ref64' % d] = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
        print("%s: %d molecules, %d atoms, %d values; e2e float32 - float64 max %.2e" % (
            name, len(mols), sum(m['n'] for m in mols), sum(len(v) for v in per_sym.values()),
            np.abs(np.asarray(ref32) - np.asarray(ref64)).max()))
    mm = mmd_cases(ref_mmd)
    cat = lambda xs, dt: np.concatenate([np.asarray(x).reshape(-1) for x in xs]).astype(dt)
    path = os.path.join(GOLDEN, 'geometry_cases.npz')
    write_npz(
        path, m_dataset=np.asarray(M['dataset'], np.uint8), m_n=np.asarray(M['n'], np.int32), m_name=np.asarray(M['name']),
        m_pos=cat(M['pos'], np.float32).reshape(-1, 3), m_type=cat(M['type'], np.uint8), m_edge=cat(M['edge'], np.uint8),
        m_counts=np.asarray(M['counts'], np.int32), m_values=cat(M['values'], np.float64),
        mmd_ns=np.asarray(mm['ns'], np.int32), mmd_nt=np.asarray(mm['nt'], np.int32), mmd_family=np.asarray(mm['family']),
        mmd_x=cat(mm['x'], np.float32), mmd_ref64=np.asarray(mm['ref64'], np.float64), mmd_ref32=np.asarray(mm['ref32'], np.float64),
        mmd3_case=np.asarray(mm['case3'], np.int32), mmd3_ref64=np.asarray(mm['ref3'], np.float64), **save)
    size = os.path.getsize(path)
    assert size < 600 * 1024, size
    print("wrote %s (%d bytes)" % (path, size))


if __name__ == '__main__':
    main()

"""Shared by tests/test_geometry_host.py and tests/test_geometry_gpu.py: the recorded cases of tests/golden/geometry_cases.npz
(tools/make_geometry_golden.py) cut back into molecules, symbol lists and MMD cases."""
import numpy as np

from helpers import load_fixture
from jodo_amd.evaluation import GeometrySymbols
from stability_common import rules

DATASETS = ('QM9', 'GeomDrug')
GROUP_KEYS = ('top_bond_sym', 'top_angle_sym', 'top_dihedral_sym')
MEANS = ('bond_length_mean', 'bond_angle_mean', 'dihedral_angle_mean')
_cache = {}


def fixture():
    if 'fx' not in _cache:
        _cache['fx'] = load_fixture('geometry_cases.npz')
    return _cache['fx']


def dataset_info(name):
    """what a reference user passes: the dataset's name, atom decoder and the three symbol lists (as recorded in the fixture)"""
    syms = [str(s) for s in fixture()['sym_%d' % DATASETS.index(name)]]
    info = {'name': name, 'atom_decoder': list(rules(name).atom_decoder)}
    info.update({k: syms[8 * g:8 * g + 8] for g, k in enumerate(GROUP_KEYS)})
    return info


def symbols(name):
    if ('sy', name) not in _cache:
        _cache['sy', name] = GeometrySymbols.from_dataset_info(dataset_info(name))
    return _cache['sy', name]


def recorded(name):
    """the dataset's recorded molecules: dicts with name, n, pos, type, edge and `values` (per symbol, in the order of symbols(name).all_syms,
    the float64 array the reference's functions returned for this molecule)"""
    if ('mols', name) in _cache:
        return _cache['mols', name]
    fx = fixture()
    ns = fx['m_n'].astype(np.int64)
    a0, e0 = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(ns * ns)])
    v0 = np.concatenate([[0], np.cumsum(fx['m_counts'].reshape(-1))])
    out = []
    for m, n in enumerate(ns):
        if DATASETS[int(fx['m_dataset'][m])] != name:
            continue
        vals = [fx['m_values'][v0[24 * m + c]:v0[24 * m + c + 1]] for c in range(24)]
        assert [len(v) for v in vals] == fx['m_counts'][m].tolist()
        out.append(dict(name=str(fx['m_name'][m]), n=int(n), pos=fx['m_pos'][a0[m]:a0[m + 1]], type=fx['m_type'][a0[m]:a0[m + 1]],
                        edge=fx['m_edge'][e0[m]:e0[m + 1]].reshape(n, n), values=vals))
    _cache['mols', name] = out
    return out


def recorded_lists(mols, keep=None):
    """per symbol the recorded values of the molecules, concatenated in molecule order (what the reference returns for the list)"""
    use = [m for b, m in enumerate(mols) if keep is None or keep[b]]
    return [np.concatenate([m['values'][c] for m in use]) if use else np.zeros(0) for c in range(24)]


def processed_list(mols):
    """the reference's processed_list: host tuples (pos, atom_type, edge_type, fc) of torch tensors"""
    import torch
    return [(torch.from_numpy(m['pos'].copy()), torch.from_numpy(m['type'].astype(np.int64)), torch.from_numpy(m['edge'].astype(np.int64)),
             torch.zeros(m['n'], 0)) for m in mols]


def mmd_cases():
    """list of dicts: ns, nt, family, source, target (float32), ref64, ref32, and ref3_64 where kernel_mul = 3 was recorded"""
    if 'mmd' in _cache:
        return _cache['mmd']
    fx = fixture()
    out, lo = [], 0
    three = dict(zip(fx['mmd3_case'].tolist(), fx['mmd3_ref64'].tolist()))
    for k, (ns, nt) in enumerate(zip(fx['mmd_ns'].tolist(), fx['mmd_nt'].tolist())):
        s, t = fx['mmd_x'][lo:lo + ns], fx['mmd_x'][lo + ns:lo + ns + nt]
        lo += ns + nt
        out.append(dict(ns=ns, nt=nt, family=str(fx['mmd_family'][k]), source=s, target=t, ref64=float(fx['mmd_ref64'][k]),
                        ref32=float(fx['mmd_ref32'][k]), ref3_64=three.get(k)))
    _cache['mmd'] = out
    return out


def mmd_bound():
    """16 x the largest distance of the reference's own float32 result from its float64 result over the recorded cases"""
    d = [abs(c['ref32'] - c['ref64']) for c in mmd_cases() if np.isfinite(c['ref64'])]
    return 16. * max(d)


def circle(a, b):
    """distance of two angles in degrees on the circle"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.
    return np.minimum(d, 360. - d)

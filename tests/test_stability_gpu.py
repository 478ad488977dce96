"""GPU: the stability kernels (csrc/eval_kernels.hip through jodo_amd.evaluation) — exact equality with the verdicts the reference
recorded (tests/golden/stability_cases.npz) and with the numpy oracle (tests/oracle_stability.py) on seeded molecules at the shapes
where the kernels change path: one wave / four waves (N = 64 / 65), adjacency words (n = 32 / 33, 64 / 65, 128 / 129), padding,
non-symmetric bond matrices, aromatic entries, valences past the mask, and the fragment count on graphs whose labels travel far.
Every seeded 3-D molecule keeps each pair at least 0.01 pm from its thresholds (stability_common.clear_of_thresholds), so the
comparison is exact whatever the summation order."""
import numpy as np
import pytest
import torch

import oracle_stability as OS
from helpers import make_config, make_model
from jodo_amd import evaluation as E
from stability_common import DATASETS, bond_molecule, clear_of_thresholds, lattice_molecule, pad_batch, recorded, rules

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _cfg(r):
    """a config whose atom-type count is the rules' (the bond rule needs one without an aromatic channel: the QM9 one)"""
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.data.atom_types = r.n_types
    return cfg


def run(r, rule, batch, want_orders=False):
    """the device function on a padded numpy batch -> (per_mol [B,4], totals [4], orders | None) as numpy, and the result dict"""
    fn = E.get_stability_fn(_cfg(r), r, rule)
    res = fn(*[torch.from_numpy(a).to(DEV) for a in batch], want_orders=want_orders)
    torch.cuda.synchronize()
    assert res['per_mol'].is_cuda and res['per_mol'].dtype == torch.int32
    totals = np.array([res[k] for k in ('n_mol_stable', 'n_atom_stable', 'n_atoms', 'n_connected')])
    orders = res['orders'].cpu().numpy() if want_orders else None
    return res['per_mol'].cpu().numpy(), totals, orders, res


def check(r, rule, mols, N=None, junk=None):
    """kernel == oracle on per-molecule rows, totals (also the sum of the rows) and, for the 3-D rule, the order matrix"""
    batch = pad_batch(mols, N, junk)
    per_mol, totals, orders, res = run(r, rule, batch, want_orders=rule == '3d')
    want_rows, want_totals, want_orders = OS.batch(r, rule, *batch)
    assert np.array_equal(per_mol, want_rows), (per_mol[(per_mol != want_rows).any(1)][:4], want_rows[(per_mol != want_rows).any(1)][:4])
    assert np.array_equal(totals, want_totals)
    real = per_mol[:, 1] > 0
    assert totals.tolist() == [int((per_mol[real, 0] == per_mol[real, 1]).sum()), int(per_mol[:, 0].sum()), int(per_mol[:, 1].sum()),
                               int((per_mol[real, 2] == 1).sum())]
    assert res['n_mols'] == int(real.sum())
    if rule == '3d':
        assert orders.dtype == np.uint8 and np.array_equal(orders, want_orders)
        assert np.array_equal(orders, orders.transpose(0, 2, 1)) and not orders[:, np.arange(orders.shape[1]), np.arange(orders.shape[1])].any()
        for b, m in enumerate(mols):
            assert not orders[b, m['n']:].any() and not orders[b, :, m['n']:].any()
    return per_mol, totals, orders


@pytest.mark.parametrize("rule", ['3d', 'bonds'])
@pytest.mark.parametrize("dataset", DATASETS)
def test_whole_fixture_equals_the_recorded_verdicts(rule, dataset):
    r = rules(dataset)
    cases = [c for c in recorded(rule) if c['dataset'] == dataset]
    batch = pad_batch(cases)
    per_mol, totals, orders, res = run(r, rule, batch, want_orders=rule == '3d')
    assert per_mol[:, 0].tolist() == [c['stable_atoms'] for c in cases]
    assert per_mol[:, 1].tolist() == [c['n'] for c in cases]
    assert (per_mol[:, 0] == per_mol[:, 1]).tolist() == [c['mol_stable'] for c in cases]
    assert not per_mol[:, 3].any()
    assert totals[:3].tolist() == [sum(c['mol_stable'] for c in cases), sum(c['stable_atoms'] for c in cases), sum(c['n'] for c in cases)]
    assert res['mol_stable'] == totals[0] / len(cases) and res['atom_stable'] == totals[1] / totals[2]
    if rule == '3d':                                              # the recorded per-atom valences are the row sums of the orders
        for b, c in enumerate(cases):
            assert orders[b, :c['n'], :c['n']].sum(1).tolist() == c['valence'].tolist(), (c['name'], c['n'])
    # and the wrappers with the reference's names, on its own tuple format
    info = dict(name=dataset, atom_decoder=list(r.atom_decoder))
    t = torch.from_numpy
    if rule == '3d':
        got = E.get_edm_metric(info, r, device=DEV)([(t(c['pos']), t(c['type']).long()) for c in cases])
    else:
        got = E.get_2D_edm_metric(info, r, device=DEV)([(None, t(c['type']).long(), t(c['edge']).float(), t(c['fc']).long()) for c in cases])
    assert got == {'mol_stable': res['mol_stable'], 'atom_stable': res['atom_stable']}


def test_lone_hydrogen_and_pairs():
    r = rules('QM9')
    per_mol, totals, _ = check(r, '3d', [dict(n=1, pos=np.zeros((1, 3), np.float32), type=np.zeros(1, np.uint8))])
    assert per_mol.tolist() == [[0, 1, 1, 0]] and totals.tolist() == [0, 0, 1, 1]                   # unstable, one fragment
    per_mol, totals = check(r, 'bonds', [dict(n=1, type=np.zeros(1, np.uint8))])[:2]
    assert per_mol.tolist() == [[0, 1, 1, 0]]
    rng = np.random.default_rng(1)
    check(r, '3d', [lattice_molecule(rng, r, 2) for _ in range(6)])
    check(r, 'bonds', [bond_molecule(rng, r, 2, symmetric=bool(k % 2)) for k in range(6)])
    h, f = r.atom_decoder.index('H'), r.atom_decoder.index('F')
    per_mol = check(r, '3d', [dict(n=2, pos=np.array([[0, 0, 0], [0.92, 0, 0]], np.float32), type=np.array([h, f], np.uint8))])[0]
    assert per_mol.tolist() == [[2, 2, 1, 0]]


@pytest.mark.parametrize("rule", ['3d', 'bonds'])
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 181])
def test_sizes_where_the_block_shape_and_the_adjacency_words_change(rule, n):
    r = rules('GeomDrug')
    rng = np.random.default_rng(100 + n)
    make = (lambda k, s: lattice_molecule(rng, r, k)) if rule == '3d' else (lambda k, s: bond_molecule(rng, r, k, s))
    mols = [make(n, True), make(max(1, n - 33), False), make(n, False)]
    per_mol = check(r, rule, mols)[0]
    assert per_mol[0, 1] == n and 0 < per_mol[:, 0].sum() < per_mol[:, 1].sum()                     # stable and unstable atoms both occur


@pytest.mark.parametrize("rule", ['3d', 'bonds'])
def test_batch_of_every_size_up_to_29(rule):
    r = rules('QM9')
    rng = np.random.default_rng(7)
    mols = [lattice_molecule(rng, r, n) if rule == '3d' else bond_molecule(rng, r, n, n % 3 != 0) for n in range(1, 30)]
    per_mol = check(r, rule, mols)[0]
    assert per_mol[:, 1].tolist() == list(range(1, 30))


@pytest.mark.parametrize("rule", ['3d', 'bonds'])
@pytest.mark.parametrize("N", [64, 100])
def test_padding_does_not_exist(rule, N):
    """N well beyond every n, one wave (64) and four (100); the padding as the decode leaves it (origin, type 0, no bonds) and filled with
    junk — the rows are the same both times, and a molecule without atoms is a zero row that no total counts."""
    r = rules('QM9')
    rng = np.random.default_rng(11)
    mols = [lattice_molecule(rng, r, n) if rule == '3d' else bond_molecule(rng, r, n, n % 2 == 0) for n in (1, 5, 12, 29, 3)]
    mols.insert(2, dict(n=0, type=np.zeros(0, np.uint8)))
    clean = check(r, rule, mols, N=N)
    junk = check(r, rule, mols, N=N, junk=np.random.default_rng(12))
    assert np.array_equal(clean[0], junk[0]) and np.array_equal(clean[1], junk[1])
    assert clean[0][2].tolist() == [0, 0, 0, 0] and clean[1][2] == sum(m['n'] for m in mols)
    # an atom near the origin next to zero padding: a kernel that forgot the mask would bond it to the padding's hydrogens
    c = r.atom_decoder.index('C')
    lone = [dict(n=1, pos=np.array([[0.5, 0, 0]], np.float32), type=np.array([c], np.uint8))]
    assert check(r, '3d', lone, N=N)[0].tolist() == [[0, 1, 1, 0]]


def test_non_symmetric_and_aromatic_bond_entries():
    r = rules('QM9')
    h, c, o = (r.atom_decoder.index(s) for s in 'HCO')
    # O=C=O in the upper triangle, junk below it: only the upper triangle is read
    e = np.array([[0, 2, 0], [3, 0, 2], [1, 3, 0]], np.uint8)
    mol = dict(n=3, type=np.array([o, c, o], np.uint8), fc=np.zeros(3, np.int8), edge=e)
    assert check(r, 'bonds', [mol])[0].tolist() == [[3, 3, 1, 0]]
    mol_t = dict(mol, edge=e.T.copy())                            # transposed: O-C 3, C-O 3, O..O 1 -> valences 4, 6, 4
    assert check(r, 'bonds', [mol_t])[0].tolist() == [[0, 3, 1, 0]]
    # a type-4 entry: counted in needs_kekulize, no valence from it, but it joins the fragments
    e4 = np.array([[0, 4, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8)
    arom = dict(n=4, type=np.array([h, h, h, h], np.uint8), fc=np.zeros(4, np.int8), edge=e4)
    rows = check(r, 'bonds', [arom, mol])[0]
    assert rows.tolist() == [[2, 4, 2, 1], [3, 3, 1, 0]]          # H1, H2 have valence 1 (stable); H0 and H3 valence 0; fragments {0,1,2}, {3}
    info = dict(name='QM9', atom_decoder=list(r.atom_decoder))
    t = torch.from_numpy
    with pytest.raises(NotImplementedError, match='Kekulize'):
        E.get_2D_edm_metric(info, r, device=DEV)([(None, t(arom['type']).long(), t(e4).float(), t(arom['fc']).long())])


def test_valence_past_the_mask():
    """made-up tables: type 0 pairs are triple below 2 A, type 0 - type 1 single below 3 A; type 0 may have valence 1 or 31, type 1 11."""
    thr = np.zeros((5, 5, 3), np.int32)
    thr[0, 0] = (300, 250, 200)
    thr[0, 1] = thr[1, 0] = (300, 0, 0)
    toy = E.StabilityRules(['H', 'C', 'N', 'O', 'F'], 'QM9', 'index', thr, [[1, 31], [11], [0], [0], [0]],
                           [{0: [1, 31]}, {0: [11]}, {0: [0]}, {0: [0]}, {0: [0]}])
    rng = np.random.default_rng(5)

    def ball(k):                                                  # k points, every pair 0.3 .. 1.8 A apart
        while True:
            p = rng.normal(size=(k, 3))
            p = (0.9 * rng.random((k, 1)) ** (1. / 3.) * p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
            d = np.linalg.norm(p[:, None] - p[None], axis=-1)[np.triu_indices(k, 1)]
            if d.min() > 0.3:
                return p
    a = dict(n=12, pos=np.concatenate([ball(11), np.array([[1.5, 0, 0]], np.float32)]), type=np.array([0] * 11 + [1], np.uint8))
    b = dict(n=12, pos=ball(12), type=np.zeros(12, np.uint8))     # 11 triple bonds each: valence 33, past the mask (and 33 & 31 == 1)
    for m in (a, b):
        assert clear_of_thresholds(toy, m['pos'], m['type'])
    assert OS.stability_3d(toy, a['pos'], a['type'])['valence'].tolist() == [31] * 11 + [11]
    assert OS.stability_3d(toy, b['pos'], b['type'])['valence'].tolist() == [33] * 12
    assert check(toy, '3d', [a, b])[0].tolist() == [[12, 12, 1, 0], [0, 12, 1, 0]]
    # the bond rule: a centre with 11 triple bonds (33) and one with 10 triple bonds and a single one (31)
    def star(orders):
        n = len(orders) + 1
        e = np.zeros((n, n), np.uint8)
        e[0, 1:] = orders
        return dict(n=n, type=np.array([0] + [2] * (n - 1), np.uint8), fc=np.zeros(n, np.int8), edge=e)
    rows = check(toy, 'bonds', [star([3] * 11), star([3] * 10 + [1])])[0]
    assert rows.tolist() == [[0, 12, 1, 0], [1, 12, 1, 0]]


def _relabel(edge, perm):
    n = len(perm)
    out = np.zeros((n, n), np.uint8)
    i, j = np.nonzero(edge)
    out[np.minimum(perm[i], perm[j]), np.maximum(perm[i], perm[j])] = edge[i, j]
    return out


@pytest.mark.parametrize("n", [7, 64, 181])
def test_fragments(n):
    """a chain, a ring, two components and no bonds at all, with the atoms in order and shuffled (labels then travel against the index
    order); 3-D: carbons 1.5 A apart on a line (QM9 rules: a single bond to each neighbour, none further) and the same line cut in two."""
    r = rules('GeomDrug')
    rng = np.random.default_rng(n)
    chain = np.zeros((n, n), np.uint8)
    chain[np.arange(n - 1), np.arange(1, n)] = 1
    ring = chain.copy()
    ring[0, n - 1] = 2
    two = chain.copy()
    two[n // 2 - 1, n // 2] = 0
    mols, want = [], []
    for e, frags in ((chain, 1), (ring, 1), (two, 2), (np.zeros((n, n), np.uint8), n)):
        for perm in (np.arange(n), rng.permutation(n)):
            mols.append(dict(n=n, type=np.full(n, 2, np.uint8), fc=np.zeros(n, np.int8), edge=_relabel(e, perm)))
            want.append(frags)
    per_mol, totals, _ = check(r, 'bonds', mols)
    assert per_mol[:, 2].tolist() == want and totals[3] == sum(f == 1 for f in want)
    q = rules('QM9')
    c = q.atom_decoder.index('C')
    m = min(n, 29)
    x = 1.5 * np.arange(m, dtype=np.float32)
    cut = x + np.where(np.arange(m) >= m // 2, 1.5, 0.).astype(np.float32)
    mols3 = []
    for xs in (x, cut):
        for perm in (np.arange(m), rng.permutation(m)):
            pos = np.zeros((m, 3), np.float32)
            pos[:, 0] = (xs - xs.mean())[perm]
            assert clear_of_thresholds(q, pos, np.full(m, c))
            mols3.append(dict(n=m, pos=pos, type=np.full(m, c, np.uint8)))
    assert check(q, '3d', mols3)[0][:, 2].tolist() == [1, 1, 2, 2]


def test_one_sampling_round_accumulates_the_oracles_totals():
    """get_sampling_fn(..., stability=fn): a seeded-weight QM9 model, B = 8, 3 ancestral steps; last_stability is the oracle applied to the
    molecules the same round returned (fused.mols_from_decoded of the same decoded tensors)."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    from oracle.stubs import FixedNodes
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = torch.device(DEV)
    cfg.sampling.steps = 3
    r = rules('QM9')
    model = make_model(cfg, 7, DEV)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    n_nodes = [1, 2, 9, 17, 29, 12, 5, 23]
    for rule in ('3d', 'bonds'):
        fn = get_sampling_fn(cfg, ns, FixedNodes(n_nodes), 8, 8, get_data_inverse_scaler(cfg), return_raw=True,
                             stability=E.get_stability_fn(cfg, r, rule))
        assert fn.last_stability is None
        torch.manual_seed(3)
        mols = fn(model)
        assert [int(m[1].shape[0]) for m in mols] == n_nodes
        want = dict(n_mol_stable=0, n_atom_stable=0, n_atoms=0, n_connected=0, n_mols=0)
        for pos, at, et, fc in mols:
            o = OS.stability_3d(r, pos.numpy(), at.numpy()) if rule == '3d' else OS.stability_bonds(r, at.numpy(), fc.numpy(), et.numpy())
            want['n_mol_stable'] += int(o['stable_atoms'] == o['atoms'])
            want['n_atom_stable'] += o['stable_atoms']
            want['n_atoms'] += o['atoms']
            want['n_connected'] += int(o['fragments'] == 1)
            want['n_mols'] += 1
        print("round (%s rule): %s" % (rule, fn.last_stability))
        assert fn.last_stability == want and want['n_atoms'] == sum(n_nodes)

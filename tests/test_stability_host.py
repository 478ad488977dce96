"""CPU: the stability rules as data (jodo_amd/evaluation/rules.py), the numpy oracle against the verdicts the reference recorded
(tests/golden/stability_cases.npz), and every refusal of the Python surface (jodo_amd/evaluation/stability.py, get_sampling_fn)."""
import json

import numpy as np
import pytest
import torch

import oracle_stability as OS
from helpers import make_config
from jodo_amd import evaluation as E
from stability_common import DATASETS, RULES_FILE, recorded, rules

# toy tables (made-up numbers): X-Y knows a double-bond length, Y-X does not; Z bonds to nothing
TOY = dict(bonds1={'X': {'X': 100, 'Y': 120}, 'Y': {'X': 120, 'Y': 140}}, bonds2={'X': {'X': 90, 'Y': 105}}, bonds3={'X': {'X': 80}},
           margins=(10, 5, 3), allowed_bonds={'X': 1, 'Y': [2, 4], 'Z': 0},
           allowed_fc_bonds={'X': {0: 1, 1: [0, 2], -1: 0}, 'Y': [2, 4], 'Z': 3})


def toy_rules(name='QM9', decoder=('X', 'Y', 'Z'), **over):
    t = dict(TOY, **over)
    return E.StabilityRules.from_tables(list(decoder), name, t['bonds1'], t['bonds2'], t['bonds3'], t['margins'], t['allowed_bonds'],
                                        t['allowed_fc_bonds'])


@pytest.mark.parametrize("rule", ['3d', 'bonds'])
def test_oracle_reproduces_every_recorded_verdict(rule):
    """Every molecule of the fixture: stable-atom count, stability flag and per-atom valence exactly as the reference gave them."""
    cases = recorded(rule)
    assert len(cases) > 150 and {c['dataset'] for c in cases} == set(DATASETS)
    for c in cases:
        r = rules(c['dataset'])
        got = OS.stability_3d(r, c['pos'], c['type']) if rule == '3d' else OS.stability_bonds(r, c['type'], c['fc'], c['edge'])
        what = (rule, c['dataset'], c['name'], c['n'])
        assert np.array_equal(got['valence'], c['valence']), what
        assert got['stable_atoms'] == c['stable_atoms'] and (got['stable_atoms'] == c['n']) == c['mol_stable'], what
        assert got['needs_kekulize'] == 0


def test_fixture_covers_what_it_should():
    d3, bd = recorded('3d'), recorded('bonds')
    names = {c['name'] for c in d3}
    assert {'CH4', 'H2O', 'NH3', 'HF', 'C2H6', 'C2H4', 'C2H2', 'HCN', 'CO2', 'C,S', 'S,C', 'lattice'} <= names
    assert all(c['mol_stable'] for c in d3 if c['name'] not in ('lattice', 'C,S', 'S,C'))
    for c in d3:
        if c['name'] in ('C,S', 'S,C'):                         # sorted by type index: a double bond in either atom order
            assert c['valence'].tolist() == [2, 2]
    assert max(c['n'] for c in d3) == 181 and min(c['n'] for c in d3) == 1
    assert set(np.concatenate([c['type'] for c in d3 if c['dataset'] == 'GeomDrug']).tolist()) == set(range(16))
    assert any(c['name'] == 'asym' and not np.array_equal(c['edge'], c['edge'].T) for c in bd)
    assert set(np.concatenate([c['fc'] for c in bd]).tolist()) == {-1, 0, 1}
    for cases in (d3, bd):
        atoms, stable = sum(c['n'] for c in cases), sum(c['stable_atoms'] for c in cases)
        assert 0.1 * atoms <= stable <= 0.9 * atoms and sum(c['mol_stable'] for c in cases) >= 8


def test_rules_file_is_numbers_and_symbols_and_keeps_the_asymmetry():
    with open(RULES_FILE) as f:
        doc = json.load(f)
    assert set(doc['datasets']) == set(DATASETS)
    qm9, geom = rules('QM9'), rules('GeomDrug')
    assert qm9.pair_order == 'index' and geom.pair_order == 'type' and qm9.n_types == 5 and geom.n_types == 16
    c, s = geom.atom_decoder.index('C'), geom.atom_decoder.index('S')
    assert geom.thr[c, s, 1] > 0 and geom.thr[s, c, 1] == 0 and geom.thr[c, s, 0] == geom.thr[s, c, 0] > 0

    def leaves(x):
        if isinstance(x, dict):
            for k, v in x.items():
                yield from leaves(v)
        elif isinstance(x, list):
            for v in x:
                yield from leaves(v)
        else:
            yield x
    symbols = set(geom.atom_decoder)
    for sec in doc['datasets'].values():
        for leaf in leaves({k: v for k, v in sec.items() if k != 'pair_order'}):
            assert (isinstance(leaf, int) and not isinstance(leaf, bool)) or leaf in symbols, leaf


def test_from_tables_round_trip(tmp_path):
    r = toy_rules()
    assert r.thr[0, 1].tolist() == [130, 110, 0] and r.thr[1, 0].tolist() == [130, 0, 0]           # X->Y has a double length, Y->X none
    assert r.thr[0, 0].tolist() == [110, 95, 83] and not r.thr[2].any() and not r.thr[:, 2].any()
    assert r.allowed_mask.tolist() == [1 << 1, (1 << 2) | (1 << 4), 1 << 0]
    # charge fallback: X lists -1, 0, +1; Y (a list) and Z (an int) ignore the charge, so every column is their entry for 0
    assert (r.fc_lo, r.fc_hi) == (-1, 1)
    assert r.allowed_fc_mask.tolist() == [[1 << 0, 1 << 1, (1 << 0) | (1 << 2)], [(1 << 2) | (1 << 4)] * 3, [1 << 3] * 3]
    geom = toy_rules('GeomDrug')
    path = str(tmp_path / 'rules.json')
    r.to_file(path, also=(geom,))
    for name, want in (('QM9', r), ('GeomDrug', geom)):
        back = E.StabilityRules.from_file(path, name)
        assert back.atom_decoder == want.atom_decoder and back.pair_order == want.pair_order and back.dataset_name == name
        assert np.array_equal(back.thr, want.thr) and back.thr.dtype == np.int32
        assert np.array_equal(back.allowed_mask, want.allowed_mask) and np.array_equal(back.allowed_fc_mask, want.allowed_fc_mask)
        assert (back.fc_lo, back.fc_hi) == (want.fc_lo, want.fc_hi) and back.allowed_fc == want.allowed_fc
    assert E.StabilityRules.from_file(path, 'QM9').thr[0, 1, 1] == 110 and E.StabilityRules.from_file(path, 'QM9').thr[1, 0, 1] == 0
    with pytest.raises(E.MissingSectionError, match='say which one'):
        E.StabilityRules.from_file(path)
    single = str(tmp_path / 'one.json')
    r.to_file(single)
    assert E.StabilityRules.from_file(single).dataset_name == 'QM9'


def test_oracle_on_the_toy_rules():
    """the ordered lookup and the charge fallback, by hand: X(0) Y(1) at 1.08 A is a double bond by atom index X,Y and a single one by Y,X."""
    r, g = toy_rules(), toy_rules('GeomDrug')
    pos = np.array([[0, 0, 0], [1.08, 0, 0]], np.float32)
    assert OS.orders_3d(r, pos, [0, 1])[0, 1] == 2 and OS.orders_3d(r, pos, [1, 0])[0, 1] == 1
    assert OS.orders_3d(g, pos, [0, 1])[0, 1] == 2 and OS.orders_3d(g, pos, [1, 0])[0, 1] == 2           # sorted by type index
    e = np.array([[0, 2], [3, 0]])                                # only the upper triangle counts
    got = OS.stability_bonds(r, [0, 1], [1, 1], e)                # X at +1 allows 0 or 2; Y ignores the charge
    assert got['valence'].tolist() == [2, 2] and got['stable'].tolist() == [True, True]
    got = OS.stability_bonds(r, [0, 0], [0, -1], np.array([[0, 4], [0, 0]]))          # aromatic: counted, no valence; X at -1 allows 0
    assert got['valence'].tolist() == [0, 0] and got['needs_kekulize'] == 1 and got['stable'].tolist() == [False, True]
    assert got['fragments'] == 1
    assert OS.fragments(np.zeros((3, 3))) == 3 and OS.fragments(np.zeros((0, 0))) == 0


def test_named_errors_of_the_rules(tmp_path):
    with pytest.raises(E.UnknownElementError, match='Q'):
        toy_rules(decoder=('X', 'Q'))
    with pytest.raises(E.UnknownElementError, match='allowed_fc_bonds'):
        toy_rules(allowed_fc_bonds={'X': 1, 'Y': 2})
    with pytest.raises(E.ValenceRangeError, match='32'):
        toy_rules(allowed_bonds={'X': 1, 'Y': [2, 32], 'Z': 0})
    with pytest.raises(E.ValenceRangeError):
        toy_rules(allowed_fc_bonds={'X': {0: -1}, 'Y': 2, 'Z': 3})
    with pytest.raises(E.MissingSectionError, match='charge 0'):
        toy_rules(allowed_fc_bonds={'X': {1: 2}, 'Y': 2, 'Z': 3})
    with pytest.raises(E.UnknownDatasetError, match='Zinc250k'):
        toy_rules('Zinc250k')
    path = str(tmp_path / 'r.json')
    toy_rules().to_file(path)
    with open(path) as f:
        doc = json.load(f)
    with pytest.raises(E.MissingSectionError, match='GeomDrug'):
        E.StabilityRules.from_file(path, 'GeomDrug')

    def broken(change):
        d = json.loads(json.dumps(doc))
        change(d['datasets']['QM9'])
        p = str(tmp_path / 'broken.json')
        with open(p, 'w') as f:
            json.dump(d, f)
        return p
    with pytest.raises(E.MissingSectionError, match='thresholds_pm'):
        E.StabilityRules.from_file(broken(lambda s: s.pop('thresholds_pm')), 'QM9')
    with pytest.raises(E.UnknownElementError, match='Q'):
        E.StabilityRules.from_file(broken(lambda s: s['thresholds_pm'].append(['X', 'Q', 100, 0, 0])), 'QM9')
    with pytest.raises(E.UnknownElementError, match='allowed_valences'):
        E.StabilityRules.from_file(broken(lambda s: s['allowed_valences'].pop('Y')), 'QM9')
    with pytest.raises(E.ValenceRangeError, match='40'):
        E.StabilityRules.from_file(broken(lambda s: s['allowed_valences'].update(Y=[40])), 'QM9')
    with pytest.raises(E.MissingSectionError, match='charge "0"'):
        E.StabilityRules.from_file(broken(lambda s: s['allowed_valences_by_charge']['X'].pop('0')), 'QM9')
    with pytest.raises(E.RulesError, match='pair_order'):
        E.StabilityRules.from_file(broken(lambda s: s.update(pair_order='sorted')), 'QM9')


def test_refusals_of_the_python_surface():
    cfg = make_config('vpsde_qm9_uncond_jodo')
    qm9, geom = rules('QM9'), rules('GeomDrug')
    fn = E.get_stability_fn(cfg, qm9, '3d')
    B, N = 2, 4
    cpu = (torch.zeros(B, N, 3), torch.zeros(B, N, dtype=torch.uint8), torch.zeros(B, N, dtype=torch.int8),
           torch.zeros(B, N, N, dtype=torch.uint8), torch.ones(B, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        fn(*cpu)
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        E.get_stability_fn(cfg, qm9, 'bonds')(*cpu)
    with pytest.raises(ValueError, match="'3d'"):
        E.get_stability_fn(cfg, qm9, '2d')
    with pytest.raises(ValueError, match='atom_types'):
        E.get_stability_fn(cfg, geom, '3d')                       # T = 16 against the QM9 config's 5
    gcfg = make_config('vpsde_geom_uncond_jodo')
    E.get_stability_fn(gcfg, geom, '3d')                          # the 3-D rule has no quarrel with an aromatic channel
    with pytest.raises(NotImplementedError, match='Kekulize'):
        E.get_stability_fn(gcfg, geom, 'bonds')
    cfg.data.include_aromatic = True
    with pytest.raises(NotImplementedError, match='Kekulize'):
        E.get_stability_fn(cfg, qm9, 'bonds')
    cfg.data.include_aromatic = False
    zinc = E.StabilityRules(qm9.atom_decoder, 'Zinc250k', 'index', qm9.thr, qm9.allowed, qm9.allowed_fc)
    with pytest.raises(E.UnknownDatasetError, match='Zinc250k'):
        E.get_stability_fn(cfg, zinc, '3d')
    info = dict(name='QM9', atom_decoder=list(qm9.atom_decoder))
    with pytest.raises(E.UnknownDatasetError, match='MOSES'):
        E.get_edm_metric(dict(name='MOSES', atom_decoder=['C']), qm9)
    with pytest.raises(ValueError, match='dataset_info'):
        E.get_2D_edm_metric(info, geom)
    mols = [(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long), torch.zeros(2, 2), torch.zeros(2, dtype=torch.long))]
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        E.get_edm_metric(info, qm9, device='cpu')(mols)
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        E.get_2D_edm_metric(info, qm9, device='cpu')(mols)
    with pytest.raises(TypeError, match='StabilityRules'):
        E.get_stability_fn(cfg, {'QM9': 1})


def test_get_sampling_fn_default_still_builds_and_refuses_what_it_cannot_do():
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.dist import allreduce_counts
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    from oracle.stubs import FixedNodes
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = 'cpu'
    cfg.sampling.steps = 2
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    inv = get_data_inverse_scaler(cfg)
    fn = get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv)
    assert fn.last_stability is None and fn.last_indices is None
    assert get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv, stability=None).last_stability is None
    sfn = E.get_stability_fn(cfg, rules('QM9'), '3d')
    with pytest.raises(ValueError, match='fused device decode'):
        get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv, stability=sfn, fused_decode=False)
    with pytest.raises(TypeError, match='get_stability_fn'):
        get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv, stability='3d')
    cfg2 = make_config('vpsde_zinc_2d_jodo')
    cfg2.device = 'cpu'
    with pytest.raises(NotImplementedError, match='3-D sampling path'):
        get_sampling_fn(cfg2, ns, FixedNodes([3, 4]), 2, 2, get_data_inverse_scaler(cfg2), stability=sfn)
    # without a process group the counts come back unchanged, dict or sequence
    assert allreduce_counts({'n_atoms': 7, 'n_mols': 2}) == {'n_atoms': 7, 'n_mols': 2} and allreduce_counts([1, 2, 3]) == [1, 2, 3]


def _counts_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    from jodo_amd.dist import allreduce_counts
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mine = {'n_mol_stable': rank, 'n_atom_stable': 10 + rank, 'n_atoms': 2 ** 40 + rank, 'n_connected': 0, 'n_mols': 3}
    q.put((rank, allreduce_counts(mine), allreduce_counts([rank + 1, 5])))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_counts_world2():
    """two ranks over gloo: the four totals and the molecule count summed by one all-reduce, beyond 32 bits, dict and sequence"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_counts_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    want = {'n_mol_stable': 1, 'n_atom_stable': 21, 'n_atoms': 2 ** 41 + 1, 'n_connected': 0, 'n_mols': 6}
    assert res == [(0, want, [3, 10]), (1, want, [3, 10])]

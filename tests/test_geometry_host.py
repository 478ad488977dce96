"""CPU: the sub-structure geometry without a GPU — symbol parsing, the numpy oracle (tests/oracle_geometry.py) against the values the
reference's own functions recorded (tests/golden/geometry_cases.npz), what the fixture covers, the nanmean rule of the result dict, the
tile table of the batched MMD, and every refusal of the Python surface (jodo_amd/evaluation/geometry.py, mmd.py, get_sampling_fn)."""
import numpy as np
import pytest
import torch

import oracle_geometry as OG
from geometry_common import DATASETS, MEANS, circle, dataset_info, fixture, mmd_bound, mmd_cases, recorded, symbols
from helpers import make_config
from jodo_amd import evaluation as E
from jodo_amd.evaluation.geometry import assemble_metric
from jodo_amd.evaluation.mmd import tile_table


def test_symbol_parsing():
    dec = ['H', 'C', 'N', 'O', 'Cl', 'Br']
    sy = E.GeometrySymbols(dec, ['C1H', 'C12C', 'Cl1C', 'C1Br', 'C1H'], ['C1C-C1Cl', 'Br1C-C12N'], ['H1C-C2C-C3N'])
    assert sy.syms[0] == ['C1H', 'C12C', 'Cl1C', 'C1Br']                       # listed twice: one class, as one key of the reference's dict
    assert sy.classes[0].tolist() == [[1, 1, 0], [1, 12, 1], [4, 1, 1], [1, 1, 5]]
    assert sy.classes[1].tolist() == [[1, 1, 1, 1, 1, 4], [5, 1, 1, 1, 12, 2]]
    assert sy.classes[2].tolist() == [[0, 1, 1, 1, 2, 1, 1, 3, 2]]
    assert all(c.dtype == np.int32 for c in sy.classes) and sy.n_types == 6
    assert sy.all_syms == ['C1H', 'C12C', 'Cl1C', 'C1Br', 'C1C-C1Cl', 'Br1C-C12N', 'H1C-C2C-C3N']
    for name in DATASETS:
        s = symbols(name)
        assert [c.shape for c in s.classes] == [(8, 3), (8, 6), (8, 9)]
        assert (s.classes[1][:, 2] == s.classes[1][:, 3]).all() and (s.classes[2][:, 5] == s.classes[2][:, 6]).all()
    g = symbols('GeomDrug')
    assert g.classes[0][g.syms[0].index('C12C')].tolist() == [2, 12, 2] and g.classes[0][g.syms[0].index('H1N')].tolist() == [0, 1, 3]
    empty = E.GeometrySymbols(dec, [], [], [])
    assert [c.shape for c in empty.classes] == [(0, 3), (0, 6), (0, 9)]


def test_refusals_of_the_symbols():
    dec = ['H', 'C', 'N']
    for bad, msg in ((['C-H'], 'not a bond symbol'), (['CH'], 'does not parse'), (['c1H'], 'does not parse'), (['C1H-C1H'], 'not a bond symbol'),
                     (['C1O'], 'lacks'), (['Cl1C'], 'lacks'), ([7], 'not a bond symbol'), (['C1.5C'], 'does not parse')):
        with pytest.raises(ValueError, match=msg):
            E.GeometrySymbols(dec, bad, [], [])
    with pytest.raises(ValueError, match='not an angle symbol'):
        E.GeometrySymbols(dec, [], ['C1H'], [])
    with pytest.raises(ValueError, match='not a dihedral symbol'):
        E.GeometrySymbols(dec, [], [], ['C1H-H1C'])
    with pytest.raises(ValueError, match='at most 32'):
        E.GeometrySymbols(dec, ['C%dH' % k for k in range(33)], [], [])
    with pytest.raises(ValueError, match="no 'top_angle_sym'"):
        E.GeometrySymbols.from_dataset_info({'atom_decoder': dec, 'top_bond_sym': [], 'top_dihedral_sym': []})


@pytest.mark.parametrize("name", DATASETS)
def test_oracle_reproduces_every_recorded_value(name):
    """the enumeration (which bonds, which roles, how often, which symbol, in which order) and the float64 formulas"""
    sy = symbols(name)
    for m in recorded(name):
        if m['n'] == 0:
            assert not sum(len(v) for v in m['values'])
            continue
        got, dropped = OG.extract(sy.classes, m['pos'], m['type'], m['edge'])
        assert dropped == [0, 0, 0]
        flat = [np.asarray(v) for g in got for v in g]
        for s, v, want in zip(sy.all_syms, flat, m['values']):
            assert len(v) == len(want), (m['name'], s)
            if len(want):
                assert (np.abs(v - want) if s in sy.syms[0] else circle(v, want)).max() < 1e-9, (m['name'], s)


def test_fixture_covers_what_it_should():
    for name in DATASETS:
        sy, mols = symbols(name), recorded(name)
        names = [m['name'] for m in mols]
        for tag in ('3-ring', '4-ring', 'degree-7', 'aromatic', '1-atom', '2-atom', 'empty', 'angle-twice', 'angle-never', 'random-asym'):
            assert tag in names, (name, tag)
        by = {m['name']: m for m in mols}
        assert by['empty']['n'] == 0 and by['1-atom']['n'] == 1 and by['2-atom']['n'] == 2
        assert (by['aromatic']['edge'] == 4).any() and ((by['degree-7']['edge'] > 0).sum(1).max() >= 6)
        assert sum(len(v) for v in by['angle-never']['values'][8:16]) == 0
        assert sum(len(v) for v in by['angle-twice']['values'][8:16]) == 2
        for half in (mols[0::2], mols[1::2]):                  # generated and target side of the end-to-end case
            hits = np.sum([[len(v) for v in m['values']] for m in half], 0)
            assert hits.min() >= 3, (name, dict(zip(sy.all_syms, hits)))
        ang = np.concatenate([v for m in mols for v in m['values'][8:16]])
        dih = np.concatenate([v for m in mols for v in m['values'][16:24]])
        assert ang.min() > 1. and ang.max() < 179. and np.abs(dih).max() < 179.
        for m in mols:
            if m['n'] > 1:
                p = m['pos'].astype(np.float64)
                assert (np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)) + 10. * np.eye(m['n'])).min() >= 0.3
        assert max(m['n'] for m in mols) >= (29 if name == 'QM9' else 65)
    fams = {(c['ns'], c['nt']) for c in mmd_cases()}
    assert fams >= {(1, 1), (63, 257), (256, 256), (1000, 1500), (5000, 3000)} and any(c['ns'] == 0 for c in mmd_cases())
    assert {c['family'] for c in mmd_cases()} == {'length', 'angle', 'dihedral'}


def test_oracle_mmd_equals_the_reference_in_float64():
    for c in mmd_cases():
        if c['ns'] * c['nt'] > 300 * 300:                     # the large cases were checked when the fixture was written
            continue
        got = OG.mmd(c['source'], c['target'])
        if c['ns'] == 0:
            assert np.isnan(got) and np.isnan(c['ref64'])
        else:
            assert abs(got - c['ref64']) < 1e-12
        if c['ref3_64'] is not None:
            assert abs(OG.mmd(c['source'], c['target'], kernel_mul=3.0) - c['ref3_64']) < 1e-12
    assert np.isnan(OG.mmd([1.5, 1.5], [1.5]))                # zero bandwidth: NaN, as the reference
    b = mmd_bound()
    print("largest float32 - float64 distance of the reference: %.3e, kernel bound %.3e" % (b / 16., b))
    assert 1e-7 < b < 1e-4


def test_the_one_exp_identity():
    """kernel_mul = 2, kernel_num = 5: the five kernels of a pair are u^16, u^8, u^4, u^2, u with u = exp(-d^2 / (bw * 4))"""
    rng = np.random.default_rng(5)
    d2, bw = rng.random(1000) * 3., 0.7
    five = sum(np.exp(-d2 / (bw / 4. * 2. ** i)) for i in range(5))
    u = np.exp(-d2 / (bw * 4.))
    assert np.abs(five - (u + u ** 2 + u ** 4 + u ** 8 + u ** 16)).max() < 1e-14


def test_nanmean_rule():
    sy = symbols('QM9')
    got = {s: 0.25 * (k + 1) for k, s in enumerate(sy.all_syms)}
    del got[sy.syms[0][1]], got[sy.syms[0][2]]
    for s in sy.syms[2]:
        del got[s]
    with np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        out = assemble_metric(sy, got)
    assert list(out) == sy.syms[0] + [MEANS[0]] + sy.syms[1] + [MEANS[1]] + sy.syms[2] + [MEANS[2]]
    assert np.isnan(out[sy.syms[0][1]]) and np.isnan(out[sy.syms[0][2]])
    assert out[MEANS[0]] == pytest.approx(np.mean([0.25 * (k + 1) for k in (0, 3, 4, 5, 6, 7)]))
    assert out[MEANS[1]] == pytest.approx(np.mean([0.25 * (k + 1) for k in range(8, 16)]))
    assert np.isnan(out[MEANS[2]]) and all(np.isnan(out[s]) for s in sy.syms[2])


def test_tile_table():
    tiles, start = tile_table([(3000, 1000), (0, 5), (1, 1)])
    assert tiles.dtype == np.int32 and start.tolist() == [0, 10, 11, 14]
    assert tiles[:6].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1024], [0, 0, 0, 2048], [0, 0, 1024, 1024], [0, 0, 1024, 2048], [0, 0, 2048, 2048]]
    assert tiles[6:10].tolist() == [[0, 1, 0, 0], [0, 2, 0, 0], [0, 2, 1024, 0], [0, 2, 2048, 0]]
    assert tiles[10].tolist() == [1, 1, 0, 0] and tiles[11:].tolist() == [[2, 0, 0, 0], [2, 1, 0, 0], [2, 2, 0, 0]]
    tiles, start = tile_table([(0, 0)])
    assert tiles.shape == (0, 4) and start.tolist() == [0, 0]


def test_refusals_of_the_python_surface():
    cfg = make_config('vpsde_qm9_uncond_jodo')
    sy = symbols('QM9')
    fn = E.get_geometry_fn(cfg, sy)
    assert fn.symbols is sy
    with pytest.raises(TypeError, match='GeometrySymbols'):
        E.get_geometry_fn(cfg, dataset_info('QM9'))
    with pytest.raises(ValueError, match='atom types'):
        E.get_geometry_fn(cfg, symbols('GeomDrug'))
    with pytest.raises(NotImplementedError, match='only_2D'):
        E.get_geometry_fn(make_config('vpsde_zinc_2d_jodo'), E.GeometrySymbols(['C'] * int(make_config('vpsde_zinc_2d_jodo').data.atom_types), [], [], []))
    pos, at, et, nd = torch.zeros(2, 3, 3), torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(2, 3, 3, dtype=torch.uint8), torch.ones(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        fn(pos, at, et, nd)
    with pytest.raises(TypeError, match='GPU tensor'):
        fn(pos.numpy(), at, et, nd)
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        E.compute_mmd(torch.zeros(3), torch.zeros(4))
    with pytest.raises(TypeError, match='1-D GPU tensor'):
        E.compute_mmd([0.1, 0.2], torch.zeros(4))
    with pytest.raises(ValueError, match='same, non-zero length'):
        E.compute_mmd_many([], [])
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        E.geometry_stat([(pos[0], at[0], et[0])], sy, device='cpu')
    with pytest.raises(TypeError, match='GeometrySymbols'):
        E.geometry_stat([(pos[0], at[0], et[0])], 'QM9')
    info = dataset_info('QM9')
    stat = {s: [1., 2., 3.] for s in sy.all_syms}
    with pytest.raises(ValueError, match='lacks the symbols C1H'):
        E.get_sub_geometry_metric({s: v for s, v in stat.items() if s != 'C1H'}, info)
    with pytest.raises(ValueError, match='max_samples'):
        E.get_sub_geometry_metric(stat, info, max_samples=0)
    metric = E.get_sub_geometry_metric(stat, info, device='cpu')
    assert metric.symbols.all_syms == sy.all_syms
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        metric([(pos[0], at[0], et[0])])


def test_get_sampling_fn_geometry_argument_checks():
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    from oracle.stubs import FixedNodes
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = 'cpu'
    cfg.sampling.steps = 2
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    inv = get_data_inverse_scaler(cfg)
    assert get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv).last_geometry is None
    assert get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv, geometry=None).last_geometry is None
    gfn = E.get_geometry_fn(cfg, symbols('QM9'))
    with pytest.raises(ValueError, match='fused device decode'):
        get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv, geometry=gfn, fused_decode=False)
    with pytest.raises(ValueError, match='fused device decode'):
        get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, lambda x: x, geometry=gfn)
    with pytest.raises(TypeError, match='get_geometry_fn'):
        get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv, geometry=symbols('QM9'))
    cfg2 = make_config('vpsde_zinc_2d_jodo')
    cfg2.device = 'cpu'
    with pytest.raises(NotImplementedError, match='3-D sampling path'):
        get_sampling_fn(cfg2, ns, FixedNodes([3, 4]), 2, 2, get_data_inverse_scaler(cfg2), geometry=gfn)
    assert get_sampling_fn(cfg, ns, FixedNodes([3, 4]), 2, 2, inv, geometry=gfn).last_geometry is None      # nothing before the first call

"""GPU: the geometry kernels (csrc/geometry_kernels.hip through jodo_amd.evaluation) against the values the reference's own functions
recorded (tests/golden/geometry_cases.npz) and the numpy oracle (tests/oracle_geometry.py).

Extraction.  Per-symbol counts are exact; values are compared as sorted multisets, dihedrals on the circle.  The tolerance per group is
4 x the largest distance from float64 of a float32 NUMPY evaluation of the same formulas on the same fixture molecules (the kernel's
operation order and atan2 differ from numpy's).  Measured on the fixture: float32 numpy 5.2e-7 A (lengths), 1.8e-5 degrees (angles),
1.8e-5 degrees (dihedrals); the kernel on an MI355X: 5.2e-7 A, 2.3e-5 degrees, 2.6e-5 degrees.

MMD.  The bound is 16 x the largest distance of the reference's own float32 result from its float64 result on the recorded cases
(6.8e-7, so 1.09e-5): the fast path raises one float32 exp to the 16th power.  Measured on an MI355X: fast path at most 6.4e-8 from the
reference's float64 value, general path (kernel_mul = 3) at most 1.2e-7, end to end (kernel-extracted float32 values) at most 7.6e-7."""
import numpy as np
import pytest
import torch

import oracle_geometry as OG
import oracle_stability as OS
from geometry_common import (DATASETS, MEANS, circle, dataset_info, fixture, mmd_bound, mmd_cases, processed_list, recorded,
                             recorded_lists, symbols)
from helpers import make_config, make_model
from jodo_amd import evaluation as E
from jodo_amd.capi import JodoHipError
from stability_common import pad_batch, rules

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_cache = {}


def _cfg(name):
    return make_config('vpsde_qm9_uncond_jodo' if name == 'QM9' else 'vpsde_geom_uncond_jodo')


def run(name, mols, N=None, junk=None, keep=None):
    pos, at, _, et, n = pad_batch(mols, N, junk)
    fn = E.get_geometry_fn(_cfg(name), symbols(name))
    up = lambda a: torch.from_numpy(a).to(DEV)
    res = fn(up(pos), up(at), up(et), up(n), keep=None if keep is None else up(np.asarray(keep, np.uint8)))
    torch.cuda.synchronize()
    return res


def f32_distance(name):
    """per group: the largest distance from the recorded float64 values of a float32 numpy evaluation of the same formulas"""
    if ('f32', name) not in _cache:
        sy, d = symbols(name), [0., 0., 0.]
        for m in recorded(name):
            if m['n'] == 0:
                continue
            got, _ = OG.extract(sy.classes, m['pos'], m['type'], m['edge'], np.float32)
            for c, (v, w) in enumerate(zip([np.asarray(v) for g in got for v in g], m['values'])):
                if len(w):
                    d[c // 8] = max(d[c // 8], float((np.abs(v - w) if c < 8 else circle(v, w)).max()))
        _cache['f32', name] = d
    return _cache['f32', name]


def multiset_distance(got, want, on_circle):
    """largest distance between two equally long value lists matched in sorted order (no recorded dihedral is within 1 degree of +-180,
    so no value can change ends of the sorted list)"""
    a, b = np.sort(np.asarray(got, np.float64)), np.sort(np.asarray(want, np.float64))
    return float((circle(a, b) if on_circle else np.abs(a - b)).max()) if len(a) else 0.


def compare(name, res, mols, keep=None, what=''):
    """counts exact, values within 4 x the float32 numpy distance of the group; returns the kernel's distances per group"""
    sy, want = symbols(name), recorded_lists(mols, keep)
    tol, seen = [4. * d for d in f32_distance(name)], [0., 0., 0.]
    for c, s in enumerate(sy.all_syms):
        v = res['values'][s]
        assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 1
        assert v.numel() == len(want[c]) == res['counts'][s], (what, s, v.numel(), len(want[c]))
        seen[c // 8] = max(seen[c // 8], multiset_distance(v.cpu().numpy(), want[c], c >= 16))
    print("%s %s: kernel distances %s, allowed %s" % (name, what, seen, tol))
    assert all(sn <= t for sn, t in zip(seen, tol)), (what, seen, tol)
    assert res['dropped'] == {'bond': 0, 'angle': 0, 'dihedral': 0}
    return seen


@pytest.mark.parametrize("N", [9, 29, 33, 65])
@pytest.mark.parametrize("name", DATASETS)
def test_extraction_equals_the_recorded_values(name, N):
    """batches of at most 8 recorded molecules padded to N (one adjacency word, its edge, two words, three words and four waves), the
    padding filled with junk; every molecule that fits is used"""
    fit = [m for m in recorded(name) if m['n'] <= N]
    assert len(fit) >= 8 and max(m['n'] for m in fit) == min(N, 29 if name == 'QM9' else 65)
    rng = np.random.default_rng(N)
    for b0 in range(0, len(fit), 8):
        mols = fit[b0:b0 + 8]
        res = run(name, mols, N, junk=rng)
        compare(name, res, mols, what='N=%d batch %d' % (N, b0 // 8))
        assert res['n_mols'] == sum(m['n'] > 0 for m in mols)


def test_special_molecules_one_by_one():
    """the multiplicity rules on the named molecules: an angle recorded twice, never, the rings, the hub, the aromatic code"""
    for name in DATASETS:
        by = {m['name']: m for m in recorded(name)}
        for tag in ('3-ring', '4-ring', 'degree-7', 'aromatic', '1-atom', '2-atom', 'empty', 'angle-twice', 'angle-never', 'random-asym'):
            compare(name, run(name, [by[tag]]), [by[tag]], what=tag)
    res = run('QM9', [{m['name']: m for m in recorded('QM9')}['angle-twice']])
    assert res['counts']['C1C-C1H'] == 2 and sum(res['counts'].values()) == 4


def test_determinism_keep_and_the_whole_set():
    for name in DATASETS:
        mols = recorded(name)
        a, b = run(name, mols), run(name, mols)
        compare(name, a, mols, what='whole set')
        for s in a['values']:
            assert torch.equal(a['values'][s], b['values'][s])                   # bit-identical, order included
        keep = [(k % 3) != 1 for k in range(len(mols))]
        kept = run(name, mols, keep=keep)
        compare(name, kept, mols, keep=keep, what='keep')
        assert kept['n_mols'] == sum(k and m['n'] > 0 for k, m in zip(keep, mols))
        only = run(name, [m for k, m in zip(keep, mols) if k])
        for s in kept['values']:
            assert torch.equal(kept['values'][s], only['values'][s])             # a masked molecule leaves no trace
        # the order inside a class is molecule order, then the reference's order inside the molecule
        want = recorded_lists(mols)
        sy = symbols(name)
        for c, s in enumerate(sy.all_syms):
            got = a['values'][s].cpu().numpy().astype(np.float64)
            assert (circle(got, want[c]) if c >= 8 else np.abs(got - want[c])).max() <= 4. * f32_distance(name)[c // 8]


def test_connected_mask_from_the_bond_rule():
    """the nearest available stand-in for the reference's filter: molecules of one fragment under the bond rule, as a keep mask"""
    mols = list(recorded('QM9')[:12])
    a, b = mols[0], mols[7]                                   # two recorded molecules as the two fragments of one (positions kept: only bonded atoms matter)
    edge = np.zeros((a['n'] + b['n'],) * 2, np.uint8)
    edge[:a['n'], :a['n']], edge[a['n']:, a['n']:] = a['edge'], b['edge']
    mols.insert(5, dict(name='two fragments', n=a['n'] + b['n'], pos=np.concatenate([a['pos'], b['pos']]),
                        type=np.concatenate([a['type'], b['type']]), edge=edge,
                        values=[np.concatenate([x, y]) for x, y in zip(a['values'], b['values'])]))
    pos, at, fc, et, n = pad_batch(mols)
    r = rules('QM9')
    stab = E.get_stability_fn(_cfg('QM9'), r, 'bonds')(*[_dev(a) for a in (pos, at, fc, et, n)])
    keep = E.connected_mask(stab)
    want = [m['n'] > 0 and OS.stability_bonds(r, m['type'], np.zeros(m['n'], np.int8), m['edge'])['fragments'] == 1 for m in mols]
    assert keep.dtype == torch.uint8 and keep.is_cuda and keep.cpu().tolist() == [int(w) for w in want] and sum(want) == len(mols) - 2
    res = E.get_geometry_fn(_cfg('QM9'), symbols('QM9'))(_dev(pos), _dev(at), _dev(et), _dev(n), keep=keep)
    compare('QM9', res, mols, keep=want, what='connected only')
    assert res['n_mols'] == sum(want) and not want[5]
    compare('QM9', run('QM9', mols), mols, what='every molecule')           # unmasked, the two-fragment molecule contributes


def test_complete_graph_k12_counts_and_dropped_values():
    """one dense junk molecule: 12 carbons, all 66 pairs single-bonded.  Bonds 66; angles: every bond (i < j) is a first bond at j with
    10 partners = 660; dihedrals: 66 central bonds x 10 x 10 = 6600 (the 3-rings with l == i's neighbour included).  Then the same with
    two atoms at one point: every value there is finite or dropped, and the sizes stay exact.  (Values of a junk molecule are not
    compared: near-collinear triples amplify float32 rounding without a bound that could be derived.)"""
    dec = ['H', 'C', 'N', 'O', 'F']
    sy = E.GeometrySymbols(dec, ['C1C'], ['C1C-C1C'], ['C1C-C1C-C1C'])
    fn = E.get_geometry_fn(make_config('vpsde_qm9_uncond_jodo'), sy)
    rng = np.random.default_rng(12)
    n, N = 12, 17
    pos = np.zeros((2, N, 3), np.float32)
    pos[:, :n] = rng.normal(0., 2., (n, 3)).astype(np.float32)
    pos[1, 5] = pos[1, 3]                                     # coincident atoms in the second copy
    at, et = np.ones((2, N), np.uint8), np.zeros((2, N, N), np.uint8)
    et[:, :n, :n] = 1 - np.eye(n, dtype=np.uint8)
    up = lambda a: torch.from_numpy(a).to(DEV)
    res = fn(up(pos), up(at), up(et), up(np.array([n, n], np.int32)), keep=up(np.array([1, 0], np.uint8)))
    assert res['counts'] == {'C1C': 66, 'C1C-C1C': 660, 'C1C-C1C-C1C': 6600} and res['dropped'] == {'bond': 0, 'angle': 0, 'dihedral': 0}
    for s in sy.all_syms:
        assert res['values'][s].numel() == res['counts'][s] and bool(torch.isfinite(res['values'][s]).all())
    both = fn(up(pos), up(at), up(et), up(np.array([n, n], np.int32)))
    want2, dropped2 = OG.extract(sy.classes, pos[1, :n], at[1, :n], et[1, :n, :n], np.float32)
    assert both['dropped']['bond'] == 0 and both['dropped']['angle'] == dropped2[1] > 0 and both['dropped']['dihedral'] > 0
    assert both['counts']['C1C'] == 132 and both['counts']['C1C-C1C'] == 1320 - both['dropped']['angle']
    assert both['counts']['C1C-C1C-C1C'] == 13200 - both['dropped']['dihedral']
    for s in sy.all_syms:
        assert both['values'][s].numel() == both['counts'][s] and bool(torch.isfinite(both['values'][s]).all())
        assert torch.equal(both['values'][s][:res['counts'][s]], res['values'][s])


def test_refusals_on_the_device():
    sy = symbols('QM9')
    fn = E.get_geometry_fn(_cfg('QM9'), sy)
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(JodoHipError, match='at most 256 atoms'):
        fn(z(1, 257, 3, dt=torch.float32), z(1, 257), z(1, 257, 257), z(1, dt=torch.int32))
    with pytest.raises(TypeError, match='torch.uint8'):
        fn(z(1, 4, 3, dt=torch.float32), z(1, 4, dt=torch.int64), z(1, 4, 4), z(1, dt=torch.int32))
    with pytest.raises(ValueError, match='keep is'):
        fn(z(2, 4, 3, dt=torch.float32), z(2, 4), z(2, 4, 4), z(2, dt=torch.int32), keep=z(3))
    with pytest.raises(ValueError, match='kernel_num'):
        E.compute_mmd(z(3, dt=torch.float32), z(3, dt=torch.float32), kernel_num=9)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_mmd_equals_the_reference_and_the_batched_call_the_single_calls():
    cases, bound = mmd_cases(), mmd_bound()
    single = [E.compute_mmd(_dev(c['source']), _dev(c['target']), batch_size=10000) for c in cases]
    many = E.compute_mmd_many([_dev(c['source']) for c in cases], [_dev(c['target']) for c in cases])
    again = E.compute_mmd_many([_dev(c['source']) for c in cases], [_dev(c['target']) for c in cases])
    worst = 0.
    for c, s, m, a in zip(cases, single, many, again):
        assert isinstance(s, float)
        if c['ns'] == 0:
            assert np.isnan(s) and np.isnan(m) and np.isnan(c['ref64'])
            continue
        assert np.float64(s).tobytes() == np.float64(m).tobytes() == np.float64(a).tobytes(), (c['ns'], c['nt'], c['family'])
        print("mmd %-8s (%4d, %4d): kernel - float64 %+.2e   reference float32 - float64 %+.2e" % (
            c['family'], c['ns'], c['nt'], s - c['ref64'], c['ref32'] - c['ref64']))
        worst = max(worst, abs(s - c['ref64']))
    print("fast path: worst %.3e, bound %.3e" % (worst, bound))
    assert worst <= bound
    three = [c for c in cases if c['ref3_64'] is not None]
    got3 = E.compute_mmd_many([_dev(c['source']) for c in three], [_dev(c['target']) for c in three], kernel_mul=3.0)
    worst3 = max(abs(g - c['ref3_64']) for g, c in zip(got3, three))
    print("general path (kernel_mul = 3): worst %.3e" % worst3)
    assert worst3 <= bound
    # the general path at kernel_mul = 2 is the same statistic as the fast path; other kernel counts and a fixed sigma against the oracle
    c = cases[4]                                              # (63, 257)
    assert (c['ns'], c['nt']) == (63, 257)
    for kw in (dict(kernel_num=4), dict(kernel_num=8), dict(fix_sigma=0.01), dict(kernel_mul=1.5, kernel_num=3)):
        got = E.compute_mmd(_dev(c['source']), _dev(c['target']), **kw)
        assert abs(got - OG.mmd(c['source'], c['target'], **kw)) <= bound, kw
    # all samples identical: a zero bandwidth, NaN as in the reference; float64 input is accepted
    assert np.isnan(E.compute_mmd(torch.full((5,), 1.25, device=DEV), torch.full((7,), 1.25, device=DEV)))
    assert E.compute_mmd(_dev(c['source'].astype(np.float64)), _dev(c['target'])) == single[4]


def test_subsampling():
    name = 'QM9'
    info, sy = dataset_info(name), symbols(name)
    rng = np.random.default_rng(77)
    stat = {s: (100. + 10. * rng.standard_normal(40)).tolist() for s in sy.all_syms}
    gen = {'values': {s: _dev((103. + 10. * rng.standard_normal(30)).astype(np.float32)) for s in sy.all_syms}}
    stat['C1H'] = (1.1 + 0.03 * rng.standard_normal(250)).tolist()
    gen['values']['C1H'] = _dev(np.unique((1.12 + 0.03 * rng.standard_normal(250)).astype(np.float32)))
    metric = E.get_sub_geometry_metric(stat, info, device=DEV, max_samples=100, seed=11)
    a = metric(gen)
    src, tgt = metric.last_samples['C1H']
    assert src.numel() == 100 and tgt.numel() == 100
    for side, full in ((src, gen['values']['C1H']), (tgt, _dev(np.asarray(stat['C1H'], np.float32)))):
        s = side.cpu().numpy()
        assert len(np.unique(s)) == min(100, len(np.unique(full.cpu().numpy()))) and np.isin(s, full.cpu().numpy()).all()
    assert abs(a['C1H'] - OG.mmd(src.cpu().numpy(), tgt.cpu().numpy())) <= mmd_bound()
    assert metric.last_samples['C1C'][0].numel() == 30 and metric.last_samples['C1C'][1].numel() == 40         # below the cap: untouched
    b = metric(gen)
    assert a == b                                             # the same seed: the same draw, the same bits
    c = E.get_sub_geometry_metric(stat, info, device=DEV, max_samples=100, seed=12)(gen)
    assert c['C1H'] != a['C1H'] and c['C1C'] == a['C1C']


@pytest.mark.parametrize("name", DATASETS)
def test_sub_geometry_metric_end_to_end(name):
    """generated = the even-numbered fixture molecules as a processed_list, target = geometry_stat of the odd-numbered ones; against the
    dict the reference's compute_geo_mmd recorded (float64), under the MMD bound; the device tuple and a geometry function's result give
    the same dict"""
    d = DATASETS.index(name)
    info, sy, mols = dataset_info(name), symbols(name), recorded(name)
    target = E.geometry_stat(processed_list(mols[1::2]), sy, DEV)
    want_t = recorded_lists(mols[1::2])
    assert list(target) == sy.all_syms and all(isinstance(v, list) and len(v) == len(w) for v, w in zip(target.values(), want_t))
    metric = E.get_sub_geometry_metric(target, info, device=DEV)
    got = metric(processed_list(mols[0::2]))
    keys = [k for g in range(3) for k in sy.syms[g] + [MEANS[g]]]
    assert list(got) == keys and all(isinstance(v, float) for v in got.values())
    ref64 = fixture()['e2e_%d_ref64' % d]
    err = np.abs(np.asarray([got[k] for k in keys]) - ref64)
    print("%s end to end: worst distance from the reference's float64 dict %.3e (its own float32: %.3e)" % (
        name, err.max(), np.abs(fixture()['e2e_%d_ref32' % d] - ref64).max()))
    assert err.max() <= mmd_bound()
    pos, at, _, et, n = pad_batch(mols[0::2])
    tup = tuple(_dev(a) for a in (pos, at, et, n))
    assert metric(tup) == got
    assert metric(E.get_geometry_fn(_cfg(name), sy)(*tup)) == got
    keep = np.ones(len(n), np.uint8)
    keep[-1] = 0                                              # a molecule that has values
    assert sum(len(v) for v in mols[0::2][-1]['values']) > 0
    less = metric(tup, keep=_dev(keep))
    assert less != got and less == metric(processed_list([m for k, m in zip(keep, mols[0::2]) if k]))
    # a pickled reference statistic is a dict of lists of Python floats: the recorded float64 values are accepted as they are
    ref_stat = {s: w.tolist() for s, w in zip(sy.all_syms, want_t)}
    again = E.get_sub_geometry_metric(ref_stat, info, device=DEV)(tup)
    assert max(abs(again[k] - got[k]) for k in keys) <= mmd_bound()
    # a symbol nobody generated: NaN, and the mean skips it
    few = metric(processed_list([{m['name']: m for m in mols}['2-atom']]))
    assert np.isnan(few['C1C']) and np.isfinite(few['C1H']) and few[MEANS[0]] == few['C1H'] and np.isnan(few[MEANS[2]])


def test_one_sampling_round_hands_the_decode_to_the_geometry_function():
    """get_sampling_fn(..., geometry=fn): a seeded-weight QM9 model, B = 4, 3 ancestral steps, two rounds; last_geometry is the function
    applied to each round's decode, concatenated, and its counts are the oracle's on the molecules the rounds returned.  The seeded
    weights decode carbons with double bonds only, so the symbols are chosen for them (the dataset's own would record nothing)."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    from oracle.stubs import FixedNodes
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = torch.device(DEV)
    cfg.sampling.steps = 3
    sy = E.GeometrySymbols(dataset_info('QM9')['atom_decoder'], ['C2C', 'C1C'], ['C2C-C2C', 'C2C-C1C'], ['C2C-C2C-C2C'])
    model = make_model(cfg, 8, DEV)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    n_nodes = [9, 17, 29, 12, 5, 23, 2, 14]
    gfn = E.get_geometry_fn(cfg, sy)
    fn = get_sampling_fn(cfg, ns, FixedNodes(n_nodes), 4, 8, get_data_inverse_scaler(cfg), return_raw=True, geometry=gfn)
    assert fn.last_geometry is None
    torch.manual_seed(3)
    mols = fn(model)
    assert [int(m[1].shape[0]) for m in mols] == n_nodes
    last = fn.last_geometry
    assert last['n_mols'] == 8 and list(last['values']) == sy.all_syms
    as_dict = lambda m: dict(n=int(m[1].shape[0]), pos=m[0].numpy(), type=m[1].numpy().astype(np.uint8), edge=m[2].numpy().astype(np.uint8))
    rounds = []
    for r in range(2):                                        # the function on the round's decode, rebuilt from what the round returned
        pos, at, _, et, n = pad_batch([as_dict(m) for m in mols[4 * r:4 * r + 4]])
        rounds.append(gfn(*[_dev(a) for a in (pos, at, et, n)]))
    for s in sy.all_syms:
        want = torch.cat([rounds[0]['values'][s], rounds[1]['values'][s]])
        assert torch.equal(last['values'][s], want) and last['counts'][s] == want.numel()
    assert last['dropped'] == {g: rounds[0]['dropped'][g] + rounds[1]['dropped'][g] for g in ('bond', 'angle', 'dihedral')}
    want, want_dropped = OG.extract_many(sy.classes, [as_dict(m) for m in mols], np.float32)
    per_group = [sum(last['counts'][s] for s in syms) for syms in sy.syms]
    print("two rounds: values per group %s, dropped %s" % (per_group, last['dropped']))
    assert min(per_group) > 0                                 # the comparison is not about empty lists
    assert [last['counts'][s] for s in sy.syms[0]] == [len(v) for v in want[0]]                # lengths are never dropped
    for g, name in enumerate(('bond', 'angle', 'dihedral')):  # what is enumerated does not depend on rounding; what is dropped may
        assert per_group[g] + last['dropped'][name] == sum(len(v) for v in want[g]) + want_dropped[g]
    metric = E.get_sub_geometry_metric({s: [1., 2., 3.] for s in sy.all_syms},
                                       dict(dataset_info('QM9'), top_bond_sym=sy.syms[0], top_angle_sym=sy.syms[1], top_dihedral_sym=sy.syms[2]),
                                       device=DEV)
    out = metric(last)                                        # ready for sub_geometry_metric
    assert set(out) == set(sy.all_syms) | set(MEANS)

"""The property prior on the host (jodo_amd/cond_gen/property_distribution.py): construction and reference-mode draws against what the
reference's own class recorded (tests/golden/prop_dist_cases.npz), the round trips, the numpy restatement of the device contract
(tests/prop_dist_common.py) and the refusals of get_sampling_fn(device_context=True) that need no GPU."""
import numpy as np
import pytest
import torch

import prop_dist_common as C
from helpers import make_config
from jodo_amd.cond_gen import DistributionProperty, compute_mean_mad


def _tables(d):
    sd = d.state_dict()
    return sd['probs'], torch.stack([sd['min'], sd['max']], -1), sd['atom_counts']


@pytest.fixture(scope='module')
def from_arrays():
    return C.golden_prior()


@pytest.fixture(scope='module')
def duck_typed():
    z = C.golden()
    prop2idx = {p: int(i) for p, i in zip(C.golden_names(), z['prop_ids'])}
    return DistributionProperty(C.StandInDataset(), prop2idx, num_bins=int(z['num_bins']), normalizer=C.golden_normalizer())


# ---- construction against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['from_arrays', 'duck_typed'])
def test_tables_equal_the_reference_bit_for_bit(which, request):
    """Probability rows and [min, max] of every (property, atom count), from both constructors, against the reference's class on the
    same inputs (property id 11 through sub_Cv_thermo); the atom count without a molecule has no entry."""
    d, z = request.getfixturevalue(which), C.golden()
    probs, minmax, counts = _tables(d)
    assert counts.tolist() == z['counts'].tolist() and 7 not in counts.tolist()
    assert torch.equal(probs, torch.from_numpy(z['probs']))
    assert torch.equal(minmax, torch.from_numpy(z['minmax']))
    assert d.properties == C.golden_names() and d.n_prop == 3 and d.num_bins == int(z['num_bins'])
    ref_layout = d.distributions
    assert sorted(ref_layout['gap'].keys()) == z['counts'].tolist() and 7 not in ref_layout['Cv']
    assert torch.equal(ref_layout['gap'][9]['probs'].probs, torch.from_numpy(z['probs'][1, 5]))
    assert float(ref_layout['gap'][9]['params'][1]) == float(z['minmax'][1, 5, 1])


def test_range_zero_slot_and_clamped_maximum(from_arrays):
    """The single molecule with 3 atoms: min == max, all weight in bin 0.  At 10 atoms several molecules tie at the maximum: the
    reference's `idx == n_bins` clamp puts them into the last bin — and the integer weights are the counts."""
    d, z = from_arrays, C.golden()
    sd = d.state_dict()
    K = d.num_bins
    s3, s10 = z['counts'].tolist().index(3), z['counts'].tolist().index(10)
    assert torch.equal(sd['min'][:, s3], sd['max'][:, s3])
    assert sd['weights'][:, s3, 0].tolist() == [1, 1, 1] and int(sd['weights'][:, s3].sum()) == 3
    vals = C.golden_values()[z['num_atoms'] == 10]
    tied = (vals == vals.max(0)).sum(0).tolist()              # the molecules AT the maximum: only the clamp puts them into a bin
    assert min(tied) >= 3 and sd['weights'][:, s10, K - 1].tolist() == tied
    per_count = np.bincount(z['num_atoms'], minlength=13)
    assert sd['weights'].sum(-1).tolist() == [[int(per_count[n]) for n in z['counts']]] * 3
    assert sd['weights'].dtype == torch.int64
    # a bin's probability is its count over the row's total (up to the reference's two float32 normalisations)
    want = sd['weights'].double() / sd['weights'].sum(-1, keepdim=True).double()
    assert float((sd['probs'].double() - want).abs().max()) < 1e-6
    assert bool(((sd['probs'] > 0) == (sd['weights'] > 0)).all())


# ---- reference-mode parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['from_arrays', 'duck_typed'])
def test_reference_mode_draws_equal_the_reference_bit_for_bit(which, request):
    """sample_batch on the recorded 64 atom counts under the two recorded torch.manual_seed values: the reference's bits (the same
    torch calls in the same order per molecule and property, the same float32 value expression and normalisation)."""
    d, z = request.getfixturevalue(which), C.golden()
    for k, seed in enumerate(z['sample_seeds']):
        torch.manual_seed(int(seed))
        got = d.sample_batch(torch.from_numpy(z['sample_counts']))
        assert got.shape == (64, 3) and got.dtype == torch.float32
        assert torch.equal(got, torch.from_numpy(z['samples'][k]))
    torch.manual_seed(int(z['sample_seeds'][0]))
    assert torch.equal(d.sample(int(z['sample_counts'][0])), torch.from_numpy(z['samples'][0, 0]))


def test_missing_atom_count_raises_key_error(from_arrays):
    with pytest.raises(KeyError):
        from_arrays.sample(7)
    with pytest.raises(KeyError):
        from_arrays.sample_batch([5, 7])
    with pytest.raises(KeyError) as e:
        from_arrays.slots_for(torch.tensor([5, 12, 40, 7]))
    assert e.value.args[0] == 40                              # the FIRST missing count is named
    with pytest.raises(KeyError):
        from_arrays.slots_for([-1])
    assert from_arrays.slots_for([3, 12, 8, 8]).tolist() == [0, 8, 4, 4]
    assert from_arrays.slots_for([]).shape == (0,)


def test_compute_mean_mad_equals_the_reference():
    z = C.golden()
    mean, mad = compute_mean_mad(torch.from_numpy(C.golden_values()))
    assert np.array_equal(mean.numpy(), z['mean_mad'][:, 0]) and np.array_equal(mad.numpy(), z['mean_mad'][:, 1])
    m1, d1 = compute_mean_mad(torch.from_numpy(C.golden_values()[:, 1].copy()))
    assert float(m1) == float(z['mean_mad'][1, 0]) and float(d1) == float(z['mean_mad'][1, 1])


# ---- round trips ---------------------------------------------------------------------------------------------------------------------
def _same_tables(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    ha, hb = a.host_tables(), b.host_tables()
    for k in ha:
        assert torch.equal(ha[k], hb[k]), k


def test_state_dict_round_trip(from_arrays, tmp_path):
    sd = from_arrays.state_dict()
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    torch.save(sd, tmp_path / 'prior.pt')
    loaded = torch.load(tmp_path / 'prior.pt', weights_only=True)
    other = C.table_prior([1, 2, 1], normalizer=None)
    other.load_state_dict(loaded)
    other.set_normalizer(C.golden_normalizer())
    _same_tables(from_arrays, other)
    assert other.properties == from_arrays.properties and other.num_bins == from_arrays.num_bins
    z = C.golden()
    torch.manual_seed(int(z['sample_seeds'][1]))
    assert torch.equal(other.sample_batch(z['sample_counts'].tolist()), torch.from_numpy(z['samples'][1]))
    fresh = DistributionProperty.from_state_dict(loaded, normalizer=C.golden_normalizer())
    _same_tables(from_arrays, fresh)


class _RefRow:
    def __init__(self, probs):
        self.probs = probs


class _RefLayout:
    """An object with the reference prior's attribute layout, as a pickled one carries it."""

    def __init__(self, probs, minmax, counts, names, normalizer):
        self.num_bins = probs.shape[-1]
        self.normalizer = normalizer
        self.distributions = {p: {int(n): {'probs': _RefRow(probs[i, s]), 'params': [minmax[i, s, 0], minmax[i, s, 1]]}
                                  for s, n in enumerate(counts)} for i, p in enumerate(names)}


def test_from_reference_preserves_the_tables(from_arrays):
    z = C.golden()
    obj = _RefLayout(torch.from_numpy(z['probs']), torch.from_numpy(z['minmax']), z['counts'], C.golden_names(), C.golden_normalizer())
    d = DistributionProperty.from_reference(obj)
    probs, minmax, counts = _tables(d)
    assert torch.equal(probs, torch.from_numpy(z['probs'])) and torch.equal(minmax, torch.from_numpy(z['minmax']))
    assert counts.tolist() == z['counts'].tolist() and d.properties == C.golden_names() and d.num_bins == int(z['num_bins'])
    for k, seed in enumerate(z['sample_seeds']):              # its reference-mode draws are the object's
        torch.manual_seed(int(seed))
        assert torch.equal(d.sample_batch(z['sample_counts'].tolist()), torch.from_numpy(z['samples'][k]))
    # quantised weights: rint(p * 2^30), every non-zero bin non-zero, no zero bin gains weight, totals inside (0, 2^31)
    w = d.state_dict()['weights']
    assert bool(((w > 0) == (probs > 0)).all())
    assert torch.equal(w, torch.round(probs.double() * 2 ** 30).long().clamp_(min=0) + ((probs > 0) & (torch.round(probs.double() * 2 ** 30) == 0)))
    assert int(w.sum(-1).min()) > 0 and int(w.sum(-1).max()) < 2 ** 31
    # and of one of these: the same tables again
    again = DistributionProperty.from_reference(from_arrays)
    assert torch.equal(_tables(again)[0], probs) and torch.equal(_tables(again)[1], minmax)


def test_quantised_weights_keep_tiny_probabilities():
    probs = torch.tensor([[[1.0 - 3e-10, 1e-10, 0.0, 2e-10]]])
    obj = _RefLayout(probs, torch.tensor([[[0.0, 1.0]]]), [5], ['p'], None)
    w = DistributionProperty.from_reference(obj).state_dict()['weights'][0, 0]
    assert w.tolist() == [2 ** 30, 1, 0, 1]


# ---- the restatement of the device contract ------------------------------------------------------------------------------------------
SEED, COUNTS, DRAWS = (1 << 40) + 7, [5, 0, 1, 10, 0, 0, 3, 1], 200000


@pytest.fixture(scope='module')
def restated_draws():
    d = C.table_prior(COUNTS, n_prop=2)
    tables = d.host_tables()
    out, idx = C.restate(tables, np.zeros(DRAWS, np.int64), seed=SEED, return_bins=True)
    u2 = (C.philox_words(SEED, C.global_indices(DRAWS), 2)[..., 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return out, idx, u2


def test_restatement_bin_frequencies(restated_draws):
    """Zero-count bins are never selected; every other bin's frequency lies within 4 binomial standard deviations of its probability."""
    _, idx, _ = restated_draws
    T = float(sum(COUNTS))
    for col in range(2):
        hist = np.bincount(idx[:, col], minlength=len(COUNTS))
        worst = 0.0
        for k, c in enumerate(COUNTS):
            if c == 0:
                assert hist[k] == 0
                continue
            p = c / T
            dev = abs(hist[k] - DRAWS * p) / np.sqrt(DRAWS * p * (1 - p))
            worst = max(worst, dev)
            assert dev <= 4.0, "column %d bin %d: %.2f standard deviations" % (col, k, dev)
        print("column %d: worst bin at %.2f standard deviations" % (col, worst))


def test_restatement_u2_mean_and_value_range(restated_draws):
    """u2 is uniform on the 2^24 grid of [0, 1): its mean lies within 4 standard errors of 0.5 - 2^-25; every value lies inside the
    range of its bin, hence inside [min, max]."""
    out, idx, u2 = restated_draws
    se = np.sqrt(1.0 / 12.0 / DRAWS)
    for col in range(2):
        dev = abs(u2[:, col].mean() - (0.5 - 2.0 ** -25)) / se
        print("column %d: u2 mean at %.2f standard errors" % (col, dev))
        assert dev <= 4.0
    lo, hi, K = -1.5, 2.25, len(COUNTS)
    width = (hi - lo) / K
    assert bool(np.all(out >= lo + idx * width - 1e-5)) and bool(np.all(out <= lo + (idx + 1) * width + 1e-5))


def test_restatement_extreme_draws_and_boundaries():
    """a = 0 selects the first non-zero bin, a = 2^24 - 1 the last; at every cumulative boundary c the two a values either side of
    r = c select the bin below and the next non-zero bin above."""
    d = C.table_prior(COUNTS)
    tables = d.host_tables()
    T = sum(COUNTS)

    def bins(a_values):
        words = np.zeros((len(a_values), 1, 2), np.int64)
        words[:, 0, 0] = np.asarray(a_values, np.int64) << 8
        return C.restate(tables, np.zeros(len(a_values), np.int64), words=words, return_bins=True)[1][:, 0].tolist()

    assert bins([0, 2 ** 24 - 1]) == [0, 7]
    cum = np.cumsum(COUNTS)
    for c in sorted(set(cum.tolist()) - {T}):
        a_hi = -(-(c << 24) // T)                              # the smallest a with (a * T) >> 24 >= c
        assert (a_hi * T) >> 24 == c and ((a_hi - 1) * T) >> 24 == c - 1
        below, above = bins([a_hi - 1, a_hi])
        assert below == int(np.searchsorted(cum, c - 1, side='right')) and above == int(np.searchsorted(cum, c, side='right'))
        assert COUNTS[below] > 0 and COUNTS[above] > 0 and above > below


# ---- wiring on the CPU ---------------------------------------------------------------------------------------------------------------
def test_device_context_refusals_on_the_cpu(from_arrays):
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models.node_distribution import DistributionNodes
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.device = torch.device('cpu')
    ns, inv, nodes = NoiseScheduleVP(cfg.sde.schedule), get_data_inverse_scaler(cfg), DistributionNodes({4: 1, 5: 2, 9: 1})
    prior = C.golden_prior(properties=['alpha'])
    with pytest.raises(ValueError, match='GPU'):
        get_sampling_fn(cfg, ns, nodes, 6, 12, inv, prop_dist=prior, device_context=True)

    class NoDevice:
        def sample_batch(self, n_nodes):
            return torch.zeros(len(n_nodes), 1)

    for device in ('cpu', 'cuda:0'):
        cfg.device = torch.device(device)
        with pytest.raises(ValueError, match='sample_batch_device'):
            get_sampling_fn(cfg, ns, nodes, 6, 12, inv, prop_dist=NoDevice(), device_context=True)
        with pytest.raises(ValueError, match='prop_dist'):
            get_sampling_fn(cfg, ns, nodes, 6, 12, inv, prop_dist=None, device_context=True)
    with pytest.raises(ValueError, match='parity'):
        get_sampling_fn(cfg, ns, nodes, 6, 12, inv, prop_dist=prior, device_context=True, shard=(0, 2), shard_mode='parity')
    with pytest.raises(ValueError, match='no CPU fallback'):
        prior.sample_batch_device([4, 5], 'cpu', seed=1)
    # off by default without a shard, and building the function draws nothing
    cfg.device = torch.device('cpu')
    state = torch.get_rng_state()
    fn = get_sampling_fn(cfg, ns, nodes, 6, 12, inv, prop_dist=prior)
    assert torch.equal(torch.get_rng_state(), state) and fn.last_context == [] and fn.device_context is False


def test_device_context_default(from_arrays):
    """None resolves to on exactly for a perf shard with a prior that has the device draw on a GPU config.device; a CPU device, a parity
    shard, no shard, a prior without the method or no prior leave it off."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models.node_distribution import DistributionNodes
    from jodo_amd.sampling import get_sampling_fn
    from jodo_amd.utils import get_data_inverse_scaler
    cfg = make_config('vpsde_qm9_cond_jodo')
    ns, inv, nodes = NoiseScheduleVP(cfg.sde.schedule), get_data_inverse_scaler(cfg), DistributionNodes({4: 1, 5: 2, 9: 1})
    prior = C.golden_prior(properties=['alpha'])

    class NoDevice:
        def sample_batch(self, n_nodes):
            return torch.zeros(len(n_nodes), 1)

    def resolved(device, prop_dist, **kw):
        cfg.device = torch.device(device)
        return get_sampling_fn(cfg, ns, nodes, 6, 12, inv, prop_dist=prop_dist, **kw).device_context

    assert resolved('cuda:0', prior, shard=(0, 2)) is True and resolved('cuda:0', prior, shard=(1, 2), shard_assign='lpt') is True
    assert resolved('cpu', prior, shard=(0, 2)) is False                      # a CPU device keeps the host draw
    assert resolved('cuda:0', prior, shard=(0, 2), shard_mode='parity') is False
    assert resolved('cuda:0', prior) is False
    assert resolved('cuda:0', NoDevice(), shard=(0, 2)) is False and resolved('cuda:0', None, shard=(0, 2)) is False
    assert resolved('cuda:0', prior, shard=(0, 2), device_context=False) is False and resolved('cuda:0', prior, device_context=True) is True

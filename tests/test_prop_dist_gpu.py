"""The property prior on the device: jodo_prop_sample (csrc/sampler_kernels.hip) against the numpy restatement of its contract
(tests/prop_dist_common.py) bit for bit, its batch independence, the table cache, the host entry's refusals, and
get_sampling_fn(device_context=True) unsharded and sharded."""

import numpy as np
import pytest
import torch

import prop_dist_common as C
from helpers import make_config, make_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = (1 << 40) + 7                                          # above 2^32: both key words matter
COUNTS8 = [5, 0, 1, 10, 0, 0, 3, 1]


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _poisoned(B, P):
    return torch.full((B, P), float('nan'), device=DEV)


def _draw(prior, counts, **kw):
    """sample_batch_device into a poisoned buffer: through the wrapper, with the prior's cached tables."""
    from jodo_amd import fused
    tables = prior.device_tables(DEV)
    out = _poisoned(len(counts), prior.n_prop)
    got = fused.prop_sample(tables, prior.slots_for(counts), kw.pop('seed', SEED), out=out, **kw)
    assert got is out
    return got


def _one_slot_counts(n_bins):
    if n_bins == 1:
        return [4]
    if n_bins == 7:
        return [2, 0, 3, 1, 0, 0, 5]
    g = np.random.default_rng(3)
    c = g.integers(0, 4, n_bins) * (g.random(n_bins) < 0.3)
    c[0], c[-1] = 2, 1
    return c.tolist()


@pytest.fixture(scope='module')
def priors():
    """Per (n_prop, n_bins): a one-slot prior (atom count 1) and the golden one (9 atom counts of 3 .. 12, none for 7)."""
    names = C.golden_names()
    out = {}
    for P in (1, 2, 3):
        for K in (1, 7, 1000):
            norm = {p: C.golden_normalizer()[p] for p in names[:P]}
            out[P, K] = (C.table_prior(_one_slot_counts(K), n_prop=P), C.golden_prior(properties=names[:P], num_bins=K))
            out[P, K][1].set_normalizer(norm)
    return out


@pytest.mark.parametrize('n_prop', [1, 2, 3])
@pytest.mark.parametrize('n_bins', [1, 7, 1000])
def test_kernel_equals_the_restatement(priors, n_prop, n_bins):
    """Bit for bit, on poisoned output buffers: one slot and the golden prior's nine, every batch size around the 64-wide wave and the
    256-wide block, a seed above 2^32, first_index just below 2^32 (the counter's high word changes inside the batch) and explicit
    shuffled indices."""
    one, ten = priors[n_prop, n_bins]
    g = np.random.default_rng(n_prop * 7 + n_bins)
    avail = ten.state_dict()['atom_counts'].numpy()
    for B in (1, 63, 64, 65, 257, 1000):
        for prior, counts in ((one, np.ones(B, np.int64)), (ten, avail[g.integers(0, len(avail), B)])):
            tables, slots = prior.host_tables(), prior.slots_for(counts).numpy()
            first = (1 << 32) - 30
            shuffled = g.permutation(B + 5)[:B] + (1 << 33)
            for kw in (dict(), dict(first_index=first), dict(indices=shuffled.tolist())):
                got = _draw(prior, counts, **kw)
                want = C.restate(tables, slots, seed=SEED, **kw)
                assert got.shape == (B, n_prop) and np.array_equal(_bits(got), want.view(np.uint32)), (B, kw.keys())
    with pytest.raises(KeyError) as e:
        ten.sample_batch_device([5, 7, 8], DEV, seed=1)
    assert e.value.args[0] == 7


def test_public_call_equals_the_restatement(priors):
    """sample_batch_device itself (fresh output, no normalizer -> mean 0, mad 1), from a list and from a CPU tensor."""
    prior = C.golden_prior(normalizer=False)
    counts = [3, 12, 9, 9, 4, 10, 3]
    want = C.restate(prior.host_tables(), prior.slots_for(counts).numpy(), seed=5, first_index=11)
    assert prior.host_tables()['norm'].tolist() == [[0.0, 1.0]] * 3
    for n in (counts, torch.tensor(counts)):
        got = prior.sample_batch_device(n, DEV, seed=5, first_index=11)
        assert got.device == torch.device(DEV) and got.dtype == torch.float32
        assert np.array_equal(_bits(got), want.view(np.uint32))
    assert prior.sample_batch_device([], DEV, seed=5).shape == (0, 3)
    mn, mx = prior.host_tables()['minmax'][:, 0, 0], prior.host_tables()['minmax'][:, 0, 1]
    three = prior.sample_batch_device([3] * 50, DEV, seed=9).cpu()          # the range-0 slot: every draw is the one value
    assert torch.equal(mn, mx) and bool((three == mn).all())


def test_injected_words():
    """The test form: a and u2 from a words tensor.  a in {0, 2^24 - 1}; at every cumulative boundary c of the 8-bin table the two a
    values either side of r = c; the bins are the restatement's and never one of weight zero.  u2 in {0, 1 - 2^-24} on the range-0 slot
    and on an ordinary one."""
    prior = C.table_prior(COUNTS8)
    tables = prior.host_tables()
    T, cum = sum(COUNTS8), np.cumsum(COUNTS8)
    a_values = [0, 2 ** 24 - 1]
    for c in sorted(set(cum.tolist()) - {T}):
        a_hi = -(-(c << 24) // T)
        assert (a_hi * T) >> 24 == c and ((a_hi - 1) * T) >> 24 == c - 1
        a_values += [a_hi - 1, a_hi]
    words = np.zeros((len(a_values), 1, 2), np.int64)
    words[:, 0, 0] = (np.asarray(a_values, np.int64) << 8) | 0xA5        # the low 8 bits are not part of a
    words[:, 0, 1] = 0x7FFFFF00
    counts = np.ones(len(a_values), np.int64)
    want, bins = C.restate(tables, prior.slots_for(counts).numpy(), words=words, return_bins=True)
    got = _draw(prior, counts, words=torch.from_numpy(words))
    assert np.array_equal(_bits(got), want.view(np.uint32))
    assert bins[:2, 0].tolist() == [0, 7] and all(COUNTS8[b] > 0 for b in bins[:, 0])
    lo, hi = -1.5, 2.25
    width = (hi - lo) / 8
    assert bool(np.all(got.cpu().numpy()[:, 0] >= lo + bins[:, 0] * width - 1e-5))
    assert bool(np.all(got.cpu().numpy()[:, 0] <= lo + (bins[:, 0] + 1) * width + 1e-5))
    # u2 at both ends, on the range-0 slot (3 atoms) and an ordinary one (9 atoms) of the golden prior
    golden = C.golden_prior()
    counts = np.array([3, 3, 9, 9])
    w = np.zeros((4, 3, 2), np.int64)
    w[..., 0] = np.array([0x12345600, 0xFFFFFF00, 0x80000000])[None, :]
    w[0::2, :, 1], w[1::2, :, 1] = 0, 0xFFFFFFFF
    want = C.restate(golden.host_tables(), golden.slots_for(counts).numpy(), words=w)
    got = _draw(golden, counts, words=torch.from_numpy(w))
    assert np.array_equal(_bits(got), want.view(np.uint32))
    assert np.array_equal(want[0], want[1]) and not np.array_equal(want[2], want[3])


def test_batch_independence(priors):
    """1000 molecules in one call = the same molecules in calls of 1, 7 and 992 = two disjoint `indices` halves put back together."""
    prior = priors[2, 1000][1]
    g = np.random.default_rng(11)
    avail = prior.state_dict()['atom_counts'].numpy()
    counts = avail[g.integers(0, len(avail), 1000)]
    first = 123456789
    whole = prior.sample_batch_device(counts, DEV, seed=SEED, first_index=first)
    parts, at = [], 0
    for n in (1, 7, 992):
        parts.append(prior.sample_batch_device(counts[at:at + n], DEV, seed=SEED, first_index=first + at))
        at += n
    assert torch.equal(torch.cat(parts), whole)
    perm = g.permutation(1000)
    halves = torch.empty_like(whole)
    for sel in (perm[:500], perm[500:]):
        halves[torch.from_numpy(sel).to(DEV)] = prior.sample_batch_device(counts[sel], DEV, seed=SEED, indices=(sel + first).tolist())
    assert torch.equal(halves, whole)
    assert not torch.equal(prior.sample_batch_device(counts, DEV, seed=SEED + 1, first_index=first), whole)


def test_table_cache_and_normalizer():
    """The tables go to the device once; set_normalizer and load_state_dict invalidate them, and the next call's output is the
    restatement's with the new tables."""
    from jodo_amd import fused
    prior = C.golden_prior(properties=['alpha', 'gap'], normalizer=False)
    counts = [4, 9, 12, 3, 9]
    slots = prior.slots_for(counts).numpy()
    n0 = fused.PropTables.uploads
    a = prior.sample_batch_device(counts, DEV, seed=3)
    assert fused.PropTables.uploads == n0 + 1
    b = prior.sample_batch_device(counts, DEV, seed=3)
    c = prior.sample_batch_device(counts[:2], DEV, seed=4, indices=[9, 1])
    assert fused.PropTables.uploads == n0 + 1 and torch.equal(a, b) and c.shape == (2, 2)
    assert np.array_equal(_bits(a), C.restate(prior.host_tables(), slots, seed=3).view(np.uint32))
    prior.set_normalizer({'alpha': {'mean': torch.tensor(75.25), 'mad': torch.tensor(6.5)}, 'gap': {'mean': 0.25, 'mad': 0.04}})
    d = prior.sample_batch_device(counts, DEV, seed=3)
    assert fused.PropTables.uploads == n0 + 2 and not torch.equal(a, d)
    assert prior.host_tables()['norm'].tolist() == [[75.25, 6.5], [0.25, float(np.float32(0.04))]]
    assert np.array_equal(_bits(d), C.restate(prior.host_tables(), slots, seed=3).view(np.uint32))
    other = C.table_prior(COUNTS8, n_slots=12, n_prop=2)
    prior.load_state_dict(other.state_dict())                # (the properties are the loaded prior's: p0, p1)
    prior.set_normalizer({'p0': {'mean': 0.5, 'mad': 2.0}, 'p1': {'mean': -1.0, 'mad': 0.75}})
    e = prior.sample_batch_device(counts, DEV, seed=3)
    assert fused.PropTables.uploads == n0 + 3
    assert np.array_equal(_bits(e), C.restate(prior.host_tables(), prior.slots_for(counts).numpy(), seed=3).view(np.uint32))


def test_host_entry_refusals():
    """A slot outside the table, more than 16 properties, more than 65 536 bins: refused by the host entry (nothing is launched: the
    poisoned output stays as it was)."""
    from jodo_amd import capi, fused
    L = capi.lib()
    prior = C.table_prior(COUNTS8, n_slots=2)
    t = prior.device_tables(DEV)
    out = _poisoned(3, 1)
    stream = capi.current_stream_ptr()

    def call(n_prop, n_bins, n_slots, slots):
        s = torch.tensor(slots, dtype=torch.int32)
        s_dev = s.clamp(0, 1).to(DEV)
        return L.jodo_prop_sample(len(slots), n_prop, n_bins, n_slots, capi.ptr(t.cum), capi.ptr(t.minmax), capi.ptr(t.norm), capi.ptr(s),
                                  capi.ptr(s_dev), None, 0, 1, None, capi.ptr(out), stream)

    assert call(1, 8, 2, [0, 2, 1]) == -1 and b'slot' in L.jodo_last_error()            # JODO_ERR_ARG
    assert call(1, 8, 2, [0, -1, 1]) == -1
    assert call(17, 8, 2, [0, 1, 1]) == -3 and call(1, 65537, 2, [0, 1, 1]) == -3       # JODO_ERR_UNSUPPORTED
    assert call(1, 0, 2, [0, 1, 1]) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(capi.JodoHipError):
        fused.prop_sample(t, torch.tensor([0, 5], dtype=torch.int32), 1)
    assert call(1, 8, 2, [0, 1, 1]) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ---- the public entry ----------------------------------------------------------------------------------------------------------------
class _ConstantContext:
    """A prior stand-in that draws nothing."""

    def sample_batch(self, n_nodes):
        return torch.zeros(len(n_nodes), 1)


@pytest.fixture(scope='module')
def entry():
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models.node_distribution import DistributionNodes
    from jodo_amd.utils import get_data_inverse_scaler
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.device = torch.device(DEV)
    cfg.sampling.steps, cfg.sampling.method = 4, 'fast'
    cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = 'singlestep_fixed', 2
    model = make_model(cfg, 12, DEV, head_gain=10.0)
    return dict(cfg=cfg, model=model, ns=NoiseScheduleVP(cfg.sde.schedule), inv=get_data_inverse_scaler(cfg),
                nodes=DistributionNodes({4: 1, 5: 2, 9: 1}), prior=C.golden_prior(properties=['alpha']))


def _sampling_fn(entry, prop_dist, **kw):
    from jodo_amd.sampling import get_sampling_fn
    return get_sampling_fn(entry['cfg'], entry['ns'], entry['nodes'], 6, 12, entry['inv'], prop_dist=prop_dist, return_raw=True, **kw)


def test_device_context_through_get_sampling_fn(entry):
    """Unsharded device_context=True: last_context is the prior's sample_batch_device for global indices 0 .. 11 under the run's key.
    Shards (0, 2) and (1, 2) under both assignments (device_context on by default there): every global index gets the unsharded
    run's context.  The sampled molecules come back; the network is not judged here."""
    from jodo_amd.fused import PROP_CONTEXT_TAG, mix64
    prior = entry['prior']
    torch.manual_seed(77)
    fn = _sampling_fn(entry, prior, device_context=True, seed=77)
    mols = fn(entry['model'])
    n_nodes = [int(m[0].shape[0]) for m in mols]
    assert len(mols) == 12 and set(n_nodes) <= {4, 5, 9} and fn.last_indices == list(range(12))
    assert len(fn.last_context) == 2 and all(c.shape == (6, 1) and c.device == torch.device(DEV) for c in fn.last_context)
    unsharded = torch.cat(fn.last_context)
    want = prior.sample_batch_device(n_nodes, DEV, seed=mix64(77, PROP_CONTEXT_TAG), indices=range(12))
    assert torch.equal(unsharded, want)
    assert np.array_equal(_bits(want), C.restate(prior.host_tables(), prior.slots_for(n_nodes).numpy(), seed=mix64(77, PROP_CONTEXT_TAG)).view(np.uint32))
    for assign in ('contiguous', 'lpt'):
        seen = []
        for rank in (0, 1):
            fn = _sampling_fn(entry, prior, shard=(rank, 2), shard_assign=assign, seed=77)
            part = fn(entry['model'])
            assert len(part) == len(fn.last_indices) > 0 and [int(m[0].shape[0]) for m in part] == [n_nodes[i] for i in fn.last_indices]
            assert torch.equal(torch.cat(fn.last_context), unsharded[torch.tensor(fn.last_indices, device=DEV)])
            seen += fn.last_indices
        assert sorted(seen) == list(range(12))


def test_device_context_off_consumes_the_generator(entry):
    """Off (the default without a shard), the prior's reference-mode draw runs on torch's CPU generator: the contexts are
    sample_batch's under the same seed, and the generator ends elsewhere than after a run whose prior draws nothing — where the
    device_context=True run ends, which leaves the generator to the atom counts alone."""
    prior = entry['prior']

    def run(prop_dist, **kw):
        torch.manual_seed(77)
        fn = _sampling_fn(entry, prop_dist, seed=77, **kw)
        mols = fn(entry['model'])
        return fn, mols, torch.get_rng_state()

    fn_off, mols_off, state_off = run(prior)
    fn_none, _, state_none = run(_ConstantContext())
    fn_on, _, state_on = run(prior, device_context=True)
    assert not torch.equal(state_off, state_none) and torch.equal(state_on, state_none)
    torch.manual_seed(77)
    n_nodes = entry['nodes'].sample(12)
    assert [int(m[0].shape[0]) for m in mols_off] == n_nodes.tolist()
    for r in range(2):
        assert torch.equal(fn_off.last_context[r].cpu(), prior.sample_batch(n_nodes[6 * r:6 * r + 6]))
    assert bool((torch.cat(fn_none.last_context) == 0).all()) and not torch.equal(torch.cat(fn_on.last_context), torch.cat(fn_off.last_context))

"""The property prior of conditional generation: p(property | atom count) as one histogram per (property, atom count), the class the
reference keeps in cond_gen/property_distribution.py (`DistributionProperty`) and hands to its sampling functions as `prop_dist`.

Two ways to draw from it:
  reference mode  `sample` / `sample_batch`: on the CPU, consuming torch's global generator exactly as the reference does — per molecule
                  and property one `torch.multinomial` over the bin probabilities (what `Categorical.sample((1,))` calls) and one
                  `torch.rand(1)`, then the reference's float32 bin -> value expression.  Under one `torch.manual_seed` the values are
                  the reference's, bit for bit.  Every existing call site (`prop_dist.sample_batch(n_nodes)`) gets this.
  device mode     `sample_batch_device`: one HIP kernel for the whole batch (jodo_prop_sample, include/jodo_hip.h): counter-based
                  Philox draws keyed by (seed, global molecule index, property column), an integer inverse-CDF search and the same
                  float32 value expression.  Same distribution, not the reference's stream; a molecule's targets depend only on
                  (seed, global index, atom count, the prior) — not on the batch, the rank or the round.  No CPU fallback.

Construction needs no dataset object (`from_arrays`), takes a reference prior as it is (`from_reference`, e.g. an unpickled one) and
round-trips through plain tensors (`state_dict` / `load_state_dict`); the reference's duck-typed constructor is kept.  Binning is
vectorised over all molecules; the bin of a value is the reference's float32 expression, so the tables are the reference's.
"""
import torch

_QUANT = 1 << 30                    # weight of probability 1 when a prior is built from probabilities instead of counts


def compute_mean_mad(values):
    """The array form of the reference's compute_mean_mad_from_dataset (cond_gen/utils.py:4-12): (mean, mean absolute deviation from it)
    of a 1-D tensor of property values, as 0-dim tensors; a 2-D [M, n_prop] tensor gives one pair of [n_prop] tensors (column by column)."""
    values = torch.as_tensor(values)
    if values.dim() == 2:
        pairs = [compute_mean_mad(values[:, k].contiguous()) for k in range(values.shape[1])]
        return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    mean = torch.mean(values)
    mad = torch.mean(torch.abs(values - mean))
    return mean, mad


class _Row:
    """One entry's 'probs' in the reference's `distributions` layout: `.probs` (the normalised bin probabilities) and `.sample`."""

    def __init__(self, probs):
        self.probs = probs

    def sample(self, sample_shape=(1,)):
        shape = torch.Size(sample_shape)
        return torch.multinomial(self.probs.reshape(-1, self.probs.shape[-1]), shape.numel(), True).T.reshape(shape)


class DistributionProperty:
    """cond_gen/property_distribution.py: `DistributionProperty(dataset, prop2idx, num_bins=1000, normalizer=None)`.

    dataset is duck-typed on what the reference touches: `indices()`, `get(i)` returning an object with `.y[0][prop_id]` and
    `.num_atom`, and `sub_Cv_thermo(data)` for property id 11.  prop2idx: {property name: column of y}, in context-column order.
    normalizer: {property name: {'mean': ..., 'mad': ...}} (set_normalizer sets it later, as the reference's callers do)."""

    def __init__(self, dataset, prop2idx, num_bins=1000, normalizer=None):
        properties = list(prop2idx.keys())
        prop_ids = [int(v) for v in prop2idx.values()]
        indices = dataset.indices()
        num_atoms, rows = [], []
        for k in range(len(indices)):                         # one pass over the dataset's own accessors; the binning below is vectorised
            data = dataset.get(indices[k])
            rows.append(torch.cat([(dataset.sub_Cv_thermo(data) if pid == 11 else data.y[0][pid]).reshape(1) for pid in prop_ids]))
            num_atoms.append(data.num_atom)
        self._init(properties, num_bins, normalizer)
        self._build(torch.cat(num_atoms), torch.stack(rows))

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, num_atoms, values, properties, num_bins=1000, normalizer=None):
        """num_atoms: [M] integers; values: [M, n_prop] floats (column k = property properties[k]).  No dataset object."""
        self = cls.__new__(cls)
        self._init(list(properties), num_bins, normalizer)
        self._build(torch.as_tensor(num_atoms), torch.as_tensor(values))
        return self

    @classmethod
    def from_reference(cls, obj):
        """A prior in the reference's layout (the reference's own object, e.g. unpickled, or one of these): reads
        `obj.distributions[prop][n]['probs'].probs` and `['params']`, `obj.num_bins` and `obj.normalizer`.  The reference-mode draws of
        the result are the object's; the device tables quantise each probability to rint(p * 2^30), at least 1 where p > 0."""
        properties = list(obj.distributions.keys())
        if not properties:
            raise ValueError("from_reference: the prior has no property")
        counts = sorted(int(n) for n in obj.distributions[properties[0]].keys())
        if not counts:
            raise ValueError("from_reference: the prior has no atom count")
        rows, mn, mx = [], [], []
        for prop in properties:
            d = obj.distributions[prop]
            if sorted(int(n) for n in d.keys()) != counts:
                raise ValueError("from_reference: property %r covers other atom counts than %r" % (prop, properties[0]))
            rows.append(torch.stack([torch.as_tensor(d[n]['probs'].probs, dtype=torch.float32).reshape(-1) for n in counts]))
            mn.append(torch.stack([torch.as_tensor(d[n]['params'][0], dtype=torch.float32).reshape(()) for n in counts]))
            mx.append(torch.stack([torch.as_tensor(d[n]['params'][1], dtype=torch.float32).reshape(()) for n in counts]))
        probs = torch.stack(rows)
        self = cls.__new__(cls)
        self._init(properties, int(probs.shape[-1]), getattr(obj, 'normalizer', None))
        w = torch.round(probs.double() * _QUANT).long()
        w = torch.where((probs > 0) & (w == 0), torch.ones_like(w), w)
        self._set_tables(torch.tensor(counts, dtype=torch.long), w, torch.stack(mn), torch.stack(mx), probs)
        return self

    def _init(self, properties, num_bins, normalizer):
        self.properties = list(properties)
        self.n_prop = len(self.properties)
        self.num_bins = int(num_bins)
        if self.n_prop < 1 or self.num_bins < 1:
            raise ValueError("DistributionProperty needs at least one property and one bin")
        self._normalizer = normalizer
        self._device_tables = {}

    def _build(self, num_atoms, values):
        """Histograms of all (property, atom count) pairs in one pass.  The bin of a value is the reference's float32 expression
        (:50-58): ((v - min) / (max - min + 1e-12) * n_bins).long(), n_bins moved to n_bins - 1, with min / max per atom count and
        property; here evaluated for all molecules at once (the same elementwise float32 operations)."""
        num_atoms = num_atoms.reshape(-1).long().cpu()
        values = values.to(torch.float32).cpu()
        P, K = self.n_prop, self.num_bins
        if values.dim() != 2 or values.shape != (num_atoms.shape[0], P) or num_atoms.shape[0] == 0:
            raise ValueError("values must be [M, %d] for [M] atom counts, M > 0 (got %s and %s)"
                             % (P, tuple(values.shape), tuple(num_atoms.shape)))
        counts, slot = torch.unique(num_atoms, sorted=True, return_inverse=True)      # atom counts without a molecule get no slot
        S = counts.shape[0]
        at = slot.unsqueeze(1).expand(-1, P)
        mn = torch.full((S, P), float('inf')).scatter_reduce_(0, at, values, 'amin', include_self=False)
        mx = torch.full((S, P), float('-inf')).scatter_reduce_(0, at, values, 'amax', include_self=False)
        rng = mx - mn + 1e-12
        idx = ((values - mn[slot]) / rng[slot] * K).long()
        idx[idx == K] = K - 1
        if bool(((idx < 0) | (idx >= K)).any()):
            raise ValueError("a property value does not fall into a bin (not finite?)")
        flat = ((torch.arange(P).unsqueeze(0) * S + slot.unsqueeze(1)) * K + idx).reshape(-1)
        weights = torch.bincount(flat, minlength=P * S * K).reshape(P, S, K)
        self._set_tables(counts, weights, mn.t().contiguous(), mx.t().contiguous(), None)

    def _set_tables(self, counts, weights, mn, mx, probs):
        """counts int64 [S] (ascending), weights int64 [P, S, K] (integer bin weights), mn / mx f32 [P, S], probs f32 [P, S, K] or
        None: the reference's probabilities of count weights — histogram / sum, normalised once more by Categorical (:62-65)."""
        P, S, K = self.n_prop, int(counts.shape[0]), self.num_bins
        if weights.shape != (P, S, K) or mn.shape != (P, S) or mx.shape != (P, S):
            raise ValueError("table shapes do not fit %d properties, %d atom counts, %d bins" % (P, S, K))
        totals = weights.sum(-1)
        if bool((weights < 0).any()) or bool((totals <= 0).any()) or bool((totals >= (1 << 31)).any()):
            raise ValueError("every (property, atom count) row needs non-negative weights with a total in (0, 2^31)")
        if probs is None:
            probs = torch.empty(P, S, K, dtype=torch.float32)
            for s in range(S):
                hist = weights[:, s, :].to(torch.float32).contiguous()
                p0 = hist / torch.sum(hist, dim=-1, keepdim=True)
                for i in range(P):
                    probs[i, s] = p0[i] / p0[i].sum(-1, keepdim=True)
        self._counts = counts.long().clone()
        self._weights = weights.long().clone()
        self._min = mn.to(torch.float32).clone()
        self._max = mx.to(torch.float32).clone()
        self._probs = probs.to(torch.float32).clone()
        self._slot_of = {int(n): s for s, n in enumerate(self._counts.tolist())}
        lut = torch.full((int(self._counts.max()) + 1,), -1, dtype=torch.int32)
        lut[self._counts] = torch.arange(S, dtype=torch.int32)
        self._lut = lut
        self._device_tables = {}

    def state_dict(self):
        """Plain tensors only: the integer bin weights, the probabilities of the reference-mode draw, minima, maxima, atom counts,
        the property names (utf-8 bytes, newline-separated) and num_bins.  The normalizer is not part of it (set_normalizer)."""
        return {'weights': self._weights.clone(), 'probs': self._probs.clone(), 'min': self._min.clone(), 'max': self._max.clone(),
                'atom_counts': self._counts.clone(),
                'properties': torch.tensor(list('\n'.join(self.properties).encode('utf-8')), dtype=torch.uint8),
                'num_bins': torch.tensor(self.num_bins, dtype=torch.long)}

    def load_state_dict(self, state):
        """Replace this prior's tables by a saved one's (properties and num_bins included); the normalizer stays.  Without 'probs' the
        reference-mode probabilities are derived from the weights as from counts."""
        properties = bytes(state['properties'].to(torch.uint8).tolist()).decode('utf-8').split('\n')
        self._init(properties, int(state['num_bins']), self._normalizer)
        self._set_tables(state['atom_counts'].cpu(), state['weights'].cpu(), state['min'].cpu(), state['max'].cpu(),
                         state['probs'].cpu() if state.get('probs') is not None else None)
        return self

    @classmethod
    def from_state_dict(cls, state, normalizer=None):
        self = cls.__new__(cls)
        self._normalizer = normalizer
        return self.load_state_dict(state)

    # ---- the reference's surface --------------------------------------------------------------------------------------------------
    @property
    def normalizer(self):
        return self._normalizer

    @normalizer.setter
    def normalizer(self, normalizer):
        self._normalizer = normalizer
        self._device_tables = {}

    def set_normalizer(self, normalizer):
        self.normalizer = normalizer

    @property
    def distributions(self):
        """The reference's attribute: {property: {atom count: {'probs': object with .probs / .sample, 'params': [min, max]}}}."""
        return {prop: {n: {'probs': _Row(self._probs[i, s]), 'params': [self._min[i, s], self._max[i, s]]}
                       for n, s in self._slot_of.items()} for i, prop in enumerate(self.properties)}

    def _centre_and_spread(self, prop):
        """What the normalizer holds for one property, as it holds it (tensors or numbers): the host draw computes with these objects,
        the device tables with their float32 values."""
        if self._normalizer is None:
            raise AssertionError("this prior has no normalizer: set_normalizer({property: {'mean': ..., 'mad': ...}}) first")
        entry = self._normalizer[prop]
        return entry['mean'], entry['mad']

    def normalize_tensor(self, tensor, prop):
        """(tensor - mean) / mad of property `prop`; AssertionError without a normalizer, as in the reference."""
        centre, spread = self._centre_and_spread(prop)
        return (tensor - centre) / spread

    def sample(self, n_nodes=19):
        """[n_prop] normalised targets for one molecule of n_nodes atoms; KeyError for an atom count without a distribution.  Per property
        one multinomial draw of the bin k, then one uniform draw inside it: the bin's edges are k / K and (k + 1) / K of the way from the
        slot's minimum to its maximum (the fraction formed in double, the rest on 0-dim float32 tensors: the reference's roundings)."""
        s = self._slot_of[n_nodes]
        K = self.num_bins
        targets = []
        for i, prop in enumerate(self.properties):
            lo, hi = self._min[i, s], self._max[i, s]
            k = int(_Row(self._probs[i, s]).sample((1,)))
            span = hi - lo
            lower_edge = k / K * span + lo
            upper_edge = (k + 1) / K * span + lo
            drawn = torch.rand(1) * (upper_edge - lower_edge) + lower_edge
            targets.append(self.normalize_tensor(drawn, prop))
        return torch.cat(targets)

    def sample_batch(self, nodesxsample):
        """[B, n_prop] on the CPU, molecule by molecule in the reference's draw order."""
        return torch.cat([self.sample(int(n)).unsqueeze(0) for n in nodesxsample], dim=0)

    # ---- device mode --------------------------------------------------------------------------------------------------------------
    def slots_for(self, n_nodes):
        """int32 [B] table slots of the atom counts (a CPU tensor or a list), one vectorised lookup; KeyError naming the first atom
        count without a distribution."""
        n = torch.as_tensor(n_nodes)
        if n.is_cuda:
            raise TypeError("n_nodes is a CPU tensor or a list (the slot lookup runs on the host)")
        n = n.reshape(-1).long()
        top = self._lut.shape[0] - 1
        inside = (n >= 0) & (n <= top)
        slots = torch.where(inside, self._lut[n.clamp(0, top)], torch.full_like(n, -1, dtype=torch.int32))
        missing = (slots < 0).nonzero()
        if missing.numel():
            raise KeyError(int(n[int(missing[0])]))
        return slots.contiguous()

    def host_tables(self):
        """The device tables as CPU tensors (what jodo_prop_sample reads; tests restate the kernel on them): 'cum' int32 [P, S, K]
        inclusive cumulative weights (totals below 2^31: the int32 bits are the kernel's uint32), 'minmax' f32 [P, S, 2], 'norm' f32
        [P, 2] = (mean, mad) per property, (0, 1) without a normalizer."""
        norm = torch.tensor([[0.0, 1.0]] * self.n_prop, dtype=torch.float32)
        if self._normalizer is not None:
            for i, prop in enumerate(self.properties):
                centre, spread = self._centre_and_spread(prop)
                norm[i, 0], norm[i, 1] = float(centre), float(spread)
        return {'cum': torch.cumsum(self._weights, -1).to(torch.int32).contiguous(),
                'minmax': torch.stack([self._min, self._max], -1).contiguous(), 'norm': norm}

    def sample_batch_device(self, n_nodes, device, seed, first_index=0, indices=None):
        """[B, n_prop] float32 on `device` (a GPU), one kernel launch.  n_nodes: CPU tensor or list of atom counts; molecule i is the
        molecule of global index indices[i] (a list or CPU tensor of B integers) when given, else first_index + i; its targets depend
        only on (seed, global index, atom count, the prior).  The tables go to each device once (until load_state_dict or
        set_normalizer); a call uploads the int32 slots and, if given, the int64 indices."""
        from .. import fused
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError("sample_batch_device draws on a GPU (device %s): there is no CPU fallback; sample_batch is the host draw" % device)
        slots = self.slots_for(n_nodes)
        return fused.prop_sample(self.device_tables(device), slots, seed, first_index=first_index, indices=indices)

    def device_tables(self, device):
        """The tables on `device` (a fused.PropTables), uploaded at the first request and kept until load_state_dict or set_normalizer."""
        from .. import fused
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError("the prior's device tables live on a GPU (device %s): there is no CPU fallback" % device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        tables = self._device_tables.get(device)
        if tables is None:
            tables = self._device_tables[device] = fused.PropTables(self.host_tables(), device)
        return tables

"""Rule tables of the stability metrics, as DATA supplied by the caller.

The kernels of csrc/eval_kernels.hip take three tables: an ordered matrix of bond-length thresholds, one mask of allowed valences per
atom type (the 3-D rule) and one per (atom type, formal charge) (the bond rule).  This package holds no such table.  A caller builds a
`StabilityRules` either from the dictionaries of the code base whose numbers they want to reproduce

    from evaluation import bond_analyze as ba                     # the reference's module, imported by the caller
    rules = StabilityRules.from_tables(info['atom_decoder'], info['name'], ba.bonds1, ba.bonds2, ba.bonds3,
                                       (ba.margin1, ba.margin2, ba.margin3), ba.allowed_bonds, ba.allowed_fc_bonds)

or from a rules file (`from_file`), a JSON document that holds numbers and element symbols only:

    {"format": "jodo-stability-rules", "version": 1,
     "datasets": {"<dataset name>": {
        "atom_decoder": ["H", "C", ...],                          # element symbol of every atom type index
        "pair_order": "index" | "type",                           # which ordered pair of an atom pair i < j is looked up (below)
        "thresholds_pm": [["C", "S", t1, t2, 0], ...],             # first, second element, then the single / double / triple threshold in
                                                                   # integer picometres, margins included, 0 = no such bond; pairs
                                                                   # that are not listed never bond
        "allowed_valences": {"H": [v, ...], ...},                 # 3-D rule: the allowed valences (0..31) of every element
        "allowed_valences_by_charge": {"N": {"0": [v, ...], "1": [...], "-1": [...]}, "B": {"0": [...]}, ...}}}}   # bond rule

The threshold list is ORDERED: ["C", "S", ...] and ["S", "C", ...] are two entries and need not agree (a table may know a double-bond
length for one and not for the other); nothing is symmetrised.  `pair_order` 'index' looks up (type[i], type[j]) for atoms i < j,
'type' the pair sorted by atom-type index.  In "allowed_valences_by_charge" a charge that an element does not list uses the element's
entry for "0", which every element has; an element that ignores the charge lists "0" alone.
"""
import json
import re

import numpy as np

FORMAT, VERSION = 'jodo-stability-rules', 1
PAIR_ORDERS = ('index', 'type')
# 'QM9' looks a pair up by atom index, 'GeomDrug' sorted by type index (evaluation/stability.py:47-52 of the reference); no other
# dataset has a distance rule there
_PAIR_ORDER_OF = {'QM9': 'index', 'GeomDrug': 'type'}
_SYMBOL = re.compile(r'^[A-Z][a-z]?$')
MAX_VALENCE = 31                                            # masks are 32 bits wide


class RulesError(ValueError):
    """A rule table that cannot be encoded; the subclasses name what is wrong."""


class UnknownElementError(RulesError):
    pass


class MissingSectionError(RulesError):
    pass


class ValenceRangeError(RulesError):
    pass


class UnknownDatasetError(RulesError):
    pass


def _valences(v, what):
    """int | list of ints -> sorted list, checked against the mask range."""
    vals = [v] if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else v
    if not isinstance(vals, (list, tuple)) or not vals or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in vals):
        raise RulesError("%s: allowed valences are an integer or a non-empty list of integers, got %r" % (what, v))
    for x in vals:
        if not 0 <= int(x) <= MAX_VALENCE:
            raise ValenceRangeError("%s: valence %d is outside the mask range 0..%d" % (what, int(x), MAX_VALENCE))
    return sorted({int(x) for x in vals})


def _mask(vals):
    m = 0
    for v in vals:
        m |= 1 << v
    return m


class StabilityRules:
    """The tables of one dataset.  atom_decoder: element symbol per type index (T of them); pair_order 'index' | 'type';
    thr int32 [T,T,3]; allowed: one sorted valence list per type; allowed_fc: per type a dict charge -> sorted valence list that always
    has the key 0.  The arrays the kernels take: `thr`, `allowed_mask` (uint32 [T]), `fc_lo` / `fc_hi` and `allowed_fc_mask`
    (uint32 [T, fc_hi - fc_lo + 1], the fallback to charge 0 already applied)."""

    def __init__(self, atom_decoder, dataset_name, pair_order, thr, allowed, allowed_fc):
        self.atom_decoder = [str(s) for s in atom_decoder]
        self.dataset_name = str(dataset_name)
        T = len(self.atom_decoder)
        if T < 1 or T > 255:
            raise RulesError("atom_decoder holds %d types; 1..255 are supported" % T)
        for s in self.atom_decoder:
            if not _SYMBOL.match(s):
                raise UnknownElementError("atom_decoder entry %r is not an element symbol" % s)
        if len(set(self.atom_decoder)) != T:
            raise RulesError("atom_decoder lists an element twice")
        if pair_order not in PAIR_ORDERS:
            raise RulesError("pair_order is 'index' or 'type', got %r" % (pair_order,))
        self.pair_order = pair_order
        thr = np.ascontiguousarray(thr, dtype=np.int32)
        if thr.shape != (T, T, 3) or (thr < 0).any():
            raise RulesError("thr must be a non-negative int32 [%d, %d, 3] array" % (T, T))
        self.thr = thr
        self.allowed = [list(a) for a in allowed]
        self.allowed_fc = [{int(q): list(v) for q, v in d.items()} for d in allowed_fc]
        if len(self.allowed) != T or len(self.allowed_fc) != T or any(0 not in d for d in self.allowed_fc):
            raise RulesError("one valence list and one charge table with an entry for charge 0 per atom type")
        self.allowed_mask = np.array([_mask(a) for a in self.allowed], dtype=np.uint32)
        charges = sorted({q for d in self.allowed_fc for q in d})
        self.fc_lo, self.fc_hi = min(charges + [0]), max(charges + [0])
        if self.fc_lo < -128 or self.fc_hi > 127:
            raise RulesError("formal charges must fit a signed byte")
        self.allowed_fc_mask = np.array([[_mask(d.get(q, d[0])) for q in range(self.fc_lo, self.fc_hi + 1)] for d in self.allowed_fc],
                                        dtype=np.uint32)

    @property
    def n_types(self):
        return len(self.atom_decoder)

    # ---- from the dictionaries of the code base being reproduced -----------------------------------------------------------------------
    @classmethod
    def from_tables(cls, atom_decoder, dataset_name, bonds1, bonds2, bonds3, margins, allowed_bonds, allowed_fc_bonds):
        """bonds1/2/3: element -> element -> length in picometres (single / double / triple); margins: the three margins added to them;
        allowed_bonds: element -> int | list; allowed_fc_bonds: element -> int | list | {charge: int | list}.  dataset_name decides the
        pair ordering ('QM9': by atom index, 'GeomDrug': by type index) and is refused otherwise."""
        if dataset_name not in _PAIR_ORDER_OF:
            raise UnknownDatasetError("no stability rule for dataset %r: the rules exist for %s" % (dataset_name, ' / '.join(_PAIR_ORDER_OF)))
        if len(margins) != 3:
            raise RulesError("margins are the three numbers added to the single, double and triple lengths")
        dec = [str(s) for s in atom_decoder]
        T = len(dec)
        thr = np.zeros((T, T, 3), dtype=np.int64)
        for a, A in enumerate(dec):
            for b, B in enumerate(dec):
                for k, tab in enumerate((bonds1, bonds2, bonds3)):
                    if A in tab and B in tab[A]:
                        v = tab[A][B] + margins[k]
                        if v != int(v) or not 0 < int(v) < 2 ** 31:
                            raise RulesError("threshold %s-%s order %d: %r is not a positive integer number of picometres" % (A, B, k + 1, v))
                        thr[a, b, k] = int(v)
        allowed, allowed_fc = [], []
        for A in dec:
            if A not in allowed_bonds:
                raise UnknownElementError("element %s of atom_decoder has no entry in allowed_bonds" % A)
            if A not in allowed_fc_bonds:
                raise UnknownElementError("element %s of atom_decoder has no entry in allowed_fc_bonds" % A)
            allowed.append(_valences(allowed_bonds[A], 'allowed_bonds[%s]' % A))
            e = allowed_fc_bonds[A]
            if isinstance(e, dict):
                if 0 not in e:
                    raise MissingSectionError("allowed_fc_bonds[%s] has no entry for charge 0, the fallback of every other charge" % A)
                allowed_fc.append({int(q): _valences(v, 'allowed_fc_bonds[%s][%s]' % (A, q)) for q, v in e.items()})
            else:                                             # an int or a list: the charge is ignored
                allowed_fc.append({0: _valences(e, 'allowed_fc_bonds[%s]' % A)})
        return cls(dec, dataset_name, _PAIR_ORDER_OF[dataset_name], thr, allowed, allowed_fc)

    # ---- the rules file ----------------------------------------------------------------------------------------------------------------
    def section(self):
        """This dataset's section of a rules file (see the module docstring)."""
        T = self.n_types
        rows = [[self.atom_decoder[a], self.atom_decoder[b]] + [int(x) for x in self.thr[a, b]]
                for a in range(T) for b in range(T) if self.thr[a, b].any()]
        return {'atom_decoder': list(self.atom_decoder), 'pair_order': self.pair_order, 'thresholds_pm': rows,
                'allowed_valences': {s: list(v) for s, v in zip(self.atom_decoder, self.allowed)},
                'allowed_valences_by_charge': {s: {str(q): list(v) for q, v in sorted(d.items())}
                                               for s, d in zip(self.atom_decoder, self.allowed_fc)}}

    def to_file(self, path, also=()):
        """Write a rules file with this dataset's section and those of `also` (further StabilityRules)."""
        sections = {}
        for r in (self,) + tuple(also):
            if r.dataset_name in sections:
                raise RulesError("two sections named %r" % r.dataset_name)
            sections[r.dataset_name] = r.section()
        with open(path, 'w') as f:
            json.dump({'format': FORMAT, 'version': VERSION, 'datasets': sections}, f, indent=1, sort_keys=True)
            f.write('\n')

    @classmethod
    def from_section(cls, dataset_name, sec):
        for key in ('atom_decoder', 'pair_order', 'thresholds_pm', 'allowed_valences', 'allowed_valences_by_charge'):
            if key not in sec:
                raise MissingSectionError("rules for %r lack the section %r" % (dataset_name, key))
        dec = [str(s) for s in sec['atom_decoder']]
        index = {s: i for i, s in enumerate(dec)}
        T = len(dec)
        thr = np.zeros((T, T, 3), dtype=np.int64)
        for row in sec['thresholds_pm']:
            if len(row) != 5:
                raise RulesError("a thresholds_pm row is [element, element, t1, t2, t3], got %r" % (row,))
            for s in row[:2]:
                if s not in index:
                    raise UnknownElementError("thresholds_pm names %r, which is not in atom_decoder" % (s,))
            t = row[2:]
            if any(isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < 2 ** 31 for x in t):
                raise RulesError("thresholds of %s-%s must be non-negative integers (picometres)" % (row[0], row[1]))
            thr[index[row[0]], index[row[1]]] = t
        allowed, allowed_fc = [], []
        for name in ('allowed_valences', 'allowed_valences_by_charge'):
            for s in sec[name]:
                if s not in index:
                    raise UnknownElementError("%s names %r, which is not in atom_decoder" % (name, s))
        for s in dec:
            if s not in sec['allowed_valences']:
                raise UnknownElementError("element %s of atom_decoder has no entry in allowed_valences" % s)
            if s not in sec['allowed_valences_by_charge']:
                raise UnknownElementError("element %s of atom_decoder has no entry in allowed_valences_by_charge" % s)
            allowed.append(_valences(sec['allowed_valences'][s], 'allowed_valences[%s]' % s))
            d = sec['allowed_valences_by_charge'][s]
            if not isinstance(d, dict) or '0' not in d:
                raise MissingSectionError("allowed_valences_by_charge[%s] has no entry for charge \"0\", the fallback of every other charge" % s)
            try:
                allowed_fc.append({int(q): _valences(v, 'allowed_valences_by_charge[%s][%s]' % (s, q)) for q, v in d.items()})
            except (TypeError, ValueError) as e:
                if isinstance(e, RulesError):
                    raise
                raise RulesError("allowed_valences_by_charge[%s]: charges are integers written as strings" % s)
        return cls(dec, dataset_name, sec['pair_order'], thr, allowed, allowed_fc)

    @classmethod
    def from_file(cls, path, dataset_name=None):
        """Read one dataset's section of a rules file; dataset_name may be left out when the file holds a single section."""
        with open(path) as f:
            doc = json.load(f)
        if not isinstance(doc, dict) or doc.get('format') != FORMAT or doc.get('version') != VERSION:
            raise RulesError("%s is not a %s version %d file" % (path, FORMAT, VERSION))
        sections = doc.get('datasets')
        if not isinstance(sections, dict) or not sections:
            raise MissingSectionError("%s has no 'datasets' section" % path)
        if dataset_name is None:
            if len(sections) != 1:
                raise MissingSectionError("%s holds the datasets %s: say which one" % (path, ', '.join(sorted(sections))))
            dataset_name = next(iter(sections))
        if dataset_name not in sections:
            raise MissingSectionError("%s has no section for dataset %r (it has %s)" % (path, dataset_name, ', '.join(sorted(sections))))
        return cls.from_section(dataset_name, sections[dataset_name])

"""Sub-structure geometry on the device: bond lengths, bond angles and dihedral angles per frequent symbol, and their MMD against a
target statistic (csrc/geometry_kernels.hip through jodo_geometry_count / jodo_geometry_write / jodo_mmd_batched).

The names are the reference's (evaluation/cal_geometry.py): `get_sub_geometry_metric` returns its `sub_geometry_metric`, whose result
is the same dict — one MMD per symbol of `top_bond_sym`, `top_angle_sym`, `top_dihedral_sym` plus 'bond_length_mean',
'bond_angle_mean', 'dihedral_angle_mean'.  RDKit is not needed: the molecule is the one the reference's check_2D_stability builds from
the decoded bond matrix, and the three value formulas are evaluated in float32 from the float32 positions.  There is no CPU fallback.

Deviations from the reference, all documented in DESIGN.md §4m: it feeds the metric its `complete_rdmols` (RDKit-sanitisable, one
fragment), here the caller chooses the molecules through `keep` (default: all; `connected_mask` builds the nearest available mask);
above `max_samples` a side is subsampled by a seeded torch.Generator, not by Python's unseeded random.sample; parity with the real
RDKit's accessors is not pinned by a test (parity with the reference's Python, driven through stand-ins, is).
"""
import re

import numpy as np
import torch

from .. import capi
from .mmd import mmd_device

GROUPS = ('bond', 'angle', 'dihedral')
GROUP_KEYS = ('top_bond_sym', 'top_angle_sym', 'top_dihedral_sym')
MEAN_NAMES = ('bond_length_mean', 'bond_angle_mean', 'dihedral_angle_mean')
_BOND = re.compile(r'([A-Z][a-z]?)(\d+)([A-Z][a-z]?)')
CHUNK = 4096                                                  # molecules per launch of a host list


class GeometrySymbols:
    """The three symbol lists of a dataset as class tuples for the kernel: per bond of a symbol (atom-type index, bond code, atom-type
    index), so 3 integers for a bond length, 6 for an angle, 9 for a dihedral.  A symbol listed twice is one class, as it is one key
    of the reference's dict."""

    def __init__(self, atom_decoder, bond_syms, angle_syms, dihedral_syms):
        self.atom_decoder = list(atom_decoder)
        self.syms, self.classes = [], []
        for g, (syms, bonds) in enumerate(zip((bond_syms, angle_syms, dihedral_syms), (1, 2, 3))):
            syms = list(dict.fromkeys(syms))
            if len(syms) > capi.GEOMETRY_MAX_CLASSES:
                raise ValueError("at most %d %s symbols, got %d" % (capi.GEOMETRY_MAX_CLASSES, GROUPS[g], len(syms)))
            self.syms.append(syms)
            self.classes.append(np.asarray([self._parse(s, bonds, GROUPS[g]) for s in syms], np.int32).reshape(len(syms), 3 * bonds))
        everything = [s for syms in self.syms for s in syms]
        if len(set(everything)) != len(everything) or set(everything) & set(MEAN_NAMES):
            raise ValueError("a symbol appears in two groups")

    def _parse(self, sym, bonds, group):
        parts = sym.split('-') if isinstance(sym, str) else []
        if len(parts) != bonds:
            raise ValueError("%r is not %s %s symbol: %d bond(s) like 'C1H', joined by '-'" % (sym, 'an' if group == 'angle' else 'a', group, bonds))
        out = []
        for part in parts:
            m = _BOND.fullmatch(part)
            if m is None:
                raise ValueError("%r does not parse: %r is not <element><bond code><element>" % (sym, part))
            for el in (m.group(1), m.group(3)):
                if el not in self.atom_decoder:
                    raise ValueError("%r names the element %s, which the atom decoder (%s) lacks" % (sym, el, ' '.join(self.atom_decoder)))
            out += [self.atom_decoder.index(m.group(1)), int(m.group(2)), self.atom_decoder.index(m.group(3))]
        return out

    @classmethod
    def from_dataset_info(cls, dataset_info):
        for key in ('atom_decoder',) + GROUP_KEYS:
            if key not in dataset_info:
                raise ValueError("dataset_info has no %r" % key)
        return cls(dataset_info['atom_decoder'], *[dataset_info[k] for k in GROUP_KEYS])

    @property
    def n_types(self):
        return len(self.atom_decoder)

    @property
    def all_syms(self):
        return [s for syms in self.syms for s in syms]


class _DeviceClasses:
    def __init__(self, symbols):
        self.symbols, self._by_dev = symbols, {}

    def on(self, device):
        key = (device.type, device.index)
        if key not in self._by_dev:                           # one row of padding: a group without classes still has a pointer
            self._by_dev[key] = tuple(torch.from_numpy(np.concatenate([c.reshape(-1), np.zeros(1, np.int32)])).to(device)
                                      for c in self.symbols.classes)
        return self._by_dev[key]


def _run(classes, pos, at, et, n_nodes_dev, keep):
    """count + scan, one device->host copy of the class sizes, allocate, write -> the result dict"""
    named = (('pos', pos, torch.float32), ('atom_type', at, torch.uint8), ('edge_type', et, torch.uint8), ('n_nodes_dev', n_nodes_dev, torch.int32))
    if keep is not None:
        if isinstance(keep, torch.Tensor) and keep.dtype == torch.bool:
            keep = keep.to(torch.uint8)
        named += (('keep', keep, torch.uint8),)
    for name, t, dt in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a %s GPU tensor" % (name, dt))
        if not t.is_cuda:
            raise NotImplementedError("geometry: %s is a CPU tensor; the extraction runs on the GPU only (no CPU fallback)" % name)
        if t.dtype != dt:
            raise TypeError("%s must be %s (the decode's format), got %s" % (name, dt, t.dtype))
    if at.dim() != 2:
        raise ValueError("atom_type is [B, N]")
    B, N = at.shape
    dev = at.device
    if pos.shape != (B, N, 3) or et.shape != (B, N, N) or pos.device != dev or et.device != dev:
        raise ValueError("pos is [B, N, 3] and edge_type [B, N, N] on the device of atom_type")
    if n_nodes_dev.shape != (B,) or n_nodes_dev.device != dev:
        raise ValueError("n_nodes_dev does not belong to this batch")
    if keep is not None and (keep.shape != (B,) or keep.device != dev):
        raise ValueError("keep is [B] on the device of atom_type")
    sy = classes.symbols
    cb, ca, cd = classes.on(dev)
    Cb, Ca, Cd = (len(s) for s in sy.syms)
    Ct = Cb + Ca + Cd
    pos, at, et, n_nodes_dev = pos.contiguous(), at.contiguous(), et.contiguous(), n_nodes_dev.contiguous()
    keep = keep.contiguous() if keep is not None else None
    counts = torch.empty(max(Ct, 1), B, dtype=torch.int32, device=dev)
    offsets = torch.empty(max(Ct, 1), B, dtype=torch.int64, device=dev)
    host = torch.empty(max(Ct, 1) + 3, dtype=torch.int64, device=dev)         # class sizes, then the dropped values per group
    L = capi.lib()
    with torch.cuda.device(dev):
        head = (B, N, Cb, Ca, Cd, capi.ptr(cb), capi.ptr(ca), capi.ptr(cd), capi.ptr(n_nodes_dev), capi.ptr(keep), capi.ptr(pos),
                capi.ptr(at), capi.ptr(et))
        capi.check(L.jodo_geometry_count(*head, capi.ptr(counts), capi.ptr(offsets), capi.ptr(host), capi.ptr(host[max(Ct, 1):]),
                                         capi.current_stream_ptr()), 'jodo_geometry_count')
        mols = (n_nodes_dev > 0) if keep is None else ((n_nodes_dev > 0) & (keep != 0))
        got = torch.cat([host, mols.sum().reshape(1)]).cpu().tolist()
        sizes, dropped, n_mols = got[:Ct], got[max(Ct, 1):max(Ct, 1) + 3], got[-1]
        per_group = [sum(sizes[:Cb]), sum(sizes[Cb:Cb + Ca]), sum(sizes[Cb + Ca:])]
        outs = [torch.empty(n, dtype=torch.float32, device=dev) for n in per_group]
        capi.check(L.jodo_geometry_write(*head, capi.ptr(offsets), *[capi.ptr(o) if o.numel() else capi.ptr(None) for o in outs],
                                         *per_group, capi.current_stream_ptr()), 'jodo_geometry_write')
    values, k = {}, 0
    for g, syms in enumerate(sy.syms):
        lo = 0
        for s in syms:
            values[s] = outs[g][lo:lo + sizes[k]]
            lo += sizes[k]
            k += 1
    return {'values': values, 'counts': {s: int(v.numel()) for s, v in values.items()},
            'dropped': dict(zip(GROUPS, (int(d) for d in dropped))), 'n_mols': int(n_mols)}


def merge_results(acc, res):
    """acc (a dict, empty at first) += one result of a geometry function: value lists concatenated in call order, integers summed"""
    if not acc:
        acc.update({'values': dict(res['values']), 'counts': dict(res['counts']), 'dropped': dict(res['dropped']), 'n_mols': res['n_mols']})
        return acc
    for s, v in res['values'].items():
        acc['values'][s] = torch.cat([acc['values'][s], v])
        acc['counts'][s] += res['counts'][s]
    for g in GROUPS:
        acc['dropped'][g] += res['dropped'][g]
    acc['n_mols'] += res['n_mols']
    return acc


def _check_symbols(symbols):
    if not isinstance(symbols, GeometrySymbols):
        raise TypeError("symbols must be a GeometrySymbols (jodo_amd.evaluation.GeometrySymbols.from_dataset_info)")


def get_geometry_fn(config, symbols):
    """fn(pos, at, et, n_nodes_dev, keep=None) on the decode's device tensors (fused.decode: pos f32 [B,N,3], atom_type u8 [B,N],
    edge_type u8 [B,N,N]; n_nodes_dev i32 [B]; keep u8 / bool [B], 0 = the molecule contributes nothing).  Returns a dict: 'values'
    {symbol: device f32 tensor} (lengths in Angstrom, angles and dihedrals in degrees; exact sizes, a fixed order: bit-identical for the
    same input), 'counts' {symbol: int}, 'dropped' {'bond' | 'angle' | 'dihedral': non-finite values left out}, 'n_mols' (molecules that
    contributed).  One small device->host copy per call (the sizes)."""
    _check_symbols(symbols)
    if symbols.n_types != int(config.data.atom_types):
        raise ValueError("the symbols were parsed against T = %d atom types (%s), config.data.atom_types is %d" % (
            symbols.n_types, ' '.join(symbols.atom_decoder), int(config.data.atom_types)))
    if config.only_2D:
        raise NotImplementedError("the geometry metric belongs to the 3-D models; config.only_2D is set (a 2-D molecule has no positions)")
    classes = _DeviceClasses(symbols)

    def geometry_fn(pos, at, et, n_nodes_dev, keep=None):
        return _run(classes, pos, at, et, n_nodes_dev, keep)

    geometry_fn.symbols = symbols
    return geometry_fn


def connected_mask(stability_result):
    """keep mask from a result of get_stability_fn(..., rule='bonds') on the same batch: molecules of one fragment (per_mol column 2).
    The nearest available stand-in for the reference's `complete_rdmols` filter, which also asks RDKit to sanitise the molecule."""
    return (stability_result['per_mol'][:, 2] == 1).to(torch.uint8)


def _chunks(processed_list, device):
    """the reference's processed_list (host tuples (pos[n,3], atom_type[n], edge_type[n,n], ...)) as padded device batches"""
    arr = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    for c0 in range(0, len(processed_list), CHUNK):
        part = processed_list[c0:c0 + CHUNK]
        ns = [int(arr(m[1]).shape[0]) for m in part]
        B, N = len(ns), max(max(ns), 1)
        pos, at, et = np.zeros((B, N, 3), np.float32), np.zeros((B, N), np.uint8), np.zeros((B, N, N), np.uint8)
        for b, (m, n) in enumerate(zip(part, ns)):
            pos[b, :n], at[b, :n], et[b, :n, :n] = arr(m[0]), arr(m[1]), arr(m[2])
        yield tuple(torch.from_numpy(a).to(device) for a in (pos, at, et, np.asarray(ns, np.int32)))


def _device(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise NotImplementedError("the geometry metric runs on the GPU only (no CPU fallback): device is %s" % dev)
    return dev


def _extract_list(classes, processed_list, dev):
    if not processed_list:
        raise ValueError("processed_list is empty")
    acc = {}
    for batch in _chunks(processed_list, dev):
        merge_results(acc, _run(classes, *batch, None))
    return acc


def geometry_stat(processed_list, symbols, device='cuda'):
    """The content of the reference's target_geometry_stat.pk (load_target_geometry) from a processed_list of dataset molecules (host
    tuples (pos, atom_type, edge_type, ...)): {symbol: list of float}, extracted on the device."""
    _check_symbols(symbols)
    res = _extract_list(_DeviceClasses(symbols), processed_list, _device(device))
    return {s: v.cpu().tolist() for s, v in res['values'].items()}


def assemble_metric(symbols, got):
    """{symbol: MMD} for the symbols that had generated values -> the reference's dict (compute_geo_mmd, three times): per group every
    symbol (NaN where `got` has none) and then the group's np.nanmean under its mean name"""
    out = {}
    for syms, mean_name in zip(symbols.syms, MEAN_NAMES):
        group = {s: float(got.get(s, float('nan'))) for s in syms}
        group[mean_name] = float(np.nanmean(list(group.values()))) if group else float('nan')
        out.update(group)
    return out


def get_sub_geometry_metric(target_stat, dataset_info, device='cuda', max_samples=20000, seed=None):
    """The reference's get_sub_geometry_metric (evaluation/cal_geometry.py:287-301) -> sub_geometry_metric(gen, keep=None).

    target_stat: {symbol: list / array / tensor of floats} — geometry_stat's result or the dict unpickled from the reference's own
    target_geometry_stat.pk.  gen: a processed_list of host tuples (pos, atom_type, edge_type, ...), the device tuple (pos, at, et,
    n_nodes_dev) of the decode (with `keep`), or a result of a geometry function (`sampling_fn.last_geometry`).  Returns the
    reference's dict of floats: one MMD per symbol (NaN for a symbol without a generated value), then the group's np.nanmean under
    'bond_length_mean' / 'bond_angle_mean' / 'dihedral_angle_mean'.  A side with more than max_samples values is subsampled without
    replacement by a torch.Generator seeded with `seed` (None: a fresh seed per call) — target first, then generated, per symbol in
    order, as the reference draws; its draws come from Python's unseeded random.sample and cannot be reproduced."""
    symbols = GeometrySymbols.from_dataset_info(dataset_info)
    missing = [s for s in symbols.all_syms if s not in target_stat]
    if missing:
        raise ValueError("target_stat lacks the symbols %s" % ' '.join(missing))
    max_samples = int(max_samples)
    if max_samples < 1:
        raise ValueError("max_samples must be positive")
    classes = _DeviceClasses(symbols)
    target_dev = {}

    def targets(dev):
        if not target_dev:
            for s in symbols.all_syms:
                t = target_stat[s]
                t = t.detach().to(torch.float32) if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t, np.float32).reshape(-1))
                target_dev[s] = t.to(dev)
        return target_dev

    def sub_geometry_metric(gen, keep=None):
        dev = _device(device)
        if isinstance(gen, dict):
            if keep is not None:
                raise ValueError("keep selects molecules: it goes to the geometry function that made these values")
            values = gen['values']
        elif isinstance(gen, tuple):
            values = _run(classes, *gen, keep)['values']
        else:
            if keep is not None:
                raise ValueError("keep belongs to the device tuple; filter a processed_list itself")
            values = _extract_list(classes, gen, dev)['values']
        tar = targets(dev)
        rng = torch.Generator()
        if seed is None:
            rng.seed()
        else:
            rng.manual_seed(int(seed))

        def cut(v):
            if v.numel() <= max_samples:
                return v
            return v[torch.randperm(v.numel(), generator=rng)[:max_samples].to(v.device)]

        src, tgt, which = [], [], []
        for s in symbols.all_syms:
            if values[s].numel() == 0:
                continue
            t = cut(tar[s])
            src.append(cut(values[s]))
            tgt.append(t)
            which.append(s)
        got = dict(zip(which, mmd_device(src, tgt).cpu().tolist())) if which else {}
        sub_geometry_metric.last_samples = dict(zip(which, zip(src, tgt)))
        return assemble_metric(symbols, got)

    sub_geometry_metric.symbols = symbols
    sub_geometry_metric.last_samples = None
    return sub_geometry_metric

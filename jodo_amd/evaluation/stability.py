"""Atom and molecule stability on the device (csrc/eval_kernels.hip through jodo_stability_3d / jodo_stability_bonds).

`get_stability_fn` works on the decode's device tensors (fused.decode); `get_edm_metric` / `get_2D_edm_metric` carry the reference's
names (evaluation/stability.py:164-230) and take its `processed_list` of host tuples.  The rule tables come from the caller as a
`StabilityRules` (rules.py); there is no CPU fallback.

'connected' (one fragment over the bonds the rule sees) is NOT the reference's `Complete`, which also asks RDKit for validity: it is an
upper bound on it.  Validity, uniqueness, novelty and the distribution metrics need RDKit and stay out of this package.
"""
import torch

from .. import capi
from .rules import StabilityRules, UnknownDatasetError

RULES = ('3d', 'bonds')
DATASETS = ('QM9', 'GeomDrug')
TOTAL_KEYS = ('n_mol_stable', 'n_atom_stable', 'n_atoms', 'n_connected')      # totals_out of the kernels, in order
COUNT_KEYS = TOTAL_KEYS + ('n_mols',)


def _check_rules(rules, rule):
    if not isinstance(rules, StabilityRules):
        raise TypeError("rules must be a StabilityRules (jodo_amd.evaluation.rules: from_tables / from_file)")
    if rule not in RULES:
        raise ValueError("rule is '3d' (distances) or 'bonds' (decoded bond orders), got %r" % (rule,))
    if rules.dataset_name not in DATASETS:
        raise UnknownDatasetError("no stability rule for dataset %r: the rules exist for %s" % (rules.dataset_name, ' / '.join(DATASETS)))


class _DeviceTables:
    """The rule tables of one StabilityRules on the devices they were asked for (uploaded once per device)."""

    def __init__(self, rules):
        self.rules = rules
        self._by_dev = {}

    def on(self, device):
        key = (device.type, device.index)
        if key not in self._by_dev:
            r = self.rules
            up = lambda a, dt: torch.from_numpy(a.view(dt) if a.dtype != dt else a).to(device).contiguous()
            import numpy as np
            self._by_dev[key] = (up(r.thr, np.int32), up(r.allowed_mask, np.int32), up(r.allowed_fc_mask, np.int32))
        return self._by_dev[key]


def _run(tables, rule, pos, at, fc, et, n_nodes_dev, want_orders):
    """One launch on checked device tensors -> (per_mol i32 [B,4], totals i64 [4], orders u8 [B,N,N] | None), all on the device."""
    r = tables.rules
    named = (('atom_type', at, torch.uint8), ('n_nodes_dev', n_nodes_dev, torch.int32)) + (
        (('pos', pos, torch.float32),) if rule == '3d' else (('fc', fc, torch.int8), ('edge_type', et, torch.uint8)))
    for name, t, dt in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a %s GPU tensor" % (name, dt))
        if not t.is_cuda:
            raise NotImplementedError("stability (%s rule): %s is a CPU tensor; the metric runs on the GPU only (no CPU fallback)" % (rule, name))
        if t.dtype != dt:
            raise TypeError("%s must be %s (the decode's format), got %s" % (name, dt, t.dtype))
    if at.dim() != 2:
        raise ValueError("atom_type is [B, N]")
    B, N = at.shape
    dev = at.device
    if n_nodes_dev.shape != (B,) or n_nodes_dev.device != dev:
        raise ValueError("n_nodes_dev does not belong to this batch")
    thr, allowed, allowed_fc = tables.on(dev)
    per_mol = torch.empty(B, 4, dtype=torch.int32, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    at, n_nodes_dev = at.contiguous(), n_nodes_dev.contiguous()
    orders = None
    if rule == '3d':
        if pos.shape != (B, N, 3) or pos.device != dev:
            raise ValueError("pos is [B, N, 3] on the device of atom_type")
        pos = pos.contiguous()
        if want_orders:
            orders = torch.empty(B, N, N, dtype=torch.uint8, device=dev)
        capi.check(capi.lib().jodo_stability_3d(
            B, N, r.n_types, capi.PAIR_BY_TYPE if r.pair_order == 'type' else capi.PAIR_BY_INDEX, capi.ptr(thr), capi.ptr(allowed),
            capi.ptr(n_nodes_dev), capi.ptr(pos), capi.ptr(at), capi.ptr(per_mol), capi.ptr(orders), capi.ptr(totals),
            capi.current_stream_ptr()), 'jodo_stability_3d')
    else:
        if want_orders:
            raise ValueError("want_orders belongs to the 3-D rule: the bond rule's orders are its edge_type input")
        if fc.shape != (B, N) or et.shape != (B, N, N) or fc.device != dev or et.device != dev:
            raise ValueError("fc is [B, N] and edge_type [B, N, N] on the device of atom_type")
        fc, et = fc.contiguous(), et.contiguous()
        capi.check(capi.lib().jodo_stability_bonds(
            B, N, r.n_types, r.fc_lo, r.fc_hi, capi.ptr(allowed_fc), capi.ptr(n_nodes_dev), capi.ptr(at), capi.ptr(fc), capi.ptr(et),
            capi.ptr(per_mol), capi.ptr(totals), capi.current_stream_ptr()), 'jodo_stability_bonds')
    return per_mol, totals, orders


def _result(per_mol, totals, orders, n_nodes_dev):
    """The result dict; the five integers come over in one device->host copy."""
    host = torch.cat([totals, (n_nodes_dev > 0).sum().reshape(1)]).cpu().tolist()
    out = dict(zip(COUNT_KEYS, (int(v) for v in host)))
    out['mol_stable'] = out['n_mol_stable'] / out['n_mols'] if out['n_mols'] else float('nan')
    out['atom_stable'] = out['n_atom_stable'] / out['n_atoms'] if out['n_atoms'] else float('nan')
    out['connected'] = out['n_connected'] / out['n_mols'] if out['n_mols'] else float('nan')
    out['per_mol'] = per_mol
    if orders is not None:
        out['orders'] = orders
    return out


def get_stability_fn(config, rules, rule='3d'):
    """fn(pos, at, fc, et, n_nodes_dev, want_orders=False) on the decode's device tensors (fused.decode: pos f32 [B,N,3], atom_type u8
    [B,N], fc i8 [B,N], edge_type u8 [B,N,N]; n_nodes_dev i32 [B]).  rule '3d' reads pos and atom_type (the reference's check_stability),
    'bonds' atom_type, fc and edge_type (its check_2D_stability for molecules without aromatic bonds); the tensors a rule does not read
    may be None.  Returns a dict: 'mol_stable', 'atom_stable', 'connected' (fractions), 'n_mol_stable', 'n_atom_stable', 'n_atoms',
    'n_connected', 'n_mols' (integers: sum them over rounds or ranks, dist.allreduce_counts), 'per_mol' (device i32 [B,4]: stable atoms,
    atoms, fragments, needs_kekulize) and, with want_orders, 'orders' (device u8 [B,N,N], the 3-D rule's bond orders)."""
    _check_rules(rules, rule)
    if rules.n_types != int(config.data.atom_types):
        raise ValueError("the rules have T = %d atom types (%s), config.data.atom_types is %d" % (
            rules.n_types, ' '.join(rules.atom_decoder), int(config.data.atom_types)))
    if rule == 'bonds' and (int(config.model.edge_ch) == 3 or bool(config.data.include_aromatic)):
        raise NotImplementedError("rule='bonds' on a config with an aromatic bond channel (model.edge_ch == 3 / data.include_aromatic): the "
                                  "valences of aromatic bonds need RDKit's Kekulize, which this package does not have")
    tables = _DeviceTables(rules)

    def stability_fn(pos, at, fc, et, n_nodes_dev, want_orders=False):
        per_mol, totals, orders = _run(tables, rule, pos, at, fc, et, n_nodes_dev, want_orders)
        return _result(per_mol, totals, orders, n_nodes_dev)

    stability_fn.rule = rule
    stability_fn.rules = rules
    return stability_fn


def _upload(processed_list, rule, device):
    """The reference's processed_list (host tuples (pos[n,3], atom_type[n], edge_type[n,n], fc[n]); the 3-D rule reads the first two
    only) padded to one batch and uploaded once."""
    import numpy as np
    if not processed_list:
        raise ValueError("processed_list is empty")
    arr = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    ns = [int(arr(m[1]).shape[0]) for m in processed_list]
    B, N = len(ns), max(max(ns), 1)
    pos, at = np.zeros((B, N, 3), np.float32), np.zeros((B, N), np.uint8)
    fc, et = np.zeros((B, N), np.int8), np.zeros((B, N, N), np.uint8)
    for b, (m, n) in enumerate(zip(processed_list, ns)):
        at[b, :n] = arr(m[1])
        if rule == '3d':
            pos[b, :n] = arr(m[0])
        else:
            et[b, :n, :n] = arr(m[2])
            q = arr(m[3])
            if q.size:                                        # a model without a charge channel hands an empty tensor: all charges 0
                fc[b, :n] = q.reshape(n)
    up = lambda a: torch.from_numpy(a).to(device)
    return up(pos), up(at), up(fc), up(et), up(np.asarray(ns, np.int32))


def _edm_metric(dataset_info, rules, rule, device):
    _check_rules(rules, rule)
    if dataset_info['name'] not in DATASETS:
        raise UnknownDatasetError("no stability rule for dataset %r: the rules exist for %s" % (dataset_info['name'], ' / '.join(DATASETS)))
    if dataset_info['name'] != rules.dataset_name or list(dataset_info['atom_decoder']) != rules.atom_decoder:
        raise ValueError("the rules are for %s (%s), dataset_info is %s (%s)" % (
            rules.dataset_name, ' '.join(rules.atom_decoder), dataset_info['name'], ' '.join(dataset_info['atom_decoder'])))
    tables = _DeviceTables(rules)

    def metric(processed_list):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise NotImplementedError("the stability metric runs on the GPU only (no CPU fallback): device is %s" % dev)
        pos, at, fc, et, nd = _upload(processed_list, rule, dev)
        res = _result(*_run(tables, rule, pos, at, fc, et, nd, False), nd)
        if rule == 'bonds' and int(res['per_mol'][:, 3].sum()):
            raise NotImplementedError("processed_list holds aromatic bonds: their valences need RDKit's Kekulize, which this package does "
                                      "not have")
        return {'mol_stable': res['mol_stable'], 'atom_stable': res['atom_stable']}

    return metric


def get_edm_metric(dataset_info, rules, device='cuda'):
    """The reference's get_edm_metric (evaluation/stability.py:164-196) for its stability half: edm_metric(processed_list) -> its
    `stability_dict` {'mol_stable', 'atom_stable'} from the 3-D rule.  The RDKit half of the reference's return value is out of scope."""
    return _edm_metric(dataset_info, rules, '3d', device)


def get_2D_edm_metric(dataset_info, rules, device='cuda'):
    """The reference's get_2D_edm_metric (evaluation/stability.py:199-230) for its stability half, from the bond rule; molecules with
    aromatic bonds are refused (their valences need RDKit's Kekulize)."""
    return _edm_metric(dataset_info, rules, 'bonds', device)

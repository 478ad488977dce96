"""Benchmark of the stability metrics (jodo_amd.evaluation, csrc/eval_kernels.hip) against the host route on the same machine, and their
share of one sampling round.

    python tools/bench_stability.py [--workloads qm9,geom] [--iters 50] [--warmup 3] [--round-steps 50] [--no-round]
                                    [--rules tests/golden/stability_rules.json] [--out-dir profiles]

Workloads: QM9 atom counts from the training histogram at B = 2500 and GEOM ones at B = 512 (seed 42); seeded random molecules — atoms
on a jittered 1.25 A lattice with hydrogen-rich types, about one bond per atom with orders 1-3, charges -1 .. +1 — laid out as the decode
leaves them on the device.  Per workload both rules are warmed up, then timed in alternation with the host route, twice:
  device   the kernel launch alone with device events over `--iters` calls (`*_kernel_ms`), and the whole stability function, its one
           small device->host copy of the totals included, by the host clock around a device synchronise (`*_fn_ms`)
  host     fused.mols_from_decoded (four device->host copies, one tuple per molecule) plus the numpy oracle's loop over the molecules
           (tests/oracle_stability.py), by the host clock (`*_host_ms`); the oracle is vectorised per molecule, which is faster than an
           O(n^2) Python pair loop
The totals of both routes are compared (`*_totals_equal`; the random 3-D molecules are not kept away from the thresholds, so a pair
within float32 rounding of one may differ).  Then one get_sampling_fn round (ancestral, `--round-steps` score-network evaluations) is
timed with and without stability=, host clock around a device synchronise.  The bond rule is timed on a config without an aromatic
channel at either size (it is refused on the GEOM config).  Writes <out-dir>/stability_<workload>.json and prints the record.  Needs a
GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import oracle_stability as OS                                                     # noqa: E402
from jodo_amd import configs, fused                                               # noqa: E402
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP                     # noqa: E402
from jodo_amd.evaluation import StabilityRules, get_stability_fn                  # noqa: E402
from jodo_amd.evaluation.stability import TOTAL_KEYS, _DeviceTables, _run         # noqa: E402
from jodo_amd.models import deterministic_init_, get_model_class, get_node_dist, load_dataset_info      # noqa: E402
from jodo_amd.sampling import get_sampling_fn                                     # noqa: E402
from jodo_amd.utils import get_data_inverse_scaler                                # noqa: E402

WORKLOADS = {'qm9': ('QM9', 'vpsde_qm9_uncond_jodo', 2500), 'geom': ('GeomDrug', 'vpsde_geom_uncond_jodo', 512)}


def random_batch(rules, n_nodes, seed):
    rng = np.random.default_rng(seed)
    B, N, T = len(n_nodes), max(n_nodes), rules.n_types
    pos, at = np.zeros((B, N, 3), np.float32), np.zeros((B, N), np.uint8)
    fc, et = np.zeros((B, N), np.int8), np.zeros((B, N, N), np.uint8)
    p = np.full(T, 0.5 / (T - 1))
    p[0] = 0.5
    for b, n in enumerate(n_nodes):
        side = max(2, int(np.ceil((2.2 * n) ** (1. / 3.))))
        sites = rng.choice(side ** 3, size=n, replace=False)
        grid = np.stack([sites // (side * side), (sites // side) % side, sites % side], 1)
        xyz = 1.25 * grid + rng.uniform(-0.22, 0.22, size=(n, 3))
        pos[b, :n] = xyz - xyz.mean(0, keepdims=True)
        at[b, :n] = rng.choice(T, size=n, p=p)
        fc[b, :n] = rng.integers(-1, 2, size=n)
        if n > 1:
            k = max(1, n)
            i, j = rng.integers(0, n, size=k), rng.integers(0, n, size=k)
            keep = i != j
            up = np.zeros((n, n), np.uint8)
            up[np.minimum(i, j)[keep], np.maximum(i, j)[keep]] = rng.choice([1, 2, 3], size=int(keep.sum()), p=[0.72, 0.2, 0.08])
            et[b, :n, :n] = up + up.T
    return pos, at, fc, et, np.asarray(n_nodes, np.int32)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def clock_ms(fn, iters=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, out


class _Nodes:
    def __init__(self, n):
        self.n = n

    def sample(self, k):
        assert k == len(self.n)
        return torch.as_tensor(self.n)


def host_route(rules, rule, dec, n_nodes):
    """the route without the kernels: copy the decoded tensors to the host, cut them into molecules, loop over them"""
    mols = fused.mols_from_decoded(*dec, n_nodes)
    totals = np.zeros(4, np.int64)
    for pos, at, et, fc in mols:
        o = OS.stability_3d(rules, pos.numpy(), at.numpy()) if rule == '3d' else OS.stability_bonds(rules, at.numpy(), fc.numpy(), et.numpy())
        totals += (int(o['stable_atoms'] == o['atoms']), o['stable_atoms'], o['atoms'], int(o['fragments'] == 1))
    return totals.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='qm9,geom')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--round-steps', type=int, default=50)
    ap.add_argument('--no-round', action='store_true')
    ap.add_argument('--rules', default=os.path.join(ROOT, 'tests', 'golden', 'stability_rules.json'))
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stability needs a GPU: nothing is measured without one")
    dev = torch.device('cuda:0')
    for w in args.workloads.split(','):
        dataset, cfg_name, B = WORKLOADS[w]
        rules = StabilityRules.from_file(args.rules, dataset)
        cfg = configs.get(cfg_name)
        cfg.device = dev
        torch.manual_seed(42)
        n_nodes = get_node_dist(load_dataset_info(cfg.data.info_name)).sample(B).tolist()
        batch = random_batch(rules, n_nodes, 1)
        pos, at, fc, et, nd = [torch.from_numpy(a).to(dev) for a in batch]
        rec = dict(workload='%s histogram, seeded random molecules' % w, dataset=dataset, batch=B, atoms=int(sum(n_nodes)),
                   pairs=int(sum(n * (n - 1) // 2 for n in n_nodes)), padded_width=int(max(n_nodes)), iters=args.iters)
        plain = configs.get('vpsde_qm9_uncond_jodo')              # the bond rule's config: no aromatic channel
        plain.data.atom_types = rules.n_types
        tables = _DeviceTables(rules)
        fns = {'3d': get_stability_fn(cfg, rules, '3d'), 'bonds': get_stability_fn(plain, rules, 'bonds')}
        for rule in ('3d', 'bonds'):
            launch = lambda: _run(tables, rule, pos, at, fc, et, nd, False)
            call = lambda: fns[rule](pos, at, fc, et, nd)
            for _ in range(args.warmup):
                launch(), call()
            legs = {'kernel': [], 'fn': [], 'host': []}
            for _ in range(2):                                    # device, host, device, host
                legs['kernel'].append(event_ms(launch, args.iters))
                ms, res = clock_ms(call, args.iters)
                legs['fn'].append(ms)
                ms, host_totals = clock_ms(lambda: host_route(rules, rule, (pos, at, fc, et), n_nodes))
                legs['host'].append(ms)
            tag = 'rule_' + rule
            for k, v in legs.items():
                rec['%s_%s_ms' % (tag, k)], rec['%s_%s_ms_runs' % (tag, k)] = min(v), v
            rec[tag + '_totals'] = [res[k] for k in TOTAL_KEYS]
            rec[tag + '_totals_equal'] = rec[tag + '_totals'] == host_totals
            rec[tag + '_host_over_fn'] = rec[tag + '_host_ms'] / rec[tag + '_fn_ms']
        if not args.no_round:
            cfg.sampling.steps, cfg.sampling.method = args.round_steps, 'ancestral'
            model = deterministic_init_(get_model_class(cfg.model.name)(cfg), seed=7).to(dev).eval()
            ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
            for name, stab in (('warm', None), ('plain', None), ('with_stability', fns['3d'])):
                fn = get_sampling_fn(cfg, ns, _Nodes(n_nodes), B, B, get_data_inverse_scaler(cfg), return_raw=True, stability=stab)
                torch.manual_seed(3)
                ms, _ = clock_ms(lambda: fn(model))
                if name != 'warm':
                    rec['round_s_%s' % name] = ms * 1e-3
            rec['round_steps'] = args.round_steps
            rec['rule_3d_fn_share_of_round'] = rec['rule_3d_fn_ms'] * 1e-3 / rec['round_s_plain']
            rec['round_stability'] = dict(fn.last_stability)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, 'stability_%s.json' % w), 'w') as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))


if __name__ == '__main__':
    main()

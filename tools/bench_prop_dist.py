"""What a round's conditioning targets cost: the property prior's reference-mode draw (the reference's per-molecule host loop, which
every `prop_dist.sample_batch` call site runs) against the device draw (jodo_prop_sample), in ONE command on one machine.

    python tools/bench_prop_dist.py [--out profiles/prop_dist_qm9.json] [--calls 200] [--repeats 5] [--ref-repeats 3]

The prior: seeded synthetic float32 values (no property labels exist offline) on the `qm9_second_half` atom-count histogram
(jodo_amd/data/n_nodes_hist.json), 1000 bins, 1 and 2 properties; B = 1 250, 2 500 and 10 000 atom counts drawn from the same
histogram.  Per (B, properties):
  reference_s      wall time of sample_batch(n_nodes) on the CPU, each repeat listed
  launch_us        device events around `calls` back-to-back jodo_prop_sample launches on slots already on the device, per launch
  call_us          device events around `calls` sample_batch_device calls (host slot lookup + slot upload + launch), per call
  call_wall_us     a host clock around the same window, ended by a device synchronise, per call
each device figure as the list over `repeats` windows (the spread is the list), after a warm-up window of its own shape.
Needs a GPU: without one it fails (a CPU run has no device time to report).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jodo_amd import capi                                            # noqa: E402
from jodo_amd.cond_gen import DistributionProperty, compute_mean_mad  # noqa: E402

ROUND_S = 0.544          # README: the conditional 50-NFE round of 1 250 molecules


def synthetic_prior(n_prop, seed=0):
    with open(os.path.join(ROOT, 'jodo_amd', 'data', 'n_nodes_hist.json')) as f:
        hist = json.load(f)['qm9_second_half']['train_n_nodes']
    num_atoms = np.concatenate([np.full(int(m), int(n), np.int64) for n, m in hist.items()])
    g = torch.Generator().manual_seed(seed)
    values = (torch.randn(len(num_atoms), n_prop, generator=g) * torch.tensor([8.0, 0.05][:n_prop]) + torch.tensor([75.0, 0.25][:n_prop])
              + torch.from_numpy(num_atoms).float().unsqueeze(1) * torch.tensor([1.5, -0.002][:n_prop])).float()
    names = ['alpha', 'gap'][:n_prop]
    t0 = time.perf_counter()
    prior = DistributionProperty.from_arrays(num_atoms, values, names, num_bins=1000)
    build_s = time.perf_counter() - t0
    mean, mad = compute_mean_mad(values)
    prior.set_normalizer({p: {'mean': mean[i], 'mad': mad[i]} for i, p in enumerate(names)})
    probs = np.array([int(m) for m in hist.values()], np.float64)
    sizes = np.array([int(n) for n in hist.keys()], np.int64)
    return prior, build_s, len(num_atoms), sizes, probs / probs.sum()


def windows(fn, calls, repeats, dev):
    """Per repeat: (device-event microseconds per call, host-clock microseconds per call) of `calls` back-to-back fn() calls."""
    ev, wall = [], []
    for _ in range(calls // 4 + 1):                           # warm-up of this very shape
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        wall.append((time.perf_counter() - t0) * 1e6 / calls)
        ev.append(a.elapsed_time(b) * 1e3 / calls)
    return ev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prop_dist_qm9.json'))
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--ref-repeats', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1250, 2500, 10000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prop_dist needs a GPU: there is no device time to report without one")
    if args.calls < 100:
        raise SystemExit("--calls: at least 100 calls per timed window")
    dev = torch.device('cuda:0')
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))
    rows, builds = [], {}
    L = capi.lib()
    for n_prop in (1, 2):
        prior, build_s, n_mol, sizes, p = synthetic_prior(n_prop)
        builds[str(n_prop)] = {'molecules': n_mol, 'from_arrays_s': build_s}
        for B in args.sizes:
            n_nodes = torch.from_numpy(sizes[np.random.default_rng(B).choice(len(sizes), B, p=p)])
            ref = []
            for r in range(args.ref_repeats):
                torch.manual_seed(r)
                t0 = time.perf_counter()
                want_shape = prior.sample_batch(n_nodes).shape
                ref.append(time.perf_counter() - t0)
            assert want_shape == (B, n_prop)
            out = prior.sample_batch_device(n_nodes, dev, seed=1)
            assert out.shape == (B, n_prop) and bool(torch.isfinite(out).all())
            tables = prior.device_tables(dev)
            slots = prior.slots_for(n_nodes)
            slots_dev = slots.to(dev)
            stream = capi.current_stream_ptr()

            def launch():
                capi.check(L.jodo_prop_sample(B, n_prop, tables.n_bins, tables.n_slots, capi.ptr(tables.cum), capi.ptr(tables.minmax),
                                              capi.ptr(tables.norm), capi.ptr(slots), capi.ptr(slots_dev), None, 0, 1, None, capi.ptr(out),
                                              stream), 'jodo_prop_sample')

            launch_ev, _ = windows(launch, args.calls, args.repeats, dev)
            call_ev, call_wall = windows(lambda: prior.sample_batch_device(n_nodes, dev, seed=1), args.calls, args.repeats, dev)
            ref_med, wall_med = float(np.median(ref)), float(np.median(call_wall))
            rows.append({'B': B, 'n_prop': n_prop, 'reference_s': ref, 'launch_us': launch_ev, 'call_us': call_ev, 'call_wall_us': call_wall,
                         'reference_share_of_round': ref_med / ROUND_S, 'device_call_share_of_round': wall_med * 1e-6 / ROUND_S,
                         'reference_over_device_call': ref_med / (wall_med * 1e-6)})
            print(json.dumps(rows[-1]), flush=True)
    record = {'what': 'property prior: reference-mode sample_batch (CPU) against sample_batch_device (jodo_prop_sample), same command',
              'device': torch.cuda.get_device_name(dev), 'gcn_arch': torch.cuda.get_device_properties(dev).gcnArchName,
              'compute_units': torch.cuda.get_device_properties(dev).multi_processor_count, 'torch': torch.__version__, 'cpu_threads': torch.get_num_threads(),
              'num_bins': 1000, 'histogram': 'qm9_second_half', 'values': 'seeded synthetic float32', 'calls_per_window': args.calls,
              'repeats': args.repeats, 'round_s': ROUND_S,
              'round_s_source': 'README: conditional 50-NFE round of 1 250 molecules; the shares are against that one figure for every B',
              'timing': 'launch_us / call_us: device events per call; call_wall_us: host clock to a device synchronise per call; '
                        'reference_s: host clock; lists hold every repeat; shares and the ratio use the medians',
              'build': builds, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()

"""Benchmark of one ancestral sampling step of the CDGS model (network + update) at the QM9 config, and of the baseline a user without
the HIP path would run on the same GPU: the dense torch evaluation of the same network (tests/oracle_cdgs.py, float32) on the device,
under the same sampler.  Both legs run in this one command on the same GPU, on the same batch.

    python tools/bench_cdgs.py [--workload qm9|geom] [--batches 500,2000] [--steps 50] [--warmup 5] [--no-baseline] [--out-dir profiles]
                               [--kernel-stats CSV --kernel-stats-steps K] [--split off|on|both] [--repeats R]

Atom counts are drawn from the training histogram of the config's dataset (`qm9_with_h`, seed 42).  Timing as bench.py does it: warm-up,
synchronise, `steps` sampler.step calls, synchronise.  Per batch size it writes profiles/cdgs_<workload>_b<B>.json: ms/step of both
legs, ns per ordered pair, and the executed fraction of the 157.3 TFLOP/s fp32-MFMA peak.  Flops: 2 x 393 216 per edge row per block
(lin_edge0 | lin_edge1 and the edge feed-forward) plus the edge readouts, embeddings and heads, plus the node GEMMs; the kernels walk
every ordered pair on its own (nothing is halved) and the n diagonal rows of a molecule besides, which the count includes because they
are executed.  The dense leg evaluates the whole padded batch at once: chunking it by molecules would change the padded width, and with
it this model's result.
--kernel-stats: the kernel table of a `rocprofv3 --kernel-trace --stats` run of this tool with --no-baseline (a run of its own); its kc_*
rows per sampler step are added to the record of the largest batch.
--split (default off: everything above, unchanged): `on` times the opt-in split-bf16 form (model.bf16x3 = True) alone and writes
cdgs_<workload>_b<B>_split_on.json - the command to profile for the split form's kernel table; `both` alternates the exact and the split
form in this one process on the same batch, --repeats times each (exact, split, exact, split, ...; `steps` sampler steps per leg after
one shared warm-up of both forms), and writes cdgs_<workload>_b<B>_split.json: every leg's ms/step, the mean per form, split / exact, and
per form the run-to-run spread (max - min of its legs) - a difference between the forms counts only beyond that spread.  No dense leg in
these modes.  With `both`, --kernel-stats / --kernel-stats-exact take the kernel tables of profiled `--split on` / `--split off
--no-baseline` runs of the same workload, batch, steps and warm-up.
--round --nfe N [--graph] [--split off|on|both] [--repeats R]: complete DPM-Solver++ rounds (sampling.method 'dpm_2d', N network
evaluations, the solver's default single-step order 2) of the same histogram batch at every size of --batches: DPM_Solver_2D.sampling
("eager") and, with --graph, GraphedDPMRound2D.run ("replayed": one capture per round, as the public entry does it), each timed
max(R, 2) times in this one process with the forms alternating, after one untimed round of each.  The ancestral step (--steps /
--warmup, as above) is timed in the same command on the same batch.  Writes profiles/cdgs_dpm_round_<workload>_nfe<N>.json: per batch
and per weight form seconds per round of every leg, their mean and spread (max - min), ms per evaluation (round / N), the ancestral
ms/step, and the 1000-step ancestral round as step time x 1000 (labelled: it is not run).
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from jodo_amd import configs                                                      # noqa: E402
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP                     # noqa: E402
from jodo_amd.models import get_model_class, get_node_dist, load_dataset_info, deterministic_init_   # noqa: E402
from jodo_amd.models.utils import sample_gaussian_with_mask, sample_symmetric_edge_feature_noise      # noqa: E402
from jodo_amd.sampling import AncestralSampler_2D, build_masks                    # noqa: E402
import oracle_cdgs as OC                                                          # noqa: E402

WORKLOADS = {'qm9': 'vpsde_qm9_2d_cdgs', 'geom': 'vpsde_geom_2d_cdgs'}
PEAK_TFLOPS = 157.3


class Dense:
    """The dense torch evaluation with the model's call signature."""

    def __init__(self, sd, hp):
        self.sd, self.hp = sd, hp

    def __call__(self, t, x, node_mask, edge_mask, context=None, **kw):
        return OC.forward(self.sd, self.hp, t, x, node_mask, edge_mask, kw['edge_x'])


def time_steps(sampler, model, z, edge_z, node_mask, edge_mask, warmup, steps):
    st = sampler.init_state(z, edge_z)
    with torch.no_grad():
        for i in range(warmup):
            st = sampler.step(model, i, st, node_mask, edge_mask, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(warmup, warmup + steps):
            st = sampler.step(model, i, st, node_mask, edge_mask, None)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, st


def flops_per_step(model, n_nodes):
    D, L = model.nf, model.n_layers
    cat = 2 * D // L
    catp = (cat + 31) // 32 * 32
    KA, KE = (L * catp + 154 + 63) // 64 * 64, (L * catp + 192 + 63) // 64 * 64
    Nn, R = sum(n_nodes), sum(n * n for n in n_nodes)
    B = len(n_nodes)
    pair_block = 393216 + D * catp                                           # E0 | E1, edge feed-forward, readout (padded as run)
    node_block = 2 * D * D + 3 * D * D + 2 * (2 * D * D) + D * catp + 2 * (2 * D * D)   # gin_nn, q k v, node FF, readout, FF(h_i)
    macs = R * (L * pair_block + D * D + KE * 2 * D + 2 * D * D + D * 32)
    macs += Nn * (L * node_block + D * D + KA * D + D * (D // 2) + (D // 2) * 32)
    macs += B * (D * 2 * D + 2 * D * D + D * 2 * D * L)
    return 2 * macs, 2 * R * L * 393216


def kernel_split(csv_path, sampler_steps):
    """kc_* rows of a rocprofv3 kernel-stats table -> {kernel: ms per sampler step}"""
    out = {}
    with open(csv_path) as f:
        for row in csv.DictReader(f):
            name = row['Name']
            if 'kc_' not in name:
                continue
            m = re.search(r'(kc_[a-z0-9_]+)(<[^>]*>|ILi\dE)?', name)
            key = (m.group(1) + (m.group(2) or '').replace(' ', '')) if m else name
            out[key] = round(out.get(key, 0.0) + float(row['TotalDurationNs']) / sampler_steps * 1e-6, 4)
    return dict(sorted(out.items(), key=lambda kv: -kv[1]))


def split_record(args, model, sampler, z, edge_z, nm, em, base):
    """--split on | both: the legs of one batch; returns the record"""
    forms = ['split'] if args.split == 'on' else ['exact', 'split']
    ran, legs, finite = {}, {f: [] for f in forms}, True
    for f in forms:                                                                  # shared warm-up: plan, blob and tape exist before any leg
        model.bf16x3 = f == 'split'
        time_steps(sampler, model, z, edge_z, nm, em, args.warmup, 1)
        ran[f] = None if model.last_flags is None else int(model.last_flags[3].item())
    for _ in range(args.repeats):
        for f in forms:
            model.bf16x3 = f == 'split'
            ms, st = time_steps(sampler, model, z, edge_z, nm, em, 0, args.steps)
            legs[f].append(round(ms, 3))
            finite = finite and bool(torch.isfinite(st['x']).all() and torch.isfinite(st['edge_x']).all())
    model.bf16x3 = False
    assert ran['split'] == 1 and ran.get('exact') is None, ran
    out = dict(base, split=args.split, repeats=args.repeats, finite=finite, split_form_ran=ran['split'])
    for f in forms:
        mean = sum(legs[f]) / len(legs[f])
        out.update({f + '_ms_per_step_legs': legs[f], f + '_ms_per_step': round(mean, 3),
                    f + '_spread_ms': round(max(legs[f]) - min(legs[f]), 3),
                    f + '_fraction_of_fp32_mfma_peak': round(base['flops_per_step'] / mean * 1e-9 / PEAK_TFLOPS, 4)})
    if args.split == 'both':
        spread = max(out['exact_spread_ms'], out['split_spread_ms'])
        out.update(split_over_exact_time=round(out['split_ms_per_step'] / out['exact_ms_per_step'], 4), spread_ms=spread,
                   split_faster_beyond_spread=bool(out['exact_ms_per_step'] - out['split_ms_per_step'] > spread))
    return out


def time_round(run, z, edge_z):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        x, e = run(z, edge_z)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, bool(torch.isfinite(x).all() and torch.isfinite(e).all()), (x, e)


def round_record(args, cfg, model, ns, sampler, z, edge_z, nm, em):
    """--round: the legs of one batch, per weight form; returns {weight form: record}"""
    from jodo_amd.graphed import GraphedDPMRound2D
    from jodo_amd.mix_dpm_solver import DPM_Solver_2D
    cfg_r = configs.get(WORKLOADS[args.workload])
    cfg_r.sampling.method, cfg_r.sampling.steps = 'dpm_2d', args.nfe
    solver = DPM_Solver_2D(ns, cfg_r)
    runs = {'eager': lambda a, b: solver.sampling(model, a, nm, em, b, None)}
    if args.graph:
        runs['replayed'] = lambda a, b: GraphedDPMRound2D(solver, model, nm, em).run(a, b)
    repeats, out = max(args.repeats, 2), {}
    for form in {'off': ['exact'], 'on': ['split'], 'both': ['exact', 'split']}[args.split]:
        model.bf16x3 = form == 'split'
        anc_ms, _ = time_steps(sampler, model, z, edge_z, nm, em, args.warmup, args.steps)
        ends = {k: time_round(run, z, edge_z)[2] for k, run in runs.items()}            # one untimed round of each
        legs, finite = {k: [] for k in runs}, True
        for _ in range(repeats):
            for k, run in runs.items():                                                  # eager, replayed, eager, replayed, ...
                sec, ok, _ = time_round(run, z, edge_z)
                legs[k].append(round(sec, 4))
                finite = finite and ok
        rec = dict(split_form_ran=None if model.last_flags is None else int(model.last_flags[3].item()), finite=finite,
                   ancestral_ms_per_step=round(anc_ms, 3), ancestral_steps_timed=args.steps,
                   ancestral_1000_step_round_s_as_step_time_x_1000_not_run=round(anc_ms, 3))
        for k in runs:
            mean = sum(legs[k]) / len(legs[k])
            rec.update({k + '_s_per_round_legs': legs[k], k + '_s_per_round': round(mean, 4),
                        k + '_spread_s': round(max(legs[k]) - min(legs[k]), 4), k + '_ms_per_evaluation': round(mean / args.nfe * 1e3, 3),
                        k + '_ms_per_evaluation_over_ancestral_step': round(mean / args.nfe * 1e3 / anc_ms, 4)})
        if args.graph:
            spread = max(rec['eager_spread_s'], rec['replayed_spread_s'])
            rec.update(replayed_over_eager_time=round(rec['replayed_s_per_round'] / rec['eager_s_per_round'], 4), spread_s=spread,
                       replay_faster_beyond_spread=bool(rec['eager_s_per_round'] - rec['replayed_s_per_round'] > spread),
                       replayed_equals_eager=bool(torch.equal(ends['eager'][0], ends['replayed'][0])
                                                  and torch.equal(ends['eager'][1], ends['replayed'][1])))
        out[form] = rec
    model.bf16x3 = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='qm9', choices=sorted(WORKLOADS))
    ap.add_argument('--batches', default='500,2000')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--kernel-stats-steps', type=int, default=None, help='sampler steps (warm-up included) of the profiled run')
    ap.add_argument('--split', default='off', choices=['off', 'on', 'both'], help='the opt-in split-bf16 form (model.bf16x3)')
    ap.add_argument('--repeats', type=int, default=3, help='--split on | both: timed legs per form')
    ap.add_argument('--kernel-stats-exact', default=None, help='--split both: kernel-stats CSV of the exact form\'s profiled run')
    ap.add_argument('--round', action='store_true', help="complete 'dpm_2d' rounds instead of single ancestral steps")
    ap.add_argument('--nfe', type=int, default=50, help='--round: network evaluations per round')
    ap.add_argument('--graph', action='store_true', help='--round: also time the replayed form (GraphedDPMRound2D)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = configs.get(WORKLOADS[args.workload])
    cfg.device = dev
    model = deterministic_init_(get_model_class('CDGS')(cfg), seed=42).to(dev).eval()
    dense = Dense({k: v.detach().clone() for k, v in model.state_dict().items()}, OC.hparams(cfg))
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    sampler = AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, cfg.sampling.steps), cfg.model.pred_data, cfg.model.self_cond)
    dist = get_node_dist(load_dataset_info(cfg.data.info_name))
    batches = [int(b) for b in args.batches.split(',')]
    rounds = dict(tool='tools/bench_cdgs.py', workload=args.workload, config=WORKLOADS[args.workload], method='dpm_2d',
                  solver='singlestep_fixed order 2', nfe=args.nfe, repeats=max(args.repeats, 2), graph=bool(args.graph), split=args.split,
                  batches={})
    for B in batches:
        torch.manual_seed(42)
        n_nodes = dist.sample(B).tolist()
        N = int(max(n_nodes))
        nm, em = build_masks(n_nodes, N, dev)
        z = sample_gaussian_with_mask((B, N, cfg.data.atom_types), dev, nm)
        edge_z = sample_symmetric_edge_feature_noise(B, N, cfg.model.edge_ch, em)
        pairs = sum(n * (n - 1) for n in n_nodes)
        flops, pair_flops = flops_per_step(model, n_nodes)
        if args.round:
            rec = dict(batch=B, padded_width=N, atoms=sum(n_nodes), ordered_pairs=pairs)
            rec.update(round_record(args, cfg, model, ns, sampler, z, edge_z, nm, em))
            rounds['batches'][str(B)] = rec
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, 'cdgs_dpm_round_%s_nfe%d.json' % (args.workload, args.nfe)), 'w') as f:
                json.dump(rounds, f, indent=1)
            print(json.dumps(rec), flush=True)
            del z, edge_z
            torch.cuda.empty_cache()
            continue
        if args.split != 'off':
            base = dict(tool='tools/bench_cdgs.py', workload=args.workload, config=WORKLOADS[args.workload], batch=B, padded_width=N,
                        atoms=sum(n_nodes), ordered_pairs=pairs, edge_rows_executed=sum(n * n for n in n_nodes), steps=args.steps,
                        warmup=args.warmup, flops_per_step=flops, peak_tflops=PEAK_TFLOPS)
            out = split_record(args, model, sampler, z, edge_z, nm, em, base)
            ksteps = args.kernel_stats_steps or args.warmup + args.steps
            for key, path in (('split', args.kernel_stats), ('exact', args.kernel_stats_exact)):
                if path and B == max(batches):
                    out[key + '_kernel_ms_per_step'] = kernel_split(path, ksteps)
                    out[key + '_kernel_stats_source'] = os.path.basename(path)
            os.makedirs(args.out_dir, exist_ok=True)
            name = 'cdgs_%s_b%d_split%s.json' % (args.workload, B, '' if args.split == 'both' else '_on')
            with open(os.path.join(args.out_dir, name), 'w') as f:
                json.dump(out, f, indent=1)
            print(json.dumps(out), flush=True)
            del z, edge_z
            torch.cuda.empty_cache()
            continue
        ms, st = time_steps(sampler, model, z, edge_z, nm, em, args.warmup, args.steps)
        out = dict(tool='tools/bench_cdgs.py', workload=args.workload, config=WORKLOADS[args.workload], batch=B, padded_width=N,
                   atoms=sum(n_nodes), ordered_pairs=pairs, edge_rows_executed=sum(n * n for n in n_nodes), steps=args.steps,
                   warmup=args.warmup, hip_ms_per_step=round(ms, 3), hip_ns_per_ordered_pair=round(ms * 1e6 / pairs, 2),
                   flops_per_step=flops, pair_chain_flops_per_step=pair_flops, hip_tflops=round(flops / ms * 1e-9, 2),
                   hip_fraction_of_fp32_mfma_peak=round(flops / ms * 1e-9 / PEAK_TFLOPS, 4), peak_tflops=PEAK_TFLOPS,
                   finite=bool(torch.isfinite(st['x']).all() and torch.isfinite(st['edge_x']).all()))
        if not args.no_baseline:
            dms, dst = time_steps(sampler, dense, z, edge_z, nm, em, min(args.warmup, 2), args.steps)
            out.update(dense_torch_ms_per_step=round(dms, 3), dense_torch_ns_per_ordered_pair=round(dms * 1e6 / pairs, 2),
                       hip_over_dense_time=round(ms / dms, 4), hip_not_slower_than_dense=bool(ms <= dms),
                       dense_padded_positions=B * N * N, dense_finite=bool(torch.isfinite(dst['x']).all()))
        if args.kernel_stats and B == max(batches):
            out['kernel_ms_per_step'] = kernel_split(args.kernel_stats, args.kernel_stats_steps or args.warmup + args.steps)
            out['kernel_stats_source'] = os.path.basename(args.kernel_stats)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, 'cdgs_%s_b%d.json' % (args.workload, B)), 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out), flush=True)
        del z, edge_z, st
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

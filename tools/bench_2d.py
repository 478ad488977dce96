"""Benchmark of the 2-D sampling step (DGT_concat_2D + AncestralSampler_2D) at the configs' evaluation batch, and of the baseline a
user without the HIP path would run on the same GPU: the dense torch evaluation of the same network (tests/oracle2d.py) on the
device, chunked by molecules to fit memory, under the same sampler.

    python tools/bench_2d.py --workload zinc|moses [--batch 2000] [--steps 20] [--warmup 3] [--baseline-steps 3] [--no-baseline]
                             [--walk directed|pair|both] [--kernel-stats CSV] [--out FILE]
    python tools/bench_2d.py --workload zinc|moses --split exact|split|both [--walk directed|pair] [--kernel-stats CSV]
                             [--kernel-stats-exact CSV] [--out profiles/dgt2d_zinc_b2000_split.json]
    python tools/bench_2d.py --workload zinc|moses --round [--steps 1000] [--batches 2000,128] [--forms a,b,c,cd] [--repeat 1]
                             [--parent-json FILE] [--out profiles/dgt2d_round_zinc.json]
    python tools/bench_2d.py --workload zinc|moses --round --nfe 50 [--dpm-method singlestep_fixed|multistep] [--batches 2000,128]
                             [--forms d,dg] [--repeat 1] [--out profiles/dgt2d_dpm2d_round_zinc_nfe50.json]

Atom counts are drawn from the training histogram (tests/golden/n_nodes_2d.json, seed 42).  Timing as bench.py does it: warm-up,
synchronise, `steps` sampler.step calls, synchronise.  Prints one JSON line: ms/step, molecules/s at 1000 steps, the directed-edge
count, ns per directed edge per step, and the same for the torch baseline with the ratio.

--walk: the attention walk of the score network.  `directed` (default) is the run described above, unchanged; `pair` sets
model.pair_attention (the opt-in pair-symmetric walk); `both` alternates directed, pair, directed, pair on the same batch in this one
process and reports ms/step per form with the spread of its two runs (no torch baseline).  --kernel-stats: the `rocprofv3
--kernel-trace --stats` kernel table of the `--walk pair` command with the same --steps and --warmup (the profiler wraps the process,
so that is a run of its own); its k2d_* rows, divided by the sampler steps of that command, become `pair_kernel_ms_per_step`.  --out writes the record.

--split: the arithmetic of the node GEMMs and the pair update.  `exact` (default) changes nothing; `split` sets model.bf16x3 (the opt-in
three-term bf16 form); `both` alternates exact, split, exact, split on the same batch in this one process, exactly as `--walk both` does
for the attention walk, and reports ms/step per form, both exact legs and their spread (no torch baseline).  It combines with
`--walk directed|pair` (not `both`: one comparison per command) and with `--round` (every form of the round is then run exact, split,
exact, split).  --kernel-stats / --kernel-stats-exact: the rocprofv3 kernel tables of the `--split split` / `--split exact` command with
the same --walk, --steps and --warmup; their k2d_* rows per sampler step become `split_kernel_ms_per_step` / `exact_kernel_ms_per_step`.

--round: ONE complete sampling round of `--steps` steps per batch size and form, timed from the initial state to the last step
(weights packed by a 3-step round before; plan creation and graph capture are inside the timed round):
    a   eager, torch draws — what AncestralSampler_2D.sampling did before in-kernel noise existed; its host decode
        (post_process_2D + mol_process_2D) is timed separately
    b   eager, both draws of a step inside jodo_sampler_step_2d_rng
    c   one captured step replayed (GraphedAncestralRound2D), in-kernel draws
    cd  c plus the device decode (jodo_decode_2d) and the per-molecule host tuples
    d   DPM-Solver++ for 2-D graphs (sampling.method 'dpm_2d', DPM_Solver_2D, order 2), eager, --nfe evaluations
    dg  d with one captured step replayed (GraphedDPMRound2D)
--nfe selects the DPM leg: the forms default to d,dg, the record counts the network evaluations of a round and goes to a file of its own
(default profiles/dgt2d_dpm2d_round_<workload>_nfe<NFE>.json).  A round of form d / dg costs NFE evaluations where a round of a - cd costs
--steps of them; the tool measures, it predicts nothing, and it says nothing about sample quality at a given NFE.
Form a uses nothing newer than the sampler itself, so this file copied into a checkout of an older commit measures that commit
(`--forms a --repeat 2`); `--parent-json` embeds such a record, with the spread of its runs, next to this run's numbers.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from jodo_amd import configs                                                      # noqa: E402
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP                     # noqa: E402
from jodo_amd.models import get_model_class, get_node_dist, deterministic_init_   # noqa: E402
from jodo_amd.models.utils import sample_gaussian_with_mask, sample_symmetric_edge_feature_noise      # noqa: E402
from jodo_amd.sampling import AncestralSampler_2D, build_masks                    # noqa: E402
import oracle2d as O2                                                             # noqa: E402

WORKLOADS = {'zinc': ('vpsde_zinc_2d_jodo', 'zinc250k'), 'moses': ('vpsde_moses_2d_jodo', 'moses')}


class ChunkedDense:
    """The dense torch evaluation on the device, `chunk` molecules at a time (each chunk cut to its own largest molecule)."""

    def __init__(self, sd, hp, n_nodes, chunk):
        self.sd, self.hp, self.n, self.chunk = sd, hp, n_nodes, chunk

    def __call__(self, t, xh, node_mask, edge_mask, context=None, **kw):
        B, N = xh.shape[0], xh.shape[1]
        em = edge_mask.reshape(B, N, N, 1)
        ox, oe = torch.zeros_like(xh), torch.zeros_like(kw['edge_x'])
        for lo in range(0, B, self.chunk):
            hi = min(lo + self.chunk, B)
            n = int(max(self.n[lo:hi]))
            cut = lambda v, two: None if v is None else (v[lo:hi, :n, :n] if two else v[lo:hi, :n])
            a, b = O2.forward_dense(self.sd, self.hp, cut(xh, 0), cut(node_mask, 0), cut(em, 1).reshape(-1, 1), cut(kw['edge_x'], 1),
                                    cut(kw.get('cond_x'), 0), cut(kw.get('cond_edge_x'), 1), kw['noise_level'][lo:hi])
            ox[lo:hi, :n], oe[lo:hi, :n, :n] = a, b
        return ox, oe


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


def kernel_split(csv_path, sampler_steps):
    """k2d_* rows of a rocprofv3 kernel-stats table -> {kernel: ms per sampler step}"""
    import csv
    import re
    known = (('13k2d_attn_pair', 'k2d_attn_pair'), ('k2d_attnILb1E', 'k2d_attn<true>'), ('k2d_attnILb0E', 'k2d_attn<false>'),
             ('k2d_gemmILi4ELi2E', 'k2d_gemm<4,2>'), ('k2d_gemmILi1ELi1E', 'k2d_gemm<1,1>'), ('k2d_gemm_sILi4ELi2E', 'k2d_gemm_s<4,2>'),
             ('k2d_gemm_sILi2ELi2E', 'k2d_gemm_s<2,2>'), ('k2d_gemm_sILi1ELi2E', 'k2d_gemm_s<1,2>'), ('10k2d_pair_s', 'k2d_pair_s'))
    out = {}
    with open(csv_path) as f:
        for row in csv.DictReader(f):
            name = row['Name']
            if 'k2d_' not in name:
                continue
            key = next((nice for tag, nice in known if tag in name), None)         # mangled names (older rocprofv3)
            if key is None:                                                        # demangled: "... k2d_gemm<4, 2>(...)"
                m = re.search(r'(k2d_[a-z0-9_]+)(<[^>]*>)?', name)
                key = m.group(1) + (m.group(2) or '').replace(' ', '') if m else name
            out[key] = round(out.get(key, 0.0) + float(row['TotalDurationNs']) / sampler_steps * 1e-6, 4)
    return dict(sorted(out.items(), key=lambda kv: -kv[1]))


def walk_leg(args, model, sampler, z, edge_z, node_mask, edge_mask, out):
    """--walk both: directed, pair, directed, pair on the same batch; --walk pair: the pair form alone."""
    order = ['directed', 'pair', 'directed', 'pair'] if args.walk == 'both' else ['pair']
    runs = {w: [] for w in order}
    walked = {}
    for w in order:
        model.pair_attention = (w == 'pair')
        ms, st = time_steps(sampler, model, z, edge_z, node_mask, edge_mask, args.warmup, args.steps)
        runs[w].append(round(ms, 4))
        walked[w] = int(model.last_flags[2].item())
        out['finite'] = out.get('finite', True) and bool(torch.isfinite(st['x']).all() and torch.isfinite(st['edge_x']).all())
    model.pair_attention = False
    out['walk'] = args.walk
    out['order_of_runs'] = order
    for w, r in runs.items():
        out[w] = dict(runs_ms_per_step=r, ms_per_step=round(sum(r) / len(r), 4), spread_ms_per_step=round(max(r) - min(r), 4),
                      pair_walk_ran=walked[w])
    if args.walk == 'both':
        gain = out['directed']['ms_per_step'] - out['pair']['ms_per_step']
        out['pair_gain_ms_per_step'] = round(gain, 4)
        out['pair_faster_beyond_directed_spread'] = bool(gain > out['directed']['spread_ms_per_step'])
        out['step_sampler_calls'] = len(order) * (args.warmup + args.steps)
    return out


def split_leg(args, model, sampler, z, edge_z, node_mask, edge_mask, out):
    """--split both: exact, split, exact, split on the same batch; --split split: the split form alone.  --walk picks the attention walk
    of every leg."""
    order = ['exact', 'split', 'exact', 'split'] if args.split == 'both' else ['split']
    runs = {w: [] for w in order}
    ran = {}
    model.pair_attention = (args.walk == 'pair')
    for w in order:
        model.bf16x3 = (w == 'split')
        ms, st = time_steps(sampler, model, z, edge_z, node_mask, edge_mask, args.warmup, args.steps)
        runs[w].append(round(ms, 4))
        ran[w] = dict(split_form_ran=int(model.last_flags[3].item()), pair_walk_ran=int(model.last_flags[2].item()))
        out['finite'] = out.get('finite', True) and bool(torch.isfinite(st['x']).all() and torch.isfinite(st['edge_x']).all())
    model.bf16x3 = model.pair_attention = False
    out['split'] = args.split
    out['walk'] = args.walk
    out['order_of_runs'] = order
    for w, r in runs.items():
        out[w] = dict(runs_ms_per_step=r, ms_per_step=round(sum(r) / len(r), 4), spread_ms_per_step=round(max(r) - min(r), 4), **ran[w])
    if args.split == 'both':
        gain = out['exact']['ms_per_step'] - out['split']['ms_per_step']
        out['split_gain_ms_per_step'] = round(gain, 4)
        out['split_faster_beyond_exact_spread'] = bool(gain > out['exact']['spread_ms_per_step'])
        out['step_sampler_calls'] = len(order) * (args.warmup + args.steps)
    return out


def _setup(workload, batch, dev):
    cfg_name, info = WORKLOADS[workload]
    cfg = configs.get(cfg_name)
    torch.manual_seed(42)
    n_nodes = get_node_dist(O2.load_n_nodes_hist(os.path.join(ROOT, 'tests', 'golden', 'n_nodes_2d.json'), info)).sample(batch).tolist()
    N = max(n_nodes)
    node_mask, edge_mask = build_masks(n_nodes, N, dev)
    nd = cfg.data.atom_types + int(cfg.model.include_fc_charge)
    z = sample_gaussian_with_mask((batch, N, nd), dev, node_mask)
    edge_z = sample_symmetric_edge_feature_noise(batch, N, cfg.model.edge_ch, edge_mask)
    return cfg, n_nodes, node_mask, edge_mask, z, edge_z


def _one_round(form, cfg, model, ns, steps, n_nodes, node_mask, edge_mask, z, edge_z):
    """-> (seconds of the loop, seconds of the decode or None, finite)"""
    from jodo_amd import sampling as S
    from jodo_amd.utils import get_data_inverse_scaler
    if form in ('d', 'dg'):
        return _one_dpm_round(form, cfg, model, ns, steps, node_mask, edge_mask, z, edge_z)
    sampler = AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), True, True)
    if form != 'a':
        from jodo_amd import fused
        sampler.device_noise = fused.DeviceNoise.for_rank(42, 0, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        if form in ('c', 'cd'):
            from jodo_amd.graphed import GraphedAncestralRound2D
            x, e = GraphedAncestralRound2D(sampler, model, node_mask, edge_mask).run(z, edge_z)
        else:
            x, e = sampler.sampling(model, z, node_mask, edge_mask, edge_z, None)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dec = None
        if form == 'a':
            one_hot, fc, et = S.post_process_2D(x, cfg.data.atom_types, cfg.model.include_fc_charge, node_mask, get_data_inverse_scaler(cfg), e,
                                                edge_mask, cfg.data.compress_edge)
            mols = S.mol_process_2D(one_hot, fc, n_nodes, et)
            dec = time.perf_counter() - t1
        elif form == 'cd':
            mols = fused.mols_from_decoded_2d(*fused.decode_2d(cfg, x, e, fused.n_nodes_from_mask(node_mask)), n_nodes,
                                              include_fc=cfg.model.include_fc_charge)
            dec = time.perf_counter() - t1
        assert dec is None or len(mols) == len(n_nodes)
    return t1 - t0, dec, bool(torch.isfinite(x).all() and torch.isfinite(e).all())


def _one_dpm_round(form, cfg, model, ns, nfe, node_mask, edge_mask, z, edge_z):
    """One round of DPM_Solver_2D at `nfe` evaluations (cfg carries the method; order 2): eager (d) or graph replay (dg)."""
    from jodo_amd.mix_dpm_solver import DPM_Solver_2D
    cfg.sampling.steps = nfe
    solver = DPM_Solver_2D(ns, cfg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if form == 'dg':
        from jodo_amd.graphed import GraphedDPMRound2D
        x, e = GraphedDPMRound2D(solver, model, node_mask, edge_mask).run(z, edge_z)
    else:
        x, e = solver.sampling(model, z, node_mask, edge_mask, edge_z, None)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, None, bool(torch.isfinite(x).all() and torch.isfinite(e).all())


def dpm_evaluations(method, nfe):
    """Network evaluations of one order-2 round: the single-step solver makes 2 * (nfe // 2), the multistep one nfe."""
    return 2 * (nfe // 2) if method == 'singlestep_fixed' else nfe


def round_leg(args):
    torch.set_num_threads(8)
    dev = torch.device('cuda:0')
    cfg_name, _ = WORKLOADS[args.workload]
    model = deterministic_init_(get_model_class('DGT_concat_2D')(configs.get(cfg_name)), seed=7).to(dev).eval()
    out = dict(workload=args.workload, config=cfg_name, steps=args.steps, split=args.split, walk=args.walk, forms={
        'a': 'eager, torch draws', 'b': 'eager, in-kernel draws', 'c': 'graph replay, in-kernel draws', 'cd': 'c + device decode',
        'd': "DPM-Solver++ 'dpm_2d', eager", 'dg': "DPM-Solver++ 'dpm_2d', graph replay"}, batches={})
    if args.nfe is not None:
        out.update(nfe=args.nfe, dpm_solver_method=args.dpm_method, dpm_solver_order=2,
                   evaluations_per_round=dpm_evaluations(args.dpm_method, args.nfe))
    for batch in [int(b) for b in args.batches.split(',')]:
        cfg, n_nodes, node_mask, edge_mask, z, edge_z = _setup(args.workload, batch, dev)
        ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
        _one_round('a', cfg, model, ns, 3, n_nodes, node_mask, edge_mask, z, edge_z)           # packs the weights, loads the kernels
        cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = args.dpm_method, 2
        rec = {}
        model.pair_attention = (args.walk == 'pair')
        for form in args.forms.split(','):
            is_dpm = form in ('d', 'dg')
            if is_dpm and args.nfe is None:
                raise SystemExit("forms d / dg need --nfe")
            count = dpm_evaluations(args.dpm_method, args.nfe) if is_dpm else args.steps       # network evaluations of the round

            def one(tag):
                loop, dec, finite = _one_round(form, cfg, model, ns, args.nfe if is_dpm else args.steps, n_nodes, node_mask, edge_mask, z, edge_z)
                total = loop + (dec or 0.0)
                r = dict(ms_per_step=round(loop / count * 1e3, 4), round_s=round(loop, 3),
                         decode_ms=None if dec is None else round(dec * 1e3, 2), molecules_per_s=round(batch / total, 2), finite=finite)
                print(json.dumps(dict(batch=batch, form=form, **tag, **r)), flush=True)
                return r

            def summary(runs):
                return dict(runs=runs, ms_per_step=round(sum(r['ms_per_step'] for r in runs) / len(runs), 4),
                            spread_ms_per_step=round(max(r['ms_per_step'] for r in runs) - min(r['ms_per_step'] for r in runs), 4))
            if args.split == 'exact':
                runs = [one({}) for _ in range(args.repeat)]
                rec[form] = runs[0] if args.repeat == 1 else summary(runs)
                continue
            order = ['exact', 'split', 'exact', 'split'] if args.split == 'both' else ['split']
            legs = {w: [] for w in order}
            for w in order * args.repeat:
                model.bf16x3 = (w == 'split')
                legs[w].append(dict(one(dict(split=w)), split_form_ran=int(model.last_flags[3].item())))
            model.bf16x3 = False
            rec[form] = dict(order_of_runs=order * args.repeat, **{w: summary(r) for w, r in legs.items()})
            if args.split == 'both':
                gain = rec[form]['exact']['ms_per_step'] - rec[form]['split']['ms_per_step']
                rec[form].update(split_gain_ms_per_step=round(gain, 4),
                                 split_faster_beyond_exact_spread=bool(gain > rec[form]['exact']['spread_ms_per_step']))
        model.pair_attention = False
        if 'a' in rec and 'c' in rec:
            rec['c_over_a'] = round(rec['c']['ms_per_step'] / rec['a']['ms_per_step'], 4)
        out['batches'][str(batch)] = dict(max_n=max(n_nodes), atoms=sum(n_nodes), **rec)
    if args.parent_json:
        with open(args.parent_json) as f:
            out['parent_commit'] = json.load(f)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--round', action='store_true', help='time complete sampling rounds in the forms a, b, c, cd (see the module docstring)')
    ap.add_argument('--batches', default='2000,128')
    ap.add_argument('--forms', default=None, help='default a,b,c,cd; d,dg with --nfe')
    ap.add_argument('--nfe', type=int, default=None, help="--round: the DPM leg (sampling.method 'dpm_2d') at this many network evaluations")
    ap.add_argument('--dpm-method', choices=('singlestep_fixed', 'multistep'), default='singlestep_fixed', help='order 2 either way')
    ap.add_argument('--repeat', type=int, default=1)
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--workload', choices=sorted(WORKLOADS), default='zinc')
    ap.add_argument('--batch', type=int, default=2000)
    ap.add_argument('--steps', type=int, default=None, help='default 20; 1000 with --round')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--baseline-steps', type=int, default=3)
    ap.add_argument('--baseline-chunk', type=int, default=250)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--walk', choices=('directed', 'pair', 'both'), default='directed', help='attention walk of the score network')
    ap.add_argument('--kernel-stats', default=None, help='rocprofv3 kernel-stats CSV of a run of the same command line')
    ap.add_argument('--split', choices=('exact', 'split', 'both'), default='exact',
                    help='arithmetic of the node GEMMs and the pair update: exact fp32 (default), the opt-in split-bf16 form (model.bf16x3), or both alternated')
    ap.add_argument('--kernel-stats-exact', default=None, help='--split: rocprofv3 kernel-stats CSV of the --split exact run of the same command line')
    args = ap.parse_args()
    if args.split != 'exact' and args.walk == 'both':
        ap.error('--split %s goes with --walk directed or --walk pair: one comparison per command' % args.split)
    if args.round and args.walk == 'both':
        ap.error('--round goes with --walk directed or --walk pair')
    if args.steps is None:
        args.steps = 1000 if args.round else 20
    if args.forms is None:
        args.forms = 'd,dg' if args.nfe is not None else 'a,b,c,cd'
    if args.round and args.nfe is not None and args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'dgt2d_dpm2d_round_%s_nfe%d.json' % (args.workload, args.nfe))
    if args.round:
        return round_leg(args)
    torch.set_num_threads(8)
    dev = torch.device('cuda:0')
    cfg_name, info = WORKLOADS[args.workload]
    cfg = configs.get(cfg_name)
    model = deterministic_init_(get_model_class('DGT_concat_2D')(cfg), seed=7).to(dev).eval()
    torch.manual_seed(42)
    n_nodes = get_node_dist(O2.load_n_nodes_hist(os.path.join(ROOT, 'tests', 'golden', 'n_nodes_2d.json'), info)).sample(args.batch).tolist()
    B, N = args.batch, max(n_nodes)
    node_mask, edge_mask = build_masks(n_nodes, N, dev)
    nd = cfg.data.atom_types + int(cfg.model.include_fc_charge)
    z = sample_gaussian_with_mask((B, N, nd), dev, node_mask)
    edge_z = sample_symmetric_edge_feature_noise(B, N, cfg.model.edge_ch, edge_mask)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    sampler = AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, 1000), True, True)
    directed = sum(n * (n - 1) for n in n_nodes)
    if args.split != 'exact':
        out = dict(workload=args.workload, config=cfg_name, batch=B, max_n=N, atoms=sum(n_nodes), directed_edges=directed, steps=args.steps,
                   warmup=args.warmup)
        split_leg(args, model, sampler, z, edge_z, node_mask, edge_mask, out)
        for key, path in (('split', args.kernel_stats), ('exact', args.kernel_stats_exact)):
            if path:
                out[key + '_kernel_ms_per_step'] = kernel_split(path, args.warmup + args.steps)
                out[key + '_kernel_stats'] = path + ' (rocprofv3 --kernel-trace --stats of the --split %s command, same walk, steps and warm-up)' % key
        print(json.dumps(out))
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(out, f, indent=1)
                f.write('\n')
        return
    if args.walk != 'directed':
        out = dict(workload=args.workload, config=cfg_name, batch=B, max_n=N, atoms=sum(n_nodes), directed_edges=directed, steps=args.steps,
                   warmup=args.warmup)
        walk_leg(args, model, sampler, z, edge_z, node_mask, edge_mask, out)
        if args.kernel_stats:
            out['pair_kernel_ms_per_step'] = kernel_split(args.kernel_stats, args.warmup + args.steps)
            out['kernel_stats'] = args.kernel_stats + ' (rocprofv3 --kernel-trace --stats of the --walk pair command, same steps and warm-up)'
        print(json.dumps(out))
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(out, f, indent=1)
                f.write('\n')
        return
    ms, st = time_steps(sampler, model, z, edge_z, node_mask, edge_mask, args.warmup, args.steps)
    out = dict(workload=args.workload, config=cfg_name, batch=B, max_n=N, atoms=sum(n_nodes), directed_edges=directed, steps=args.steps,
               warmup=args.warmup, hip_ms_per_step=round(ms, 4), hip_molecules_per_s_1000_steps=round(B / (ms * 1e-3 * 1000), 2),
               hip_ns_per_directed_edge_step=round(ms * 1e6 / directed, 3), finite=bool(torch.isfinite(st['x']).all() and torch.isfinite(st['edge_x']).all()))
    if not args.no_baseline:
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        base = ChunkedDense(sd, O2.Hyper2D.from_config(cfg), n_nodes, args.baseline_chunk)
        bms, _ = time_steps(sampler, base, z, edge_z, node_mask, edge_mask, 2, args.baseline_steps)
        out.update(torch_dense_ms_per_step=round(bms, 3), torch_dense_molecules_per_s_1000_steps=round(B / (bms * 1e-3 * 1000), 3),
                   torch_dense_chunk=args.baseline_chunk, torch_dense_steps=args.baseline_steps, speedup_vs_torch_dense=round(bms / ms, 2))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

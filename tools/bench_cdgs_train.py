"""Benchmark of one optimiser step of CDGS (forward + backward + AdamW) through the HIP training path (CDGS.hip_training,
csrc/cdgs_train.hip) against loss.backward() through the dense torch evaluation of the same network (tests/oracle_cdgs.forward, float32,
whole padded batch at once) on the same GPU in the same command, under the same loss (jodo_amd.losses.get_step_fn) and optimiser.

    python tools/bench_cdgs_train.py [--batch 128] [--iters 8] [--warmup 2] [--repeats 3] [--pool 4] [--out-dir profiles] [--hip-only]
                                     [--split off|on|both] [--split-mask M]

Workload: QM9 config (vpsde_qm9_2d_cdgs), atom counts from the `qm9_with_h` training histogram (seed 42), a new batch every step (a
pool of `--pool` loader-shaped batches taken in turn, so every step meets other atom counts and another padded width), seeded weights.
The HIP leg runs under model.train() with the config's dropout 0.1; THE DENSE LEG HAS NO DROPOUT (the oracle has no mask generator of
its own): it does strictly less work per step.  Legs alternate HIP, dense, HIP, dense; the record holds every leg and the minimum.
Forward and backward alone are timed with device events on the engine of the pool's first batch.  torch.cuda.max_memory_allocated is
reset before each form's first timed leg.  The per-kernel split of one HIP step comes from torch.profiler; `--hip-only` runs nothing but
HIP steps, for a `rocprofv3 --kernel-trace --stats` run of its own.  Writes <out-dir>/train_cdgs_qm9_b<B>.json and prints the record.
--split (default off: everything above, unchanged): `on` runs the HIP legs with the opt-in split-bf16 training products
(model.train_bf16x3 = --split-mask; with --hip-only the command to profile for the split form's kernel table); `both` runs HIP steps only
and alternates the fp32 and the split form in this one process on the same pool of batches (fp32, split, fp32, split, ...: --repeats legs
of --iters steps per form after one shared warm-up of both), and writes <out-dir>/train_cdgs_qm9_b<B>_split.json: every leg's ms per
step, the mean and the spread (max - min) per form, split / fp32, and whether the split form is faster by more than the larger spread.
--split-mask (default 7): 1 forward products, 2 data gradients, 4 weight gradients.
Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import oracle_cdgs as OC                                                             # noqa: E402
from bench_classifier import event_ms                                                # noqa: E402
from bench_classifier_train import kernel_split                                      # noqa: E402
from jodo_amd import configs, losses as L                                            # noqa: E402
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP                        # noqa: E402
from jodo_amd.models import deterministic_init_, get_model_class, get_node_dist, load_dataset_info      # noqa: E402
from jodo_amd.models.ema import ExponentialMovingAverage                             # noqa: E402
from jodo_amd.sampling import build_masks                                            # noqa: E402
from jodo_amd.utils import get_data_scaler                                           # noqa: E402


class DenseCDGS(torch.nn.Module):
    """The dense torch oracle as a module with the model's call, on its own trainable copies of the weights."""

    def __init__(self, model, cfg):
        super().__init__()
        sd = model.state_dict()
        self.names = list(sd.keys())
        self.is_param = [not k.endswith('local_model.eps') for k in self.names]
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(sd[k].detach().clone()) for k, p in zip(self.names, self.is_param) if p])
        self.bufs = [sd[k].detach().clone() for k, p in zip(self.names, self.is_param) if not p]
        self.hp = OC.hparams(cfg)

    def forward(self, t, x, node_mask, edge_mask, **kw):
        ps, bufs = iter(self.ps), iter(self.bufs)
        sd = {k: (next(ps) if p else next(bufs)) for k, p in zip(self.names, self.is_param)}
        return OC.forward(sd, self.hp, t, x, node_mask, edge_mask, kw['edge_x'])


def loader_batch(cfg, n_nodes, seed):
    B, N = len(n_nodes), max(n_nodes)
    nm, em = build_masks(list(n_nodes), N, 'cpu')
    g = torch.Generator().manual_seed(seed)
    at = torch.randint(0, cfg.data.atom_types, (B, N), generator=g)
    bond = torch.triu(torch.randint(0, 4, (B, N, N), generator=g), 1)
    bond = bond + bond.transpose(1, 2)
    chans = [(bond > 0).float(), bond.float() / 3.] + ([(bond == 3).float()] if cfg.model.edge_ch == 3 else [])
    return dict(atom_mask=nm[..., 0], edge_mask=em, atom_one_hot=torch.nn.functional.one_hot(at, cfg.data.atom_types).float() * nm,
                edge_one_hot=torch.stack(chans, -1) * em.reshape(B, N, N, 1), formal_charges=torch.zeros(B, N, 1))


def split_both(args, hip, hip_step, counts, n_batches):
    """--split both: alternating legs of the fp32 and the split form of the HIP step; returns the record"""
    forms = (('fp32', 0), ('split', args.split_mask))

    def leg(mask, iters):
        hip.train_bf16x3 = mask
        ms = event_ms(hip_step, iters)
        assert hip.last_train_form == mask, (hip.last_train_form, mask)
        return ms
    for _ in range(max(1, args.warmup)):                        # one shared warm-up: every batch of the pool in both forms
        for _, mask in forms:
            leg(mask, n_batches)
    legs = {name: [] for name, _ in forms}
    for _ in range(args.repeats):
        for name, mask in forms:
            legs[name].append(leg(mask, args.iters))
    hip.train_bf16x3 = False
    mean = {k: sum(v) / len(v) for k, v in legs.items()}
    spread = {k: max(v) - min(v) for k, v in legs.items()}
    return dict(workload='qm9_with_h histogram, one optimiser step (forward + backward + AdamW), a new batch every step, HIP legs only',
                batch=args.batch, split='both', split_mask=args.split_mask, iters=args.iters, repeats=args.repeats,
                pool=[dict(atoms=int(sum(n)), padded_width=int(max(n)), tile_rows=int(args.batch * max(n) ** 2)) for n in counts],
                fp32_ms_runs=legs['fp32'], split_ms_runs=legs['split'], fp32_ms=mean['fp32'], split_ms=mean['split'],
                fp32_spread_ms=spread['fp32'], split_spread_ms=spread['split'], split_over_fp32_time=mean['split'] / mean['fp32'],
                split_faster_beyond_spread=bool(mean['fp32'] - mean['split'] > max(spread.values())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--iters', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--pool', type=int, default=4)
    ap.add_argument('--hip-only', action='store_true')
    ap.add_argument('--split', default='off', choices=['off', 'on', 'both'], help='the opt-in split-bf16 training products (model.train_bf16x3)')
    ap.add_argument('--split-mask', type=int, default=7, help='--split on | both: 1 forward products, 2 data gradients, 4 weight gradients')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cdgs_train needs a GPU: nothing is measured without one")
    dev = torch.device('cuda:0')
    cfg = configs.get('vpsde_qm9_2d_cdgs')
    cfg.device = dev
    B = args.batch
    torch.manual_seed(42)
    dist = get_node_dist(load_dataset_info('qm9_with_h'))
    counts = [dist.sample(B).tolist() for _ in range(args.pool)]
    batches = [loader_batch(cfg, n, 100 + i) for i, n in enumerate(counts)]
    hip = deterministic_init_(get_model_class('CDGS')(cfg), seed=7).to(dev)
    if args.split == 'on':
        hip.train_bf16x3 = args.split_mask
    dense = DenseCDGS(hip, cfg).to(dev)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)

    def stepper(model):
        state = dict(model=model, optimizer=L.get_optimizer(cfg, model.parameters()),
                     ema=ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_decay), step=1)
        fn = L.get_step_fn(ns, True, L.optimization_manager(cfg), get_data_scaler(cfg), cfg)
        at = [0]

        def step():
            at[0] += 1
            return fn(state, batches[at[0] % len(batches)])
        return step

    random.seed(0)
    hip_step, dense_step = stepper(hip), stepper(dense)
    if args.split == 'both':
        rec = split_both(args, hip, hip_step, counts, len(batches))
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, 'train_cdgs_qm9_b%d_split.json' % B), 'w') as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return
    forms = [('hip', hip_step, args.iters)] + ([] if args.hip_only else [('dense', dense_step, max(1, args.iters // 2))])
    first = {name: float(fn()) for name, fn, _ in forms}
    for _ in range(args.warmup * len(batches)):                 # every batch of the pool once per warm-up round: engines and workspace exist
        for _, fn, _ in forms:
            fn()
    torch.cuda.synchronize()
    legs, peak, base = {name: [] for name, _, _ in forms}, {}, {}
    for r in range(args.repeats):
        for name, fn, it in forms:
            if r == 0:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base[name] = int(torch.cuda.memory_allocated())
            legs[name].append(event_ms(fn, it))
            if r == 0:
                peak[name] = int(torch.cuda.max_memory_allocated())
    # forward and backward alone, on the engine of the first batch
    n0 = counts[0]
    nm, em = build_masks(n0, max(n0), dev)
    eng = hip._train_engine(nm, em, dev)
    eng.set_form(args.split_mask if args.split == 'on' else 0)
    ts = [v.detach().contiguous() for v in hip.state_dict().values()]
    freq = hip._time_freq().to(dev)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, max(n0), cfg.data.atom_types, generator=g).to(dev) * nm).contiguous()
    ex = torch.randn(B, max(n0), max(n0), cfg.model.edge_ch, generator=g).to(dev)
    ex = ((ex + ex.transpose(1, 2)) * em.reshape(B, max(n0), max(n0), 1)).contiguous()
    t = torch.rand(B, generator=g).to(dev)
    d_x, d_e = torch.randn_like(x), torch.randn_like(ex)
    p = float(cfg.model.dropout)
    fwd_ms = event_ms(lambda: eng.forward(ts, freq, t, x, ex, p, 5), args.iters)
    bwd_ms = event_ms(lambda: eng.backward(ts, x, ex, d_x, d_e, p, 5), args.iters)
    rec = dict(workload='qm9_with_h histogram, one optimiser step (forward + backward + AdamW), a new batch every step', batch=B,
               pool=[dict(atoms=int(sum(n)), padded_width=int(max(n)), tile_rows=int(B * max(n) ** 2), sum_n2=int(sum(v * v for v in n))) for n in counts],
               train_bf16x3=hip.last_train_form, hip_dropout=p, dense_dropout=0.0, note='the dense leg has no dropout', iters=args.iters, repeats=args.repeats, first_step_loss=first,
               hip_ms=min(legs['hip']), hip_ms_runs=legs['hip'], hip_forward_ms=fwd_ms, hip_backward_ms=bwd_ms,
               hip_peak_bytes=peak['hip'], hip_baseline_bytes=base['hip'],
               hip_workspace_bytes=int(sum(s_['buf'].numel() for s_ in hip._train_pool['slots'] if s_['buf'] is not None)),
               hip_engine_workspace_bytes=int(eng.ws_bytes))
    if not args.hip_only:
        rec.update(dense_torch_ms=min(legs['dense']), dense_torch_ms_runs=legs['dense'], dense_peak_bytes=peak['dense'],
                   dense_baseline_bytes=base['dense'], dense_over_hip=min(legs['dense']) / min(legs['hip']))
        rec['hip_kernel_split'] = kernel_split(hip_step)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, 'train_cdgs_qm9_b%d%s.json' % (B, '_split_on' if args.split == 'on' else '')), 'w') as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()

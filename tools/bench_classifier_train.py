"""Benchmark of one optimiser step of the property classifier (forward + backward + Adam) through the HIP training path
(EGNN.hip_training, csrc/egnn_train.hip) against loss.backward() through the dense torch evaluation of the same network
(tools/bench_classifier.py DenseEGNN: per-edge tensors [B, N, N, nf] kept by autograd) on the same GPU in the same run.

    python tools/bench_classifier_train.py [--batches 96,1250] [--iters 10] [--warmup 3] [--repeats 3] [--out-dir profiles]

Workload: QM9 atom counts from the training histogram (seed 42), the published classifier's settings (nf 128, 7 layers, attention on,
no node attributes), seeded weights, one-hot atoms, positions 1.5 N(0, 1), random labels; B = 96 is the published classifier's training
batch.  Both forms are warmed up, then timed with device events over `--iters` steps per leg, `--repeats` legs each, alternating HIP,
dense, HIP, dense; the record holds every leg, the minimum and the spread.  torch.cuda.max_memory_allocated is reset before each form's
first timed leg and read after its last (the other form's persistent tensors are in the baseline, which is recorded too).  The
per-kernel split of one HIP step comes from torch.profiler (device time per kernel name).  Writes
<out-dir>/egnn_train_qm9_b<B>.json and prints the record.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_classifier import DenseEGNN, event_ms                                  # noqa: E402
from jodo_amd.cond_gen import EGNN, classifier_loss, get_classifier_step_fn      # noqa: E402
from jodo_amd.models import deterministic_init_, get_node_dist, load_dataset_info      # noqa: E402
from jodo_amd.sampling import build_masks, full_edge_index                       # noqa: E402


class DenseTrain(DenseEGNN):
    """DenseEGNN on its own trainable copies of the weights."""

    def __init__(self, egnn):
        super().__init__(egnn)
        self.params = torch.nn.ParameterList([torch.nn.Parameter(v.detach().clone()) for v in self.sd.values()])
        self.sd = dict(zip(self.sd.keys(), self.params))


def kernel_split(step, top=24):
    """Device time per kernel name over one call of `step`, largest first (microseconds); a string when the profiler is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        from torch.autograd import DeviceType
        rows = []
        for e in prof.key_averages():
            t = float(getattr(e, 'self_device_time_total', 0.0) or getattr(e, 'self_cuda_time_total', 0.0) or 0.0)
            if t > 0 and e.device_type == DeviceType.CUDA and 'Memcpy' not in e.key and 'Memset' not in e.key:      # kernels, not host ranges
                rows.append((e.key[:96], t, int(e.count)))
        rows.sort(key=lambda r: -r[1])
        total = sum(r[1] for r in rows)
        return dict(total_us=total, kernels=[dict(name=n, us=t, calls=c, share=t / total if total else 0.0) for n, t, c in rows[:top]])
    except Exception as e:                                                        # the record says so instead of holding numbers
        return "profiler unavailable: %r" % (e,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='96,1250')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classifier_train needs a GPU: nothing is measured without one")
    dev = torch.device('cuda:0')
    mean, mad = 75.3, 6.3
    for B in [int(b) for b in args.batches.split(',')]:
        hip = deterministic_init_(EGNN(5, 0, 128, n_layers=7, attention=True, node_attr=0), seed=11).to(dev)
        dense = DenseTrain(hip).to(dev)
        torch.manual_seed(42)
        n_nodes = get_node_dist(load_dataset_info('qm9_second_half')).sample(B).tolist()
        N = max(n_nodes)
        nm, em = build_masks(n_nodes, N, dev)
        g = torch.Generator().manual_seed(1)
        one_hot = F.one_hot(torch.randint(0, 5, (B, N), generator=g), 5).float().to(dev) * nm
        pos = 1.5 * torch.randn(B, N, 3, generator=g).to(dev) * nm
        label = (mean + mad * torch.randn(B, generator=g)).to(dev)
        kw = dict(h0=one_hot.reshape(B * N, 5), x=pos.reshape(B * N, 3), edges=full_edge_index(N, B, dev), edge_attr=None,
                  node_mask=nm.reshape(B * N, 1), edge_mask=em, n_nodes=N)
        opt_hip = torch.optim.Adam(hip.parameters(), lr=1e-4)
        opt_dense = torch.optim.Adam(dense.parameters(), lr=1e-4)
        hip_step_fn = get_classifier_step_fn(opt_hip, mean, mad)

        def hip_step():
            return hip_step_fn(hip, one_hot, pos, n_nodes, label)

        def dense_step():
            opt_dense.zero_grad(set_to_none=True)
            loss = classifier_loss(dense(**kw), label, mean, mad)
            loss.backward()
            opt_dense.step()
            return loss.detach()

        first = (float(hip_step()), float(dense_step()))                          # same weights, same batch: the two losses of step one
        for _ in range(args.warmup):
            hip_step(), dense_step()
        torch.cuda.synchronize()
        legs, peak, base = {'hip': [], 'dense': []}, {}, {}
        for r in range(args.repeats):
            for name, fn, it in (('hip', hip_step, args.iters), ('dense', dense_step, max(1, args.iters // 2))):
                if r == 0:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base[name] = int(torch.cuda.memory_allocated())
                legs[name].append(event_ms(fn, it))
                if r == 0:
                    peak[name] = int(torch.cuda.max_memory_allocated())
        rec = dict(workload='qm9 histogram, one optimiser step (forward + backward + Adam)', batch=B, atoms=int(sum(n_nodes)),
                   directed_edges=int(sum(n * (n - 1) for n in n_nodes)), padded_width=N, hidden_nf=128, n_layers=7, attention=True,
                   iters=args.iters, repeats=args.repeats, first_step_loss_hip=first[0], first_step_loss_dense=first[1],
                   hip_ms=min(legs['hip']), hip_ms_runs=legs['hip'], dense_torch_ms=min(legs['dense']), dense_torch_ms_runs=legs['dense'],
                   hip_spread=(max(legs['hip']) - min(legs['hip'])) / min(legs['hip']),
                   dense_spread=(max(legs['dense']) - min(legs['dense'])) / min(legs['dense']),
                   hip_peak_bytes=peak['hip'], hip_baseline_bytes=base['hip'], dense_peak_bytes=peak['dense'],
                   dense_baseline_bytes=base['dense'],
                   hip_workspace_bytes=int(sum(s_['buf'].numel() for s_ in hip._train_pool['slots'] if s_['buf'] is not None)))
        rec['dense_over_hip'] = rec['dense_torch_ms'] / rec['hip_ms']
        rec['hip_kernel_split'] = kernel_split(hip_step)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, 'egnn_train_qm9_b%d.json' % B), 'w') as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        del hip, dense, opt_hip, opt_dense
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

"""Benchmark of the property classifier (jodo_amd.cond_gen.EGNN, csrc/egnn_forward.hip) against a dense torch evaluation of the same
network on the same GPU, and its share of one conditional evaluation round.

    python tools/bench_classifier.py [--batches 1250,2500] [--iters 20] [--warmup 3] [--round-steps 50] [--no-round] [--out-dir profiles]

Workload: QM9 atom counts from the training histogram (seed 42), the published classifier's settings (nf 128, 7 layers, attention on,
no node attributes), seeded weights, one-hot atoms and positions 1.5 N(0, 1).  The dense form keeps the per-edge state as
[B, N, N, nf] on the device (first edge layer hoisted to the atoms as in the kernels, so it is the cheaper of the obvious torch forms).
Per batch size: both forms are warmed up, then timed with device events over `--iters` calls, alternating HIP, dense, HIP, dense;
outputs are compared.  Then one get_cond_sampling_eval_fn round (ancestral, `--round-steps` score-network evaluations) is timed with
each classifier, host clock around a device synchronise.  Writes <out-dir>/egnn_qm9_b<B>.json and prints the record: both times, their
ratio, the classifier's share of the round.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jodo_amd import configs                                                      # noqa: E402
from jodo_amd.cond_gen import EGNN                                                # noqa: E402
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP                     # noqa: E402
from jodo_amd.models import deterministic_init_, get_model_class, get_node_dist, load_dataset_info      # noqa: E402
from jodo_amd.sampling import build_masks, full_edge_index, get_cond_sampling_eval_fn                  # noqa: E402
from jodo_amd.utils import get_data_inverse_scaler                                # noqa: E402


class DenseEGNN(torch.nn.Module):
    """The same network in dense torch form on the weights of an EGNN module: per-edge tensors [B, N, N, nf]."""

    def __init__(self, egnn):
        super().__init__()
        self.sd = {k: v.detach() for k, v in egnn.state_dict().items()}
        self.nf, self.layers, self.attention, self.node_attr = egnn.hidden_nf, egnn.n_layers, egnn.attention, egnn.node_attr

    def forward(self, h0, x, edges, edge_attr, node_mask, edge_mask, n_nodes):
        sd, nf, N = self.sd, self.nf, n_nodes
        B = h0.shape[0] // N
        lin = lambda name, t: F.linear(t, sd[name + '.weight'], sd[name + '.bias'])
        h0, x, nm, em = h0.reshape(B, N, -1), x.reshape(B, N, 3), node_mask.reshape(B, N, 1), edge_mask.reshape(B, N, N, 1)
        radial = (x.unsqueeze(2) - x.unsqueeze(1)).square().sum(-1, keepdim=True)
        h = lin('embedding', h0)
        for l in range(self.layers):
            pre = 'gcl_%d.' % l
            w1 = sd[pre + 'edge_mlp.0.weight']
            src = F.linear(h, w1[:, :nf], sd[pre + 'edge_mlp.0.bias'])
            tgt = F.linear(h, w1[:, nf:2 * nf])
            m = F.silu(src.unsqueeze(2) + tgt.unsqueeze(1) + radial * w1[:, 2 * nf])
            m = F.silu(lin(pre + 'edge_mlp.2', m))
            if self.attention:
                m = m * torch.sigmoid(lin(pre + 'att_mlp.0', m))
            agg = (m * em).sum(2)
            feats = [h, agg] + ([h0] if self.node_attr else [])
            h = h + lin(pre + 'node_mlp.2', F.silu(lin(pre + 'node_mlp.0', torch.cat(feats, -1))))
        hd = lin('node_dec.2', F.silu(lin('node_dec.0', h))) * nm
        return lin('graph_dec.2', F.silu(lin('graph_dec.0', hd.sum(1)))).squeeze(-1)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


class _Nodes:
    def __init__(self, n):
        self.n = n

    def sample(self, k):
        assert k == len(self.n)
        return torch.as_tensor(self.n)


class _Ctx:
    def sample_batch(self, n_nodes):
        return torch.randn(len(n_nodes), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1250,2500')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--round-steps', type=int, default=50)
    ap.add_argument('--no-round', action='store_true')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classifier needs a GPU: nothing is measured without one")
    dev = torch.device('cuda:0')
    hip = deterministic_init_(EGNN(5, 0, 128, n_layers=7, attention=True, node_attr=0), seed=11).to(dev).eval()
    dense = DenseEGNN(hip).eval()
    cfg = configs.get('vpsde_qm9_cond_jodo')
    cfg.device = dev
    cfg.sampling.steps, cfg.sampling.method = args.round_steps, 'ancestral'
    score_model = None
    for B in [int(b) for b in args.batches.split(',')]:
        torch.manual_seed(42)
        n_nodes = get_node_dist(load_dataset_info('qm9_second_half')).sample(B).tolist()
        N = max(n_nodes)
        nm, em = build_masks(n_nodes, N, dev)
        g = torch.Generator().manual_seed(1)
        h0 = (F.one_hot(torch.randint(0, 5, (B, N), generator=g), 5).float().to(dev) * nm).reshape(B * N, 5)
        x = (1.5 * torch.randn(B, N, 3, generator=g).to(dev) * nm).reshape(B * N, 3)
        kw = dict(h0=h0, x=x, edges=full_edge_index(N, B, dev), edge_attr=None, node_mask=nm.reshape(B * N, 1), edge_mask=em, n_nodes=N)
        with torch.no_grad():
            for _ in range(args.warmup):
                o_hip, o_dense = hip(**kw), dense(**kw)
            torch.cuda.synchronize()
            legs = {'hip': [], 'dense': []}
            for _ in range(2):
                legs['hip'].append(event_ms(lambda: hip(**kw), args.iters))
                legs['dense'].append(event_ms(lambda: dense(**kw), max(1, args.iters // 4)))
        rec = dict(workload='qm9 histogram', batch=B, atoms=int(sum(n_nodes)), directed_edges=int(sum(n * (n - 1) for n in n_nodes)),
                   padded_width=N, hidden_nf=128, n_layers=7, attention=True, iters=args.iters,
                   hip_ms=min(legs['hip']), hip_ms_runs=legs['hip'], dense_torch_ms=min(legs['dense']), dense_torch_ms_runs=legs['dense'],
                   max_abs_diff=float((o_hip - o_dense).abs().max()), max_abs_out=float(o_dense.abs().max()))
        rec['dense_over_hip'] = rec['dense_torch_ms'] / rec['hip_ms']
        if not args.no_round:
            if score_model is None:
                score_model = deterministic_init_(get_model_class(cfg.model.name)(cfg), seed=7).to(dev).eval()
            ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
            norm = {cfg.cond_property: {'mean': 75.3, 'mad': 6.3}}
            for name, clf in (('warm', hip), ('hip', hip), ('dense', dense)):
                fn = get_cond_sampling_eval_fn(cfg, ns, _Nodes(n_nodes), B, B, get_data_inverse_scaler(cfg), prop_dist=_Ctx(), prop_norm=norm)
                torch.manual_seed(3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(score_model, clf)
                torch.cuda.synchronize()
                if name != 'warm':
                    rec['round_s_%s_classifier' % name] = time.perf_counter() - t0
            rec['round_steps'] = args.round_steps
            rec['classifier_share_of_round_hip'] = rec['hip_ms'] * 1e-3 / rec['round_s_hip_classifier']
            rec['classifier_share_of_round_dense'] = rec['dense_torch_ms'] * 1e-3 / rec['round_s_dense_classifier']
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, 'egnn_qm9_b%d.json' % B), 'w') as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))


if __name__ == '__main__':
    main()

"""Benchmark of the sub-structure geometry metric (jodo_amd.evaluation.geometry / mmd, csrc/geometry_kernels.hip): the extraction, the
batched MMD against a dense torch evaluation of the same formula on the same GPU, and the extraction's share of one sampling round.

    python tools/bench_geometry.py [--workloads qm9,geom] [--iters 20] [--warmup 3] [--repeats 3] [--mmd-n 20000] [--mmd-symbols 24]
                                   [--round-steps 50] [--no-round] [--no-dense] [--out-dir profiles]

Workloads: QM9 atom counts from the training histogram at B = 2500 and GEOM ones at B = 512 (seed 42); seeded random molecules — random
positions, hydrogen-rich types, every atom bonded to an earlier one plus some further bonds, edge types 1-4 — laid out as the decode
leaves them on the device; the symbol lists are the dataset's (read from tests/golden/geometry_cases.npz).  Every leg is warmed up, then
run `--repeats` times; the record keeps every run, the minimum and the spread (max - min) / min.
  extraction   the two launches (count + scan, write) with device events over `--iters` calls on pre-sized outputs (`extract_kernel_ms`),
               and the whole geometry function, its device->host copy of the sizes and the allocations included, by the host clock
               around a device synchronise (`extract_fn_ms`)
  MMD          `--mmd-symbols` segments of `--mmd-n` x `--mmd-n` seeded samples (lengths, angles, bimodal dihedrals in turn): the
               three launches alone with device events on uploaded tables (`mmd_kernel_ms`), the whole compute_mmd_many call with its
               table upload and the copy of the results (`mmd_fn_ms`), and `mmd_dense_torch_ms`: the same statistic for the same
               segments as dense float32 torch expressions in row blocks of 2000 (one exp per pair and kernel, no symmetry) on the same
               GPU, in the same run; `mmd_max_abs_diff` compares the two.  `mmd_exp_per_s` counts one exp per evaluated pair;
               `mmd_exp_rate_fraction` relates it to 256 CUs x 4 SIMDs x 8 lanes per cycle at 2.4 GHz.
  round        one get_sampling_fn round (ancestral, `--round-steps` score-network evaluations) with and without geometry=.
Writes <out-dir>/geometry_<workload>.json and prints the record.  Needs a GPU: there is no CPU fallback."""
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

from geometry_common import dataset_info                                          # noqa: E402
from jodo_amd import capi, configs                                                # noqa: E402
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP                     # noqa: E402
from jodo_amd.evaluation import GeometrySymbols, compute_mmd_many, get_geometry_fn             # noqa: E402
from jodo_amd.evaluation.mmd import tile_table                                    # noqa: E402
from jodo_amd.models import deterministic_init_, get_model_class, get_node_dist, load_dataset_info      # noqa: E402
from jodo_amd.sampling import get_sampling_fn                                     # noqa: E402
from jodo_amd.utils import get_data_inverse_scaler                                # noqa: E402

WORKLOADS = {'qm9': ('QM9', 'vpsde_qm9_uncond_jodo', 2500), 'geom': ('GeomDrug', 'vpsde_geom_uncond_jodo', 512)}
EXP_PEAK = 256 * 4 * 8 * 2.4e9                                # v_exp_f32 lanes per second: 8 cycles per 64-lane instruction and SIMD


def random_batch(T, n_nodes, aromatic, seed):
    rng = np.random.default_rng(seed)
    B, N = len(n_nodes), max(n_nodes)
    pos, at, et = np.zeros((B, N, 3), np.float32), np.zeros((B, N), np.uint8), np.zeros((B, N, N), np.uint8)
    p = np.full(T, 0.2 / (T - 2))
    p[0], p[1 if T == 5 else 2] = 0.45, 0.35                  # hydrogen and carbon
    codes = [0.55, 0.08, 0.02, 0.35] if aromatic else [0.84, 0.12, 0.04, 0.]
    for b, n in enumerate(n_nodes):
        side = (3.4 * n) ** (1. / 3.)
        pos[b, :n] = rng.uniform(-side / 2, side / 2, size=(n, 3))
        at[b, :n] = rng.choice(T, size=n, p=p)
        up = np.zeros((n, n), np.uint8)
        for a in range(1, n):
            up[rng.integers(0, a), a] = rng.choice([1, 2, 3, 4], p=codes)
        for _ in range(n // 8):
            a, c = sorted(rng.integers(0, n, size=2).tolist())
            if a != c:
                up[a, c] = rng.choice([1, 2, 3, 4], p=codes)
        et[b, :n, :n] = up + up.T
    return pos, at, et, np.asarray(n_nodes, np.int32)


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


def keep_runs(rec, key, runs):
    rec[key], rec[key + '_runs'], rec[key + '_spread'] = min(runs), runs, (max(runs) - min(runs)) / min(runs)


class _Nodes:
    def __init__(self, n):
        self.n = n

    def sample(self, k):
        assert k == len(self.n)
        return torch.as_tensor(self.n)


def extraction_launches(sy, pos, at, et, nd):
    """the two C calls on pre-sized buffers -> a function that launches them again (nothing allocated, nothing copied)"""
    dev = at.device
    B, N = at.shape
    cls = [torch.from_numpy(np.concatenate([c.reshape(-1), np.zeros(1, np.int32)])).to(dev) for c in sy.classes]
    Cb, Ca, Cd = (len(s) for s in sy.syms)
    Ct = Cb + Ca + Cd
    counts = torch.empty(Ct, B, dtype=torch.int32, device=dev)
    offsets = torch.empty(Ct, B, dtype=torch.int64, device=dev)
    host = torch.empty(Ct + 3, dtype=torch.int64, device=dev)
    L = capi.lib()
    head = (B, N, Cb, Ca, Cd, capi.ptr(cls[0]), capi.ptr(cls[1]), capi.ptr(cls[2]), capi.ptr(nd), capi.ptr(None), capi.ptr(pos), capi.ptr(at),
            capi.ptr(et))
    count = lambda: capi.check(L.jodo_geometry_count(*head, capi.ptr(counts), capi.ptr(offsets), capi.ptr(host), capi.ptr(host[Ct:]),
                                                     capi.current_stream_ptr()), 'jodo_geometry_count')
    count()
    sizes = host[:Ct].cpu().tolist()
    per_group = [sum(sizes[:Cb]), sum(sizes[Cb:Cb + Ca]), sum(sizes[Cb + Ca:])]
    outs = [torch.empty(max(n, 1), dtype=torch.float32, device=dev) for n in per_group]

    def both():
        count()
        capi.check(L.jodo_geometry_write(*head, capi.ptr(offsets), *[capi.ptr(o) for o in outs], *per_group, capi.current_stream_ptr()),
                   'jodo_geometry_write')
    return both, per_group, (cls, counts, offsets, host, outs)


def samples(rng, kind, n, shift):
    if kind == 0:
        return (1.10 + shift * 0.01 + 0.03 * rng.standard_normal(n)).astype(np.float32)
    if kind == 1:
        return (110. + shift * 2. + 5. * rng.standard_normal(n)).astype(np.float32)
    side = rng.random(n) < 0.5 + 0.1 * shift
    return np.where(side, -60. + 12. * rng.standard_normal(n), 175. - 15. * rng.random(n)).astype(np.float32)


def mmd_launches(src, tgt):
    """jodo_mmd_batched on uploaded tables -> (a function that launches it again, the output tensor)"""
    dev = src[0].device
    sizes = [(a.numel(), b.numel()) for a, b in zip(src, tgt)]
    S = len(sizes)
    so = np.concatenate([[0], np.cumsum([n for n, _ in sizes])])[:-1]
    to = np.concatenate([[0], np.cumsum([n for _, n in sizes])])[:-1]
    seg = torch.from_numpy(np.stack([so, [n for n, _ in sizes], to, [n for _, n in sizes]], 1).astype(np.int64)).to(dev)
    tiles_np, start_np = tile_table(sizes)
    tiles, start = torch.from_numpy(tiles_np).to(dev), torch.from_numpy(start_np).to(dev)
    T = len(tiles_np)
    src_all, tgt_all = torch.cat(src), torch.cat(tgt)
    params = torch.empty(S, 12, dtype=torch.float32, device=dev)
    partials = torch.empty(T, dtype=torch.float64, device=dev)
    out = torch.empty(S, dtype=torch.float64, device=dev)
    L = capi.lib()
    fn = lambda: capi.check(L.jodo_mmd_batched(S, T, capi.ptr(seg), capi.ptr(tiles), capi.ptr(start), capi.ptr(src_all), capi.ptr(tgt_all),
                                               2.0, 5, 0., capi.ptr(params), capi.ptr(partials), capi.ptr(out), capi.current_stream_ptr()),
                            'jodo_mmd_batched')
    return fn, out, T, (seg, tiles, start, src_all, tgt_all, params, partials)


def dense_torch_mmd(src, tgt, block=2000):
    """compute_mmd's formula as dense float32 torch expressions: bandwidth from the variance, then for XX, YY and XY every pair and every
    one of the five kernels, in row blocks; float64 accumulation of the block sums"""
    out = []
    for s, t in zip(src, tgt):
        z = torch.cat([s, t])
        n = z.numel()
        bw = (2. * n * ((z.double() - z.double().mean()) ** 2).sum() / (n * n - n) / 4.).float()

        def total(a, b):
            acc = torch.zeros((), dtype=torch.float64, device=a.device)
            for r0 in range(0, a.numel(), block):
                d2 = (a[r0:r0 + block, None] - b[None, :]) ** 2
                for i in range(5):
                    acc += torch.exp(-d2 / (bw * 2. ** i)).sum(dtype=torch.float64)
            return acc
        out.append(total(s, s) / s.numel() ** 2 + total(t, t) / t.numel() ** 2 - 2. * total(s, t) / (s.numel() * t.numel()))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='qm9,geom')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--mmd-n', type=int, default=20000)
    ap.add_argument('--mmd-symbols', type=int, default=24)
    ap.add_argument('--round-steps', type=int, default=50)
    ap.add_argument('--no-round', action='store_true')
    ap.add_argument('--no-dense', action='store_true')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry needs a GPU: nothing is measured without one")
    dev = torch.device('cuda:0')
    for w in args.workloads.split(','):
        dataset, cfg_name, B = WORKLOADS[w]
        info = dataset_info(dataset)
        sy = GeometrySymbols.from_dataset_info(info)
        cfg = configs.get(cfg_name)
        cfg.device = dev
        torch.manual_seed(42)
        n_nodes = get_node_dist(load_dataset_info(cfg.data.info_name)).sample(B).tolist()
        pos, at, et, nd = [torch.from_numpy(a).to(dev) for a in random_batch(sy.n_types, n_nodes, dataset == 'GeomDrug', 1)]
        rec = dict(workload='%s histogram, seeded random molecules' % w, dataset=dataset, batch=B, atoms=int(sum(n_nodes)),
                   padded_width=int(max(n_nodes)), iters=args.iters, repeats=args.repeats)
        # ---- extraction
        gfn = get_geometry_fn(cfg, sy)
        both, per_group, _hold = extraction_launches(sy, pos, at, et, nd)
        call = lambda: gfn(pos, at, et, nd)
        for _ in range(args.warmup):
            both(), call()
        keep_runs(rec, 'extract_kernel_ms', [event_ms(both, args.iters) for _ in range(args.repeats)])
        runs = []
        for _ in range(args.repeats):
            ms, res = clock_ms(call, args.iters)
            runs.append(ms)
        keep_runs(rec, 'extract_fn_ms', runs)
        rec['extract_values'] = dict(zip(('bond', 'angle', 'dihedral'), per_group))
        rec['extract_dropped'] = res['dropped']
        again = call()
        rec['extract_bit_identical'] = all(torch.equal(res['values'][s], again['values'][s]) for s in sy.all_syms)
        # ---- MMD
        rng = np.random.default_rng(2)
        n, S = args.mmd_n, args.mmd_symbols
        src = [torch.from_numpy(samples(rng, k % 3, n, 0.)).to(dev) for k in range(S)]
        tgt = [torch.from_numpy(samples(rng, k % 3, n, 1.)).to(dev) for k in range(S)]
        launch, out, T, _hold2 = mmd_launches(src, tgt)
        many = lambda: compute_mmd_many(src, tgt)
        for _ in range(args.warmup):
            launch(), many()
        keep_runs(rec, 'mmd_kernel_ms', [event_ms(launch, max(args.iters // 4, 2)) for _ in range(args.repeats)])
        runs = []
        for _ in range(args.repeats):
            ms, got = clock_ms(many, max(args.iters // 4, 2))
            runs.append(ms)
        keep_runs(rec, 'mmd_fn_ms', runs)
        pairs = T * capi.MMD_TILE * capi.MMD_TILE                 # evaluated pairs, padding of the edge tiles included
        rec.update(mmd_symbols=S, mmd_n=n, mmd_tiles=T, mmd_kernel_ms_per_symbol=rec['mmd_kernel_ms'] / S,
                   mmd_exp_per_s=pairs / (rec['mmd_kernel_ms'] * 1e-3), mmd_values=got[:3])
        rec['mmd_exp_rate_fraction'] = rec['mmd_exp_per_s'] / EXP_PEAK
        rec['mmd_bit_identical'] = np.asarray(got).tobytes() == np.asarray(many()).tobytes() == out.cpu().numpy().tobytes()
        if args.no_dense:
            rec['mmd_dense_torch_ms'] = 'unmeasured'
        else:
            dense = lambda: dense_torch_mmd(src, tgt)
            dense()
            runs = []
            for _ in range(args.repeats):
                ms, ref = clock_ms(dense)
                runs.append(ms)
            keep_runs(rec, 'mmd_dense_torch_ms', runs)
            rec['mmd_max_abs_diff'] = float((ref.cpu() - torch.as_tensor(got, dtype=torch.float64)).abs().max())
            rec['mmd_dense_over_fn'] = rec['mmd_dense_torch_ms'] / rec['mmd_fn_ms']
        # ---- share of a round
        if not args.no_round:
            cfg.sampling.steps, cfg.sampling.method = args.round_steps, 'ancestral'
            model = deterministic_init_(get_model_class(cfg.model.name)(cfg), seed=7).to(dev).eval()
            ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
            for name, g in (('warm', None), ('plain', None), ('with_geometry', gfn)):
                fn = get_sampling_fn(cfg, ns, _Nodes(n_nodes), B, B, get_data_inverse_scaler(cfg), return_raw=True, geometry=g)
                torch.manual_seed(3)
                ms, _ = clock_ms(lambda: fn(model))
                if name != 'warm':
                    rec['round_s_%s' % name] = ms * 1e-3
            rec['round_steps'] = args.round_steps
            rec['extract_fn_share_of_round'] = rec['extract_fn_ms'] * 1e-3 / rec['round_s_plain']
            rec['round_values'] = int(sum(fn.last_geometry['counts'].values()))
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, 'geometry_%s.json' % w), 'w') as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))


if __name__ == '__main__':
    main()

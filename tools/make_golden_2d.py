"""Fixtures of the 2-D model (DGT_concat_2D, AncestralSampler_2D) from the upstream reference, run on the CPU through
oracle/ref_import.py with 8 torch threads.  Weights are deterministic_init_ (seeded by name): the files store seeds, not weights.

  tests/golden/fwd2d_zinc.npz, fwd2d_moses.npz   inputs, first-step and self-conditioned outputs, per-molecule noise levels
  tests/golden/blocks2d_zinc.npz                 h (real atoms) and e (real ordered pairs, row-major) after every block
  tests/golden/traj2d_zinc_anc5.npz, traj2d_moses_anc5.npz
                                                 AncestralSampler_2D, 5 steps: all draws, every step's inputs and predictions, end
                                                 state, decodes, per-entry decision margins and the share below 1e-3 per kind
  tests/golden/samplefn2d_zinc.npz               the reference's own get_sampling_fn (2-D), batch 16, 10 steps, seeded; the draws
                                                 are a function of the seed (checksums stored), results before the final shuffle
  tests/golden/sd2d_manifest.json                state_dict keys, shapes and order for both configs
  tests/golden/n_nodes_2d.json                   the two train_n_nodes tables

While doing so it asserts tests/oracle2d.py against the reference within 1e-5 (float32).
Run:  python tools/make_golden_2d.py [name-prefix ...]
"""
import importlib.util
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle.ref_import import load_reference, reference_config, REFERENCE_ROOT      # noqa: E402
from jodo_amd.models.init_utils import deterministic_init_                          # noqa: E402
import oracle2d as O2                                                               # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
THREADS = 8
HEAD_GAIN_2D = 8.0          # heads' last layers scaled so that the decodes are not degenerate (>= 2 atom types, >= 2 bond types)
MARGIN = 1e-3
MARGIN_CAP = 0.05           # at most 5 % of the real entries of a decision kind within MARGIN of a threshold
CFG = {'zinc': 'vpsde_zinc_2d_jodo', 'moses': 'vpsde_moses_2d_jodo'}


def build_reference_model(ref, cfg_name, seed, head_gain=1.0):
    cfg = reference_config(cfg_name)
    cfg.device = torch.device('cpu')
    model = ref.models.utils._MODELS[cfg.model.name](cfg).eval()
    deterministic_init_(model, seed=seed)
    if head_gain != 1.0:
        with torch.no_grad():
            for k in ('node_pred_mlp.4.weight', 'edge_type_mlp.4.weight', 'edge_exist_mlp.4.weight'):
                model.state_dict()[k].mul_(head_gain)
    return cfg, model


def masks(n_nodes):
    B, N = len(n_nodes), max(n_nodes)
    nm = torch.zeros(B, N)
    for i, n in enumerate(n_nodes):
        nm[i, :n] = 1
    em = nm.unsqueeze(1) * nm.unsqueeze(2) * (~torch.eye(N, dtype=torch.bool)).unsqueeze(0)
    return nm.unsqueeze(2), em.reshape(-1, 1)


def make_inputs(cfg, n_nodes, seed):
    nd = cfg.data.atom_types + int(cfg.model.include_fc_charge)
    ch = cfg.model.edge_ch
    g = torch.Generator().manual_seed(seed + 100)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    xh = torch.randn(B, N, nd, generator=g) * nm
    ex = torch.randn(B, ch, N, N, generator=g)
    ex = torch.tril(ex, -1)
    ex = (ex + ex.transpose(-1, -2)).permute(0, 2, 3, 1) * em.reshape(B, N, N, 1)
    nl = torch.randn(B, generator=g) * 2.0
    return nm, em, xh, ex.contiguous(), nl


def forward_fixture(ref, which, n_nodes, seed=7):
    cfg, model = build_reference_model(ref, CFG[which], seed)
    hp = O2.Hyper2D.from_config(cfg)
    nm, em, xh, ex, nl = make_inputs(cfg, n_nodes, seed)
    B = len(n_nodes)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        r1 = model(torch.ones(B), xh, nm, em, edge_x=ex, noise_level=nl, cond_x=None, cond_edge_x=None)
        r2 = model(torch.ones(B), xh, nm, em, edge_x=ex, noise_level=nl, cond_x=r1[0], cond_edge_x=r1[1])
        for cx, cex, want in ((None, None, r1), (r1[0], r1[1], r2)):
            d = O2.forward_dense(sd, hp, xh, nm, em, ex, cx, cex, nl)
            err = max((d[0] - want[0]).abs().max().item(), (d[1] - want[1]).abs().max().item())
            assert err < 1e-5, "dense 2-D oracle vs reference: %g" % err
    fname = 'fwd2d_%s.npz' % which
    np.savez_compressed(os.path.join(OUT, fname), torch_num_threads=torch.get_num_threads(), cfg_name=CFG[which], seed=seed,
                        n_nodes=np.array(n_nodes), xh=xh.numpy(), edge_x=ex.numpy(), noise_level=nl.numpy(),
                        out1_x=r1[0].numpy(), out1_e=r1[1].numpy(), out2_x=r2[0].numpy(), out2_e=r2[1].numpy())
    print(fname, 'ok; |out| =', r2[0].abs().max().item(), r2[1].abs().max().item())


def blocks_fixture(ref, n_nodes=(9, 1, 2, 14, 6), seed=7):
    cfg, model = build_reference_model(ref, CFG['zinc'], seed)
    hp = O2.Hyper2D.from_config(cfg)
    nm, em, xh, ex, nl = make_inputs(cfg, list(n_nodes), seed)
    B, N = len(n_nodes), max(n_nodes)
    rec = []
    hooks = [model._modules['e_block_%d' % l].register_forward_hook(lambda m, i, o: rec.append((o[0].clone(), o[1].clone())))
             for l in range(hp.L)]
    with torch.no_grad():
        r1 = model(torch.ones(B), xh, nm, em, edge_x=ex, noise_level=nl, cond_x=None, cond_edge_x=None)
        del rec[:]
        model(torch.ones(B), xh, nm, em, edge_x=ex, noise_level=nl, cond_x=r1[0], cond_edge_x=r1[1])
    for h_ in hooks:
        h_.remove()
    real = nm.reshape(-1) > 0
    h_all = np.stack([h[real].numpy() for h, _ in rec])              # [L, Nn, D] (real atoms, batch-major)
    e_all = np.stack([e.numpy() for _, e in rec])                    # [L, E, De] (real ordered pairs, (b, r, c) row-major)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _, _, blocks = O2.forward_dense(sd, hp, xh, nm, em, ex, r1[0], r1[1], nl, return_blocks=True)
    emk = em.reshape(B, N, N) > 0
    for l, (h, e) in enumerate(blocks):
        err = max((h.reshape(B * N, -1)[real] - torch.from_numpy(h_all[l])).abs().max().item(),
                  (e[emk] - torch.from_numpy(e_all[l])).abs().max().item())
        assert err < 1e-5, "dense 2-D oracle vs reference, block %d: %g" % (l, err)
    np.savez_compressed(os.path.join(OUT, 'blocks2d_zinc.npz'), torch_num_threads=torch.get_num_threads(), cfg_name=CFG['zinc'], seed=seed,
                        n_nodes=np.array(n_nodes), xh=xh.numpy(), edge_x=ex.numpy(), noise_level=nl.numpy(),
                        cond_x=r1[0].numpy(), cond_edge_x=r1[1].numpy(), h=h_all, e=e_all)
    print('blocks2d_zinc.npz ok', h_all.shape, e_all.shape)


def decision_margins(cfg, inv, x_mean, e_mean, nm, em):
    """Distance of every decisive value to its nearest threshold, per decision kind (dense arrays, 0 outside the masks are ignored)."""
    B, N = x_mean.shape[0], x_mean.shape[1]
    fc_on = bool(cfg.model.include_fc_charge)
    h_cat_in = x_mean[:, :, :-1] if fc_on else x_mean
    h_int_in = x_mean[:, :, -1:] if fc_on else torch.zeros(0)
    _, h_cat, h_int, h_edge = inv(None, h_cat_in, h_int_in, nm, e_mean, em)
    top2 = h_cat.topk(2, dim=2).values
    out = {'atom': (top2[..., 0] - top2[..., 1])}
    if fc_on:
        out['charge'] = (0.5 - (h_int[..., 0] - h_int[..., 0].round()).abs())
    out['exist'] = (h_edge[..., 0] - 0.5).abs()
    o3 = h_edge[..., 1] * 3.
    out['order'] = torch.stack([(o3 - t).abs() for t in (0.5, 1.5, 2.5)]).min(0).values / 3.
    if h_edge.size(-1) == 3:
        out['aromatic'] = (h_edge[..., 2] - 0.5).abs()
    node_real = nm[..., 0] > 0
    edge_real = em.reshape(B, N, N) > 0
    shares = {k: float((v[node_real if v.dim() == 2 else edge_real] < MARGIN).float().mean()) for k, v in out.items()}
    return out, shares


def traj_fixture(ref, which, steps=5, n_nodes=(38, 23, 6, 30, 17, 9), seed=21):
    cfg, model = build_reference_model(ref, CFG[which], seed, head_gain=HEAD_GAIN_2D)
    n_nodes = [min(n, cfg.data.max_node) for n in n_nodes]
    S = ref.sampling
    ns = ref.diffusion.noise_schedule.NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                                                      continuous_beta_1=cfg.sde.continuous_beta_1)
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    nd = cfg.data.atom_types + int(cfg.model.include_fc_charge)
    torch.manual_seed(seed)
    z = S.sample_gaussian_with_mask((B, N, nd), 'cpu', nm)
    ez = S.sample_symmetric_edge_feature_noise(B, N, cfg.model.edge_ch, em)
    rec_node, rec_edge, rec_in = [], [], []
    orig_n, orig_e = S.sample_gaussian_with_mask, S.sample_symmetric_edge_feature_noise

    def rn(*a, **k):
        v = orig_n(*a, **k)
        rec_node.append(v.clone())
        return v

    def re_(*a, **k):
        v = orig_e(*a, **k)
        rec_edge.append(v.clone())
        return v

    def model_rec(t, x, node_mask, edge_mask, **kw):
        out = model(t, x, node_mask, edge_mask, **kw)
        rec_in.append((x.clone(), kw['edge_x'].clone(), kw['noise_level'].clone(), out[0].clone(), out[1].clone()))
        return out

    S.sample_gaussian_with_mask, S.sample_symmetric_edge_feature_noise = rn, re_
    try:
        with torch.no_grad():
            x_mean, e_mean = sampler.sampling(model_rec, z, nm, em, ez, None)
    finally:
        S.sample_gaussian_with_mask, S.sample_symmetric_edge_feature_noise = orig_n, orig_e
    inv = ref.utils.get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_mean.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_mean.clone(), em,
                                        cfg.data.compress_edge)
    margins, shares = decision_margins(cfg, inv, x_mean, e_mean, nm, em)
    atoms, bonds = np.unique(one_hot.argmax(2).numpy()[nm[..., 0].numpy() > 0]), np.unique(et.numpy())
    assert len(atoms) >= 2 and len(bonds) >= 2, "degenerate decodes: atom types %s bond types %s" % (atoms, bonds)
    for k, s in shares.items():
        assert s <= MARGIN_CAP, "%s: %.3f of the real entries within %g of a threshold" % (k, s, MARGIN)
    fname = 'traj2d_%s_anc%d.npz' % (which, steps)
    arrays = dict(torch_num_threads=torch.get_num_threads(), cfg_name=CFG[which], seed=seed, steps=steps, head_gain=HEAD_GAIN_2D,
                  n_nodes=np.array(n_nodes), z=z.numpy(), edge_z=ez.numpy(), node_noise=torch.stack(rec_node).numpy(),
                  edge_noise=torch.stack(rec_edge).numpy(), x_mean=x_mean.numpy(), edge_x_mean=e_mean.numpy(),
                  step_x=torch.stack([r[0] for r in rec_in]).numpy(), step_edge_x=torch.stack([r[1] for r in rec_in]).numpy(),
                  step_noise_level=torch.stack([r[2] for r in rec_in]).numpy(),
                  step_pred_x=torch.stack([r[3] for r in rec_in]).numpy(), step_pred_e=torch.stack([r[4] for r in rec_in]).numpy(),
                  atom_type=one_hot.argmax(2).numpy(), fc=fc.numpy(), edge_type=et.numpy(),
                  margin_kinds=np.array(sorted(margins)), margin_shares=np.array([shares[k] for k in sorted(margins)]),
                  margin_cap=MARGIN_CAP)
    for k, v in margins.items():
        arrays['margin_' + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, fname), **arrays)
    print(fname, 'ok; shares', shares, 'atom types', atoms, 'bond types', bonds)


def _dataset_info(name):
    spec = importlib.util.spec_from_file_location('jodo_ref_datasets_config', os.path.join(REFERENCE_ROOT, 'datasets', 'datasets_config.py'))
    dsc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dsc)
    return dsc.get_dataset_info(name)


def samplefn_fixture(ref, batch=16, steps=10, seed=42, model_seed=42):
    cfg, model = build_reference_model(ref, CFG['zinc'], model_seed, head_gain=HEAD_GAIN_2D)
    cfg.sampling.steps = steps
    S = ref.sampling
    ns = ref.diffusion.noise_schedule.NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                                                      continuous_beta_1=cfg.sde.continuous_beta_1)
    nodes_dist = ref.models.node_distribution.get_node_dist(_dataset_info(cfg.data.info_name))
    inv = ref.utils.get_data_inverse_scaler(cfg)
    fn = S.get_sampling_fn(cfg, ns, nodes_dist, batch, batch, inv)
    rec, sums = {}, {'node': [], 'edge': []}
    orig_sampling, orig_pp, orig_mp = S.AncestralSampler_2D.sampling, S.post_process_2D, S.mol_process_2D
    orig_n, orig_e = S.sample_gaussian_with_mask, S.sample_symmetric_edge_feature_noise

    def rec_sampling(self, model_, z, node_mask, edge_mask, edge_z, context):
        rec['nm'], rec['em'] = node_mask.clone(), edge_mask.clone()
        out = orig_sampling(self, model_, z, node_mask, edge_mask, edge_z, context)
        rec['x_mean'], rec['edge_x_mean'] = out[0].clone(), out[1].clone()
        return out

    def rec_pp(*a, **k):
        out = orig_pp(*a, **k)
        rec['one_hot'], rec['fc'], rec['et'] = [t.clone() for t in out]
        return out

    def rec_mp(one_hot, fc, n_nodes, edge_types):
        rec['n_nodes'] = torch.as_tensor(n_nodes).clone()
        return orig_mp(one_hot, fc, n_nodes, edge_types)

    def rn(*a, **k):
        v = orig_n(*a, **k)
        sums['node'].append(float(v.double().sum()))
        return v

    def re_(*a, **k):
        v = orig_e(*a, **k)
        sums['edge'].append(float(v.double().abs().sum()))
        return v

    S.AncestralSampler_2D.sampling, S.post_process_2D, S.mol_process_2D = rec_sampling, rec_pp, rec_mp
    S.sample_gaussian_with_mask, S.sample_symmetric_edge_feature_noise = rn, re_
    try:
        torch.manual_seed(seed)
        random.seed(seed)
        mols = fn(model)
    finally:
        S.AncestralSampler_2D.sampling, S.post_process_2D, S.mol_process_2D = orig_sampling, orig_pp, orig_mp
        S.sample_gaussian_with_mask, S.sample_symmetric_edge_feature_noise = orig_n, orig_e
    assert len(mols) == batch and len(sums['node']) == steps + 1 and len(sums['edge']) == steps + 1
    margins, shares = decision_margins(cfg, inv, rec['x_mean'], rec['edge_x_mean'], rec['nm'], rec['em'])
    arrays = dict(torch_num_threads=torch.get_num_threads(), cfg_name=CFG['zinc'], seed=seed, model_seed=model_seed, steps=steps, batch=batch,
                  head_gain=HEAD_GAIN_2D, n_nodes=rec['n_nodes'].numpy(), node_noise_sums=np.array(sums['node']),
                  edge_noise_sums=np.array(sums['edge']), x_mean=rec['x_mean'].numpy(), edge_x_mean=rec['edge_x_mean'].numpy(),
                  atom_type=rec['one_hot'].argmax(2).numpy(), fc=rec['fc'].numpy(), edge_type=rec['et'].numpy(),
                  margin_kinds=np.array(sorted(margins)), margin_shares=np.array([shares[k] for k in sorted(margins)]))
    for k, v in margins.items():
        arrays['margin_' + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, 'samplefn2d_zinc.npz'), **arrays)
    print('samplefn2d_zinc.npz ok; n_nodes', rec['n_nodes'].tolist(), 'shares', shares)


def manifest(ref):
    out = {}
    for which, name in CFG.items():
        cfg, model = build_reference_model(ref, name, 7)
        out[name] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(OUT, 'sd2d_manifest.json'), 'w') as f:
        json.dump(out, f, indent=0)
        f.write('\n')
    print('sd2d_manifest.json ok', {k: len(v) for k, v in out.items()})
    hist = {n: {str(k): int(v) for k, v in _dataset_info(n)['train_n_nodes'].items()} for n in ('zinc250k', 'moses')}
    with open(os.path.join(OUT, 'n_nodes_2d.json'), 'w') as f:
        json.dump(hist, f, indent=0, sort_keys=True)
        f.write('\n')
    print('n_nodes_2d.json ok')


def main():
    torch.set_num_threads(THREADS)
    ref = load_reference()
    jobs = {
        'sd2d_manifest': lambda: manifest(ref),
        'fwd2d_zinc': lambda: forward_fixture(ref, 'zinc', [38, 1, 2, 23, 17, 9]),
        'fwd2d_moses': lambda: forward_fixture(ref, 'moses', [27, 1, 2, 21, 14, 8]),
        'blocks2d_zinc': lambda: blocks_fixture(ref),
        'traj2d_zinc': lambda: traj_fixture(ref, 'zinc'),
        'traj2d_moses': lambda: traj_fixture(ref, 'moses'),
        'samplefn2d_zinc': lambda: samplefn_fixture(ref),
    }
    want = sys.argv[1:]
    for name, job in jobs.items():
        if not want or any(name.startswith(w) for w in want):
            job()


if __name__ == '__main__':
    main()

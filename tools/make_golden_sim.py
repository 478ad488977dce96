"""Fixtures of DGT_concat_sim (the 3-D score network without extra attention heads) from the upstream reference, run on the CPU
through oracle/ref_import.py with 8 torch threads.  Weights are deterministic_init_ (seeded by name): the files store seeds, not
weights.  The configs are the reference's two 3-D JODO configs with model.name = 'DGT_concat_sim' and nothing else changed
(n_extra_heads stays 2: the class never reads it).

  tests/golden/fwd_sim_qm9.npz, fwd_sim_geom.npz  inputs, per-molecule noise levels, first-step and self-conditioned outputs, and a
                                                  self-conditioned call on an ASYMMETRIC edge_x (asym_edge_x -> out_asym_x / out_asym_e)
  tests/golden/blocks_sim_qm9.npz                 h, e (real ordered pairs, (b, i, j) row-major) and pos after every block of a
                                                  self-conditioned call (layout of blocks_qm9.npz)
  tests/golden/traj_sim_qm9_anc5.npz              the reference's AncestralSampler, 5 steps: all draws, every step's inputs and
                                                  predictions, end state, decodes, per-entry decision margins and shares below 1e-3
  tests/golden/traj_sim_qm9_dpm_single2.npz       the reference's DPM_Solver_hybrid, single-step order 2, NFE 6: position-noise draws,
                                                  every evaluation's inputs and prediction, end state, decodes, margins
  tests/golden/sd_sim_manifest.json               state_dict keys, shapes and order for both configs; sha256 of the seeded DEFAULT
                                                  initialisation (torch.manual_seed(s); Model(config)) of the QM9 config

While doing so it asserts tests/oracle_sim.py against the reference within 1e-5 (float32) on outputs and 2e-5 on per-block tensors,
and that at most 5 % of the real entries of each decision kind lie within 1e-3 of a threshold (MARGIN / MARGIN_CAP): the seed and
the head gain below were chosen so that the reference alone satisfies it.
Run:  python tools/make_golden_sim.py [name-prefix ...]
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle.ref_import import load_reference, reference_config                      # noqa: E402
from oracle.make_golden import masks, savez_stable                                  # noqa: E402
from jodo_amd.models.init_utils import deterministic_init_                          # noqa: E402
import oracle_sim as OS                                                             # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
THREADS = 8
NAME = 'DGT_concat_sim'
HEAD_GAIN = 30.0            # heads' last layers scaled so that the decodes are not degenerate (as oracle/make_golden.py)
MARGIN = 1e-3
MARGIN_CAP = 0.05           # at most 5 % of the real entries of a decision kind within MARGIN of a threshold
TRAJ_SEED = 21
DEFAULT_INIT_SEED = 1234
CFG = {'qm9': 'vpsde_qm9_uncond_jodo', 'geom': 'vpsde_geom_uncond_jodo'}


def build_reference_model(ref, cfg_name, seed, head_gain=1.0):
    cfg = reference_config(cfg_name)
    cfg.device = torch.device('cpu')
    cfg.model.name = NAME
    model = ref.models.utils._MODELS[NAME](cfg).eval()
    deterministic_init_(model, seed=seed)
    if head_gain != 1.0:
        with torch.no_grad():
            for k in ('node_pred_mlp.4.weight', 'edge_type_mlp.4.weight', 'edge_exist_mlp.4.weight'):
                model.state_dict()[k].mul_(head_gain)
    return cfg, model


def make_inputs(hp, n_nodes, seed):
    g = torch.Generator().manual_seed(seed + 100)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    xh = torch.randn(B, N, 3 + hp.in_node_dim, generator=g) * nm
    xh[:, :, :3] = xh[:, :, :3] - xh[:, :, :3].sum(1, keepdim=True) / nm.sum(1, keepdim=True) * nm
    raw = torch.randn(B, N, N, hp.edge_ch, generator=g)
    low = torch.tril(raw.permute(0, 3, 1, 2), -1)
    ex = (low + low.transpose(-1, -2)).permute(0, 2, 3, 1) * em.reshape(B, N, N, 1)
    ex_asym = raw * em.reshape(B, N, N, 1)
    nl = torch.randn(B, generator=g) * 2.0
    return nm, em, xh, ex.contiguous(), ex_asym.contiguous(), nl


def check_oracle(sd, hp, args, want, what):
    d = OS.forward_dense(sd, hp, *args)
    err = max((d[0] - want[0]).abs().max().item(), (d[1] - want[1]).abs().max().item())
    assert err < 1e-5, "tests/oracle_sim.py vs reference (%s): %g" % (what, err)
    return err


def forward_fixture(ref, which, n_nodes, seed=7):
    cfg, model = build_reference_model(ref, CFG[which], seed)
    hp = OS.HyperSim.from_config(cfg)
    nm, em, xh, ex, exa, nl = make_inputs(hp, n_nodes, seed)
    B = len(n_nodes)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        call = lambda e_, cx, cex: model(torch.ones(B), xh, nm, em, edge_x=e_, noise_level=nl, cond_x=cx, cond_edge_x=cex)
        r1 = call(ex, None, None)
        r2 = call(ex, r1[0], r1[1])
        ra = call(exa, r1[0], r1[1])
        errs = [check_oracle(sd, hp, (xh, nm, em, ex, None, None, nl), r1, 'first step'),
                check_oracle(sd, hp, (xh, nm, em, ex, r1[0], r1[1], nl), r2, 'self-conditioned'),
                check_oracle(sd, hp, (xh, nm, em, exa, r1[0], r1[1], nl), ra, 'asymmetric edge_x')]
    assert (ra[0] - r2[0]).abs().max().item() > 1e-3                  # the asymmetric case is another function value
    fname = 'fwd_sim_%s.npz' % which
    savez_stable(os.path.join(OUT, fname), torch_num_threads=np.int64(torch.get_num_threads()), cfg_name=np.array(CFG[which]),
                 model_name=np.array(NAME), seed=np.int64(seed), n_nodes=np.array(n_nodes), xh=xh.numpy(), edge_x=ex.numpy(),
                 asym_edge_x=exa.numpy(), noise_level=nl.numpy(), out1_x=r1[0].numpy(), out1_e=r1[1].numpy(), out2_x=r2[0].numpy(),
                 out2_e=r2[1].numpy(), out_asym_x=ra[0].numpy(), out_asym_e=ra[1].numpy())
    print(fname, 'ok; oracle errs', errs, 'bytes', os.path.getsize(os.path.join(OUT, fname)))


def blocks_fixture(ref, n_nodes=(6, 1, 2, 9), seed=7):
    cfg, model = build_reference_model(ref, CFG['qm9'], seed)
    hp = OS.HyperSim.from_config(cfg)
    n_nodes = list(n_nodes)
    nm, em, xh, ex, _, nl = make_inputs(hp, n_nodes, seed)
    B, N = len(n_nodes), max(n_nodes)
    rec = []
    hooks = [model._modules['e_block_%d' % i].register_forward_hook(lambda m, a, out: rec.append([t.detach().clone() for t in out]))
             for i in range(hp.n_layers)]
    with torch.no_grad():
        r1 = model(torch.ones(B), xh, nm, em, edge_x=ex, noise_level=nl, cond_x=None, cond_edge_x=None)
        del rec[:]
        r2 = model(torch.ones(B), xh, nm, em, edge_x=ex, noise_level=nl, cond_x=r1[0], cond_edge_x=r1[1])
    for h_ in hooks:
        h_.remove()
    assert len(rec) == hp.n_layers
    hs = torch.stack([r[0] for r in rec]).reshape(hp.n_layers, B, N, -1)
    es = torch.stack([r[1] for r in rec])
    ps = torch.stack([ref.models.utils.remove_mean_with_mask(r[2].reshape(B, N, 3), nm) for r in rec])
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        _, _, inter = OS.forward_dense(sd, hp, xh, nm, em, ex, r1[0], r1[1], nl, return_intermediates=True)
    eoff = 0
    for b, n in enumerate(n_nodes):
        for l in range(hp.n_layers):
            blk = inter[b][l]
            offd = ~torch.eye(n, dtype=torch.bool)
            assert (blk['h'] - hs[l, b, :n]).abs().max() < 2e-5 and (blk['pos'] - ps[l, b, :n]).abs().max() < 2e-5
            assert n == 1 or (blk['e'][offd] - es[l, eoff:eoff + n * (n - 1)]).abs().max() < 2e-5
        eoff += n * (n - 1)
    savez_stable(os.path.join(OUT, 'blocks_sim_qm9.npz'), torch_num_threads=np.int64(torch.get_num_threads()), cfg_name=np.array(CFG['qm9']),
                 model_name=np.array(NAME), seed=np.int64(seed), n_nodes=np.array(n_nodes), xh=xh.numpy(), edge_x=ex.numpy(),
                 noise_level=nl.numpy(), out1_x=r1[0].numpy(), out1_e=r1[1].numpy(), out2_x=r2[0].numpy(), out2_e=r2[1].numpy(),
                 h=hs.numpy(), e=es.numpy(), pos=ps.numpy())
    print('blocks_sim_qm9.npz ok; E', es.shape[1], 'bytes', os.path.getsize(os.path.join(OUT, 'blocks_sim_qm9.npz')))


def decision_margins(inv, x_mean, e_mean, nm, em):
    """Distance of every decisive value of the 3-D decode to its nearest threshold, per kind (dense), and the share of the real
    entries of each kind below MARGIN."""
    B, N = x_mean.shape[0], x_mean.shape[1]
    _, h_cat, h_int, h_edge = inv(x_mean[:, :, :3], x_mean[:, :, 3:-1], x_mean[:, :, -1:], nm, e_mean, em)
    top2 = h_cat.topk(2, dim=2).values
    o3 = h_edge[..., 1] * 3.
    out = {'atom': top2[..., 0] - top2[..., 1], 'charge': 0.5 - (h_int[..., 0] - h_int[..., 0].round()).abs(),
           'exist': (h_edge[..., 0] - 0.5).abs(), 'order': torch.stack([(o3 - t).abs() for t in (0.5, 1.5, 2.5)]).min(0).values / 3.}
    node_real, edge_real = nm[..., 0] > 0, em.reshape(B, N, N) > 0
    shares = {k: float((v[node_real if v.dim() == 2 else edge_real] < MARGIN).float().mean()) for k, v in out.items()}
    return out, shares


def finish_traj(ref, cfg, fname, x_end, e_end, nm, em, arrays):
    """Decodes, margins and the cap; writes the file."""
    S = ref.sampling
    inv = ref.utils.get_data_inverse_scaler(cfg)
    pos, one_hot, fc, et = S.post_process(x_end.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_end.clone(), em,
                                          cfg.data.compress_edge)
    margins, shares = decision_margins(inv, x_end, e_end, nm, em)
    atoms, bonds = np.unique(one_hot.argmax(2).numpy()[nm[..., 0].numpy() > 0]), np.unique(et.numpy())
    assert len(atoms) >= 2 and len(bonds) >= 2, "degenerate decodes: atom types %s bond types %s" % (atoms, bonds)
    for k, s in shares.items():
        assert s <= MARGIN_CAP, "%s: %.3f of the real entries within %g of a threshold" % (k, s, MARGIN)
    arrays.update(pos=pos.numpy(), atom_type=one_hot.argmax(2).numpy(), fc=fc.numpy(), edge_type=et.numpy(),
                  margin_kinds=np.array(sorted(margins)), margin_shares=np.array([shares[k] for k in sorted(margins)]),
                  margin_cap=np.float64(MARGIN_CAP))
    for k, v in margins.items():
        arrays['margin_' + k] = v.numpy()
    savez_stable(os.path.join(OUT, fname), **arrays)
    print(fname, 'ok; shares', shares, 'atom types', atoms, 'bond types', bonds, 'bytes', os.path.getsize(os.path.join(OUT, fname)))


def traj_fixture(ref, steps=5, n_nodes=(9, 5, 17, 12), seed=TRAJ_SEED):
    cfg, model = build_reference_model(ref, CFG['qm9'], seed, head_gain=HEAD_GAIN)
    cfg.sampling.steps = steps
    S = ref.sampling
    ns = ref.diffusion.noise_schedule.NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                                                      continuous_beta_1=cfg.sde.continuous_beta_1)
    sampler = S.AncestralSampler(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.pred_edge, cfg.model.self_cond,
                                 ref.utils.get_self_cond_fn(cfg))
    n_nodes = list(n_nodes)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    torch.manual_seed(seed)
    node_nf = cfg.data.atom_types + int(cfg.model.include_fc_charge)
    z = S.sample_combined_position_feature_noise(B, N, node_nf, nm)
    ez = S.sample_symmetric_edge_feature_noise(B, N, cfg.model.edge_ch, em)
    rec_node, rec_edge, rec_in = [], [], []
    orig_n, orig_e = S.sample_combined_position_feature_noise, S.sample_symmetric_edge_feature_noise

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

    S.sample_combined_position_feature_noise, S.sample_symmetric_edge_feature_noise = rn, re_
    try:
        with torch.no_grad():
            x_mean, e_mean = sampler.sampling(model_rec, z, nm, em, ez, None)
    finally:
        S.sample_combined_position_feature_noise, S.sample_symmetric_edge_feature_noise = orig_n, orig_e
    arrays = dict(torch_num_threads=np.int64(torch.get_num_threads()), cfg_name=np.array(CFG['qm9']), model_name=np.array(NAME),
                  seed=np.int64(seed), steps=np.int64(steps), head_gain=np.float64(HEAD_GAIN), n_nodes=np.array(n_nodes), z=z.numpy(),
                  edge_z=ez.numpy(), node_noise=torch.stack(rec_node).numpy(), edge_noise=torch.stack(rec_edge).numpy(),
                  x_mean=x_mean.numpy(), edge_x_mean=e_mean.numpy(),
                  step_x=torch.stack([r[0] for r in rec_in]).numpy(), step_edge_x=torch.stack([r[1] for r in rec_in]).numpy(),
                  step_noise_level=torch.stack([r[2] for r in rec_in]).numpy(),
                  step_pred=torch.stack([r[3] for r in rec_in]).numpy(), step_edge_pred=torch.stack([r[4] for r in rec_in]).numpy())
    finish_traj(ref, cfg, 'traj_sim_qm9_anc%d.npz' % steps, x_mean, e_mean, nm, em, arrays)


def dpm_fixture(ref, nfe=6, n_nodes=(9, 5, 17, 12), seed=TRAJ_SEED, method='singlestep_fixed', order=2):
    cfg, model = build_reference_model(ref, CFG['qm9'], seed, head_gain=HEAD_GAIN)
    cfg.sampling.steps, cfg.sampling.method = nfe, 'fast'
    cfg.sampling.dpm_solver_method, cfg.sampling.dpm_solver_order = method, order
    M, S = ref.mix_dpm_solver, ref.sampling
    ns = ref.diffusion.noise_schedule.NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                                                      continuous_beta_1=cfg.sde.continuous_beta_1)
    solver = M.DPM_Solver_hybrid(ns, cfg)
    n_nodes = list(n_nodes)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    torch.manual_seed(seed)
    node_nf = cfg.data.atom_types + int(cfg.model.include_fc_charge)
    z = S.sample_combined_position_feature_noise(B, N, node_nf, nm)
    ez = S.sample_symmetric_edge_feature_noise(B, N, cfg.model.edge_ch, em)
    rec, rec_in = [], []
    orig = M.sample_center_gravity_zero_gaussian_with_mask

    def rp(*a, **k):
        v = orig(*a, **k)
        rec.append(v.clone())
        return v

    def model_rec(t, x, node_mask, edge_mask, *a, **kw):
        out = model(t, x, node_mask, edge_mask, *a, **kw)
        rec_in.append((x.clone(), kw['edge_x'].clone(), kw['noise_level'].clone(), out[0].clone(), out[1].clone()))
        return out

    M.sample_center_gravity_zero_gaussian_with_mask = rp
    try:
        with torch.no_grad():
            x, e = solver.sampling(model_rec, z, nm, em, ez, None)
    finally:
        M.sample_center_gravity_zero_gaussian_with_mask = orig
    assert len(rec_in) == nfe, "model calls %d != NFE %d" % (len(rec_in), nfe)
    arrays = dict(torch_num_threads=np.int64(torch.get_num_threads()), cfg_name=np.array(CFG['qm9']), model_name=np.array(NAME),
                  seed=np.int64(seed), nfe=np.int64(nfe), method=np.array(method), order=np.int64(order), head_gain=np.float64(HEAD_GAIN),
                  n_nodes=np.array(n_nodes), z=z.numpy(), edge_z=ez.numpy(), pos_noise=torch.stack(rec).numpy(),
                  x_mean=x.numpy(), edge_x_mean=e.numpy(),
                  step_x=torch.stack([r[0] for r in rec_in]).numpy(), step_edge_x=torch.stack([r[1] for r in rec_in]).numpy(),
                  step_noise_level=torch.stack([r[2] for r in rec_in]).numpy(),
                  step_pred=torch.stack([r[3] for r in rec_in]).numpy(), step_edge_pred=torch.stack([r[4] for r in rec_in]).numpy())
    finish_traj(ref, cfg, 'traj_sim_qm9_dpm_single2.npz', x, e, nm, em, arrays)


def default_init_sha256(model):
    h = hashlib.sha256()
    for v in model.state_dict().values():
        h.update(v.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def manifest(ref):
    out = {}
    for which, name in CFG.items():
        cfg, model = build_reference_model(ref, name, 7)
        out[name] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    cfg = reference_config(CFG['qm9'])
    cfg.device = torch.device('cpu')
    cfg.model.name = NAME
    torch.manual_seed(DEFAULT_INIT_SEED)
    out['default_init'] = dict(cfg_name=CFG['qm9'], seed=DEFAULT_INIT_SEED, torch=torch.__version__.split('+')[0],
                               sha256=default_init_sha256(ref.models.utils._MODELS[NAME](cfg)))
    with open(os.path.join(OUT, 'sd_sim_manifest.json'), 'w') as f:
        json.dump(out, f, indent=0)
        f.write('\n')
    print('sd_sim_manifest.json ok', {k: len(v) for k, v in out.items()})


def main():
    torch.set_num_threads(THREADS)
    ref = load_reference()
    jobs = {
        'sd_sim_manifest': lambda: manifest(ref),
        'fwd_sim_qm9': lambda: forward_fixture(ref, 'qm9', [29, 1, 2, 18, 7, 23]),
        'fwd_sim_geom': lambda: forward_fixture(ref, 'geom', [40, 33, 12, 1, 2]),
        'blocks_sim_qm9': lambda: blocks_fixture(ref),
        'traj_sim_qm9_anc5': lambda: traj_fixture(ref),
        'traj_sim_qm9_dpm_single2': lambda: dpm_fixture(ref),
    }
    want = sys.argv[1:]
    for name, job in jobs.items():
        if not want or any(name.startswith(w) for w in want):
            job()


if __name__ == '__main__':
    main()

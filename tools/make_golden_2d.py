"""Fixtures of the 2-D model (DGT_concat_2D, AncestralSampler_2D) from the upstream reference, run on the CPU through
oracle/ref_import.py with 8 torch threads.  Weights are deterministic_init_ (seeded by name): the files store seeds, not weights.

  tests/golden/fwd2d_zinc.npz, fwd2d_moses.npz   inputs, first-step and self-conditioned outputs, per-molecule noise levels
  tests/golden/blocks2d_zinc.npz                 h (real atoms) and e (real ordered pairs, row-major) after every block
  tests/golden/traj2d_zinc_anc5.npz, traj2d_moses_anc5.npz
                                                 AncestralSampler_2D, 5 steps: all draws, every step's inputs and predictions, end
                                                 state, decodes, per-entry decision margins and the share below 1e-3 per kind
  tests/golden/traj2d_zinc_dpm_{single2,single3,single1,multi2}.npz, traj2d_moses_dpm_single2.npz
                                                 the reference's DPM_Solver_hybrid (all four solver variants, NFE 4 - 6) around the 2-D model
                                                 with three zero position columns (dpm_fixture): every evaluation's inputs and
                                                 prediction, end state, decodes, margins — the oracle of sampling.method 'dpm_2d'
  tests/golden/samplefn2d_zinc.npz               the reference's own get_sampling_fn (2-D), batch 16, 10 steps, seeded; the draws
                                                 are a function of the seed (checksums stored), results before the final shuffle
  tests/golden/grad2d_zinc.npz, grad2d_moses.npz the reference's own get_sde_2D_loss_fn + loss.backward() (eval-mode dropout, self-conditioned
                                                 branch) on a small synthetic batch: inputs, draws, predictions, loss, ~20 parameter gradients
  tests/golden/loss2d_zinc.npz                   the same loss_fn call as data of the loss alone: batch, seeds, t, both noises, the coin, loss
  tests/golden/train_drop2d_zinc.npz             the reference under model.train() with the training path's dropout masks injected
                                                 (oracle/make_golden.py DropInjector, oracle/philox_ref.dropout_masks): no-grad call with
                                                 seed 1, grad-enabled call on its outputs with seed 2, output and parameter gradients
  tests/golden/sd2d_manifest.json                state_dict keys, shapes and order for both configs
  tests/golden/n_nodes_2d.json                   the two train_n_nodes tables

While doing so it asserts tests/oracle2d.py (and tests/oracle2d_train.py, the masked form) against the reference within 1e-5
(float32) on outputs and 2e-4 relative on the recorded gradients.
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


def build_reference_model(ref, cfg_name, seed, head_gain=1.0, gain=1.0):
    cfg = reference_config(cfg_name)
    cfg.device = torch.device('cpu')
    model = ref.models.utils._MODELS[cfg.model.name](cfg).eval()
    deterministic_init_(model, seed=seed, gain=gain)
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


TRAIN_NODES = {'zinc': [1, 2, 3, 9, 33, 38], 'moses': [2, 5, 27]}     # tests/test_train2d_*.py: the smallest shapes that reach every path
TRAIN_GAIN = 1.5


def synthetic_batch_2d(cfg, n_nodes, seed):
    """A loader-shaped batch of 2-D graphs (tests/test_losses2d_host.py rebuilds nothing: the batch is stored)."""
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    ch = cfg.model.edge_ch
    g = torch.Generator().manual_seed(seed)
    at = torch.randint(0, cfg.data.atom_types, (B, N), generator=g)
    bond = torch.randint(0, 4, (B, N, N), generator=g)
    bond = torch.triu(bond, 1)
    bond = bond + bond.transpose(1, 2)
    chans = [(bond > 0).float(), bond.float() / 3.]
    if ch == 3:
        chans.append((bond == 3).float())
    return dict(atom_mask=nm[..., 0], edge_mask=em, atom_one_hot=torch.nn.functional.one_hot(at, cfg.data.atom_types).float() * nm,
                edge_one_hot=torch.stack(chans, -1) * em.reshape(B, N, N, 1),
                formal_charges=torch.randint(-1, 2, (B, N, 1), generator=g).float() * nm)


def grad_names_2d(L):
    mid, last = L // 2, L - 1
    return ['e_block_0.ff_linear3.weight', 'e_block_0.ff_linear3.bias', 'e_block_0.ff_linear4.bias', 'e_block_0.ff_linear1.bias',
            'e_block_0.attn_mpnn.lin_edge0.weight', 'e_block_%d.attn_mpnn.lin_query.weight' % mid, 'e_block_%d.attn_mpnn.lin_edge1.weight' % mid,
            'e_block_%d.node2edge_lin.weight' % mid, 'e_block_%d.node2edge_lin.bias' % mid,
            'e_block_%d.node_time_mlp.1.bias' % mid, 'e_block_%d.edge_time_mlp.1.bias' % mid,
            'e_block_%d.ff_linear2.bias' % last, 'e_block_%d.ff_linear4.weight' % last, 'e_block_%d.attn_mpnn.lin_key.bias' % last,
            'node_%d.weight' % last, 'edge_0.weight', 'time_mlp.0.weights', 'time_mlp.3.bias',
            'node_pred_mlp.4.weight', 'edge_type_mlp.4.weight', 'edge_exist_mlp.4.weight', 'node_emb.weight', 'edge_emb.weight']


def grad2d_fixture(ref, which, seed=41):
    """The reference's OWN 2-D training loss and loss.backward() (losses.py:210-283, self-conditioned branch taken, eval mode so that
    dropout is the identity) on a small synthetic batch; layout of grad_qm9.npz.  For zinc the same call is stored once more as
    loss2d_zinc.npz: the data of the loss function alone (batch, seeds, draws, coin, loss)."""
    import random as pyrandom
    cfg, model = build_reference_model(ref, CFG[which], seed, head_gain=HEAD_GAIN_2D, gain=TRAIN_GAIN)
    hp = O2.Hyper2D.from_config(cfg)
    L = ref.losses
    ns = ref.diffusion.noise_schedule.NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                                                      continuous_beta_1=cfg.sde.continuous_beta_1)
    scaler = ref.utils.get_data_scaler(cfg)
    n_nodes = TRAIN_NODES[which]
    nm, em = masks(n_nodes)
    batch = synthetic_batch_2d(cfg, n_nodes, seed)
    loss_fn = L.get_sde_2D_loss_fn(ns, False, scaler, cfg)
    rec = {}
    inner = model.forward

    def recording_forward(t, xh, node_mask, edge_mask, context=None, **kw):
        if torch.is_grad_enabled():
            rec.update(t=t.clone(), z_t=xh.clone(), edge_z_t=kw['edge_x'].clone(), noise_level=kw['noise_level'].clone(),
                       cond_x=None if kw.get('cond_x') is None else kw['cond_x'].clone(),
                       cond_edge_x=None if kw.get('cond_edge_x') is None else kw['cond_edge_x'].clone())
        out = inner(t, xh, node_mask, edge_mask, context, **kw)
        if torch.is_grad_enabled():
            rec.update(pred=out[0].detach().clone(), edge_pred=out[1].detach().clone())
        return out

    orig_n, orig_e = L.sample_gaussian_with_mask, L.sample_symmetric_edge_feature_noise

    def rn(*a, **k):
        v = orig_n(*a, **k)
        rec['noise'] = v.clone()
        return v

    def re_(*a, **k):
        v = orig_e(*a, **k)
        rec['edge_noise'] = v.clone()
        return v

    model.forward = recording_forward
    L.sample_gaussian_with_mask, L.sample_symmetric_edge_feature_noise = rn, re_
    for tries in range(64):                                    # a python-random seed whose first draw takes the self-cond branch
        pyrandom.seed(seed + tries)
        coin = pyrandom.random()
        if coin < 0.5:
            py_seed = seed + tries
            pyrandom.seed(py_seed)
            break
    torch.manual_seed(seed)
    model.zero_grad()
    try:
        loss = loss_fn(model, batch)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)                               # the CPU backward's scatter sums are reordered by threads: keep the file reproducible
        loss.backward()
        torch.set_num_threads(threads)
    finally:
        L.sample_gaussian_with_mask, L.sample_symmetric_edge_feature_noise = orig_n, orig_e
        del model.forward
    assert rec['cond_x'] is not None
    xh, edge_x, _, _ = L.process_batch_2D(batch, cfg.device, cfg.model.include_fc_charge, scaler)
    alpha_t, sigma_t = ns.marginal_prob(rec['t'])
    names = grad_names_2d(hp.L)
    params = dict(model.named_parameters())
    assert len(set(names)) == len(names) and all(params[k].grad is not None and float(params[k].grad.abs().max()) > 0 for k in names)
    # the oracle's autograd against the reference's, here and now
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    px, pe = O2.forward_dense(sd, hp, rec['z_t'], nm, em, rec['edge_z_t'], rec['cond_x'], rec['cond_edge_x'], rec['noise_level'])
    err = max((px - rec['pred']).abs().max().item(), (pe - rec['edge_pred']).abs().max().item())
    assert err < 1e-5, "dense 2-D oracle vs reference (training step): %g" % err
    ol = loss2d_from_outputs(cfg, px, pe, xh, edge_x, nm, em, alpha_t, sigma_t)
    assert abs(ol.item() - loss.item()) < 1e-5 * abs(loss.item()), (ol.item(), loss.item())
    ol.backward()
    for k in names:
        a, b = sd[k].grad, params[k].grad
        rel = (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)
        assert rel < 2e-4, "oracle gradient of %s: rel err %g" % (k, rel)
    from oracle.make_golden import savez_stable
    fname = 'grad2d_%s.npz' % which
    savez_stable(os.path.join(OUT, fname), torch_num_threads=np.int64(torch.get_num_threads()), cfg_name=np.array(CFG[which]), seed=np.int64(seed),
                 gain=np.float32(TRAIN_GAIN), head_gain=np.float32(HEAD_GAIN_2D), n_nodes=np.array(n_nodes),
                 t=rec['t'].numpy(), z_t=rec['z_t'].numpy(), edge_z_t=rec['edge_z_t'].numpy(), noise_level=rec['noise_level'].numpy(),
                 cond_x=rec['cond_x'].numpy(), cond_edge_x=rec['cond_edge_x'].numpy(), xh=xh.numpy(), edge_x=edge_x.numpy(),
                 noise=rec['noise'].numpy(), edge_noise=rec['edge_noise'].numpy(), alpha_t=alpha_t.numpy(), sigma_t=sigma_t.numpy(),
                 pred=rec['pred'].numpy(), edge_pred=rec['edge_pred'].numpy(), loss=np.float64(loss.item()),
                 grad_names=np.array(names), **{'grad_%d' % i: params[k].grad.numpy() for i, k in enumerate(names)})
    print(fname, 'ok; loss', loss.item(), 'dense err', err, 'bytes', os.path.getsize(os.path.join(OUT, fname)))
    if which == 'zinc':
        savez_stable(os.path.join(OUT, 'loss2d_zinc.npz'), cfg_name=np.array(CFG[which]), seed=np.int64(seed), py_seed=np.int64(py_seed),
                     gain=np.float32(TRAIN_GAIN), head_gain=np.float32(HEAD_GAIN_2D), n_nodes=np.array(n_nodes), coin=np.float64(coin),
                     t=rec['t'].numpy(), noise=rec['noise'].numpy(), edge_noise=rec['edge_noise'].numpy(), loss=np.float64(loss.item()),
                     **{'batch_' + k: v.numpy() for k, v in batch.items()})
        print('loss2d_zinc.npz ok; bytes', os.path.getsize(os.path.join(OUT, 'loss2d_zinc.npz')))


def loss2d_from_outputs(cfg, pred, edge_pred, xh, edge_x, nm, em, alpha_t, sigma_t):
    """The data-prediction branch of losses.py:256-281 on given predictions (the oracle's autograd starts here)."""
    B = xh.shape[0]
    _, w_atom, w_edge = (float(w) for w in cfg.model.loss_weights.split(','))
    l_atom = torch.square(pred - xh).mean(-1).sum(-1)
    l_edge = torch.square(edge_x - edge_pred).mean(-1).reshape(B, -1).sum(-1)
    if cfg.training.reduce_mean:
        l_atom = l_atom / nm.squeeze(-1).sum(-1)
        l_edge = l_edge / (em.reshape(B, -1).sum(-1) + 1e-8)
    return (torch.sqrt(alpha_t / sigma_t) * (w_atom * l_atom + w_edge * l_edge)).mean()


def train_drop2d_fixture(ref, which='zinc', seed=43, s1=0x2545F4914F6CDD1D, s2=0x9E3779B97F4A7C15 >> 2):
    """Training-mode dropout of the reference with the training path's masks: the 2-D model under model.train(), each block's
    nn.Dropout replaced by oracle/make_golden.py's DropInjector fed from oracle/philox_ref.dropout_masks.  A no-grad
    self-conditioning call with the masks of seed s1, a grad-enabled call on its outputs with seed s2, then backward of seeded
    output gradients.  tests/oracle2d_train.forward_dense_drop with the same masks is checked here too."""
    from oracle import philox_ref as PR
    from oracle.make_golden import DropInjector, savez_stable
    import oracle2d_train as O2T
    cfg, model = build_reference_model(ref, CFG[which], seed, head_gain=HEAD_GAIN_2D, gain=TRAIN_GAIN)
    hp = O2.Hyper2D.from_config(cfg)
    p = float(cfg.model.dropout)
    assert p > 0
    model.train()
    n_nodes = TRAIN_NODES[which]
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    D, De, r, L = hp.D, hp.De, hp.r, hp.L
    widths = {'A1': r * D, 'F2': D, 'A3': r * De, 'F4': De}
    inj, hooks = [], []
    for l in range(L):
        blk = model._modules['e_block_%d' % l]
        assert isinstance(blk.dropout, torch.nn.Dropout) and blk.dropout.p == p
        d = DropInjector(l, widths)
        d.N = N
        blk.dropout = d
        inj.append(d)

        def pre(m, args, d=d):
            d.edge_index = args[2]                          # forward(h, edge_attr, edge_index, ...)
        hooks.append(blk.register_forward_pre_hook(pre))
    _, _, xh, ex, nl = make_inputs(cfg, n_nodes, seed)
    g = torch.Generator().manual_seed(seed + 200)
    d_x = torch.randn(B, N, hp.nd, generator=g)
    d_e = torch.randn(B, N, N, hp.ch, generator=g)
    m1 = PR.dropout_masks(s1, p, n_nodes, L, D, De, r)
    m2 = PR.dropout_masks(s2, p, n_nodes, L, D, De, r)

    def run(ms, cx, cex):
        for d in inj:
            d.masks, d.calls = ms, 0
        out = model(torch.ones(B), xh, nm, em, edge_x=ex, noise_level=nl, cond_x=cx, cond_edge_x=cex)
        assert all(d.calls == 4 for d in inj)
        return out

    try:
        with torch.no_grad():
            r1 = run(m1, None, None)
        model.zero_grad()
        r2 = run(m2, r1[0], r1[1])
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        ((r2[0] * d_x).sum() + (r2[1] * d_e).sum()).backward()
        torch.set_num_threads(threads)
    finally:
        for h_ in hooks:
            h_.remove()
    params = dict(model.named_parameters())
    names = ['e_block_%d.ff_linear%d.bias' % (l, k) for l in range(L) for k in (1, 2, 3, 4)]
    names += ['e_block_0.ff_linear3.weight', 'e_block_%d.ff_linear4.weight' % (L - 1), 'e_block_%d.node2edge_lin.bias' % (L // 2),
              'e_block_%d.attn_mpnn.lin_edge0.weight' % (L - 2), 'node_emb.bias', 'edge_emb.bias', 'time_mlp.0.weights',
              'edge_exist_mlp.4.weight', 'node_pred_mlp.4.weight']
    assert len(set(names)) == len(names) and all(params[k].grad is not None for k in names)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    with torch.no_grad():
        o1 = O2T.forward_dense_drop(sd, hp, xh, nm, em, ex, None, None, nl, drop=m1)
    err1 = max((o1[0] - r1[0]).abs().max().item(), (o1[1] - r1[1]).abs().max().item())
    px, pe = O2T.forward_dense_drop(sd, hp, xh, nm, em, ex, r1[0], r1[1], nl, drop=m2)
    err = max(err1, (px - r2[0]).abs().max().item(), (pe - r2[1]).abs().max().item())
    assert err < 1e-5, "masked dense 2-D oracle vs reference (dropout): %g" % err
    ((px * d_x).sum() + (pe * d_e).sum()).backward()
    for k in names:
        a, b = sd[k].grad, params[k].grad
        rel = (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)
        assert rel < 2e-4, "masked oracle gradient of %s (dropout): rel err %g" % (k, rel)
    with torch.no_grad():                                   # the masks matter: eval mode gives another function
        e2 = O2.forward_dense(sd, hp, xh, nm, em, ex, r1[0], r1[1], nl)
    assert (e2[0] - r2[0]).abs().max().item() > 1e-2 and (e2[1] - r2[1]).abs().max().item() > 1e-2
    fname = 'train_drop2d_%s.npz' % which
    savez_stable(os.path.join(OUT, fname), cfg_name=np.array(CFG[which]), seed=np.int64(seed), gain=np.float32(TRAIN_GAIN),
                 head_gain=np.float32(HEAD_GAIN_2D), n_nodes=np.array(n_nodes), p=np.float32(p),
                 seed1=np.uint64(s1), seed2=np.uint64(s2), xh=xh.numpy(), edge_x=ex.numpy(), noise_level=nl.numpy(),
                 out1_x=r1[0].numpy(), out1_e=r1[1].numpy(), out2_x=r2[0].detach().numpy(), out2_e=r2[1].detach().numpy(),
                 d_out_x=d_x.numpy(), d_out_e=d_e.numpy(), grad_names=np.array(names),
                 **{'grad_%d' % i: params[k].grad.numpy() for i, k in enumerate(names)})
    print(fname, 'ok; dense err', err, 'bytes', os.path.getsize(os.path.join(OUT, fname)))


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
        'grad2d_zinc': lambda: grad2d_fixture(ref, 'zinc'),
        'grad2d_moses': lambda: grad2d_fixture(ref, 'moses'),
        'train_drop2d_zinc': lambda: train_drop2d_fixture(ref, 'zinc'),
    }
    want = sys.argv[1:]
    for name, job in jobs.items():
        if not want or any(name.startswith(w) for w in want):
            job()


DPM_VARIANTS = {            # file suffix -> (dpm_solver_method, dpm_solver_order, NFE): a single-step NFE is a multiple of its order
    'single2': ('singlestep_fixed', 2, 6),
    'single3': ('singlestep_fixed', 3, 6),
    'single1': ('singlestep_fixed', 1, 4),
    'multi2': ('multistep', 2, 5),
}


def dpm_fixture(ref, which, variant, n_nodes=(38, 1, 2, 17, 9), seed=21, nfe=None):
    """traj2d_<which>_dpm_<variant>.npz: the reference's own DPM_Solver_hybrid (mix_dpm_solver.py) around its DGT_concat_2D.  The
    solver wants three position channels in front of the node state; the state gets three zero columns, and the model wrapper strips
    them from x and cond_x and puts zeros in front of the prediction.  The position branch then turns zeros into centre-of-gravity-free
    noise that nobody reads; the atom / charge channels and the edge tensor go through the reference's DPM-Solver++ arithmetic
    untouched.  Recorded: z, edge_z, every evaluation's input state / noise level / prediction, the end state, decodes, decision
    margins and shares (layout of traj2d_*_anc5.npz).  If a seed fails the margin cap or gives degenerate decodes, pick another one
    here (it is stored in the file); the cap stays."""
    method, order, steps = DPM_VARIANTS[variant]
    steps = steps if nfe is None else nfe
    cfg, model = build_reference_model(ref, CFG[which], seed, head_gain=HEAD_GAIN_2D)
    cfg.sampling.method, cfg.sampling.steps = 'fast', steps
    cfg.sampling.dpm_solver_method, cfg.sampling.dpm_solver_order = method, order
    n_nodes = [min(n, cfg.data.max_node) for n in n_nodes]
    assert 1 in n_nodes and 2 in n_nodes and cfg.data.max_node in n_nodes
    assert method == 'multistep' or steps % order == 0          # single-step: K = steps // order outer steps, NFE = K * order
    S = ref.sampling
    ns = ref.diffusion.noise_schedule.NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                                                      continuous_beta_1=cfg.sde.continuous_beta_1)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    nd = cfg.data.atom_types + int(cfg.model.include_fc_charge)
    torch.manual_seed(seed)
    z = S.sample_gaussian_with_mask((B, N, nd), 'cpu', nm)
    ez = S.sample_symmetric_edge_feature_noise(B, N, cfg.model.edge_ch, em)
    rec_in = []

    def model3(t, x, node_mask, edge_mask, edge_x=None, noise_level=None, cond_x=None, cond_edge_x=None, context=None):
        cx = None if cond_x is None else cond_x[:, :, 3:]
        out = model(t, x[:, :, 3:], node_mask, edge_mask, edge_x=edge_x, noise_level=noise_level, cond_x=cx, cond_edge_x=cond_edge_x)
        rec_in.append((x[:, :, 3:].clone(), edge_x.clone(), noise_level.clone(), out[0].clone(), out[1].clone()))
        return torch.cat([torch.zeros(B, N, 3), out[0]], dim=2), out[1]

    solver = ref.mix_dpm_solver.DPM_Solver_hybrid(ns, cfg)
    x3, e_end = solver.sampling(model3, torch.cat([torch.zeros(B, N, 3), z], dim=2), nm, em, ez, None)
    x_end = x3[:, :, 3:].contiguous()
    emd = em.reshape(B, N, N, 1)
    assert len(rec_in) == steps, "model calls %d != NFE %d" % (len(rec_in), steps)
    assert torch.equal(e_end, e_end.transpose(1, 2)), "edge end state not symmetric"
    assert float((x_end * (1 - nm)).abs().max()) == 0.0 and float((e_end * (1 - emd)).abs().max()) == 0.0, "padding not zero"
    inv = ref.utils.get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_end.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_end.clone(), em,
                                        cfg.data.compress_edge)
    margins, shares = decision_margins(cfg, inv, x_end, e_end, nm, em)
    atoms, bonds = np.unique(one_hot.argmax(2).numpy()[nm[..., 0].numpy() > 0]), np.unique(et.numpy())
    assert len(atoms) >= 2 and len(bonds) >= 2, "degenerate decodes: atom types %s bond types %s" % (atoms, bonds)
    for k, s in shares.items():
        assert s <= MARGIN_CAP, "%s: %.3f of the real entries within %g of a threshold" % (k, s, MARGIN)
    from oracle.make_golden import savez_stable
    fname = 'traj2d_%s_dpm_%s.npz' % (which, variant)
    arrays = dict(torch_num_threads=np.int64(torch.get_num_threads()), cfg_name=np.array(CFG[which]), seed=np.int64(seed),
                  steps=np.int64(steps), dpm_solver_method=np.array(method), dpm_solver_order=np.int64(order),
                  head_gain=np.float64(HEAD_GAIN_2D), n_nodes=np.array(n_nodes), z=z.numpy(), edge_z=ez.numpy(),
                  x_end=x_end.numpy(), edge_x_end=e_end.numpy(),
                  step_x=torch.stack([r[0] for r in rec_in]).numpy(), step_edge_x=torch.stack([r[1] for r in rec_in]).numpy(),
                  step_noise_level=torch.stack([r[2] for r in rec_in]).numpy(),
                  step_pred_x=torch.stack([r[3] for r in rec_in]).numpy(), step_pred_e=torch.stack([r[4] for r in rec_in]).numpy(),
                  atom_type=one_hot.argmax(2).numpy(), fc=fc.numpy(), edge_type=et.numpy(),
                  margin_kinds=np.array(sorted(margins)), margin_shares=np.array([shares[k] for k in sorted(margins)]),
                  margin_cap=np.float64(MARGIN_CAP))
    for k, v in margins.items():
        arrays['margin_' + k] = v.numpy()
    savez_stable(os.path.join(OUT, fname), **arrays)
    print(fname, 'ok; NFE', steps, 'shares', shares, 'atom types', atoms, 'bond types', bonds, 'bytes',
          os.path.getsize(os.path.join(OUT, fname)))


def main_dpm():
    """The DPM-Solver++ trajectories of the 2-D model (sampling.method 'dpm_2d'); name prefixes select as in main()."""
    torch.set_num_threads(THREADS)
    ref = load_reference()
    jobs = {'traj2d_zinc_dpm_%s' % v: (lambda v=v: dpm_fixture(ref, 'zinc', v)) for v in DPM_VARIANTS}
    jobs['traj2d_moses_dpm_single2'] = lambda: dpm_fixture(ref, 'moses', 'single2', nfe=4)
    want = sys.argv[1:]
    for name, job in jobs.items():
        if not want or any(name.startswith(w) for w in want):
            job()


if __name__ == '__main__':
    main()
    main_dpm()

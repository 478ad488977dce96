"""Training fixture of DGT_concat_sim (the 3-D score network without extra attention heads) from the upstream reference, run on the CPU
through oracle/ref_import.py with 8 torch threads.  Weights are deterministic_init_ (seeded by name): the file stores the seed.

  tests/golden/grad_sim_qm9.npz   the reference's OWN training loss and loss.backward() (losses.py:286-385: get_sde_graph_loss_fn, the
                                  self-conditioning branch taken, eval mode so that dropout is the identity) for the QM9 config with
                                  model.name = 'DGT_concat_sim' on the synthetic batch of tests/helpers.grad_fixture_batch with
                                  n_nodes (5, 9, 7): what it fed to the grad-enabled model call, the targets it built, its loss, and its
                                  gradients of 17 parameters spread over the network (layout of grad_qm9.npz, oracle/make_golden.py
                                  grad_fixture)

While writing it asserts that float32 autograd through tests/oracle_sim.forward_dense reproduces the reference's loss within 1e-5
relative and each recorded gradient within 2e-4 relative (the bound of grad_fixture).
Run:  python tools/make_golden_sim_train.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from oracle.ref_import import load_reference                                        # noqa: E402
from oracle.make_golden import savez_stable                                         # noqa: E402
from oracle import train_ref as T                                                   # noqa: E402
import oracle_sim as OS                                                             # noqa: E402
from helpers import grad_fixture_batch, masks                                       # noqa: E402
from make_golden_sim import CFG, NAME, OUT, THREADS, build_reference_model          # noqa: E402

GRAD_NAMES = ['e_block_0.ff_linear3.weight', 'e_block_0.ff_linear3.bias', 'e_block_5.ff_linear4.weight', 'e_block_5.ff_linear4.bias',
              'e_block_1.attn_mpnn.lin_query.weight', 'e_block_6.attn_mpnn.lin_key.weight', 'e_block_3.attn_mpnn.lin_edge0.weight',
              'e_block_2.node2edge_lin.weight', 'e_block_7.equi_update.coord_mlp.2.weight', 'e_block_0.equi_update.coord_mlp.0.bias',
              'e_block_4.equi_update.coord_norm.scale', 'e_block_6.edge_emb.weight', 'edge_emb.weight', 'node_emb.weight',
              'edge_exist_mlp.4.weight', 'time_mlp.0.weights', 'dist_layer.means.weight']


def grad_fixture(ref, fname='grad_sim_qm9.npz', n_nodes=(5, 9, 7), seed=41):
    import random as pyrandom
    cfg, model = build_reference_model(ref, CFG['qm9'], seed)
    L = ref.losses
    ns = ref.diffusion.noise_schedule.NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                                                      continuous_beta_1=cfg.sde.continuous_beta_1)
    scaler = ref.utils.get_data_scaler(cfg)
    n_nodes = list(n_nodes)
    nm, em = masks(n_nodes)
    batch, py_seed = grad_fixture_batch(cfg, n_nodes, seed)
    loss_fn = L.get_sde_graph_loss_fn(ns, False, scaler, cfg)
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

    model.forward = recording_forward
    orig_align = L.get_align_position

    def rec_align(z_t, xh):
        a = orig_align(z_t, xh)
        rec.update(align_pos=a.clone(), xh=xh.clone())
        return a

    L.get_align_position = rec_align
    pyrandom.seed(py_seed)                                     # first draw < 0.5: the self-conditioning branch of losses.py:335
    torch.manual_seed(seed)
    model.zero_grad()
    try:
        loss = loss_fn(model, batch)
        loss.backward()
    finally:
        L.get_align_position = orig_align
        del model.forward
    assert rec['cond_x'] is not None
    xh, edge_x, _, _, _ = L.process_edge_batch(batch, cfg.device, cfg.model.include_fc_charge, scaler, None)
    assert torch.equal(xh, rec['xh'])
    alpha_t, sigma_t = ns.marginal_prob(rec['t'])
    params = dict(model.named_parameters())
    assert all(k in params and params[k].grad is not None for k in GRAD_NAMES)
    # float32 autograd through tests/oracle_sim.py against the reference's, here and now (the CPU suite checks the committed file again)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    hp = OS.HyperSim.from_config(cfg)
    px, pe = OS.forward_dense(sd, hp, rec['z_t'], nm, em, rec['edge_z_t'], rec['cond_x'], rec['cond_edge_x'], rec['noise_level'])
    assert (px - rec['pred']).abs().max() < 1e-5 and (pe - rec['edge_pred']).abs().max() < 1e-5
    lw = [float(w) for w in cfg.model.loss_weights.split(',')]
    ol = T.sde_graph_loss(px, pe, xh, edge_x, rec['align_pos'], nm, em, alpha_t, sigma_t, lw, cfg.training.reduce_mean)
    ol.backward()
    assert abs(ol.item() - loss.item()) < 1e-5 * abs(loss.item()), (ol.item(), loss.item())
    worst = 0.0
    for k in GRAD_NAMES:
        a, b = sd[k].grad, params[k].grad
        assert float(b.abs().max()) > 0, "the reference's gradient of %s is identically zero" % k
        rel = (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)
        assert rel < 2e-4, "oracle gradient of %s: rel err %g" % (k, rel)
        worst = max(worst, rel)
    path = os.path.join(OUT, fname)
    savez_stable(path, torch_num_threads=np.int64(torch.get_num_threads()), cfg_name=np.array(CFG['qm9']), model_name=np.array(NAME),
                 seed=np.int64(seed), py_seed=np.int64(py_seed), n_nodes=np.array(n_nodes), t=rec['t'].numpy(), z_t=rec['z_t'].numpy(),
                 edge_z_t=rec['edge_z_t'].numpy(), noise_level=rec['noise_level'].numpy(), cond_x=rec['cond_x'].numpy(),
                 cond_edge_x=rec['cond_edge_x'].numpy(), xh=xh.numpy(), edge_x=edge_x.numpy(), align_pos=rec['align_pos'].numpy(),
                 alpha_t=alpha_t.numpy(), sigma_t=sigma_t.numpy(), pred=rec['pred'].numpy(), edge_pred=rec['edge_pred'].numpy(),
                 loss=np.float64(loss.item()), grad_names=np.array(GRAD_NAMES),
                 **{'grad_%d' % i: params[k].grad.numpy() for i, k in enumerate(GRAD_NAMES)})
    print(fname, 'ok; loss', loss.item(), 'oracle worst rel', worst, 'bytes', os.path.getsize(path))


def main():
    torch.set_num_threads(THREADS)
    grad_fixture(load_reference())


if __name__ == '__main__':
    main()

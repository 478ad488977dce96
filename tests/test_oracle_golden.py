"""CPU: the oracle restatement and the host-side samplers against fixtures produced by the real
reference (oracle/make_golden.py).  No GPU, no /root/reference needed."""
import numpy as np
import pytest
import torch

from jodo_amd.diffusion import NoiseScheduleVP
from jodo_amd.mix_dpm_solver import DPM_Solver_hybrid
from jodo_amd.sampling import AncestralSampler, post_process
from jodo_amd.utils import get_data_inverse_scaler, get_self_cond_fn
from oracle import dgt_oracle as O

from helpers import OracleModel, check_decodes, load_fixture, make_config, make_model, masks, state_dict_cpu


@pytest.mark.parametrize("fname", ["fwd_qm9.npz", "fwd_geom.npz", "fwd_cond.npz", "fwd_geom_base.npz"])
def test_oracle_matches_reference_fixture(fname):
    fx = load_fixture(fname)
    over = {k: int(fx[k]) for k in ('nf', 'n_layers') if k in fx}       # fwd_geom_base: the README's nf 128 / 6-layer GEOM model
    cfg = make_config(str(fx['cfg_name']), **over)
    sd = state_dict_cpu(make_model(cfg, int(fx['seed'])))
    hp = O.Hyper.from_config(cfg)
    nm, em = masks(fx['n_nodes'].tolist())
    t = lambda k: torch.from_numpy(fx[k])
    ctx = t('context') if hp.cond_ch else None
    with torch.no_grad():
        f1 = O.forward_faithful(sd, hp, t('xh'), nm, em, t('edge_x'), None, None, t('noise_level'), ctx)
        assert torch.equal(f1[0], t('out1_x')) and torch.equal(f1[1], t('out1_e'))      # bit-exact port
        d2 = O.forward_dense(sd, hp, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), ctx)
    assert (d2[0] - t('out2_x')).abs().max() < 1e-5
    assert (d2[1] - t('out2_e')).abs().max() < 1e-5


def _schedule(cfg):
    return NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0,
                           continuous_beta_1=cfg.sde.continuous_beta_1)


def test_ancestral_sampler_reproduces_reference_trajectory():
    fx = load_fixture('traj_qm9_anc5.npz')
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = 'cpu'
    model = make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain']))
    hp = O.Hyper.from_config(cfg)
    om = OracleModel(state_dict_cpu(model), hp, faithful=True)
    nm, em = masks(fx['n_nodes'].tolist())
    ns = _schedule(cfg)
    steps = int(fx['steps'])
    noise = {'node': torch.from_numpy(fx['node_noise']), 'edge': torch.from_numpy(fx['edge_noise'])}
    sampler = AncestralSampler(ns, torch.linspace(ns.T, 1e-3, steps), True, True, True, get_self_cond_fn(cfg),
                               noise_fn=lambda i, kind, like: noise[kind][i])
    x_mean, e_mean = sampler.sampling(om, torch.from_numpy(fx['z']), nm, em, torch.from_numpy(fx['edge_z']), None)
    # same host logic + oracle model => the reference's trajectory to fp32 reorder noise
    # (the reference's own model differs from the oracle by <= 5e-6 over 5 steps: op-order in scatter sums)
    assert (x_mean - torch.from_numpy(fx['x_mean'])).abs().max() < 1e-3   # K-step trajectory tolerance
    assert (e_mean - torch.from_numpy(fx['edge_x_mean'])).abs().max() < 1e-3   # K-step trajectory tolerance
    check_decodes(cfg, fx, x_mean, e_mean, nm, em)


# hybrid DPM-solver (mix_dpm_solver.py): single-step order 2 (BASELINE config 5), 2nd-order multistep (:230-265 and
# the warm-up / history shifting of :340-372), single-step order 3 (:150-227) and order 1 (:61-93)
@pytest.mark.parametrize("fname", ['traj_cond_dpm4.npz', 'traj_cond_dpm_multi8.npz', 'traj_cond_dpm_single3.npz',
                                   'traj_cond_dpm_single1.npz'])
def test_dpm_solver_reproduces_reference_trajectory(fname):
    fx = load_fixture(fname)
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.device = 'cpu'
    cfg.sampling.steps = int(fx['nfe'])
    cfg.sampling.method = 'fast'
    cfg.sampling.dpm_solver_method = str(fx['method']) if 'method' in fx else 'singlestep_fixed'
    cfg.sampling.dpm_solver_order = int(fx['order']) if 'order' in fx else 2
    model = make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain']))
    om = OracleModel(state_dict_cpu(model), O.Hyper.from_config(cfg), faithful=True)
    nm, em = masks(fx['n_nodes'].tolist())
    pn = torch.from_numpy(fx['pos_noise'])
    solver = DPM_Solver_hybrid(_schedule(cfg), cfg, noise_fn=lambda i, kind, like: pn[i])
    x, ex = solver.sampling(om, torch.from_numpy(fx['z']), nm, em, torch.from_numpy(fx['edge_z']),
                            torch.from_numpy(fx['context']))
    assert (x - torch.from_numpy(fx['x'])).abs().max() < 1e-3   # K-step trajectory tolerance
    assert (ex - torch.from_numpy(fx['edge_x'])).abs().max() < 1e-3   # K-step trajectory tolerance


def test_ancestral_sampler_50_steps_and_teacher_forced_oracle():
    """K = 50 (upper end of SURVEY.md §8c's K-step range): the host sampler + faithful oracle reproduce the
    reference's trajectory, and the dense oracle reproduces every recorded per-step prediction from the recorded
    per-step inputs (teacher forcing; the tolerance of a single forward)."""
    fx = load_fixture('traj_qm9_anc50.npz')
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.device = 'cpu'
    model = make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain']))
    hp = O.Hyper.from_config(cfg)
    sd = state_dict_cpu(model)
    nm, em = masks(fx['n_nodes'].tolist())
    ns = _schedule(cfg)
    steps = int(fx['steps'])
    assert steps == 50 and fx['step_x'].shape[0] == 50
    noise = {'node': torch.from_numpy(fx['node_noise']), 'edge': torch.from_numpy(fx['edge_noise'])}
    sampler = AncestralSampler(ns, torch.linspace(ns.T, 1e-3, steps), True, True, True, get_self_cond_fn(cfg),
                               noise_fn=lambda i, kind, like: noise[kind][i])
    x_mean, e_mean = sampler.sampling(OracleModel(sd, hp, faithful=True), torch.from_numpy(fx['z']), nm, em,
                                      torch.from_numpy(fx['edge_z']), None)
    assert (x_mean - torch.from_numpy(fx['x_mean'])).abs().max() < 1e-3      # K-step trajectory tolerance
    assert (e_mean - torch.from_numpy(fx['edge_x_mean'])).abs().max() < 1e-3
    check_decodes(cfg, fx, x_mean, e_mean, nm, em)
    t = lambda k, i: torch.from_numpy(fx[k][i])
    with torch.no_grad():
        for i in (0, 1, 7, 24, 49):
            cx = None if i == 0 else t('step_pred', i - 1)
            cex = None if i == 0 else t('step_edge_pred', i - 1)
            d = O.forward_dense(sd, hp, t('step_x', i), nm, em, t('step_edge_x', i), cx, cex, t('step_noise_level', i))
            assert (d[0] - t('step_pred', i)).abs().max() < 2e-5
            assert (d[1] - t('step_edge_pred', i)).abs().max() < 5e-5


@pytest.mark.parametrize("fname", ['blocks_qm9.npz', 'blocks_geom.npz'])
def test_oracle_intermediates_match_reference_blocks(fname):
    """The reference's own h / edge_attr / pos after every block (mol_gnn.py:562-568) against the dense oracle's
    per-block intermediates — the same tensors the -m gpu test fetches from the kernels."""
    from helpers import reference_blocks_dense
    fx = load_fixture(fname)
    cfg = make_config(str(fx['cfg_name']))
    sd = state_dict_cpu(make_model(cfg, int(fx['seed'])))
    hp = O.Hyper.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        ox, oe, inter = O.forward_dense(sd, hp, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'),
                                        None, return_intermediates=True)
    assert (ox - t('out2_x')).abs().max() < 1e-5 and (oe - t('out2_e')).abs().max() < 1e-5
    for l in range(hp.n_layers):
        for b, (h, e, pos) in enumerate(reference_blocks_dense(fx, l)):
            n = n_nodes[b]
            offd = ~torch.eye(n, dtype=torch.bool)
            assert (inter[b][l]['h'] - h).abs().max() < 1e-4                     # per-block tolerance
            assert (inter[b][l]['e'][offd] - e[offd]).abs().max() < 1e-4
            assert (inter[b][l]['pos'] - pos).abs().max() < 1e-4


def test_large_molecule_fixture_against_dense_oracle():
    """n = 100 molecule of the GEOM size-range fixture, evaluated alone by the dense oracle (batch independence,
    SURVEY.md §4) — the n = 181 / 140 molecules were checked when the fixture was generated (oracle/make_golden.py
    asserts dense == reference < 1e-5 on the whole batch) and are checked against the kernels in -m gpu."""
    fx = load_fixture('fwd_geom_big.npz')
    cfg = make_config(str(fx['cfg_name']))
    sd = state_dict_cpu(make_model(cfg, int(fx['seed'])))
    hp = O.Hyper.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    assert max(n_nodes) == 181
    b = n_nodes.index(100)
    nm, em = masks([100])
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        d = O.forward_dense(sd, hp, t('xh')[b:b + 1, :100], nm, em, t('edge_x')[b:b + 1, :100, :100],
                            t('out1_x')[b:b + 1, :100], t('out1_e')[b:b + 1, :100, :100], t('noise_level')[b:b + 1])
    assert (d[0] - t('out2_x')[b:b + 1, :100]).abs().max() < 2e-5
    assert (d[1] - t('out2_e')[b:b + 1, :100, :100]).abs().max() < 2e-5


def test_dense_and_faithful_agree_with_edge_cases():
    cfg = make_config('vpsde_qm9_uncond_jodo')
    sd = state_dict_cpu(make_model(cfg, 3, gain=1.5))
    hp = O.Hyper.from_config(cfg)
    from helpers import random_inputs
    xh, ex, nl, ctx, nm, em = random_inputs(hp, [1, 2, 7, 3], 5)
    with torch.no_grad():
        a = O.forward_faithful(sd, hp, xh, nm, em, ex, None, None, nl)
        b = O.forward_dense(sd, hp, xh, nm, em, ex, None, None, nl)
    assert (a[0] - b[0]).abs().max() < 1e-5 and (a[1] - b[1]).abs().max() < 1e-5
    # padded rows / diagonal exactly zero, edge output exactly symmetric
    assert a[0][0, 1:].abs().max() == 0 and a[1][0].abs().max() == 0
    assert torch.equal(a[1], a[1].transpose(1, 2))


def test_oracle_gradients_match_reference_backward():
    """tests/golden/grad_qm9.npz holds the reference's own loss and loss.backward() gradients
    (losses.py:286-385, self-conditioned branch).  Autograd through the dense oracle + the loss restatement must reproduce
    them — that pins the checker of the backward kernels; and phase D as a function (oracle/train_ref.edge_ffn_phase) must
    reproduce the oracle's own block outputs exactly."""
    from oracle import train_ref as T
    fx = load_fixture('grad_qm9.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']))
    hp = O.Hyper.from_config(cfg)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    nm, em = masks(fx['n_nodes'].tolist())
    t = lambda k: torch.from_numpy(fx[k])
    px, pe, inter = O.forward_dense(sd, hp, t('z_t'), nm, em, t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), None,
                                    return_intermediates='graph')
    assert (px.detach() - t('pred')).abs().max() < 2e-5 and (pe.detach() - t('edge_pred')).abs().max() < 2e-5
    lw = [float(w) for w in cfg.model.loss_weights.split(',')]
    loss = T.sde_graph_loss(px, pe, t('xh'), t('edge_x'), t('align_pos'), nm, em, t('alpha_t'), t('sigma_t'), lw, cfg.training.reduce_mean)
    assert abs(loss.item() - float(fx['loss'])) < 1e-5 * float(fx['loss'])
    loss.backward()
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (sd[k].grad - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < 2e-4, "%s: %g" % (k, rel)
    blk = inter[1][5]                                          # molecule 1 (n = 9), block 5
    p5 = 'e_block_5.'
    out = T.edge_ffn_phase(blk['e_in'], blk['ehat'], blk['eg1'], blk['es2'], blk['ec2'], blk['eg2'], sd[p5 + 'ff_linear3.weight'],
                           sd[p5 + 'ff_linear3.bias'], sd[p5 + 'ff_linear4.weight'], sd[p5 + 'ff_linear4.bias'])
    assert torch.equal(out, blk['e_out'])


def test_cond_sampling_eval_fn_reproduces_the_reference():
    """get_cond_sampling_eval_fn (sampling.py:283-392): the reference's own function on its conditional model, two rounds of three
    molecules, ancestral sampler, a stub property classifier (oracle/make_golden.py cond_eval_fixture).  The mirror, driven by the
    faithful oracle port of the model and the same seed, consumes the RNG identically: the same molecules (positions to the K-step
    tolerance, atom / bond types and charges exactly) and the same scaled MAE."""
    from jodo_amd.sampling import get_cond_sampling_eval_fn, full_edge_index
    from oracle.stubs import StubClassifier, FixedNodes, NormalContext
    fx = load_fixture('cond_eval.npz')
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.device = 'cpu'
    cfg.sampling.steps = int(fx['steps'])
    cfg.sampling.method = 'ancestral'
    model = make_model(cfg, int(fx['seed']), head_gain=float(fx['head_gain']))
    om = OracleModel(state_dict_cpu(model), O.Hyper.from_config(cfg), faithful=True)
    prop_norm = {str(fx['cond_property']): {'mean': float(fx['prop_mean']), 'mad': float(fx['prop_mad'])}}
    assert str(fx['cond_property']) == cfg.cond_property
    fn = get_cond_sampling_eval_fn(cfg, _schedule(cfg), FixedNodes(fx['n_nodes'].tolist()), int(fx['batch']), int(fx['n_samples']),
                                   get_data_inverse_scaler(cfg), prop_dist=NormalContext(), prop_norm=prop_norm)
    torch.manual_seed(int(fx['seed']))
    mols, score = fn(om, StubClassifier())
    assert len(mols) == int(fx['n_mols'])
    for i, (pos, at, et, fc) in enumerate(mols):
        assert (pos - torch.from_numpy(fx['pos_%d' % i])).abs().max() < 1e-3
        assert torch.equal(at, torch.from_numpy(fx['atom_%d' % i])) and torch.equal(et, torch.from_numpy(fx['edge_%d' % i]))
        assert torch.equal(fc, torch.from_numpy(fx['fc_%d' % i]))
    assert abs(score - float(fx['score'])) < 1e-3 * max(1.0, abs(float(fx['score'])))
    # the classifier's edge list: fully connected with self-loops, batch offsets, row-major (cond_gen/utils.py:15-38)
    r, c = full_edge_index(3, 2, 'cpu')
    assert r.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5] and c.tolist() == [0, 1, 2] * 3 + [3, 4, 5] * 3


def _drop_fixture_model():
    from oracle import philox_ref as PR
    fx = load_fixture('train_drop_qm9.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), gain=float(fx['gain']))
    hp = O.Hyper.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    p = float(fx['p'])
    assert p == np.float32(cfg.model.dropout)
    ms = [PR.dropout_masks(int(fx['seed%d' % i]), p, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio) for i in (1, 2)]
    return fx, cfg, model, hp, n_nodes, ms


def test_masked_oracle_reproduces_the_reference_in_train_mode():
    """tests/golden/train_drop_qm9.npz: the reference's QM9 model under model.train() with its dropout modules multiplying by the
    training path's masks.  Both oracle forwards with the restated masks reproduce its two calls (faithful bit for bit, dense within
    1e-5), and autograd through the dense oracle its recorded gradients (2e-4 relative) — every block's FFN biases among them."""
    fx, cfg, model, hp, n_nodes, (m1, m2) = _drop_fixture_model()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        f1 = O.forward_faithful(sd, hp, t('xh'), nm, em, t('edge_x'), None, None, t('noise_level'), None, drop=m1)
        f2 = O.forward_faithful(sd, hp, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), None, drop=m2)
        d1 = O.forward_dense(sd, hp, t('xh'), nm, em, t('edge_x'), None, None, t('noise_level'), None, drop=m1)
    assert torch.equal(f1[0], t('out1_x')) and torch.equal(f1[1], t('out1_e'))
    assert torch.equal(f2[0], t('out2_x')) and torch.equal(f2[1], t('out2_e'))
    assert (d1[0] - t('out1_x')).abs().max() < 1e-5 and (d1[1] - t('out1_e')).abs().max() < 1e-5
    px, pe = O.forward_dense(sd, hp, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), None, drop=m2)
    assert (px.detach() - t('out2_x')).abs().max() < 1e-5 and (pe.detach() - t('out2_e')).abs().max() < 1e-5
    ((px * t('d_out_x')).sum() + (pe * t('d_out_e')).sum()).backward()
    names = fx['grad_names'].tolist()
    assert all('e_block_%d.ff_linear%d.bias' % (l, k) in names for l in range(hp.n_layers) for k in (1, 2, 3, 4))
    for i, k in enumerate(names):
        want = t('grad_%d' % i)
        rel = (sd[k].grad - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < 2e-4, "%s: %g" % (k, rel)
    # the fixture sees the masks: the same call with the other seed's masks, or without dropout, is far from it
    with torch.no_grad():
        for other in (m1, None):
            o = O.forward_dense(sd, hp, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'), None, drop=other)
            assert (o[0] - t('out2_x')).abs().max() > 0.1


def test_oracle_drop_none_and_all_ones_masks_leave_the_forward_unchanged():
    """drop=None is the eval-mode oracle of before; masks of ones (p = 0) give the same bits through the dropout branch."""
    from oracle import philox_ref as PR
    fx = load_fixture('fwd_qm9.npz')
    cfg = make_config(str(fx['cfg_name']), n_layers=4)
    sd = state_dict_cpu(make_model(cfg, int(fx['seed'])))
    hp = O.Hyper.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k])
    ones = PR.dropout_masks(123, 0.0, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio)
    with torch.no_grad():
        for fn in (O.forward_faithful, O.forward_dense):
            for cx, cex in ((None, None), (t('out1_x'), t('out1_e'))):
                a = fn(sd, hp, t('xh'), nm, em, t('edge_x'), cx, cex, t('noise_level'), None)
                b = fn(sd, hp, t('xh'), nm, em, t('edge_x'), cx, cex, t('noise_level'), None, drop=None)
                c = fn(sd, hp, t('xh'), nm, em, t('edge_x'), cx, cex, t('noise_level'), None, drop=ones)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
                assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])

"""GPU: the HIP 2-D score network (DGT_concat_2D) and 2-D sampler against the reference's fixtures and the dense CPU oracle
(tests/oracle2d.py).  One forward agrees within the project's forward tolerance atol 2e-5 + rtol 1e-4 as it stands (no yardstick
factor: the reference's own float32 evaluation is within 2 % of that bound of its float64 evaluation for this model); a K-step
trajectory within atol 1e-3 with identical decodes wherever the recorded decision margin exceeds 1e-3."""
import os
import random

import numpy as np
import pytest
import torch

from jodo_amd import sampling as S
from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
from jodo_amd.models import get_node_dist
from jodo_amd.models import utils as mutils
from jodo_amd.utils import get_data_inverse_scaler
from helpers import load_fixture, make_config, make_model, state_dict_cpu, masks, GOLDEN
import oracle2d as O2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL, RTOL = 2e-5, 1e-4
CFG = {'zinc': 'vpsde_zinc_2d_jodo', 'moses': 'vpsde_moses_2d_jodo'}


def fwd_close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = ATOL + RTOL * want.abs()
    print('%s: max |err| %.3e, worst err / bound %.3f' % (what, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all()), "%s: max |err| %g, worst err / bound %g" % (what, err.max().item(), (err / bound).max().item())


def call(model, xh, nm, em, ex, cx, cex, nl):
    with torch.no_grad():
        return model(nl, xh, nm, em, edge_x=ex, cond_x=cx, cond_edge_x=cex, noise_level=nl)


def sym_inputs(cfg, n_nodes, seed, shared_level=None):
    nd, ch = cfg.data.atom_types + int(cfg.model.include_fc_charge), cfg.model.edge_ch
    g = torch.Generator().manual_seed(seed)
    B, N = len(n_nodes), int(max(n_nodes))
    nm, em = masks(n_nodes)
    xh = torch.randn(B, N, nd, generator=g) * nm
    ex = torch.randn(B, N, N, ch, generator=g)
    ex = (ex + ex.transpose(1, 2)) * em.reshape(B, N, N, 1)
    nl = torch.full((B,), float(shared_level)) if shared_level is not None else torch.randn(B, generator=g) * 2
    return xh, ex, nl, nm, em


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_forward_matches_reference_fixture(which):
    fx = load_fixture('fwd2d_%s.npz' % which)
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    o1 = call(model, t('xh'), nm, em, t('edge_x'), None, None, t('noise_level'))
    assert model.last_flags[0].item() == 1                   # symmetric inputs: the once-per-pair path ran
    fwd_close(o1[0], torch.from_numpy(fx['out1_x']), which + ' first step x')
    fwd_close(o1[1], torch.from_numpy(fx['out1_e']), which + ' first step e')
    o2 = call(model, t('xh'), nm, em, t('edge_x'), t('out1_x'), t('out1_e'), t('noise_level'))
    fwd_close(o2[0], torch.from_numpy(fx['out2_x']), which + ' self-conditioned x')
    fwd_close(o2[1], torch.from_numpy(fx['out2_e']), which + ' self-conditioned e')


def test_blocks_match_reference_fixture():
    fx = load_fixture('blocks2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    rows, off = [], 0                                        # fixture order (b, r, c) row-major -> workspace row of the unordered pair
    for n in n_nodes:
        rows += [off + min(r, c) * n + max(r, c) for r in range(n) for c in range(n) if r != c]
        off += n * n
    rows = torch.tensor(rows)
    for l in range(cfg.model.n_layers):
        model.max_blocks = l + 1
        call(model, t('xh'), nm, em, t('edge_x'), t('cond_x'), t('cond_edge_x'), t('noise_level'))
        h, e = model.debug_state()
        fwd_close(h, torch.from_numpy(fx['h'][l]), 'h after block %d' % l)
        fwd_close(e.cpu()[rows], torch.from_numpy(fx['e'][l]), 'e after block %d' % l)


def _oracle64_subset(cfg, sd, idx, xh, ex, cx, cex, nl, n_nodes, chunk=24):
    """float64 dense oracle on the molecules `idx` (outputs are per-molecule independent), chunked by molecules."""
    hp = O2.Hyper2D.from_config(cfg)
    sd64 = {k: v.double() for k, v in sd.items()}
    outs = []
    order = sorted(idx, key=lambda b: n_nodes[b])            # similar sizes together: less padding per chunk
    for i in range(0, len(order), chunk):
        sel = order[i:i + chunk]
        ns = [int(n_nodes[b]) for b in sel]
        N = max(ns)
        nm, em = masks(ns)
        s = torch.tensor(sel)
        cut = lambda v, two: v[s][:, :N, :N].double() if two else v[s][:, :N].double()
        with torch.no_grad():
            ox, oe = O2.forward_dense(sd64, hp, cut(xh, 0), nm, em, cut(ex, 1), cut(cx, 0), cut(cex, 1), nl[s].double())
        outs += [(b, ox[j], oe[j]) for j, b in enumerate(sel)]
    return outs


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_full_size_batch_against_float64_oracle(which):
    """The configs' evaluation batch (2000 molecules, atom counts drawn from the training histogram), self-conditioned step on the
    HIP model's own first-step output; every 10th molecule plus the smallest and the largest against the float64 oracle."""
    cfg = make_config(CFG[which])
    model = make_model(cfg, 7, DEV)
    torch.manual_seed(5)
    n_nodes = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), cfg.data.info_name)).sample(2000).tolist()
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 17, shared_level=0.7 if which == 'zinc' else None)
    d = lambda v: v.to(DEV)
    o1 = call(model, d(xh), d(nm), d(em), d(ex), None, None, d(nl))
    o2 = call(model, d(xh), d(nm), d(em), d(ex), o1[0], o1[1], d(nl))
    assert model.last_flags.tolist()[:2] == [1, 1 if which == 'zinc' else 0]
    c1x, c1e, o2x, o2e = o1[0].cpu(), o1[1].cpu(), o2[0].cpu(), o2[1].cpu()
    idx = sorted(set(range(0, 2000, 10)) | {int(np.argmin(n_nodes)), int(np.argmax(n_nodes))})
    worst = 0.0
    for b, ox, oe in _oracle64_subset(cfg, state_dict_cpu(model), idx, xh, ex, c1x, c1e, nl, n_nodes):
        n = ox.shape[0]
        for got, want in ((o2x[b, :n].double(), ox), (o2e[b, :n, :n].double(), oe)):
            err = (got - want).abs()
            worst = max(worst, float((err / (ATOL + RTOL * want.abs())).max()))
    print(which, 'B=2000 subset of', len(idx), 'molecules: worst err / bound', worst)
    assert worst <= 1.0
    # padding and the diagonal exactly zero, edge output exactly symmetric — on the whole batch
    assert float((o2x * (1 - nm)).abs().max()) == 0.0
    assert float((o2e * (1 - em.reshape(o2e.shape[0], o2e.shape[1], o2e.shape[1], 1))).abs().max()) == 0.0
    assert torch.equal(o2e, o2e.transpose(1, 2))


def test_invariants_permutation_and_batch_independence():
    cfg = make_config(CFG['zinc'])
    model = make_model(cfg, 7, DEV)
    n_nodes = [11, 38, 1, 2, 33, 20]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 3)
    d = lambda v: v.to(DEV)
    o1 = call(model, d(xh), d(nm), d(em), d(ex), None, None, d(nl))
    o2 = call(model, d(xh), d(nm), d(em), d(ex), o1[0], o1[1], d(nl))
    B, N = len(n_nodes), max(n_nodes)
    for ox, oe in (o1, o2):
        assert float((ox.cpu() * (1 - nm)).abs().max()) == 0.0
        assert float((oe.cpu() * (1 - em.reshape(B, N, N, 1))).abs().max()) == 0.0
        assert torch.equal(oe, oe.transpose(1, 2))
    # an atom permutation inside every molecule permutes the outputs
    g = torch.Generator().manual_seed(9)
    perm = torch.stack([torch.cat([torch.randperm(n, generator=g), torch.arange(n, N)]) for n in n_nodes])
    bi = torch.arange(B).unsqueeze(1)
    px = lambda v: v[bi, perm]
    pe = lambda v: v[bi.unsqueeze(2), perm.unsqueeze(2), perm.unsqueeze(1)]
    c1x, c1e = o1[0].cpu(), o1[1].cpu()
    q2 = call(model, d(px(xh)), d(nm), d(em), d(pe(ex)), d(px(c1x)), d(pe(c1e)), d(nl))
    fwd_close(q2[0], px(o2[0].cpu()), 'permuted atoms x')
    fwd_close(q2[1], pe(o2[1].cpu()), 'permuted atoms e')
    # a molecule alone equals the same molecule inside the batch
    for b in (1, 4):
        n = n_nodes[b]
        nm1, em1 = masks([n], DEV)
        s2 = call(model, d(xh[b:b + 1, :n]), nm1, em1, d(ex[b:b + 1, :n, :n]), d(c1x[b:b + 1, :n]), d(c1e[b:b + 1, :n, :n]), d(nl[b:b + 1]))
        fwd_close(s2[0][0], o2[0][b, :n].cpu(), 'molecule %d alone x' % b)
        fwd_close(s2[1][0], o2[1][b, :n, :n].cpu(), 'molecule %d alone e' % b)


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_asymmetric_edge_input_matches_oracle(which):
    cfg = make_config(CFG[which])
    model = make_model(cfg, 7, DEV)
    n_nodes = [9, 27, 1, 2, 16]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 4)
    g = torch.Generator().manual_seed(12)
    B, N = len(n_nodes), max(n_nodes)
    ex = torch.randn(B, N, N, cfg.model.edge_ch, generator=g) * em.reshape(B, N, N, 1)          # not symmetric
    cx = torch.randn(xh.shape, generator=g) * nm
    cex = torch.randn(ex.shape, generator=g) * em.reshape(B, N, N, 1)
    om = O2.OracleModel2D(state_dict_cpu(model), O2.Hyper2D.from_config(cfg), dtype=torch.float64)
    d = lambda v: v.to(DEV)
    for c1, c2, tag in ((None, None, 'first step'), (cx, cex, 'self-conditioned')):
        got = call(model, d(xh), d(nm), d(em), d(ex), None if c1 is None else d(c1), None if c2 is None else d(c2), d(nl))
        assert model.last_flags[0].item() == 0               # the directed fallback ran
        want = om(None, xh.double(), nm, em, edge_x=ex.double(), cond_x=c1, cond_edge_x=c2, noise_level=nl.double())
        fwd_close(got[0], want[0], which + ' asymmetric ' + tag + ' x')
        fwd_close(got[1], want[1], which + ' asymmetric ' + tag + ' e')
        assert torch.equal(got[1], got[1].transpose(1, 2))   # 0.5 (E + E^T) is symmetric whatever the input
    # symmetric inputs through the directed fallback give the once-per-pair result within the bound
    xs, es, nls, nms, ems = sym_inputs(cfg, n_nodes, 5)
    a = call(model, d(xs), d(nms), d(ems), d(es), None, None, d(nls))
    model.force_directed = True
    b = call(model, d(xs), d(nms), d(ems), d(es), None, None, d(nls))
    model.force_directed = False
    fwd_close(b[0], a[0].cpu(), 'directed vs pair x')
    fwd_close(b[1], a[1].cpu(), 'directed vs pair e')


def test_weight_updates_reach_the_kernels():
    """The stale-blob cases: a `.data` write + invalidate_packed_weights(), a `.data` write caught by the fingerprint on a new batch,
    and load_state_dict must all change the output like the oracle says."""
    cfg = make_config(CFG['zinc'])
    model = make_model(cfg, 7, DEV)
    n_nodes = [7, 12, 3]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 6)
    d = lambda v: v.to(DEV)
    nmd, emd = d(nm), d(em)
    hp = O2.Hyper2D.from_config(cfg)

    def check(tag, masks_=None):
        m_ = masks_ or (nmd, emd)
        got = call(model, d(xh), m_[0], m_[1], d(ex), None, None, d(nl))
        want = O2.OracleModel2D(state_dict_cpu(model), hp)(None, xh, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)
        fwd_close(got[0], want[0], tag + ' x')
        fwd_close(got[1], want[1], tag + ' e')
        return got

    base = check('initial weights')
    with torch.no_grad():
        model.e_block_2.attn_mpnn.lin_edge1.weight.data.mul_(1.5)
        model.node_pred_mlp[4].weight.data.mul_(2.0)
    model.invalidate_packed_weights()
    upd = check('after .data.mul_ + invalidate_packed_weights')
    assert float((upd[0] - base[0]).abs().max()) > 1e-3
    with torch.no_grad():
        model.edge_exist_mlp[4].weight.data.mul_(3.0)
    upd2 = check('after .data.mul_ seen by a new batch', masks([7, 12, 3], DEV))
    assert float((upd2[1] - upd[1]).abs().max()) > 1e-3
    fresh = make_model(cfg, 19)
    model.load_state_dict(fresh.state_dict())
    upd3 = check('after load_state_dict')
    assert float((upd3[0] - upd2[0]).abs().max()) > 1e-3


def _replay(fx):
    return lambda i, kind, like: torch.from_numpy(fx['node_noise' if kind == 'node' else 'edge_noise'][i]).to(like.device)


@pytest.mark.parametrize('which', ['zinc', 'moses'])
def test_trajectory_free_running_and_teacher_forced(which):
    fx = load_fixture('traj2d_%s_anc5.npz' % which)
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    steps = int(fx['steps'])
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    # free-running
    sampler = S.AncestralSampler_2D(ns, torch.linspace(ns.T, 1e-3, steps), cfg.model.pred_data, cfg.model.self_cond, noise_fn=_replay(fx))
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    ex_, ee_ = (x_mean.cpu() - torch.from_numpy(fx['x_mean'])).abs().max().item(), (e_mean.cpu() - torch.from_numpy(fx['edge_x_mean'])).abs().max().item()
    print(which, 'free-running end state: max |err|', ex_, ee_)
    assert ex_ <= 1e-3 and ee_ <= 1e-3
    inv = get_data_inverse_scaler(cfg)
    one_hot, fc, et = S.post_process_2D(x_mean.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, e_mean.clone(), em,
                                        cfg.data.compress_edge)
    bad, excluded = O2.decode_agrees(fx, one_hot.argmax(2).cpu().numpy(), fc.cpu().numpy(), et.cpu().numpy(), n_nodes)
    print(which, 'decodes: mismatches', bad, 'excluded share', excluded)
    assert bad == 0
    assert excluded <= float(fx['margin_cap']) and float(fx['margin_shares'].max()) <= float(fx['margin_cap']) == 0.05
    # teacher-forced: every recorded step input reproduces the recorded prediction at the forward bound
    t = lambda k, i: torch.from_numpy(fx[k][i]).to(DEV)
    for i in range(steps):
        cx, cex = (None, None) if i == 0 else (t('step_pred_x', i - 1), t('step_pred_e', i - 1))
        got = call(model, t('step_x', i), nm, em, t('step_edge_x', i), cx, cex, t('step_noise_level', i))
        fwd_close(got[0], torch.from_numpy(fx['step_pred_x'][i]), '%s teacher-forced step %d x' % (which, i))
        fwd_close(got[1], torch.from_numpy(fx['step_pred_e'][i]), '%s teacher-forced step %d e' % (which, i))


def test_sampling_fn_2d_on_gpu_reproduces_reference_run():
    """samplefn2d_zinc through get_sampling_fn with the draws replayed from the CPU generator (cpu_noise), the model wrapped like the
    reference's create_model does (DataParallel over the one device)."""
    fx = load_fixture('samplefn2d_zinc.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.device = torch.device(DEV)
    cfg.sampling.steps = int(fx['steps'])
    model = mutils.create_model(cfg, wrap='dataparallel')
    from jodo_amd.models import deterministic_init_
    deterministic_init_(model.module, seed=int(fx['model_seed']))
    with torch.no_grad():
        sd = model.module.state_dict()
        for k in ('node_pred_mlp.4.weight', 'edge_type_mlp.4.weight', 'edge_exist_mlp.4.weight'):
            sd[k].mul_(float(fx['head_gain']))
    model.module.invalidate_packed_weights()
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    dist = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k'))
    batch = int(fx['batch'])
    fn = S.get_sampling_fn(cfg, ns, dist, batch, batch, get_data_inverse_scaler(cfg), return_raw=True, cpu_noise=True)
    torch.manual_seed(int(fx['seed']))
    random.seed(int(fx['seed']))
    mols = fn(model)
    assert [int(m[1].shape[0]) for m in mols] == fx['n_nodes'].tolist()
    at, fc, et = np.zeros_like(fx['atom_type']), np.zeros_like(fx['fc']), np.zeros_like(fx['edge_type'])
    for b, (pos, a, e, q) in enumerate(mols):
        n = a.shape[0]
        assert pos is None
        at[b, :n], et[b, :n, :n], fc[b, :n, 0] = a.numpy(), e.numpy(), q.numpy()
    bad, excluded = O2.decode_agrees(fx, at, fc, et, fx['n_nodes'].tolist())
    print('samplefn2d: mismatches', bad, 'excluded share', excluded)
    assert bad == 0 and excluded <= 0.05


def test_runs_under_single_device_dataparallel_and_reuses_its_plan():
    cfg = make_config(CFG['moses'])
    cfg.device = torch.device(DEV)
    model = mutils.create_model(cfg, wrap='dataparallel')
    inner = model.module
    n_nodes = [5, 9, 2]
    xh, ex, nl, nm, em = sym_inputs(cfg, n_nodes, 8)
    d = lambda v: v.to(DEV)
    nmd, emd = d(nm), d(em)
    with torch.no_grad():
        a = model(d(nl), d(xh), nmd, emd, edge_x=d(ex), cond_x=None, cond_edge_x=None, noise_level=d(nl))
        plans = len(inner._plans)
        b = model(d(nl), d(xh), nmd, emd, edge_x=d(ex), cond_x=a[0], cond_edge_x=a[1], noise_level=d(nl))
    assert len(inner._plans) == plans == 1                   # the second call found the first one's descriptor and workspace
    om = O2.OracleModel2D(state_dict_cpu(inner), O2.Hyper2D.from_config(cfg))
    want = om(None, xh, nm, em, edge_x=ex, cond_x=a[0].cpu(), cond_edge_x=a[1].cpu(), noise_level=nl)
    fwd_close(b[0], want[0], 'DataParallel x')
    fwd_close(b[1], want[1], 'DataParallel e')
    with pytest.raises(RuntimeError, match='cannot be replicated'):
        inner._replicate_for_data_parallel()


def test_sampler_step_2d_kernel_matches_torch():
    from jodo_amd import fused
    g = torch.Generator().manual_seed(2)
    n_nodes = [4, 9, 1]
    B, N, nd, ch = 3, 9, 10, 2
    nm, em = masks(n_nodes)
    x, pred = torch.randn(B, N, nd, generator=g) * nm, torch.randn(B, N, nd, generator=g) * nm
    emd = em.reshape(B, N, N, 1)
    sym = lambda v: (torch.tril(v.permute(0, 3, 1, 2), -1) + torch.tril(v.permute(0, 3, 1, 2), -1).transpose(-1, -2)).permute(0, 2, 3, 1) * emd
    e, epred, eeps = sym(torch.randn(B, N, N, ch, generator=g)), sym(torch.randn(B, N, N, ch, generator=g)), sym(torch.randn(B, N, N, ch, generator=g))
    eps = torch.randn(B, N, nd, generator=g) * nm
    d = lambda v: v.to(DEV)
    xn, en, xm, emn = fused.sampler_step_2d(d(torch.tensor(n_nodes, dtype=torch.int32)), 0.9, 0.2, 0.3, d(x), d(e), d(pred), d(epred), d(eps), d(eeps))
    assert torch.allclose(xm.cpu(), 0.9 * x + 0.2 * pred, atol=1e-6) and torch.allclose(emn.cpu(), 0.9 * e + 0.2 * epred, atol=1e-6)
    assert torch.allclose(xn.cpu(), 0.9 * x + 0.2 * pred + 0.3 * eps, atol=1e-6)
    assert torch.allclose(en.cpu(), 0.9 * e + 0.2 * epred + 0.3 * eeps, atol=1e-6)
    assert torch.equal(en, en.transpose(1, 2))

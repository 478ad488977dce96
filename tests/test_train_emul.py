"""CPU checks of the training path: the SAME kernel sources that libjodo_hip.so runs on the GPU
(jodo_amd/csrc/dgt_train.hip + train_ops.h), compiled for the host by tests/emul/Makefile against a sequential stand-in for the HIP
runtime (tests/emul/hip/hip_runtime.h; the MFMA GEMM is replaced by plain loops), driven with host pointers and compared with
torch.autograd through the oracle and with the reference's own loss.backward() (tests/golden/grad_qm9.npz).  This checks the
calculus and the index arithmetic of every training kernel where there is no GPU; tests/test_train_gpu.py repeats it on the device."""
import ctypes
import os
import subprocess

import pytest
import torch

from oracle import dgt_oracle as O
from oracle import train_ref as T

from helpers import load_fixture, make_config, make_model, masks, random_inputs

EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emul')


@pytest.fixture(scope='module')
def emul():
    subprocess.run(['make', '-C', EMUL_DIR], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(EMUL_DIR, 'libjodo_train_emul.so'))


def engine_for(emul, model, n_nodes):
    from jodo_amd.train import TrainEngine
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    return TrainEngine(model._cfg(), n_nodes, max(n_nodes), named, 'cpu', lib=emul, stream_ptr=lambda: ctypes.c_void_p(0)), [k for k, _ in named]


def oracle_grads(model, hp, xh, nm, em, ex, cx, cex, nl, ctx, d_out_x, d_out_e, dtype=torch.float64):
    """d <d_out, outputs> / d parameters by autograd through oracle.forward_dense."""
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in model.state_dict().items()}
    c = lambda t: None if t is None else t.to(dtype)
    px, pe = O.forward_dense(sd, hp, c(xh), c(nm), c(em), c(ex), c(cx), c(cex), c(nl), c(ctx))
    ((px * d_out_x.to(dtype)).sum() + (pe * d_out_e.to(dtype)).sum()).backward()
    return px.detach(), pe.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}


def compare_all(names, grads, want, rel_tol):
    bad = []
    for k, g in zip(names, grads):
        w = want[k].double()
        scale = float(w.abs().max())
        err = float((g.double() - w).abs().max())
        if not err <= rel_tol * max(scale, 1e-12) + 1e-12:
            bad.append("%s: err %.3e scale %.3e" % (k, err, scale))
    assert not bad, "%d of %d parameter gradients differ:\n  %s" % (len(bad), len(names), "\n  ".join(bad[:40]))


def test_training_step_reproduces_the_reference_backward(emul):
    """The reference's recorded training step (grad_qm9: QM9 model, self-conditioned branch, eval-mode dropout): forward ==
    the reference's prediction, loss == its loss, and after loss.backward() through the kernels the 17 recorded parameter
    gradients == the reference's, every other parameter == autograd through the oracle."""
    fx = load_fixture('grad_qm9.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']))
    hp = O.Hyper.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes)
    t = lambda k: torch.from_numpy(fx[k]).contiguous()
    eng, names = engine_for(emul, model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    out_x, out_e = eng.forward(params, t('z_t'), t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), None, 0.0, 0)
    assert eng.flags.tolist()[0] == 0 and eng.flags.tolist()[3] == 1
    assert (out_x - t('pred')).abs().max() < 2e-5 and (out_e - t('edge_pred')).abs().max() < 2e-5
    px, pe = out_x.clone().requires_grad_(True), out_e.clone().requires_grad_(True)
    lw = [float(w) for w in cfg.model.loss_weights.split(',')]
    loss = T.sde_graph_loss(px, pe, t('xh'), t('edge_x'), t('align_pos'), nm, em, t('alpha_t'), t('sigma_t'), lw, cfg.training.reduce_mean)
    assert abs(loss.item() - float(fx['loss'])) < 1e-5 * float(fx['loss'])
    loss.backward()
    grads = eng.backward(params, t('noise_level'), px.grad.contiguous(), pe.grad.contiguous(), 0.0, 0)
    by_name = dict(zip(names, grads))
    for i, k in enumerate(fx['grad_names'].tolist()):
        want = t('grad_%d' % i)
        rel = (by_name[k] - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert rel < 2e-4, "%s: %g" % (k, rel)
    _, _, want = oracle_grads(model, hp, t('z_t'), nm, em, t('edge_z_t'), t('cond_x'), t('cond_edge_x'), t('noise_level'), None, px.grad, pe.grad)
    compare_all(names, grads, want, 2e-4)


@pytest.mark.parametrize("cfg_name,n_nodes,over,selfcond", [
    ('vpsde_qm9_uncond_jodo', [4, 1, 2, 6], dict(nf=128, n_layers=2), False),       # first-step branch, n = 1 and 2
    ('vpsde_qm9_cond_jodo', [3, 5], dict(nf=128, n_layers=2), True),                # conditional model: cond_mlp / cond_lin
    ('vpsde_geom_uncond_jodo', [7, 3], dict(nf=128, n_layers=2), True),             # edge_ch 3, mlp_ratio 4, nd 17
])
def test_all_parameter_gradients_match_autograd_through_the_oracle(emul, cfg_name, n_nodes, over, selfcond):
    cfg = make_config(cfg_name, **over)
    model = make_model(cfg, 3, gain=1.5, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=5)
    g = torch.Generator().manual_seed(9)
    cx = cex = None
    if selfcond:
        cx = torch.randn(xh.shape, generator=g) * nm
        cex = torch.randn(ex.shape, generator=g)
        cex = (cex + cex.transpose(1, 2)) * em.reshape(ex.shape[0], ex.shape[1], ex.shape[1], 1)
    d_x = torch.randn(xh.shape, generator=g)
    d_e = torch.randn(ex.shape, generator=g)                   # not symmetric, not masked: the kernels must mask and symmetrise
    eng, names = engine_for(emul, model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    out_x, out_e = eng.forward(params, xh, ex, cx, cex, nl, ctx, 0.0, 0)
    px, pe, want = oracle_grads(model, hp, xh, nm, em, ex, cx, cex, nl, ctx, d_x, d_e)
    assert (out_x.double() - px).abs().max() < 2e-5 and (out_e.double() - pe).abs().max() < 2e-5
    assert eng.flags.tolist()[3] == (1 if selfcond else 0)
    grads = eng.backward(params, nl, d_x, d_e, 0.0, 0)
    compare_all(names, grads, want, 3e-4)


# ---- the batch sizes at which the backward's reductions change form (tests/train_scale_common.py) ---------------------
@pytest.mark.parametrize("case,passes", [
    ('ABOVE_64K', (None, 3, 0)),        # R = 67 663: second-level chunk 34, the Gaussian layer's colsum in two levels; bulk | last | first molecule
    ('CHUNK_EDGES', (None,)),           # per-molecule edge chunks of 34 | 32 | 64 rows
    ('GBF_BY_SIZE', (3,)),              # R = 131 044: both colsum levels behind 4 096 chunk rows; the last molecule alone
])
def test_size_selected_reductions_match_autograd_through_the_oracle(emul, case, passes):
    """The colsum levels, the FinJob queue and the per-molecule chunk tables of csrc/dgt_train.hip, run on the host from the same source,
    against float64 autograd through the oracle by the gradient rule (3e-4 of the tensor's scale, widened to 16 x the float32-autograd
    distance).  One forward serves every pass.  Passes confined to one molecule: train_scale_common.UNWIDENED says what they assert of the
    widened bounds.  tests/test_train_scale_gpu.py repeats the cases on the device."""
    import time
    import train_scale_common as S
    from helpers import compare_grads
    n_nodes = getattr(S, case)
    xh, ex, nl, nm, em, _, _ = S.batch(n_nodes)
    t0 = time.time()
    eng, names, params = S.make_engine(n_nodes, 'cpu', lib=emul)
    out_x, out_e = eng.forward(params, xh, ex, None, None, nl, None, 0.0, 0)
    assert eng.flags.tolist()[0] == 0 and eng.flags.tolist()[3] == 0
    t_eng = time.time() - t0
    for local in passes:
        d_x, d_e = S.out_grads(n_nodes, local)
        t0 = time.time()
        grads = eng.backward(params, nl, d_x, d_e, 0.0, 0)
        t_eng += time.time() - t0
        px, pe, want = S.yardstick(n_nodes, local)
        want32 = S.yardstick(n_nodes, local, torch.float32)[2]
        assert (out_x.double() - px).abs().max() < 2e-5 and (out_e.double() - pe).abs().max() < 2e-5
        S.assert_reduced_nonzero(want, '%s pass %s' % (case, local))
        what = '%s, output gradient on %s' % (case, 'every molecule' if local is None else 'molecule %d' % local)
        ratio, widened = compare_grads(zip(names, grads), want, S.GRAD_REL, want32, S.K32, what=what)
        S.check_widening(n_nodes, local, widened, what)
    print('%s: forward + %d backwards through the emulation build %.1f s' % (case, len(passes), t_eng))


def test_dropout_masks_are_shared_by_forward_and_backward(emul):
    """With dropout on, the backward must differentiate the function the forward evaluated: directional finite differences of
    <d_out, forward(theta + eps v)> at a fixed seed against <grads, v>; another seed gives another function; p = 0 is the eval path."""
    cfg = make_config('vpsde_qm9_uncond_jodo', nf=128, n_layers=2)
    model = make_model(cfg, 4, gain=1.5, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    n_nodes = [5, 3]
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=8)
    g = torch.Generator().manual_seed(2)
    d_x, d_e = torch.randn(xh.shape, generator=g), torch.randn(ex.shape, generator=g)
    eng, names = engine_for(emul, model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    p, seed = 0.1, 1234
    o0 = eng.forward(params, xh, ex, None, None, nl, None, 0.0, seed)
    alpha0, hhat0 = eng.debug_fetch(1, 0), eng.debug_fetch(0, 0)
    hhat0_last = eng.debug_fetch(0, hp.n_layers - 1)
    o1 = eng.forward(params, xh, ex, None, None, nl, None, p, seed)
    # Where dropout acts.  The reference drops in the four FFN positions of a block (mol_gnn.py:262-268) and NOT on the attention
    # weights: F.dropout(alpha, p=self.dropout) at layers.py:179 runs with TransMixLayer's default dropout = 0 because the block
    # never passes its own (mol_gnn.py:230-231).  Block 0's attention precedes every live site, so its softmax weights and its
    # output must not move with p; the last block's input has been through the FFN sites and must.
    assert torch.equal(eng.debug_fetch(1, 0), alpha0) and torch.equal(eng.debug_fetch(0, 0), hhat0)
    assert float(alpha0.abs().max()) > 0 and not torch.equal(eng.debug_fetch(0, hp.n_layers - 1), hhat0_last)
    o1b = eng.forward(params, xh, ex, None, None, nl, None, p, seed)
    o2 = eng.forward(params, xh, ex, None, None, nl, None, p, seed + 1)
    assert torch.equal(o1[0], o1b[0]) and torch.equal(o1[1], o1b[1])
    assert not torch.equal(o1[0], o0[0]) and not torch.equal(o1[0], o2[0])
    eng.forward(params, xh, ex, None, None, nl, None, p, seed)
    grads = eng.backward(params, nl, d_x, d_e, p, seed)
    f = lambda ps: float(sum((a.double() * b.double()).sum() for a, b in zip(eng.forward(ps, xh, ex, None, None, nl, None, p, seed), (d_x, d_e))))
    vs = [torch.randn(q.shape, generator=g) * q.abs().mean().clamp(min=1e-3) for q in params]
    eps = 1e-3
    plus = f([(q.double() + eps * v.double()).float() for q, v in zip(params, vs)])
    minus = f([(q.double() - eps * v.double()).float() for q, v in zip(params, vs)])
    fd = (plus - minus) / (2 * eps)
    an = float(sum((gq.double() * v.double()).sum() for gq, v in zip(grads, vs)))
    assert abs(fd - an) <= 2e-2 * max(abs(an), abs(fd), 1e-6), (fd, an)


# ---- dropout on: the kernels against the float64 oracle with the restated masks (oracle/philox_ref.dropout_masks) ----------------
DROP_SEED = (0x5DEECE66D << 20) | 0x1234567           # >= 2^32: the key's high word matters


def drop_masks_for(hp, n_nodes, p, seed):
    from oracle import philox_ref as PR
    return PR.dropout_masks(seed, p, n_nodes, hp.n_layers, hp.nf, hp.de, hp.mlp_ratio)


def oracle_grads_masked(model, hp, xh, nm, em, ex, cx, cex, nl, ctx, d_out_x, d_out_e, drop, dtype=torch.float64):
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in model.state_dict().items()}
    c = lambda t: None if t is None else t.to(dtype)
    px, pe = O.forward_dense(sd, hp, c(xh), c(nm), c(em), c(ex), c(cx), c(cex), c(nl), c(ctx), drop=drop)
    ((px * d_out_x.to(dtype)).sum() + (pe * d_out_e.to(dtype)).sum()).backward()
    return px.detach(), pe.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}


@pytest.mark.parametrize("cfg_name,n_nodes,over,selfcond", [
    ('vpsde_qm9_uncond_jodo', [4, 1, 2, 6], dict(nf=128, n_layers=2), False),
    ('vpsde_qm9_uncond_jodo', [5, 3, 7], dict(nf=128, n_layers=2), True),
    ('vpsde_qm9_cond_jodo', [3, 5], dict(nf=128, n_layers=2), True),
    ('vpsde_qm9_cond_jodo', [6, 2, 4], dict(nf=128, n_layers=2), False),
])
def test_dropout_on_matches_autograd_through_the_masked_oracle(emul, cfg_name, n_nodes, over, selfcond):
    """Training-mode dropout (p = 0.1, a seed above 2^32) through the emulation build against float64 autograd through the oracle
    with the restated masks: the outputs and every parameter's gradient.  Pins the site numbering, the row numbering of nodes and
    edge pairs, the scale, and that nothing else (the attention weights) is dropped."""
    cfg = make_config(cfg_name, **over)
    model = make_model(cfg, 3, gain=1.5, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=5)
    g = torch.Generator().manual_seed(9)
    cx = cex = None
    if selfcond:
        cx = torch.randn(xh.shape, generator=g) * nm
        cex = torch.randn(ex.shape, generator=g)
        cex = (cex + cex.transpose(1, 2)) * em.reshape(ex.shape[0], ex.shape[1], ex.shape[1], 1)
    d_x = torch.randn(xh.shape, generator=g)
    d_e = torch.randn(ex.shape, generator=g)
    p = 0.1
    drop = drop_masks_for(hp, n_nodes, p, DROP_SEED)
    eng, names = engine_for(emul, model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    out_x, out_e = eng.forward(params, xh, ex, cx, cex, nl, ctx, p, DROP_SEED)
    px, pe, want = oracle_grads_masked(model, hp, xh, nm, em, ex, cx, cex, nl, ctx, d_x, d_e, drop)
    assert (out_x.double() - px).abs().max() < 2e-5 and (out_e.double() - pe).abs().max() < 2e-5
    with torch.no_grad():                                       # the masks matter at this size: eval mode is far away
        ev = O.forward_dense({k: v.double() for k, v in model.state_dict().items()}, hp, xh.double(), nm.double(), em.double(), ex.double(),
                             None if cx is None else cx.double(), None if cex is None else cex.double(), nl.double(),
                             None if ctx is None else ctx.double())
    assert (ev[0] - px).abs().max() > 1e-3
    grads = eng.backward(params, nl, d_x, d_e, p, DROP_SEED)
    compare_all(names, grads, want, 3e-4)


def test_dropout_kernel_activations_follow_the_restated_masks(emul):
    """The kept FFN activations of the emulation build (jodo_train_debug_locate 2 - 7): a1 and a3 are zero exactly where the
    restatement drops, and elsewhere SiLU(f) x 1 / (1 - p) to a few ulps; first and last block, p 0.1 and 0.5, a seed above 2^32."""
    from oracle import philox_ref as PR
    cfg = make_config('vpsde_qm9_uncond_jodo', nf=128, n_layers=3)
    model = make_model(cfg, 4, gain=1.5, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    n_nodes = [5, 1, 8, 3]
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=8)
    eng, names = engine_for(emul, model, n_nodes)
    params = [v.detach().float().contiguous() for v in model.state_dict().values()]
    for p, seed in ((0.1, DROP_SEED), (0.5, 7)):
        eng.forward(params, xh, ex, None, None, nl, None, p, seed)
        for l in (0, hp.n_layers - 1):
            check_ffn_masks(eng, hp, n_nodes, p, seed, l, PR)


_MASKS = {}


def check_ffn_masks(eng, hp, n_nodes, p, seed, l, PR):
    """a1 / a3 of block l against the restated masks of sites A1 / A3 (shared with tests/test_train_dropout_gpu.py)."""
    Nn, R = sum(n_nodes), sum(n * n for n in n_nodes)
    r, D, De = hp.mlp_ratio, hp.nf, hp.de
    scale = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)))
    for f_sel, a_sel, site, count in ((2, 3, 'A1', Nn * r * D), (5, 6, 'A3', R * r * De)):
        f, a = eng.debug_fetch(f_sel, l).cpu().double(), eng.debug_fetch(a_sel, l).cpu().double()
        assert f.numel() == count and a.numel() == count
        key = (seed, PR.drop_site(l, site), p, count)
        if key not in _MASKS:
            _MASKS[key] = torch.from_numpy(PR.drop_mul(*key))
        m = _MASKS[key]
        dropped = m == 0
        frac = float(dropped.double().mean())
        assert abs(frac - p) < 5 * (p * (1 - p) / count) ** 0.5 + 1e-12, (l, site, frac)
        want = torch.where(dropped, 0.0, (f * torch.sigmoid(f)) * scale)
        # dropped: exactly 0; kept: SiLU(f) / (1 - p) to a few ulps (0 only where SiLU(f) is)
        bad = (a - want).abs() > 4 * 2.0 ** -23 * want.abs()
        if bool(bad.any()):
            i = bad.nonzero()[:8, 0].tolist()
            w = count // (Nn if site == 'A1' else R)
            raise AssertionError("block %d site %s (p %g, seed %d): %d of %d elements differ; first (row, feature, f, a, restated multiplier): %s"
                                 % (l, site, p, seed, int(bad.sum()), count, [(j // w, j % w, float(f[j]), float(a[j]), float(m[j])) for j in i]))


# ---- host properties of the mask restatement ------------------------------------------------------------------------------------
def test_dropout_restatement_host_properties():
    """p = 0 is exactly 1; the keep rate of every site of every block lies within 5 sigma of 1 - p on the config's training batch
    (128 QM9 molecules); seeds that differ only in their high 32 bits give different masks; the multiplier is the float32 1 / (1 - p)."""
    import numpy as np
    from jodo_amd.models import load_dataset_info, get_node_dist
    from oracle import philox_ref as PR
    assert np.array_equal(PR.drop_mul(DROP_SEED, 9, 0.0, 1001), np.ones(1001, np.float32))
    z = PR.dropout_masks(DROP_SEED, 0.0, [3, 2], 2, 16, 4, 2)
    assert all(np.array_equal(v, np.ones_like(v)) for mol in z for blk in mol for v in blk.values())
    cfg = make_config('vpsde_qm9_uncond_jodo')
    hp = O.Hyper.from_config(cfg)
    torch.manual_seed(5)
    n_nodes = get_node_dist(load_dataset_info('qm9_with_h')).sample(int(cfg.training.batch_size)).tolist()
    Nn, R = sum(n_nodes), sum(n * n for n in n_nodes)
    assert R > 30000
    p = 0.1
    widths = {'A1': (Nn, hp.mlp_ratio * hp.nf), 'F2': (Nn, hp.nf), 'A3': (R, hp.mlp_ratio * hp.de), 'F4': (R, hp.de)}
    keep = np.float32(1) / (np.float32(1) - np.float32(p))
    for l in range(hp.n_layers):
        for site, (rows, w) in widths.items():
            m = PR.drop_mul(DROP_SEED, PR.drop_site(l, site), p, rows * w)
            assert set(np.unique(m).tolist()) == {0.0, float(keep)}
            kept = float((m != 0).mean())
            assert abs(kept - (1 - p)) < 5 * (p * (1 - p) / m.size) ** 0.5, (l, site, kept)
    lo = DROP_SEED & 0xFFFFFFFF
    a = PR.drop_mul(lo | (1 << 32), PR.drop_site(0, 'A1'), p, 4096)
    b = PR.drop_mul(lo | (2 << 32), PR.drop_site(0, 'A1'), p, 4096)
    c = PR.drop_mul(lo, PR.drop_site(0, 'A1'), p, 4096)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    # sites and layers are distinct streams
    assert not np.array_equal(PR.drop_mul(7, PR.drop_site(0, 'F2'), p, 4096), PR.drop_mul(7, PR.drop_site(0, 'F4'), p, 4096))
    assert not np.array_equal(PR.drop_mul(7, PR.drop_site(0, 'A1'), p, 4096), PR.drop_mul(7, PR.drop_site(1, 'A1'), p, 4096))

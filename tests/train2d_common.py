"""Shared by tests/test_train2d_emul.py (host emulation) and tests/test_train2d_gpu.py (device): the cases, their inputs, the
float64 / float32 autograd yardsticks through the dense oracle (computed once per case and never modified), and the tolerances.

Shapes — the smallest at which the training kernels can go wrong:
  ZINC  (nd = 10, ch = 2)  n_nodes = [1, 2, 3, 9, 33, 38]: a molecule without any edge (empty softmax), tiles straddling the 32-row wave
                           boundary, sum n^2 = 2 628 (no multiple of 32), several molecules with different modulation rows inside one
                           32-row strip, n = 33 (more than one 32-source chunk), n = 38 (the config's maximum)
  MOSES (nd = 7, ch = 3)   n_nodes = [2, 5, 27]
  ZINC model, chunk edges  n_nodes = [46, 45, 64, 1] ('zinc_chunks'): the per-molecule edge chunks of the two-level sums are
                           max(32, ceil(n^2 / 64)) rows long (dgt2d_train.hip jodo_train2d_create) — 34 rows for n = 46 (n^2 = 2 116, the
                           last chunk 8 rows), 32 for n = 45 (2 025, the last one 9), 64 for n = 64 (the widest molecule the engine
                           and the inference kernels take), one row for n = 1.  Beyond the config's own maximum of 38 atoms, where no
                           chunk is longer than 32 rows
Per-molecule noise levels throughout; trunk gain 1.5 and the fixtures' head gain so that no gradient vanishes.

Tolerances are the project's own: forward 2e-5 + 1e-4 |x| (the 2-D suite's fwd_close); recorded reference gradients 2e-4 relative;
every gradient against float64 autograd through the dense oracle rel_tol = 3e-4, widened to 16 x the float32-autograd distance
where that is larger (the rule of tests/test_train_gpu.py::_compare_grads, restated here)."""
import functools

import torch

import oracle2d as O2
import oracle2d_train as O2T
from helpers import make_config, make_model, masks

CFG = {'zinc': 'vpsde_zinc_2d_jodo', 'moses': 'vpsde_moses_2d_jodo', 'zinc_chunks': 'vpsde_zinc_2d_jodo'}
TRAIN_NODES = {'zinc': [1, 2, 3, 9, 33, 38], 'moses': [2, 5, 27], 'zinc_chunks': [46, 45, 64, 1]}
GAIN, HEAD_GAIN = 1.5, 8.0
ATOL, RTOL = 2e-5, 1e-4
GRAD_REL, GRAD_REF_REL, K32 = 3e-4, 2e-4, 16.0


def fwd_close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = ATOL + RTOL * want.abs()
    print('%s: max |err| %.3e, worst err / bound %.3f' % (what, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all()), "%s: max |err| %g, worst err / bound %g" % (what, err.max().item(), (err / bound).max().item())


def model_for(which, seed, device='cpu'):
    cfg = make_config(CFG[which])
    return cfg, make_model(cfg, seed, device, gain=GAIN, head_gain=HEAD_GAIN)


def random_case(which, seed=5, n_nodes=None):
    """(cfg, hp, n_nodes, nm, em, xh, ex, nl, cx, cex, d_x, d_e) on the CPU: symmetric masked inputs, per-molecule noise levels, output
    gradients that are neither symmetric nor masked (the kernels must mask and symmetrise)."""
    cfg = make_config(CFG[which])
    hp = O2.Hyper2D.from_config(cfg)
    n_nodes = list(TRAIN_NODES[which] if n_nodes is None else n_nodes)
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    g = torch.Generator().manual_seed(seed)
    sym = lambda t: (t + t.transpose(1, 2)) * em.reshape(B, N, N, 1)
    xh = torch.randn(B, N, hp.nd, generator=g) * nm
    ex = sym(torch.randn(B, N, N, hp.ch, generator=g))
    nl = torch.randn(B, generator=g) * 2
    cx = torch.randn(B, N, hp.nd, generator=g) * nm
    cex = sym(torch.randn(B, N, N, hp.ch, generator=g))
    d_x, d_e = torch.randn(B, N, hp.nd, generator=g), torch.randn(B, N, N, hp.ch, generator=g)
    return dict(cfg=cfg, hp=hp, n_nodes=n_nodes, nm=nm, em=em, xh=xh, ex=ex, nl=nl, cx=cx, cex=cex, d_x=d_x, d_e=d_e)


def oracle_grads(sd, hp, nm, em, xh, ex, cx, cex, nl, d_x, d_e, dtype=torch.float64, drop=None):
    """(pred, edge_pred, {name: d <d_out, outputs> / d parameter}) by autograd through the dense oracle (masked form when drop is given)."""
    sdg = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    c = lambda t: None if t is None else t.detach().cpu().to(dtype)
    if drop is None:
        px, pe = O2.forward_dense(sdg, hp, c(xh), nm, em, c(ex), c(cx), c(cex), c(nl))
    else:
        px, pe = O2T.forward_dense_drop(sdg, hp, c(xh), nm, em, c(ex), c(cx), c(cex), c(nl), drop=drop)
    ((px * c(d_x)).sum() + (pe * c(d_e)).sum()).backward()
    return px.detach(), pe.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sdg.items()}


@functools.lru_cache(maxsize=None)
def random_case_yardsticks(which, selfcond, model_seed=3, seed=5):
    """The case, its model's CPU state_dict and the float64 / float32 yardsticks: computed once, shared, left unchanged."""
    c = random_case(which, seed)
    _, model = model_for(which, model_seed)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cx, cex = (c['cx'], c['cex']) if selfcond else (None, None)
    args = (sd, c['hp'], c['nm'], c['em'], c['xh'], c['ex'], cx, cex, c['nl'], c['d_x'], c['d_e'])
    p64 = oracle_grads(*args, dtype=torch.float64)
    p32 = oracle_grads(*args, dtype=torch.float32)
    return c, sd, p64, p32


def compare_grads(named_grads, want, rel_tol=GRAD_REL, want32=None, k32=K32, only=None, what=''):
    """|got - want| <= rel_tol x max |want| per tensor, widened to k32 x the distance of FLOAT32 autograd through the same oracle from
    float64 where that is larger.  Prints the worst ratio err / (rel_tol x scale) and whether the widening was ever the active bound."""
    bad, worst, widened = [], 0.0, 0
    for k, g in named_grads:
        if only is not None and k not in only:
            continue
        w = want[k].double()
        scale, err = float(w.abs().max()), float((g.detach().cpu().double() - w).abs().max())
        e32 = float((want32[k].double() - w).abs().max()) if want32 is not None else 0.0
        base = rel_tol * max(scale, 1e-12)
        worst = max(worst, err / base)
        widened += int(k32 * e32 > base)
        if not err <= max(base, k32 * e32) + 1e-12:
            bad.append("%s: err %.3e scale %.3e (float32 autograd %.3e)" % (k, err, scale, e32))
    print("%s: worst gradient error / bound %.4f (rel_tol %.0e), widened bounds active on %d tensors" % (what, worst, rel_tol, widened))
    assert not bad, "%d parameter gradients differ:\n  %s" % (len(bad), "\n  ".join(bad[:40]))
    return worst


def assert_all_nonzero(want):
    dead = [k for k, v in want.items() if not (bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0)]
    assert not dead, "gradients vanish or are not finite in the yardstick: %s" % dead[:10]


def loss2d_from_outputs(cfg, pred, edge_pred, xh, edge_x, nm, em, alpha_t, sigma_t):
    """The data-prediction branch of the reference's 2-D loss (losses.py:256-281) on given predictions."""
    B = xh.shape[0]
    _, w_atom, w_edge = (float(w) for w in cfg.model.loss_weights.split(','))
    l_atom = torch.square(pred - xh).mean(-1).sum(-1)
    l_edge = torch.square(edge_x - edge_pred).mean(-1).reshape(B, -1).sum(-1)
    if cfg.training.reduce_mean:
        l_atom = l_atom / nm.squeeze(-1).sum(-1)
        l_edge = l_edge / (em.reshape(B, -1).sum(-1) + 1e-8)
    return (torch.sqrt(alpha_t / sigma_t) * (w_atom * l_atom + w_edge * l_edge)).mean()

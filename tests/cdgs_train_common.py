"""Shared by tests/test_cdgs_train_host.py (host emulation) and tests/test_cdgs_train_gpu.py (device): the cases of the CDGS training
path, their inputs, the float64 / float32 autograd yardsticks through the dense oracle (computed once per case and never modified), and
the tolerances, which are the project's own (helpers.close64 for the forward, train2d_common.compare_grads for the gradients).

Cases — the smallest at which the training kernels can go wrong (seeded deterministic_init_ weights, seed 7; output gradients that are
neither symmetric nor masked):
  mixed   QM9  [1, 2, 5, 17, 29, 9], N = 29   a molecule without any pair (empty softmax); n = N (no padding) beside n = 1 (28 padded
                                              columns); 63 atoms; 5 046 tile rows = 9 split-K slices of 512 + 438, no multiple of 32
  w12/w9  QM9  [9, 4, 7, 2] at N = 12 / 9     no molecule reaches the width at N = 12: the padded rows carry gradient
  geom    GEOM [3, 40, 1], N = 44             6 blocks, 254 parameters, readout width 85, n > 32
  b65     QM9  65 molecules, n = 1, 2, 3 ..   time-MLP rows across the 64-row strip of the GEMM
  single  QM9  one-atom molecules only        the yardstick's gradients of modules 2 - 5 are exactly zero, the engine's must be too"""
import functools

import torch

import oracle_cdgs as OC
import oracle_cdgs_train as OCT
from helpers import make_config
from jodo_amd.models import get_model_class, deterministic_init_
from jodo_amd.sampling import build_masks
from train2d_common import GRAD_REL, GRAD_REF_REL, K32, assert_all_nonzero, compare_grads  # noqa: F401  (re-exported)

CFG = {'qm9': 'vpsde_qm9_2d_cdgs', 'geom': 'vpsde_geom_2d_cdgs'}
CASES = {
    'mixed': ('qm9', [1, 2, 5, 17, 29, 9], 29),
    'w12': ('qm9', [9, 4, 7, 2], 12),
    'w9': ('qm9', [9, 4, 7, 2], 9),
    'geom': ('geom', [3, 40, 1], 44),
    'b65': ('qm9', [1 + i % 3 for i in range(65)], 3),
    'single': ('qm9', [1, 1, 1], 2),
}
MODEL_SEED = 7
# Conditioning of a gradient check through ReLU.  The block has two ReLUs on the gradient path (the GINE message relu(hs_j + he_ji) and the
# ReLU inside the GINE nn); a case evaluates up to 1.2 million of them on arguments of magnitude 1.  An argument within float32 rounding
# of zero (a few 1e-7 after the GroupNorm / projection chain before it) takes either branch in a float32 evaluation, and ONE such flip
# moves a handful of gradient entries by a whole upstream gradient value (measured with the inputs of seed 5: |argument| 4.5e-7 in
# block 1 of `mixed` and 6.7e-7 in block 1 of `geom`, one channel of d t_node.bias off by 14 x the bound, everything else inside it).
# That measures the kink, not the calculus, so the inputs are drawn at the first seed whose float64 evaluation keeps every
# gradient-carrying ReLU argument at least RELU_MARGIN = 5e-6 (about 40 float32 ulps at magnitude 1) from zero: conditioned_case below.
RELU_MARGIN = 5e-6


@functools.lru_cache(maxsize=None)
def model_for(which, seed=MODEL_SEED):
    """(cfg, CPU model in eval mode, CPU float32 state_dict): shared, never modified (tests that change weights build their own)."""
    cfg = make_config(CFG[which])
    model = deterministic_init_(get_model_class('CDGS')(cfg), seed=seed).eval()
    return cfg, model, {k: v.detach().clone() for k, v in model.state_dict().items()}


def fresh_model(which, seed=MODEL_SEED, device='cpu'):
    cfg = make_config(CFG[which])
    return cfg, deterministic_init_(get_model_class('CDGS')(cfg), seed=seed).to(device).eval()


PARTNER = {'w9': 'w12', 'w12': 'w9'}       # the same molecules and output gradients at two padded widths


def random_case(name, seed=5):
    if name == 'w12':                        # `w9` padded with zeros: nothing but the width differs
        c = random_case('w9', seed)
        N, pad = 12, 12 - c['N']
        c['nm'], c['em'] = build_masks(c['n_nodes'], N, 'cpu')
        for k in ('x', 'd_x'):
            c[k] = torch.nn.functional.pad(c[k], (0, 0, 0, pad)).contiguous()
        for k in ('ex', 'd_e'):
            c[k] = torch.nn.functional.pad(c[k], (0, 0, 0, pad, 0, pad)).contiguous()
        c['N'] = N
        return c
    which, n_nodes, N = CASES[name]
    cfg = make_config(CFG[which])
    g = torch.Generator().manual_seed(seed)
    B = len(n_nodes)
    nm, em = build_masks(list(n_nodes), N, 'cpu')
    x = torch.randn(B, N, cfg.data.atom_types, generator=g) * nm
    ex = torch.randn(B, N, N, cfg.model.edge_ch, generator=g)
    ex = (ex + ex.transpose(1, 2)) * em.reshape(B, N, N, 1)
    t = torch.rand(B, generator=g) * 0.999 + 1e-3
    d_x, d_e = torch.randn(B, N, cfg.data.atom_types, generator=g), torch.randn(B, N, N, cfg.model.edge_ch, generator=g)
    return dict(which=which, cfg=cfg, hp=OC.hparams(cfg), n_nodes=list(n_nodes), N=N, B=B, nm=nm, em=em, t=t, x=x, ex=ex, d_x=d_x, d_e=d_e)


def oracle_grads(sd, c, dtype=torch.float64, drop=None, d_x=None, d_e=None):
    """(atom, bond, {name: d <d_out, outputs> / d tensor}) by autograd through the dense oracle (the masked form when drop is given)."""
    sdg = {k: v.detach().cpu().to(dtype).clone().requires_grad_(not k.endswith('local_model.eps')) for k, v in sd.items()}
    if drop is None:
        px, pe = OC.forward(sdg, c['hp'], c['t'], c['x'], c['nm'], c['em'], c['ex'])
    else:
        px, pe = OCT.forward_drop(sdg, c['hp'], c['t'], c['x'], c['nm'], c['em'], c['ex'], drop=drop)
    d_x, d_e = (c['d_x'] if d_x is None else d_x), (c['d_e'] if d_e is None else d_e)
    ((px * d_x.to(dtype)).sum() + (pe * d_e.to(dtype)).sum()).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sdg.items() if v.requires_grad}
    return px.detach(), pe.detach(), grads


def relu_margin(c, sd, drop=None):
    """The smallest |argument| of a gradient-carrying ReLU (GINE message, GINE nn) in the float64 evaluation of the case."""
    sd64 = {k: v.detach().cpu().double() for k, v in sd.items()}
    margins = []
    with torch.no_grad():
        OCT.forward_drop(sd64, c['hp'], c['t'], c['x'], c['nm'], c['em'], c['ex'], drop=drop, margins=margins)
    return min(margins)


def conditioned_case(name, drop=None, first_seed=5):
    """random_case at the first input seed >= 5 whose ReLU arguments all keep RELU_MARGIN from zero in float64 (drop: None, or (p, seed)
    of the dropout masks).  Decided by the yardstick alone, never by the code under test."""
    for seed in range(first_seed, first_seed + 64):
        c = random_case(name, seed)
        _, _, sd = model_for(c['which'])
        hp = c['hp']
        masks = None if drop is None else OCT.drop_masks(drop[1], drop[0], c['B'], c['N'], hp.n_layers, hp.nf)
        m = relu_margin(c, sd, masks)
        if drop is None and name in PARTNER:
            m = min(m, relu_margin(random_case(PARTNER[name], seed), sd))
        if m > RELU_MARGIN:
            c['seed'], c['relu_margin'] = seed, m
            return c, sd, masks
    raise AssertionError("no input seed in %d .. %d keeps the ReLU arguments of case %s away from zero" % (first_seed, first_seed + 63, name))


@functools.lru_cache(maxsize=None)
def yardsticks(name):
    """The case and its float64 / float32 yardsticks (outputs and gradients): computed once, shared, left unchanged."""
    c, sd, _ = conditioned_case(name)
    return c, oracle_grads(sd, c, torch.float64), oracle_grads(sd, c, torch.float32)


@functools.lru_cache(maxsize=None)
def drop_yardsticks(name, p, drop_seed):
    c, sd, masks = conditioned_case(name, drop=(p, drop_seed))
    return c, oracle_grads(sd, c, torch.float64, drop=masks), oracle_grads(sd, c, torch.float32, drop=masks)


def param_names(model):
    """state_dict keys, and which of them are parameters (the GINE eps buffers are not)."""
    keys = list(model.state_dict().keys())
    return keys, [k for k in keys if not k.endswith('local_model.eps')]

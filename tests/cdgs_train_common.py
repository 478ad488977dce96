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
  single  QM9  one-atom molecules only        the yardstick's gradients of modules 2 - 5 are exactly zero, the engine's must be too
  wide    GEOM with n_layers = 1, [100, 65, 1], N = 100 (device only)   the first run of the engine above N = 44 and above 64: 30 000
                                              tile rows per tensor, which float64 autograd on a CPU affords at one block
  full    GEOM with n_layers = 1, [181, 2], N = 181 (device only, forward and kept activations only)   the config's own max_node
The two one-block cases draw a SPARSE adjacency (a path through every molecule plus one chord per four atoms, as molecules have; the
attention still walks every real pair): with half of all pairs adjacent, as the other cases draw them, N = 100 evaluates 1.8 million
GINE ReLU arguments and no input seed keeps them all RELU_MARGIN from zero.

kept_yardsticks / check_kept: the tensors the training forward keeps in its workspace (jodo_cdgs_train_debug_locate selectors 0 - 3: h and
e after every block, alpha and the xhat of norm2_edge of every block) against the oracle's per-block tensors under helpers.close64."""
import functools

import torch

import oracle_cdgs as OC
import oracle_cdgs_train as OCT
from helpers import make_config
from jodo_amd.models import get_model_class, deterministic_init_
from jodo_amd.sampling import build_masks
from train2d_common import GRAD_REL, GRAD_REF_REL, K32, assert_all_nonzero, compare_grads  # noqa: F401  (re-exported)

CFG = {'qm9': 'vpsde_qm9_2d_cdgs', 'geom': 'vpsde_geom_2d_cdgs'}
ONE_BLOCK = {'geom1': 'geom'}              # `which` -> the config it is, with model.n_layers = 1
CASES = {
    'wide': ('geom1', [100, 65, 1], 100),
    'full': ('geom1', [181, 2], 181),
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


def config_for(which):
    return make_config(CFG[ONE_BLOCK[which]], n_layers=1) if which in ONE_BLOCK else make_config(CFG[which])


@functools.lru_cache(maxsize=None)
def model_for(which, seed=MODEL_SEED):
    """(cfg, CPU model in eval mode, CPU float32 state_dict): shared, never modified (tests that change weights build their own)."""
    cfg = config_for(which)
    model = deterministic_init_(get_model_class('CDGS')(cfg), seed=seed).eval()
    return cfg, model, {k: v.detach().clone() for k, v in model.state_dict().items()}


def fresh_model(which, seed=MODEL_SEED, device='cpu'):
    cfg = config_for(which)
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
    cfg = config_for(which)
    g = torch.Generator().manual_seed(seed)
    B = len(n_nodes)
    nm, em = build_masks(list(n_nodes), N, 'cpu')
    x = torch.randn(B, N, cfg.data.atom_types, generator=g) * nm
    ex = torch.randn(B, N, N, cfg.model.edge_ch, generator=g)
    ex = (ex + ex.transpose(1, 2)) * em.reshape(B, N, N, 1)
    if which in ONE_BLOCK:                   # sparse adjacency (first channel >= 0): a path and one chord per four atoms
        r, c_ = torch.arange(N)[:, None], torch.arange(N)[None, :]
        bond = ((r - c_).abs() == 1) | (((r - c_).abs() == 7) & (torch.minimum(r, c_) % 4 == 0))
        ex[..., 0] = torch.where(bond[None], ex[..., 0].abs() + 0.1, -ex[..., 0].abs() - 0.1) * em.reshape(B, N, N)
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


# ---- the kept activations ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kept_yardsticks(name, p=0.0, drop_seed=0):
    """(case, {dtype: (atom, bond, states, taps)}) of random_case(name) through the no-grad oracle (masked form when p > 0), in float64
    and float32: computed once, shared, left unchanged."""
    c = random_case(name)
    _, _, sd = model_for(c['which'])
    hp = c['hp']
    out = {}
    for dtype in (torch.float64, torch.float32):
        masks = OCT.drop_masks(drop_seed, p, c['B'], c['N'], hp.n_layers, hp.nf, dtype=dtype) if p > 0 else None
        taps = []
        with torch.no_grad():
            px, pe, states = OCT.forward_drop({k: v.to(dtype) for k, v in sd.items()}, hp, c['t'], c['x'], c['nm'], c['em'], c['ex'], drop=masks,
                                              return_blocks=True, taps=taps)
        out[dtype] = (px, pe, states, taps)
    return c, out


def check_kept(fetch, c, yard, what=''):
    """fetch(selector, layer) -> flat float32 tensor (TrainEngineCDGS.debug_fetch after a training-mode forward).  Every block's selectors
    0 - 3 under helpers.close64; alpha off the real pairs, e off the real pairs and h on the padded rows (after a block) exactly 0."""
    from helpers import close64
    (_, _, st64, tp64), (_, _, st32, tp32) = yard[torch.float64], yard[torch.float32]
    B, N, L = c['B'], c['N'], c['hp'].n_layers
    dead_n, dead_e = (c['nm'].reshape(B, N) == 0), (c['em'].reshape(B, N, N) == 0)
    for l in range(L + 1):
        h, e = fetch(0, l).cpu().reshape(st64[l][0].shape), fetch(1, l).cpu().reshape(st64[l][1].shape)
        close64(h, st32[l][0], st64[l][0], '%s kept h %d' % (what, l))
        close64(e, st32[l][1], st64[l][1], '%s kept e %d' % (what, l))
        assert float(e[dead_e].abs().max() if bool(dead_e.any()) else 0.0) == 0.0, '%s: e %d is not exactly zero off the real pairs' % (what, l)
        if l > 0 and bool(dead_n.any()):
            assert float(h[dead_n].abs().max()) == 0.0, '%s: h %d is not exactly zero on the padded rows' % (what, l)
        if l < L:
            al, xh = fetch(2, l).cpu().reshape(tp64[l]['alpha'].shape), fetch(3, l).cpu().reshape(tp64[l]['xhat'].shape)
            close64(al, tp32[l]['alpha'], tp64[l]['alpha'], '%s kept alpha %d' % (what, l))
            close64(xh, tp32[l]['xhat'], tp64[l]['xhat'], '%s kept xhat %d' % (what, l))
            assert float(al[dead_e].abs().max() if bool(dead_e.any()) else 0.0) == 0.0, '%s: alpha %d is not exactly zero off the real pairs' % (what, l)

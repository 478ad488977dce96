"""Shared by tests/test_train_scale_gpu.py (device) and tests/test_train_emul.py (host emulation): the batches at which the 3-D training
backward changes form by SIZE, their inputs, and the float64 / float32 autograd yardsticks through the dense oracle (computed once per
case and never modified).

Everything runs the smallest configuration the module accepts — vpsde_geom_uncond_jodo at nf = 128, n_layers = 2 (De = 32: 31 Gaussians,
edge_ch 3), trunk gain 1.0, coord_scale 0.05, dropout off — on helpers.random_inputs(seed 5), first-step call (no self-conditioning
input: the top-level dist_layer then has zero gradient, the blocks' own dist_layers do not).

The switches (DESIGN.md 9a has the table), with R = sum n^2 edge rows:
  ABOVE_64K     [181, 181, 46, 5]     R = 67 663 (no multiple of 32): colsum's first level has n = 2 115 > 2 048 chunks for
                                      coord_norm.scale (second-level chunk c2 = 34 instead of 32), and nch = 2 115 chunk rows of the
                                      Gaussian layer's d means / d stds, whose colsum gains its second level (n = 67 > 64)
  GBF_BY_SIZE   [181, 181, 181, 181]  R = 131 044, nch = 4 096: the wave-per-chunk Gaussian backward is taken by size
  GBF_BELOW     [181, 181, 181, 180]  R = 130 683, nch = 4 084: it is not
  CHUNK_EDGES   [46, 45, 64, 1]       n^2 = 2 116 | 2 025 | 4 096 | 1: per-molecule edge chunks of 34 | 32 | 64 rows
  attention_nodes(16 383 | 16 384)    molecules of 3 .. 6 atoms on either side of the one-wave-per-atom attention switch

Output gradients: one random draw (seed 9) everywhere (`local` None), or the same draw confined to ONE molecule (`local` = its index).
Confined to a small molecule the float32 oracle sits within a few 1e-6 of float64 on every tensor, so no bound of the gradient rule is
widened and a lost tail, first chunk or whole level shows at full size."""
import functools

import torch

from oracle import dgt_oracle as O
from helpers import make_config, make_model, oracle_param_grads, random_inputs

CFG_NAME, OVER = 'vpsde_geom_uncond_jodo', dict(nf=128, n_layers=2)
ABOVE_64K = (181, 181, 46, 5)
GBF_BY_SIZE = (181, 181, 181, 181)
GBF_BELOW = (181, 181, 181, 180)
CHUNK_EDGES = (46, 45, 64, 1)
GRAD_REL, K32 = 3e-4, 16.0
# Passes confined to one molecule exist so that no bound is widened and a lost tail, first chunk or level shows at full size.  That can be
# asserted where the float32 yardstick supports it: on the 5-atom last molecule of ABOVE_64K float32 autograd is at most 2.5e-6 of scale
# from float64 on any tensor (16 x that is far under 3e-4) — there the widening must be active on NO tensor.  Confined to a 181-atom
# molecule float32 autograd is itself 3.0e-3 of scale from float64 on e_block_0's coord_norm.scale and above 3e-4 / 16 on 30 tensors
# (measured: ABOVE_64K, first molecule), and the kernels sit on the same noise (9.3 x the un-widened bound on that tensor, 0.94 x on
# e_block_0.dist_layer.means through the emulation build): such a pass follows the rule with its widening, and must leave un-widened the
# tensor that a lost chunk of colsum's one-column form moves at full size, the SECOND block's coord_norm.scale (float32 autograd 1e-6 of
# its scale).
UNWIDENED = {(ABOVE_64K, 3)}
SHARP = 'e_block_1.equi_update.coord_norm.scale'
# the tensors fed by the size-selected reductions; they must not vanish in a yardstick (the top-level dist_layer does, see above)
REDUCED = tuple('e_block_%d.%s' % (l, k) for l in range(2) for k in ('equi_update.coord_norm.scale', 'dist_layer.means.weight', 'dist_layer.stds.weight'))


def rows(n_nodes):
    return sum(n * n for n in n_nodes)


@functools.lru_cache(maxsize=None)
def model_and_hp():
    cfg = make_config(CFG_NAME, **OVER)
    return make_model(cfg, 3, 'cpu', gain=1.0, coord_scale=0.05), O.Hyper.from_config(cfg)


@functools.lru_cache(maxsize=None)
def batch(n_nodes):
    """(xh, ex, nl, nm, em, d_x, d_e) of the tuple n_nodes, on the CPU."""
    _, hp = model_and_hp()
    xh, ex, nl, ctx, nm, em = random_inputs(hp, list(n_nodes), seed=5)
    assert ctx is None
    g = torch.Generator().manual_seed(9)
    d_x, d_e = torch.randn(xh.shape, generator=g), torch.randn(ex.shape, generator=g)
    return xh, ex, nl, nm, em, d_x, d_e


def out_grads(n_nodes, local=None):
    """The output gradient of the case: everywhere, or on molecule `local` alone (neither symmetric nor masked inside it)."""
    d_x, d_e = batch(n_nodes)[5:]
    if local is None:
        return d_x, d_e
    m = torch.zeros(len(n_nodes))
    m[local] = 1.0
    return (d_x * m.view(-1, 1, 1)).contiguous(), (d_e * m.view(-1, 1, 1, 1)).contiguous()


@functools.lru_cache(maxsize=None)
def yardstick(n_nodes, local=None, dtype=torch.float64):
    """(pred, edge_pred, gradients) by autograd through the oracle in `dtype`: computed once per (case, pass, dtype), left unchanged."""
    model, hp = model_and_hp()
    xh, ex, nl, nm, em = batch(n_nodes)[:5]
    d_x, d_e = out_grads(n_nodes, local)
    return oracle_param_grads(model, hp, xh, nm, em, ex, None, None, nl, None, d_x, d_e, dtype=dtype)


def check_widening(n_nodes, local, widened, what=''):
    """What a pass confined to one molecule asserts of the widened bounds (see UNWIDENED above); nothing for a bulk pass."""
    if (n_nodes, local) in UNWIDENED:
        assert not widened, "%s: bounds widened in a pass confined to a small molecule: %s" % (what, widened[:10])
    elif local is not None:
        assert SHARP not in widened, "%s: the bound of %s is widened" % (what, SHARP)


def assert_reduced_nonzero(want, what=''):
    dead = [k for k in REDUCED if not (bool(torch.isfinite(want[k]).all()) and float(want[k].abs().max()) > 0)]
    assert not dead, "%s: the yardstick's gradient vanishes on %s" % (what, dead)


def attention_nodes(total, seed=11):
    """Molecules of 3 .. 6 atoms (softmax rows of 2 .. 5 sources) from a fixed seed, `total` atoms in all: the draw is cut where it would
    pass `total` and the last molecule resized to land on it (the last two re-split when the remainder alone would be under 3 atoms)."""
    g = torch.Generator().manual_seed(seed)
    draw = torch.randint(3, 7, (total // 3 + 1,), generator=g).tolist()
    out, cum = [], 0
    for n in draw:
        if cum + n > total:
            break
        out.append(n)
        cum += n
    rem = total - cum
    if 0 < rem < 3:
        rem += out.pop()                                       # 4 .. 8
        if rem > 6:
            out.append(rem // 2)
            rem -= rem // 2
    if rem:
        out.append(rem)
    assert sum(out) == total and min(out) >= 3 and max(out) <= 6
    return tuple(out)


def make_engine(n_nodes, device, lib=None, options=None, pool=None):
    """(engine, parameter names, parameters on `device`) for the case: TrainEngine driven directly, so that one forward serves several
    backwards.  lib: the host emulation build (tests/emul) instead of the product library."""
    import ctypes
    from jodo_amd.train import TrainEngine
    model, _ = model_and_hp()
    named = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    kw = dict(lib=lib, stream_ptr=lambda: ctypes.c_void_p(0)) if lib is not None else {}
    eng = TrainEngine(model._cfg(), list(n_nodes), max(n_nodes), named, device, pool=pool, options=options, **kw)
    params = [v.detach().float().contiguous().to(device) for v in model.state_dict().values()]
    return eng, [k for k, _ in named], params


def dw_group_launches(n_nodes):
    """How the fused backward's queued weight-gradient products fall into grouped launches (csrc/dgt_train.hip backward, lin_dw /
    flush_dw; csrc/train_gemm.hip gemm_dw_group) for a batch of the case's model: a restatement in integers, the plan from
    tests/test_train_gemm_split_gpu.py plan() (held against train_gemm.h by tests/test_train_gemm_plan.py).  Returns
    [(where, products queued at that flush_dw, launches they take, cut by 'table' | 'scratch' | None)]: a group is cut where its table
    holds GEMM_GROUP_MAX = 24 products, or where the next product's split-K partial tiles no longer fit the scratch (6 x the plan's)."""
    from test_train_gemm_split_gpu import plan
    model, _ = model_and_hp()
    dm = model.dims
    D, L, H, XH, r, nd, ch, cc = dm.D, dm.L, dm.H, dm.XH, dm.r, dm.nd, dm.ch, dm.cond_ch
    De, T, C = D // 4, 4 * D, D // H
    QK = (H - XH) * ((H * C) // (H - XH))
    cn, ce = 2 * D // L, 2 * De // L
    catn, cate, F3, Mtot = D + L * cn, De + L * ce, 2 * QK + D, 2 + L * (6 * D + 6 * De + 2 * D + 2)
    Nn, R, B = sum(n_nodes), rows(n_nodes), len(n_nodes)
    # (M, N, K) of dW[M, N] += dY[K, M]^T X[K, N], in queue order, per flush_dw
    block_a = [(cn, D, Nn), (ce, De, R), (3, D, R), (D, D, R), (D, D, Nn), (D, D, Nn), (D, De, R), (D, De, R), (De, r * De, R), (r * De, De, R),
               (De, D, Nn), (D, r * D, Nn), (r * D, D, Nn)]
    block_b = [(D, De, R), (QK, De, R), (F3, D, Nn), (De, De, R), (De, De, R)]
    flushes = [('node head', [(nd, D // 2, Nn), (D // 2, D, Nn), (D, catn, Nn)]),
               ('edge-exist head', [(1, De // 2, R), (De // 2, De, R), (De, cate, R)]),
               ('edge-type head', [(ch - 1, De // 2, R), (De // 2, De, R), (De, cate, R)])]
    for l in reversed(range(L)):
        flushes += [('block %d, up to the attention' % l, block_a), ('block %d, from the attention' % l, block_b)]
    flushes += [('embeddings', [(D, 2 * nd, Nn), (De, 2 * ch + De, R)]), ('modulation projections', [(Mtot, T, B)]),
                ('time / context MLPs', ([(T, cc * D, B), (D, D, B * cc), (D, 1, B * cc)] if cc else []) + [(T, T, B), (T, 17, B)])]
    plan_floats = min(32 << 20, ((max(R, Nn) + 1023) // 1024 + 1) * D * (2 * D + 2 * De))
    ws_floats, out = 6 * plan_floats, []
    for where, jobs in flushes:
        launches, in_group, used, cut = 1, 0, 0, None
        for M, N, K in jobs:
            nsplit = plan(1, M, N, K, True, plan_floats)[0]
            need = nsplit * (M * N + M) if nsplit > 1 else 0
            if in_group == 24 or used + need > ws_floats:
                cut = 'table' if in_group == 24 else 'scratch'
                launches, in_group, used = launches + 1, 0, 0
            used += (need + 63) // 64 * 64
            in_group += 1
        out.append((where, len(jobs), launches, cut))
    return out

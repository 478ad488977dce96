"""The opt-in split-bf16 pair update of the CONDITIONAL model (cond_DGT_concat at nf 256; csrc/dgt_kernels_split_cond.h): the un-folded,
pair-symmetric update with every projection in the three-term bf16 form, reached through model.split_bf16 = True + pin_paths().

CPU: the conditional weight tape is the kernel's consumption order.  GPU: the split path runs (every plan of a call carries the tape),
stays within the project's forward tolerance of the exact path and of the float64 oracle (tests/helpers.py: 2e-5 + 1e-4 |x|, K64 = 4 — no
tolerance of its own), reproduces the reference's recorded conditional outputs and DPM-solver trajectories, and follows weight updates."""
import ctypes

import numpy as np
import pytest
import torch

from jodo_amd import capi, configs
from jodo_amd.models import get_model_class, deterministic_init_
from oracle import dgt_oracle as O

from forms_common import assert_pinned_call
from helpers import K64, close64, load_fixture, make_config, make_model, masks, oracle_32_64, random_inputs, state_dict_cpu

DEV = 'cuda:0'
STEP = 3 * 64 * 8                                                # uint16 per K16 step: hi | mid | lo x 64 lanes x 8


def _pack(W):
    n_out, n_in = W.shape
    s = np.zeros(n_out * n_in * 3, dtype=np.uint16)
    Wc = np.ascontiguousarray(W, dtype=np.float32)
    capi.check(capi.lib().jodo_debug_pack_split(Wc.ctypes.data_as(ctypes.c_void_p), n_out, n_in, None, s.ctypes.data_as(ctypes.c_void_p)), 'pack_split')
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: tape layout
@pytest.mark.parametrize("over", [{}, dict(cond_ch=2), dict(mlp_ratio=4)])
def test_conditional_split_tape_is_the_consumption_order_of_the_unfolded_pair_update(over):
    """jodo_dgt_pack_split_cond_host: per block [for every hidden chunk c: ff_linear3 output blocks 2c, 2c + 1 | ff_linear4 output blocks,
    steps 4c .. 4c + 3] [readout] [input_lin's e and distance columns, 8 blocks x 8 steps] [coord_mlp.0, 8 blocks x 16 steps] as K16 steps
    of 3 KiB — slice by slice against the generic split packing of the same matrices (jodo_debug_pack_split, natural maps)."""
    cfg = make_config('vpsde_qm9_cond_jodo', **over)
    model = deterministic_init_(get_model_class('cond_DGT_concat')(cfg), seed=3)
    sd = model.state_dict()
    D, De, r, L = 256, 64, cfg.model.mlp_ratio, cfg.model.n_layers
    NCH, NSE, NE, ND = r * De // 64, De // 16, De // 32, D // 32
    steps = NCH * (2 * NSE + NE * 4) + NSE + ND * (2 * De // 16) + ND * (D // 16)
    assert steps == (228 if r == 2 else 260) and steps % 4 == 0          # whole four-step chunks of the kernel's ring
    total, pair_b = ctypes.c_size_t(), ctypes.c_size_t()
    capi.check(capi.lib().jodo_dgt_split_cond_size(ctypes.byref(model._cfg()), ctypes.byref(total), ctypes.byref(pair_b)), 'split_cond_size')
    assert pair_b.value == steps * 3072 and total.value == steps * 3072 * L
    tape = capi.pack_split_cond_tape(model._cfg(), sd).numpy().view(np.uint16)
    assert tape.size * 2 == total.value
    for l in (0, L - 1):
        blk = tape[l * steps * STEP:(l + 1) * steps * STEP].reshape(steps, STEP)
        s3 = _pack(sd['e_block_%d.ff_linear3.weight' % l].numpy()).reshape(r * De // 32, NSE, STEP)
        s4 = _pack(sd['e_block_%d.ff_linear4.weight' % l].numpy()).reshape(NE, r * De // 16, STEP)
        at = 0
        for c in range(NCH):
            for b2 in range(2):
                assert np.array_equal(blk[at:at + NSE], s3[2 * c + b2]); at += NSE
            for ob in range(NE):
                assert np.array_equal(blk[at:at + 4], s4[ob, 4 * c:4 * c + 4]); at += 4
        # readout: edge_l [2 De / L, De], rows padded to one 32-row block
        wro = np.zeros((32, De), dtype=np.float32)
        w = sd['edge_%d.weight' % l].numpy()
        wro[:w.shape[0]] = w
        assert np.array_equal(blk[at:at + NSE], _pack(wro).reshape(NSE, STEP)); at += NSE
        # input_lin [D, 2 D + De + De] = h_row | h_col | e | G: the e and distance columns, whole output blocks in order
        win = sd['e_block_%d.equi_update.input_lin.weight' % l].numpy()
        assert win.shape == (D, 2 * D + 2 * De)
        sin = _pack(win[:, 2 * D:]).reshape(ND * 8, STEP)
        assert np.array_equal(blk[at:at + ND * 8], sin); at += ND * 8
        s0 = _pack(sd['e_block_%d.equi_update.coord_mlp.0.weight' % l].numpy()).reshape(ND * 16, STEP)
        assert np.array_equal(blk[at:at + ND * 16], s0); at += ND * 16
        assert at == steps


def test_conditional_split_tape_refuses_other_configurations_by_name():
    uncond = get_model_class('DGT_concat')(configs.get('vpsde_qm9_uncond_jodo'))
    with pytest.raises(capi.JodoHipError, match='nf = 256 conditional'):
        capi.pack_split_cond_tape(uncond._cfg(), {})
    c384 = make_config('vpsde_qm9_cond_jodo', nf=384)
    with pytest.raises(capi.JodoHipError, match='nf = 256 conditional'):
        capi.pack_split_cond_tape(get_model_class('cond_DGT_concat')(c384)._cfg(), {})
    total, pair_b = ctypes.c_size_t(), ctypes.c_size_t()
    assert capi.lib().jodo_dgt_split_cond_size(ctypes.byref(uncond._cfg()), ctypes.byref(total), ctypes.byref(pair_b)) != 0
    # and the unconditional tape keeps refusing the conditional model
    with pytest.raises(capi.JodoHipError, match='unconditional'):
        capi.pack_split_tape(get_model_class('cond_DGT_concat')(configs.get('vpsde_qm9_cond_jodo'))._cfg(), {})


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
def _split_ran(model):
    plans = model._last_plans
    assert plans and all('split_tape' in p for p in plans), "the conditional split kernel did not take over (split_bf16 ignored)"


def _run(model, xh, ex, nl, ctx, nm, em, cx=None, cex=None):
    d = lambda x: None if x is None else x.to(DEV)
    with torch.no_grad():
        o = model(d(nl), d(xh), d(nm), d(em), edge_x=d(ex), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(nl), context=d(ctx))
    torch.cuda.synchronize()
    return o[0].cpu(), o[1].cpu()


SEVERAL = [3, 9, 17, 29, 12, 5, 1, 2, 28, 29, 29, 18, 7] * 3      # n = 1, 2, several strips, idle waves in the last workgroups


@pytest.mark.gpu
@pytest.mark.parametrize("over,n_nodes,uniform", [
    ({}, SEVERAL, True),
    (dict(cond_ch=2), SEVERAL, True),
    (dict(mlp_ratio=4), [29, 1, 2, 18, 7, 23, 11], True),
    (dict(kernel_layout='wide'), [29, 1, 2, 18, 7, 23, 11], True),
    ({}, SEVERAL, False),                                          # per-molecule noise levels: no shared row anywhere
], ids=['qm9cond', 'cond_ch2', 'mlp_ratio4', 'wide', 'per_molecule_noise'])
def test_conditional_split_pair_update_against_the_default_path_and_float64(over, n_nodes, uniform):
    """First evaluation, self-conditioned evaluation, pin_paths(), both again under the pin, split_bf16 False and True.  (a) the split
    kernel ran and its outputs differ from the exact path's, (b) max |split - exact| <= 2e-5 + 1e-4 max |exact|, (c) both paths pass
    close64 against the float64 oracle at K64 with per-molecule context, (d) no NaN guard, (e) e is exactly symmetric."""
    cfg = make_config('vpsde_qm9_cond_jodo', **over)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=23)
    if uniform:
        nl = torch.full_like(nl, 0.3)
    assert ctx is not None and ctx.shape == (len(n_nodes), hp.cond_ch)
    nmd, emd = nm.to(DEV), em.to(DEV)                              # one pair of mask tensors: the plan (and its pins) is keyed by them
    outs = {}
    for split in (False, True):
        model = make_model(cfg, 13, DEV)
        model.split_bf16 = split
        first = _run(model, xh, ex, nl, ctx, nmd, emd)
        _run(model, xh, ex, nl, ctx, nmd, emd, first[0], first[1])
        model.pin_paths()
        assert model._last_plan.get('pinned') and (('split_tape' in model._last_plan) == split)
        pinned = list(model._last_plans)
        o2 = _run(model, xh, ex, nl, ctx, nmd, emd, first[0], first[1])
        assert_pinned_call(model, pinned)                          # AFTER the call: it ran on the plan that was pinned
        o1 = _run(model, xh, ex, nl, ctx, nmd, emd)
        assert_pinned_call(model, pinned)
        if split:
            _split_ran(model)
        assert model.take_nan_count() == 0
        outs[split] = (o1, o2)
        if not split:
            sd = state_dict_cpu(model)
    for k in (0, 1):
        for j in (0, 1):
            a, b = outs[True][k][j], outs[False][k][j]
            diff = float((a - b).abs().max())
            print('conditional split vs exact, evaluation %d %s: max |diff| %.3e (max |exact| %.3f)' % (k + 1, 'nodes' if j == 0 else 'edges', diff, float(b.abs().max())))
            assert not torch.equal(a, b), "the split kernel did not run"
            assert diff <= 2e-5 + 1e-4 * float(b.abs().max()), diff
        for split in (False, True):
            e = outs[split][k][1]
            assert torch.equal(e, e.transpose(1, 2))
    r1 = oracle_32_64(sd, hp, xh, nm, em, ex, None, None, nl, ctx)
    r2 = oracle_32_64(sd, hp, xh, nm, em, ex, outs[False][0][0], outs[False][0][1], nl, ctx)
    for step, (r32, r64) in ((0, r1), (1, r2)):
        for split in (False, True):
            close64(outs[split][step][0], r32[0], r64[0], 'cond split_bf16=%s step %d nodes' % (split, step + 1), k=K64)
            close64(outs[split][step][1], r32[1], r64[1], 'cond split_bf16=%s step %d edges' % (split, step + 1), k=K64)


def _close(got, want, atol=2e-5, rtol=1e-4):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    assert bool((err <= atol + rtol * want.abs()).all()), "max err %.3e (bound %.1e + %.0e*|x|)" % (err.max().item(), atol, rtol)


@pytest.mark.gpu
def test_reference_conditional_fixture_through_the_split_path():
    """fwd_cond.npz (outputs the reference itself recorded): the second call repeated under pin_paths() with split_bf16 on, at the
    fixture test's 2e-5 + 1e-4 |x|."""
    fx = load_fixture('fwd_cond.npz')
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV)
    model.split_bf16 = True
    nm, em = masks(fx['n_nodes'].tolist())
    t = lambda k: torch.from_numpy(fx[k])
    args = (t('xh'), t('edge_x'), t('noise_level'), t('context'), nm.to(DEV), em.to(DEV))
    o1 = _run(model, *args)
    _close(o1[0], t('out1_x')); _close(o1[1], t('out1_e'))
    _run(model, *args, t('out1_x'), t('out1_e'))
    model.pin_paths()
    pinned = list(model._last_plans)
    o2 = _run(model, *args, t('out1_x'), t('out1_e'))
    assert_pinned_call(model, pinned)                             # AFTER the call: it ran on the plan that was pinned
    _split_ran(model)
    _close(o2[0], t('out2_x')); _close(o2[1], t('out2_e'))
    o1p = _run(model, *args)                                      # and the first call under the pin
    assert_pinned_call(model, pinned)
    _close(o1p[0], t('out1_x')); _close(o1p[1], t('out1_e'))
    assert model.take_nan_count() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fname", ['traj_cond_dpm4.npz', 'traj_cond_dpm_multi8.npz', 'traj_cond_dpm_single3.npz', 'traj_cond_dpm_single1.npz'])
def test_dpm_solver_trajectory_through_the_split_path(fname):
    """The reference's recorded conditional DPM-solver trajectories with model.split_bf16 = True, at that test's atol 1e-3."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.mix_dpm_solver import DPM_Solver_hybrid
    fx = load_fixture(fname)
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.sampling.steps = int(fx['nfe'])
    cfg.sampling.method = 'fast'
    cfg.sampling.dpm_solver_method = str(fx['method'])
    cfg.sampling.dpm_solver_order = int(fx['order'])
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    model.split_bf16 = True
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    pn = torch.from_numpy(fx['pos_noise']).to(DEV)
    solver = DPM_Solver_hybrid(NoiseScheduleVP(cfg.sde.schedule), cfg, noise_fn=lambda i, kind, like: pn[i])
    x, ex = solver.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV),
                            torch.from_numpy(fx['context']).to(DEV))
    _split_ran(model)
    _close(x, torch.from_numpy(fx['x']), atol=1e-3, rtol=0)
    _close(ex, torch.from_numpy(fx['edge_x']), atol=1e-3, rtol=0)
    assert model.take_nan_count() == 0


@pytest.mark.gpu
def test_conditional_split_on_a_real_batch():
    """qm9_second_half, B = 1250 (6 295 pair items: six full rounds of the chip and a remainder), one noise level, per-molecule context:
    pinned split outputs finite, symmetric, zero on padding; 24 whole molecules spread over the size range (largest and smallest included)
    re-evaluated by the float64 oracle under close64, K64 = 4 (outputs are batch-independent)."""
    from jodo_amd.models import get_node_dist, load_dataset_info
    cfg = make_config('vpsde_qm9_cond_jodo')
    hp = O.Hyper.from_config(cfg)
    torch.manual_seed(cfg.seed)
    n_nodes = get_node_dist(load_dataset_info('qm9_second_half')).sample(1250).tolist()
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=41)
    nl = torch.full_like(nl, 0.3)
    model = make_model(cfg, 13, DEV)
    model.split_bf16 = True
    nmd, emd = nm.to(DEV), em.to(DEV)
    first = _run(model, xh, ex, nl, ctx, nmd, emd)
    _run(model, xh, ex, nl, ctx, nmd, emd, first[0], first[1])
    model.pin_paths()
    pinned = list(model._last_plans)
    o2 = _run(model, xh, ex, nl, ctx, nmd, emd, first[0], first[1])
    assert_pinned_call(model, pinned)                             # AFTER each call: it ran on the plan that was pinned
    o1 = _run(model, xh, ex, nl, ctx, nmd, emd)
    assert_pinned_call(model, pinned)
    _split_ran(model)
    assert model._last_plan.get('pinned')
    assert model.take_nan_count() == 0
    B, N = nm.shape[0], nm.shape[1]
    for x, e in (o1, o2):
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(e).all())
        assert torch.equal(e, e.transpose(1, 2))
        assert not bool((x * (1 - nm)).any()) and not bool((e * (1 - em.reshape(B, N, N, 1))).any())
    order = sorted(range(B), key=lambda b: (n_nodes[b], b))
    pick = sorted({order[round(i * (B - 1) / 23)] for i in range(24)})      # spread over the sizes; order[0] = smallest, order[-1] = largest
    assert n_nodes[order[0]] == min(n_nodes) and n_nodes[order[-1]] == max(n_nodes) and order[0] in pick and order[-1] in pick
    idx = torch.tensor(pick)
    ns = [n_nodes[b] for b in pick]
    Ns = max(ns)
    nms, ems = masks(ns)
    cn = lambda t: t[idx][:, :Ns]
    ce = lambda t: t[idx][:, :Ns, :Ns]
    sd = state_dict_cpu(model)
    r1 = oracle_32_64(sd, hp, cn(xh), nms, ems, ce(ex), None, None, nl[idx], ctx[idx])
    r2 = oracle_32_64(sd, hp, cn(xh), nms, ems, ce(ex), cn(first[0]), ce(first[1]), nl[idx], ctx[idx])
    for step, got, (r32, r64) in ((1, o1, r1), (2, o2, r2)):
        close64(cn(got[0]), r32[0], r64[0], 'cond split B=1250 sub-batch step %d nodes' % step, k=K64)
        close64(ce(got[1]), r32[1], r64[1], 'cond split B=1250 sub-batch step %d edges' % step, k=K64)


# ---- the tape follows the weights (the pattern of tests/test_weight_coherence_gpu.py, path cond-s1, with split on) ----
COND_N = [12, 29, 3, 17, 1, 8, 22, 5, 9, 14]


def _build(cfg, sd, streams):
    model = get_model_class(cfg.model.name)(cfg)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    model.split_bf16, model.n_streams = True, streams
    return model


def _settle(model, inp, nm, em, unpin=True):
    """First evaluation, self-conditioned evaluation, pin_paths(), the self-conditioned evaluation again under the pins, unpin."""
    xh, ex, nl, ctx = inp

    def ev(cx, cex):
        with torch.no_grad():
            return model(nl, xh, nm, em, edge_x=ex, cond_x=cx, cond_edge_x=cex, noise_level=nl, context=ctx)

    o1 = ev(None, None)
    o2 = ev(*o1)
    model.pin_paths()
    pinned = list(model._last_plans)
    o3 = ev(*o1)
    assert_pinned_call(model, pinned)                             # AFTER the call: it ran on the plan(s) that were pinned
    _split_ran(model)
    assert model.take_nan_count() == 0
    if unpin:
        model.unpin_paths()
    torch.cuda.synchronize()
    return [t.cpu() for o in (o1, o2, o3) for t in o]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [1, 2])
def test_conditional_split_tape_follows_the_weights(streams):
    """W -> W' through (1) `.data` writes + invalidate_packed_weights(), (2) an in-place versioned update while the plans stay pinned,
    (3) load_state_dict: each time the split outputs are bit-equal to a freshly built model's on W' and differ from those on W."""
    cfg = make_config('vpsde_qm9_cond_jodo')
    hp = O.Hyper.from_config(cfg)
    W = state_dict_cpu(make_model(cfg, 11, 'cpu', coord_scale=0.05))
    Wp = state_dict_cpu(make_model(cfg, 12, 'cpu', gain=1.2, coord_scale=0.05))
    xh, ex, nl, ctx, nm, em = random_inputs(hp, COND_N, seed=5)
    nl = torch.full_like(nl, 0.3)
    inp = tuple(t.to(DEV) for t in (xh, ex, nl, ctx))
    nm, em = nm.to(DEV), em.to(DEV)
    want = _settle(_build(cfg, Wp, streams), inp, nm, em)
    r32, r64 = oracle_32_64(Wp, hp, xh, nm, em, ex, want[0], want[1], nl, ctx)        # once: both models do not share a bug
    close64(want[4], r32[0], r64[0], "cond split fresh(W') pinned self-conditioned nodes, streams %d" % streams, k=K64)
    close64(want[5], r32[1], r64[1], "cond split fresh(W') pinned self-conditioned edges, streams %d" % streams, k=K64)

    def fresh_on_W():
        model = _build(cfg, W, streams)
        a = _settle(model, inp, nm, em)
        assert len(model._last_plans) == streams
        assert all(not torch.equal(x, y) for x, y in zip(a, want)), "the two weight sets give the same outputs: the test is vacuous"
        return model

    # (1) .data writes + invalidate
    model = fresh_on_W()
    for n, p in model.named_parameters():
        p.data.copy_(Wp[n].to(DEV))
    model.invalidate_packed_weights()
    assert _same(_settle(model, inp, nm, em), want), "after .data writes + invalidate the split tape (or the blob) is stale"
    # (2) versioned in-place update under pinned plans: the next call reads the new tape on every sub-batch plan
    model = _build(cfg, W, streams)
    _settle(model, inp, nm, em, unpin=False)
    assert all(p.get('pinned') for p in model._last_plans) and len(model._last_plans) == streams
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(Wp[n].to(DEV))
        got = model(inp[2], inp[0], nm, em, edge_x=inp[1], cond_x=want[0].to(DEV), cond_edge_x=want[1].to(DEV), noise_level=inp[2], context=inp[3])
    _split_ran(model)
    assert model.take_nan_count() == 0
    assert torch.equal(got[0].cpu(), want[4]) and torch.equal(got[1].cpu(), want[5]), "a pinned plan kept the old conditional split tape"
    # (3) load_state_dict
    model = fresh_on_W()
    model.load_state_dict(Wp)
    assert _same(_settle(model, inp, nm, em), want), "after load_state_dict the split tape (or the blob) is stale"

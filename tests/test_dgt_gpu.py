"""GPU parity tests proper: the HIP path (through the C ABI in libjodo_hip.so, via the registered
DGT_concat / cond_DGT_concat modules) against (a) fixtures produced by the real reference and (b) the
CPU oracle on fresh seeded inputs, plus the size-independent properties the reference satisfies
(SURVEY.md §4): rotation equivariance/invariance, exact symmetry, exact zeros on padding, batch
independence.  Tolerances: single forward atol 2e-5 + rtol 1e-4; K-step trajectory
atol 1e-3 with bit-exact discrete decodes where the reference's decision margin exceeds 1e-3.
"""
import numpy as np
import pytest
import torch

from oracle import dgt_oracle as O

from forms_common import DeviceBatch, assert_pinned_call
from helpers import (check_decodes, close64, debug_fetch, load_fixture, make_config, make_model, masks, oracle_32_64, random_inputs,
                     reference_blocks_dense, state_dict_cpu, K64, K64_HARD, K64_ROT_BIG, k64_for)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def close(got, want, atol=2e-5, rtol=1e-4):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    assert bool((err <= bound).all()), "max err %.3e (bound %.1e + %.0e*|x|)" % (err.max().item(), atol, rtol)


def check64(got, sd, hp, xh, nm, em, ex, cx, cex, nl, ctx=None, what='', k=K64):
    """HIP outputs against the float64 oracle on the same inputs, at the forward tolerance (helpers.close64: the stated
    2e-5 + 1e-4 |x|, widened only where the float32 oracle itself is further than that from float64).  Returns the float32
    oracle's outputs (self-conditioning inputs of a following call)."""
    r32, r64 = oracle_32_64(sd, hp, xh, nm, em, ex, cx, cex, nl, ctx)
    close64(got[0], r32[0], r64[0], what + ' nodes', k=k)
    close64(got[1], r32[1], r64[1], what + ' edges', k=k)
    return r32


def run(model, xh, ex, nl, nm, em, cx=None, cex=None, ctx=None):
    d = lambda x: None if x is None else x.to(DEV)
    with torch.no_grad():
        out = model(d(nl), d(xh), d(nm), d(em), edge_x=d(ex), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(nl),
                    context=d(ctx))
    torch.cuda.synchronize()
    return out[0].cpu(), out[1].cpu()


# layout 'wide' = the width-generic kernel set (csrc/dgt_kernels_wide.h); it is the only set at nf = 384 and
# is pinned at nf = 256 against the same reference fixtures as the tuned kernels
@pytest.mark.parametrize("fname,layout", [("fwd_qm9.npz", "auto"), ("fwd_geom.npz", "auto"), ("fwd_cond.npz", "auto"),
                                          ("fwd_geom384.npz", "auto"),
                                          # n = 181 (GEOM maximum), 140, 100: strips spanning many work-item parts,
                                          # circulant pair walks of up to 90 offsets
                                          ("fwd_geom_big.npz", "auto"), ("fwd_geom_big.npz", "wide"),
                                          ("fwd_geom384_big.npz", "auto"),
                                          ("fwd_qm9.npz", "wide"), ("fwd_geom.npz", "wide"), ("fwd_cond.npz", "wide"),
                                          # BASELINE configs[2] as worded: GEOM nf 256 with 8 layers (r 4, nd 17, ch 3)
                                          ("fwd_geom_l8.npz", "auto"), ("fwd_geom_l8.npz", "wide"),
                                          # the README's GEOM Base model (README.md:150): nf 128, 6 layers, n up to 131
                                          ("fwd_geom_base.npz", "auto")])
def test_hip_matches_reference_fixture(fname, layout):
    fx = load_fixture(fname)
    over = dict(kernel_layout=layout)
    if 'nf' in fx:
        over['nf'] = int(fx['nf'])
    if 'n_layers' in fx:
        over['n_layers'] = int(fx['n_layers'])
    cfg = make_config(str(fx['cfg_name']), **over)
    model = make_model(cfg, int(fx['seed']), DEV)
    hp = O.Hyper.from_config(cfg)
    nm, em = masks(fx['n_nodes'].tolist())
    t = lambda k: torch.from_numpy(fx[k])
    ctx = t('context') if hp.cond_ch else None
    o1 = run(model, t('xh'), t('edge_x'), t('noise_level'), nm, em, None, None, ctx)
    close(o1[0], t('out1_x'))
    close(o1[1], t('out1_e'))
    o2 = run(model, t('xh'), t('edge_x'), t('noise_level'), nm, em, t('out1_x'), t('out1_e'), ctx)
    close(o2[0], t('out2_x'))
    close(o2[1], t('out2_e'))
    assert model.last_flags.cpu().tolist()[0] == 0          # NaN guard did not fire


@pytest.mark.parametrize("cfg_name,n_nodes,gain,chunk,over", [
    ('vpsde_qm9_uncond_jodo', [29, 1, 2, 18, 18, 7, 23], 1.0, 0, {}),
    ('vpsde_qm9_uncond_jodo', [5] * 20 + [19] * 14, 1.5, 3, {}),      # multi-strip, odd chunking, larger activations
    ('vpsde_geom_uncond_jodo', [70, 33, 12], 1.5, 16, {}),
    ('vpsde_qm9_cond_jodo', [9, 9, 14], 1.0, 5, {}),
    ('vpsde_geom_uncond_jodo', [70, 33, 12, 1, 2], 1.5, 0, dict(nf=384)),               # BASELINE config 4 width
    ('vpsde_geom_uncond_jodo', [19] * 10 + [6] * 12, 1.0, 5, dict(nf=384, n_layers=8, mlp_ratio=2)),
    ('vpsde_qm9_cond_jodo', [9, 9, 14], 1.0, 5, dict(nf=384)),
    ('vpsde_qm9_uncond_jodo', [29, 1, 2, 18, 18, 7, 23], 1.5, 3, dict(kernel_layout='wide')),
    ('vpsde_geom_uncond_jodo', [70, 33, 12, 1, 2], 1.5, 0, dict(n_layers=8)),             # BASELINE configs[2] as worded
])
def test_hip_matches_oracle(cfg_name, n_nodes, gain, chunk, over):
    cfg = make_config(cfg_name, **over)
    model = make_model(cfg, 5, DEV, gain=gain, coord_scale=0.05)
    model.max_chunk = chunk
    hp = O.Hyper.from_config(cfg)
    sd = state_dict_cpu(model)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=len(n_nodes))
    o1 = run(model, xh, ex, nl, nm, em, None, None, ctx)
    r1 = check64(o1, sd, hp, xh, nm, em, ex, None, None, nl, ctx, 'first step')
    o2 = run(model, xh, ex, nl, nm, em, r1[0], r1[1], ctx)
    check64(o2, sd, hp, xh, nm, em, ex, r1[0], r1[1], nl, ctx, 'self-conditioned')


def test_attention_kernel_variants_agree():
    """The nf = 256 pair attention kernel exists in four weight-residency / hand-over variants (JODO_OPT_ATTN_VARIANT,
    dgt_kernels_attn.h): same arithmetic in the same order, so bit-equal outputs, and all match the oracle."""
    cfg = make_config('vpsde_qm9_uncond_jodo')
    hp = O.Hyper.from_config(cfg)
    n_nodes = [29, 1, 2, 18, 18, 7, 23, 12, 12, 9] * 4
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=31)
    outs = []
    for var in (0, 1, 2, 3):
        model = make_model(cfg, 5, DEV, gain=1.5, coord_scale=0.05)
        model.plan_options = {3: var}
        o1 = run(model, xh, ex, nl, nm, em)
        outs.append(run(model, xh, ex, nl, nm, em, o1[0], o1[1]))
    sd = state_dict_cpu(model)
    check64(outs[0], sd, hp, xh, nm, em, ex, o1[0], o1[1], nl, None, 'variant 0, self-conditioned on its own first step')
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


@pytest.mark.parametrize("cfg_name,n_nodes,over,uniform", [
    ('vpsde_qm9_uncond_jodo', [29, 1, 2, 18, 18, 7, 23, 12, 12, 9] * 7, {}, True),        # 434 pair items: two waves under option 2; folded + rotated
    ('vpsde_qm9_uncond_jodo', [29, 1, 2, 18, 18, 7, 23, 12, 12, 9] * 3, {}, False),       # per-molecule rows at nf 256: the unfolded hoisted form, four waves
    ('vpsde_qm9_cond_jodo', [27, 9, 14, 20, 5] * 6, {}, True),                             # conditional model
    ('vpsde_geom_uncond_jodo', [44, 33, 12, 2, 1], dict(nf=384), True),                   # nf 384 folded (12 output blocks dealt to 2 / 4 waves)
    ('vpsde_geom_uncond_jodo', [40, 33, 7], dict(nf=128, n_layers=6), True),
])
def test_pair_update_z_split_agrees(cfg_name, n_nodes, over, uniform):
    """JODO_OPT_Z_SPLIT (round 5): the pair-update items of a launch's last round run as workgroups of 4 (<= 256 items, default) or 2
    (<= 512 items, option value 2) waves that share the output blocks of the per-pair coord_mlp.0 projection; their partial
    coord_mlp.2 dot products meet in LDS in wave order.  Same items, another summation order of 2 x 3 numbers per pair: outputs
    within the single-forward tolerance of the one-wave form (option 0) and of the oracle, and bit-deterministic."""
    cfg = make_config(cfg_name, **over)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=23)
    if uniform:
        nl[:] = 0.3
    outs = {}
    for z in (0, 1, 2):
        model = make_model(cfg, 5, DEV, gain=1.3, coord_scale=0.05)
        model.plan_options = {12: z}
        o1 = run(model, xh, ex, nl, nm, em, None, None, ctx)
        outs[z] = (o1, run(model, xh, ex, nl, nm, em, o1[0], o1[1], ctx))
        again = run(model, xh, ex, nl, nm, em, o1[0], o1[1], ctx)
        assert torch.equal(again[0], outs[z][1][0]) and torch.equal(again[1], outs[z][1][1])
    sd = state_dict_cpu(model)
    check64(outs[1][0], sd, hp, xh, nm, em, ex, None, None, nl, ctx, 'z split (default), first step', k=k64_for(hp, n_nodes))
    for z in (1, 2):
        for step in (0, 1):
            close(outs[z][step][0], outs[0][step][0], atol=2e-5)
            close(outs[z][step][1], outs[0][step][1], atol=2e-5)
    assert not torch.equal(outs[2][1][0], outs[0][1][0])               # the split really ran (another summation order)


@pytest.mark.parametrize("cfg_name,n_nodes,gain,over", [
    ('vpsde_qm9_uncond_jodo', [6, 11, 20, 29, 1, 2], 1.0, {}),
    ('vpsde_qm9_uncond_jodo', [5] * 14 + [19] * 10, 1.5, {}),                            # several strips
    ('vpsde_geom_uncond_jodo', [70, 33, 12], 1.5, {}),
    ('vpsde_geom_uncond_jodo', [70, 33, 12, 1, 2], 1.5, dict(nf=384)),                  # BASELINE config 4 width
    ('vpsde_geom_uncond_jodo', [19] * 8 + [6] * 10, 1.0, dict(nf=384, n_layers=8, mlp_ratio=2)),
    ('vpsde_qm9_uncond_jodo', [29, 1, 2, 18, 18, 7, 23], 1.5, dict(kernel_layout='wide')),
    ('vpsde_geom_uncond_jodo', [40, 33, 12, 1, 2], 1.5, dict(nf=128, n_layers=6)),           # GEOM Base
    ('vpsde_qm9_uncond_jodo', [29, 1, 2, 18, 18, 7, 23], 1.5, dict(n_layers=6)),              # nf 256 with the 96-wide node readout
    ('vpsde_qm9_uncond_jodo', [29, 1, 2, 18, 18, 7, 23], 1.5, dict(n_layers=5)),              # an odd number of blocks
])
def test_uniform_and_per_molecule_noise_levels_agree(cfg_name, n_nodes, gain, over):
    """One noise level for the whole batch (how every sampler calls an unconditional model) takes the shared-row path:
    modulation GEMVs once per batch and, at nf = 256, the pair update with coord_mlp.0 (1 + sc) input_lin folded into one
    matrix per block (k_fold_coord).  Different arithmetic from the per-molecule path, so both are held to the oracle and
    to each other within the forward tolerance.  At nf = 384 only the shared-row path pushes coord_mlp.0 through."""
    cfg = make_config(cfg_name, **over)
    model = make_model(cfg, 9, DEV, gain=gain, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    sd = state_dict_cpu(model)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=1)
    nl_u = torch.full_like(nl, 0.37)
    k = k64_for(hp, n_nodes)
    a1 = run(model, xh, ex, nl_u, nm, em)
    assert model.last_flags.cpu().tolist()[2] == 1          # shared time row
    r1 = check64(a1, sd, hp, xh, nm, em, ex, None, None, nl_u, ctx, 'shared row, first step', k=k)
    a2 = run(model, xh, ex, nl_u, nm, em, r1[0], r1[1])
    assert model.last_flags.cpu().tolist()[2] == 1
    check64(a2, sd, hp, xh, nm, em, ex, r1[0], r1[1], nl_u, ctx, 'shared row, self-conditioned', k=k)
    nl_p = nl_u.clone()
    nl_p[0] += 1e-6                                          # forces the per-molecule path for the others
    b = run(model, xh, ex, nl_p, nm, em)
    assert model.last_flags.cpu().tolist()[2] == 0
    check64(b, sd, hp, xh, nm, em, ex, None, None, nl_p, ctx, 'per-molecule rows, first step', k=k)
    # path against path: each side is held to the forward tolerance above, so the two differ by at most twice that
    close(a1[0][1:], b[0][1:], atol=4e-5, rtol=2e-4)
    close(a1[1][1:], b[1][1:], atol=4e-5, rtol=2e-4)


@pytest.mark.parametrize("cfg_name,n_nodes,gain,over", [
    ('vpsde_qm9_uncond_jodo', [6, 11, 20, 29, 1, 2, 29, 29, 17, 3], 1.5, {}),
    ('vpsde_qm9_uncond_jodo', [5] * 14 + [19] * 10, 1.5, dict(kernel_layout='wide')),
    # molecules across many strips, n > 128: position sums over 149 neighbours at gain 1.5 — here the float32 oracle itself
    # is ~4e-5 from float64 (round 3 measured rotated 1.1e-4, plain fold 2.7e-4 against float64 and used atol 4e-4)
    ('vpsde_geom_uncond_jodo', [70, 33, 12, 150, 1, 2], 1.5, {}),
    ('vpsde_geom_uncond_jodo', [70, 33, 12, 1, 2], 1.5, dict(nf=384)),
    ('vpsde_geom_uncond_jodo', [70, 33, 12, 1, 2], 1.5, dict(nf=128, n_layers=6)),
])
def test_rotated_statistics_match_plain_fold_and_oracle(cfg_name, n_nodes, gain, over):
    """JODO_OPT_ROT_STATS (default on): under a shared modulation row the pair update takes the LayerNorm statistics of
    equi_update in the rotated basis (triangular L [e ; G] per pair, Q P W_row h / Q P W_col h per node, Gram tile per molecule).
    Different arithmetic from the plain folded path (option 6 = 0): both — first-step AND self-conditioned outputs — are held to
    the float64 oracle at the forward tolerance, and to each other at twice that."""
    cfg = make_config(cfg_name, **over)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=17)
    nl = torch.full_like(nl, -0.8)
    outs = {}
    model = make_model(cfg, 11, DEV, gain=gain, coord_scale=0.05)
    sd = state_dict_cpu(model)
    r1 = r2 = None
    for rot in (1, 0):
        model = make_model(cfg, 11, DEV, gain=gain, coord_scale=0.05)
        model.plan_options = {6: rot}
        o1 = run(model, xh, ex, nl, nm, em)
        assert model.last_flags.cpu().tolist()[2] == 1 and model.last_flags.cpu().tolist()[4] == 0
        if r1 is None:
            r1 = oracle_32_64(sd, hp, xh, nm, em, ex, None, None, nl)
            r2 = oracle_32_64(sd, hp, xh, nm, em, ex, r1[0][0], r1[0][1], nl)
        outs[rot] = (o1, run(model, xh, ex, nl, nm, em, r1[0][0], r1[0][1]))     # self-conditioned on the oracle's prediction: same inputs
        for step, got, (r32, r64) in ((1, outs[rot][0], r1), (2, outs[rot][1], r2)):
            kk = K64_ROT_BIG if max(n_nodes) > 128 else k64_for(hp, n_nodes)       # helpers.py: the one named exception (n = 150 at gain 1.5)
            close64(got[0], r32[0], r64[0], 'rot %d step %d nodes' % (rot, step), k=kk)
            close64(got[1], r32[1], r64[1], 'rot %d step %d edges' % (rot, step), k=kk)
    e32 = max(float((r1[0][k].double() - r1[1][k]).abs().max()) for k in (0, 1))
    for k in (0, 1):
        close(outs[1][k][0], outs[0][k][0], atol=max(4e-5, 8 * e32), rtol=2e-4)
        close(outs[1][k][1], outs[0][k][1], atol=max(4e-5, 8 * e32), rtol=2e-4)
    assert not torch.equal(outs[1][0][0], outs[0][0][0])          # the two paths really differ


def _make_adversarial(model, D, L, eps, common, seed=0):
    """Weights random initialisation never visits and trained ones plausibly do (round-3 review): a DISTANCE-LIKE input_lin,
    W_col = -W_row + eps * noise, so that the per-node halves of `pre` cancel wherever two atoms carry similar features, and a large
    component shared by all atoms of a molecule in h (the LayerNorm2 shift of every block, node_time_mlp chunk ns2, + common *
    unit-variance vector) — kappa = |W_row h_a| / |W_row h_a + W_col h_c| ~ common / sqrt(2).  The uncentred Gram form of the rotated
    statistics loses kappa^2 eps_fp32 there (modelled in tests/test_packing.py), the reference-centred one kappa eps_fp32."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        sd = model.state_dict()
        for l in range(L):
            W = sd['e_block_%d.equi_update.input_lin.weight' % l]
            b = float(W[:, :D].abs().max())
            noise = ((torch.rand(D, D, generator=g) * 2 - 1) * b).to(W.device)
            W[:, D:2 * D] = -W[:, :D] + eps * noise
            sd['e_block_%d.node_time_mlp.1.bias' % l][3 * D:4 * D] += common * torch.randn(D, generator=g).to(W.device)
    return model


@pytest.mark.parametrize("cfg_name,n_nodes,gain,eps,common,over", [
    ('vpsde_qm9_uncond_jodo', [2, 29, 29, 17, 5, 1, 23, 29, 9, 2], 1.5, 1e-3, 100.0, {}),
    ('vpsde_qm9_uncond_jodo', [2, 29, 29, 17, 5, 1, 23, 29, 9, 2], 3.0, 1e-2, 30.0, {}),
    ('vpsde_qm9_uncond_jodo', [2, 29, 18, 18, 7], 5.0, 0.0, 100.0, dict(kernel_layout='wide')),
    ('vpsde_geom_uncond_jodo', [181, 2, 29, 70], 3.0, 1e-3, 100.0, {}),
    ('vpsde_geom_uncond_jodo', [181, 2, 29, 70], 1.5, 1e-3, 100.0, dict(nf=384)),
])
def test_rotated_statistics_on_adversarial_weights(cfg_name, n_nodes, gain, eps, common, over):
    """JODO_OPT_ROT_STATS on weights built to make the two per-node rows of equi_update's LayerNorm input cancel (see
    _make_adversarial), uniform noise level (the only case the rotated path runs in), n in {1, 2, 29, 181}, trunk gain 1.5 - 5.
    The default path (rotated statistics, Gram tiles taken around a reference atom) and the plain fold must both stay within the
    forward tolerance of the float64 oracle; the uncentred Gram tiles of round 3 (option value 2) are run beside them and their
    error is logged — on these weights they are the ones that drift."""
    cfg = make_config(cfg_name, **over)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=23)
    nl = torch.full_like(nl, 0.4)
    errs, outs, r = {}, {}, None
    for rot in (1, 0, 2):
        model = _make_adversarial(make_model(cfg, 13, DEV, gain=gain, coord_scale=0.05), hp.nf, hp.n_layers, eps, common)
        model.plan_options = {6: rot}
        o1 = run(model, xh, ex, nl, nm, em)
        fl = model.last_flags.cpu().tolist()
        assert fl[0] == 0 and fl[2] == 1 and fl[4] == 0          # no NaN, shared row, pair path
        if r is None:
            sd = state_dict_cpu(model)
            r1 = oracle_32_64(sd, hp, xh, nm, em, ex, None, None, nl)
            r = (r1, oracle_32_64(sd, hp, xh, nm, em, ex, r1[0][0], r1[0][1], nl))
        o2 = run(model, xh, ex, nl, nm, em, r[0][0][0], r[0][0][1])
        errs[rot] = max(float((g.cpu().double() - w64[k]).abs().max()) for g2, (w32, w64) in ((o1, r[0]), (o2, r[1])) for k, g in enumerate(g2))
        outs[rot] = (o1, o2)
    e32 = max(float((a.double() - b).abs().max()) for (r32, r64) in r for a, b in zip(r32, r64))
    print("adversarial %s gain %g eps %g common %g: |HIP - f64| rotated %.2e, plain fold %.2e, uncentred Gram %.2e; float32 oracle %.2e"
          % (cfg_name, gain, eps, common, errs[1], errs[0], errs[2], e32))
    from helpers import _log_parity
    _log_parity(dict(what='adversarial summary', rotated=errs[1], plain=errs[0], uncentred=errs[2], oracle32=e32, gain=gain, eps=eps, common=common))
    # everything has been evaluated and logged; now the assertions.  At trunk gain 3 - 5 the outputs reach 1e3 - 1e7 and the float32
    # oracle itself is 1e-2 - 1e3 from float64: the forward tolerance can only be held relative to that (K64_HARD, helpers.py).
    failures = []
    for rot in (1, 0):
        for step, got, (r32, r64) in ((1, outs[rot][0], r[0]), (2, outs[rot][1], r[1])):
            for k, name in ((0, 'nodes'), (1, 'edges')):
                try:
                    close64(got[k], r32[k], r64[k], 'adversarial rot %d step %d %s' % (rot, step, name), k=K64_HARD)
                except AssertionError as e:
                    failures.append(str(e).split('\n')[0])
    assert not failures, '; '.join(failures)
    # the point of the exercise: the rotated statistics are no worse than the plain fold on weights built against them
    assert errs[1] <= max(2.0 * errs[0], K64 * e32), "rotated %.3e vs plain fold %.3e (float32 oracle %.3e)" % (errs[1], errs[0], e32)


def test_invariants():
    cfg = make_config('vpsde_qm9_uncond_jodo')
    model = make_model(cfg, 4, DEV, gain=1.5, coord_scale=0.05)
    hp = O.Hyper.from_config(cfg)
    n_nodes = [12, 29, 3, 17]
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=2)
    xh[:, :, :3] -= xh[:, :, :3].sum(1, keepdim=True) / nm.sum(1, keepdim=True) * nm
    x1, e1 = run(model, xh, ex, nl, nm, em)
    # exact structure
    assert torch.equal(e1, e1.transpose(1, 2))
    B, N = len(n_nodes), max(n_nodes)
    assert (x1 * (1 - nm)).abs().max() == 0
    assert (e1 * (1 - em.reshape(B, N, N, 1))).abs().max() == 0
    assert x1[:, :, :3].sum(1).abs().max() < 1e-5            # centre of mass removed
    # rotation: positions equivariant, everything else invariant
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(0)))
    xr = xh.clone()
    xr[:, :, :3] = xh[:, :, :3] @ q
    x2, e2 = run(model, xr, ex, nl, nm, em)
    close(x2[:, :, :3], x1[:, :, :3] @ q, atol=2e-5)
    close(x2[:, :, 3:], x1[:, :, 3:], atol=2e-5)
    close(e2, e1, atol=2e-5)
    # batch independence: molecule 1 alone == in batch (different plan, different lane placement)
    nm1, em1 = masks([29])
    x3, e3 = run(model, xh[1:2], ex[1:2], nl[1:2], nm1, em1)
    close(x3[0], x1[1], atol=2e-5)
    close(e3[0], e1[1], atol=2e-5)
    # permuting the batch permutes the result exactly (deterministic, no atomics on the data path)
    perm = [2, 0, 3, 1]
    nmp, emp = masks([n_nodes[p] for p in perm])
    x4, e4 = run(model, xh[perm], ex[perm], nl[perm], nmp, emp)
    close(x4, x1[perm], atol=1e-5)
    close(e4, e1[perm], atol=1e-5)
    # run-to-run determinism
    x5, e5 = run(model, xh, ex, nl, nm, em)
    assert torch.equal(x5, x1) and torch.equal(e5, e1)


def test_asymmetric_inputs_follow_the_reference_semantics():
    """No symmetry of edge_x / cond_edge_x is assumed by the kernels."""
    cfg = make_config('vpsde_qm9_uncond_jodo')
    model = make_model(cfg, 6, DEV, gain=1.5)
    hp = O.Hyper.from_config(cfg)
    sd = state_dict_cpu(model)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, [8, 13], seed=3, symmetric=False)
    cx = torch.randn_like(xh) * nm
    cex = torch.randn_like(ex) * em.reshape(2, 13, 13, 1)
    with torch.no_grad():
        want = O.forward_faithful(sd, hp, xh, nm, em, ex, cx, cex, nl)      # the reference's own (sparse) formulation
    got = run(model, xh, ex, nl, nm, em, cx, cex)
    r32 = check64(got, sd, hp, xh, nm, em, ex, cx, cex, nl, None, 'asymmetric inputs')
    assert (want[0] - r32[0]).abs().max() < 1e-5 and (want[1] - r32[1]).abs().max() < 1e-5      # dense == faithful on them too


def test_nan_guard_zeroes_positions():
    cfg = make_config('vpsde_qm9_uncond_jodo')
    model = make_model(cfg, 4, DEV)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, [5, 9], seed=4)
    xh[1, 2, 0] = float('nan')
    x, e = run(model, xh, ex, nl, nm, em)
    assert model.nan_guard_fired()
    assert x[:, :, :3].abs().max() == 0                      # batch-global reset (mol_gnn.py:587-589)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("fname,fused_on", [('traj_qm9_anc5.npz', True), ('traj_qm9_anc5.npz', False),
                                            ('traj_geom_anc3.npz', True), ('traj_geom_anc3.npz', False)])
def test_ancestral_trajectory_with_hip_model(fname, fused_on, split):
    """The reference's recorded trajectory (its own noise draws replayed) with the HIP model; fused_on: the per-step update
    runs as the fused kernel jodo_sampler_step on the recorded draws (the product path), otherwise op by op in torch.
    split: the same with the OPT-IN split-bf16 kernels (model.split_bf16; they take over when the sampler pins its paths after the first
    self-conditioned evaluation) — same reference trajectory, same tolerance, same decodes."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import AncestralSampler
    from jodo_amd.utils import get_self_cond_fn
    fx = load_fixture(fname)
    cfg = make_config(str(fx['cfg_name']))
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    model.split_bf16 = split
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    ns = NoiseScheduleVP(cfg.sde.schedule)
    noise = {'node': torch.from_numpy(fx['node_noise']).to(DEV), 'edge': torch.from_numpy(fx['edge_noise']).to(DEV)}
    sampler = AncestralSampler(ns, torch.linspace(ns.T, 1e-3, int(fx['steps'])), True, True, True,
                               get_self_cond_fn(cfg), noise_fn=lambda i, kind, like: noise[kind][i], fused=fused_on)
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em,
                                          torch.from_numpy(fx['edge_z']).to(DEV), None)
    assert ('split_tape' in model._last_plan) == split          # the split kernels really ran from the pin on (or not at all)
    close(x_mean, torch.from_numpy(fx['x_mean']), atol=1e-3, rtol=0)
    close(e_mean, torch.from_numpy(fx['edge_x_mean']), atol=1e-3, rtol=0)
    check_decodes(cfg, fx, x_mean, e_mean, nm, em)


def test_drop_in_under_the_references_dataparallel_wrapper(tmp_path):
    """The boundary where the reference puts it (models/utils.py:24-28): the registered class is built from the config, moved to
    config.device and wrapped in torch.nn.DataParallel; a checkpoint written the reference's way (`module.`-prefixed keys,
    utils.py:23-30) is loaded into that wrapper with strict=True (utils.py:17); the reference's recorded 5-step trajectory then runs
    through the WRAPPED model.  DataParallel over one device scatters the arguments (fresh views of the masks every call) and calls
    the module in place: the plan cache must recognise the views, not rebuild a plan per call."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models import utils as mutils
    from jodo_amd.models.ema import ExponentialMovingAverage
    from jodo_amd.sampling import AncestralSampler
    from jodo_amd.utils import get_self_cond_fn, restore_checkpoint, save_checkpoint
    fx = load_fixture('traj_qm9_anc5.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.device = torch.device(DEV)
    # the checkpoint: the fixture's weights, saved from a DataParallel-wrapped model as the reference's training loop does
    src = torch.nn.DataParallel(make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain'])), device_ids=[0])
    path = str(tmp_path / 'checkpoint_dp.pth')
    save_checkpoint(path, dict(optimizer=torch.optim.Adam(src.parameters()), model=src,
                               ema=ExponentialMovingAverage(src.parameters(), decay=0.999), step=9))
    assert all(k.startswith('module.') for k in torch.load(path)['model'])
    # the model: exactly create_model's three steps (registry lookup, .to(device), DataParallel), then the strict load
    model = mutils.create_model(cfg, wrap='dataparallel')
    assert isinstance(model, torch.nn.DataParallel) and type(model.module).__name__ == 'DGT_concat'
    state = dict(optimizer=torch.optim.Adam(model.parameters()), model=model, ema=ExponentialMovingAverage(model.parameters(), decay=0.999), step=0)
    state = restore_checkpoint(path, state, cfg.device)
    assert state['step'] == 9
    model.eval()
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    ns = NoiseScheduleVP(cfg.sde.schedule)
    noise = {'node': torch.from_numpy(fx['node_noise']).to(DEV), 'edge': torch.from_numpy(fx['edge_noise']).to(DEV)}
    sampler = AncestralSampler(ns, torch.linspace(ns.T, 1e-3, int(fx['steps'])), True, True, True,
                               get_self_cond_fn(cfg), noise_fn=lambda i, kind, like: noise[kind][i], fused=True)
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV), None)
    close(x_mean, torch.from_numpy(fx['x_mean']), atol=1e-3, rtol=0)
    close(e_mean, torch.from_numpy(fx['edge_x_mean']), atol=1e-3, rtol=0)
    check_decodes(cfg, fx, x_mean, e_mean, nm, em)
    assert len(model.module._plans) == 1, "one batch, one plan: the scattered mask views must hit the plan cache"


@pytest.mark.parametrize("split", [False, True])
def test_baseline_config0_at_its_own_size_through_get_sampling_fn(split):
    """BASELINE.json configs[0] — vpsde_qm9_uncond_jodo, batch 64, 50 ancestral steps — as the REFERENCE ran it on the CPU
    (tests/golden/traj_qm9_cfg0.npz: its own get_sampling_fn, sampling.py:148-232, seeded torch.manual_seed(42)), replayed through this
    package's get_sampling_fn on the GPU: shard=(0, 1) in parity mode re-draws the unsharded run's atom counts and every noise tensor
    from the CPU generator in the reference's order (checked against the fixture's stream checksums), the score network is the HIP
    path.  End state at the K-step tolerance (K <= 50, atol 1e-3), decodes bit-identical above margin."""
    import jodo_amd.sampling as JS
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.models import get_node_dist, load_dataset_info
    from jodo_amd.utils import get_data_inverse_scaler
    fx = load_fixture('traj_qm9_cfg0.npz')
    cfg = make_config(str(fx['cfg_name']))
    cfg.device = torch.device(DEV)
    cfg.sampling.steps = int(fx['steps'])
    B = int(fx['batch'])
    model = make_model(cfg, int(fx['model_seed']), DEV, head_gain=float(fx['head_gain']))
    model.split_bf16 = split                                     # True: the same replay with the opt-in split-bf16 kernels from the pin on
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    fn = JS.get_sampling_fn(cfg, ns, get_node_dist(load_dataset_info(cfg.data.info_name)), B, B, get_data_inverse_scaler(cfg),
                            shard=(0, 1), shard_mode='parity', seed=int(fx['seed']))
    rec, sums = {}, {'node': [], 'edge': []}
    orig_sampling, orig_n, orig_e = JS.AncestralSampler.sampling, JS.sample_combined_position_feature_noise, JS.sample_symmetric_edge_feature_noise

    def rec_sampling(self, model_, z, node_mask, edge_mask, edge_z, context):
        out = orig_sampling(self, model_, z, node_mask, edge_mask, edge_z, context)
        rec['x_mean'], rec['edge_x_mean'], rec['nm'], rec['em'] = out[0], out[1], node_mask, edge_mask
        return out

    def rn(*a, **k):
        v = orig_n(*a, **k)
        sums['node'].append(float(v.double().sum()))
        return v

    def re_(*a, **k):
        v = orig_e(*a, **k)
        sums['edge'].append(float(v.double().abs().sum()))
        return v

    JS.AncestralSampler.sampling, JS.sample_combined_position_feature_noise, JS.sample_symmetric_edge_feature_noise = rec_sampling, rn, re_
    try:
        mols = fn(model)
    finally:
        JS.AncestralSampler.sampling, JS.sample_combined_position_feature_noise, JS.sample_symmetric_edge_feature_noise = orig_sampling, orig_n, orig_e
    # the replayed RNG stream is the reference's: atom counts and every draw's checksum
    assert [int(m[0].shape[0]) for m in mols] == fx['n_nodes'].tolist()
    assert np.allclose(sums['node'], fx['node_noise_sums'], rtol=0, atol=1e-9) and np.allclose(sums['edge'], fx['edge_noise_sums'], rtol=0, atol=1e-9)
    close(rec['x_mean'], torch.from_numpy(fx['x_mean']), atol=1e-3, rtol=0)
    close(rec['edge_x_mean'], torch.from_numpy(fx['edge_x_mean']), atol=1e-3, rtol=0)
    print("config 0 (B = %d, %d steps, split_bf16 = %s) end state vs the reference's: max |dx| %.2e, max |de| %.2e" % (
        B, int(fx['steps']), split, (rec['x_mean'].cpu() - torch.from_numpy(fx['x_mean'])).abs().max(),
        (rec['edge_x_mean'].cpu() - torch.from_numpy(fx['edge_x_mean'])).abs().max()))
    check_decodes(cfg, fx, rec['x_mean'], rec['edge_x_mean'], rec['nm'], rec['em'])
    # and the molecules the sampling function returned are the decoded tensors, cut to size (mol_process, sampling.py:12-32)
    dec = fn.last_decoded[0]
    assert np.array_equal(dec[1].cpu().numpy()[0, :mols[0][1].shape[0]], mols[0][1].numpy())


@pytest.mark.parametrize("fused_on", [True, False])
@pytest.mark.parametrize("fname", ['traj_cond_dpm4.npz', 'traj_cond_dpm_multi8.npz', 'traj_cond_dpm_single3.npz',
                                   'traj_cond_dpm_single1.npz'])
def test_dpm_solver_trajectory_with_hip_model(fname, fused_on):
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.mix_dpm_solver import DPM_Solver_hybrid
    fx = load_fixture(fname)
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.sampling.steps = int(fx['nfe'])
    cfg.sampling.method = 'fast'
    cfg.sampling.dpm_solver_method = str(fx['method'])
    cfg.sampling.dpm_solver_order = int(fx['order'])
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    pn = torch.from_numpy(fx['pos_noise']).to(DEV)
    solver = DPM_Solver_hybrid(NoiseScheduleVP(cfg.sde.schedule), cfg, noise_fn=lambda i, kind, like: pn[i], fused=fused_on)
    x, ex = solver.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em, torch.from_numpy(fx['edge_z']).to(DEV),
                            torch.from_numpy(fx['context']).to(DEV))
    close(x, torch.from_numpy(fx['x']), atol=1e-3, rtol=0)
    close(ex, torch.from_numpy(fx['edge_x']), atol=1e-3, rtol=0)


@pytest.mark.parametrize("fused_on,split", [(True, False), (False, False), (True, True)])
def test_ancestral_50_steps_free_running_and_teacher_forced(fused_on, split):
    """K = 50: (a) free-running with the recorded noise (fused_on: updates by jodo_sampler_step), end state within the K-step tolerance and decodes
    bit-exact above margin; (b) teacher-forced: every one of the reference's 50 recorded step inputs through the
    kernels, against the reference's recorded prediction at the single-forward tolerance."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import AncestralSampler
    from jodo_amd.utils import get_self_cond_fn
    fx = load_fixture('traj_qm9_anc50.npz')
    cfg = make_config('vpsde_qm9_uncond_jodo')
    model = make_model(cfg, int(fx['seed']), DEV, head_gain=float(fx['head_gain']))
    model.split_bf16 = split                                     # (True: 48 of the 50 free-running steps run the opt-in split-bf16 kernels)
    nm, em = masks(fx['n_nodes'].tolist(), DEV)
    ns = NoiseScheduleVP(cfg.sde.schedule)
    steps = int(fx['steps'])
    noise = {'node': torch.from_numpy(fx['node_noise']).to(DEV), 'edge': torch.from_numpy(fx['edge_noise']).to(DEV)}
    sampler = AncestralSampler(ns, torch.linspace(ns.T, 1e-3, steps), True, True, True,
                               get_self_cond_fn(cfg), noise_fn=lambda i, kind, like: noise[kind][i], fused=fused_on)
    with torch.no_grad():
        x_mean, e_mean = sampler.sampling(model, torch.from_numpy(fx['z']).to(DEV), nm, em,
                                          torch.from_numpy(fx['edge_z']).to(DEV), None)
    close(x_mean, torch.from_numpy(fx['x_mean']), atol=1e-3, rtol=0)
    close(e_mean, torch.from_numpy(fx['edge_x_mean']), atol=1e-3, rtol=0)
    check_decodes(cfg, fx, x_mean, e_mean, nm, em)
    assert ('split_tape' in model._last_plan) == split
    if not fused_on or split:
        return                                                   # the teacher-forced half does not depend on the update path (and runs unpinned: exact kernels)
    t = lambda k, i: torch.from_numpy(fx[k][i]).to(DEV)
    worst = 0.0
    with torch.no_grad():
        for i in range(steps):
            cx = None if i == 0 else t('step_pred', i - 1)
            cex = None if i == 0 else t('step_edge_pred', i - 1)
            nl = t('step_noise_level', i)
            px, pe = model(nl, t('step_x', i), nm, em, edge_x=t('step_edge_x', i), cond_x=cx, cond_edge_x=cex, noise_level=nl)
            close(px, t('step_pred', i), atol=5e-5)          # head_gain 30 amplifies the output error accordingly
            close(pe, t('step_edge_pred', i), atol=5e-5)
            worst = max(worst, (px - t('step_pred', i)).abs().max().item(), (pe - t('step_edge_pred', i)).abs().max().item())
    print("teacher-forced worst |err| over 50 steps: %.2e" % worst)


@pytest.mark.parametrize("fname,layout", [("blocks_qm9.npz", "auto"), ("blocks_qm9.npz", "wide"), ("blocks_geom.npz", "auto"),
                                          ("blocks_geom.npz", "wide")])
def test_per_block_intermediates(fname, layout):
    """h, edge state and positions after EVERY block against the reference's own per-block tensors
    (models/mol_gnn.py:562-568, captured by oracle/make_golden.py) at the per-block tolerance atol 1e-4
    (SURVEY.md §8c): an error that cancels by the last block or hides behind the small gain of the output heads
    would show here.  jodo_debug_set_max_blocks stops the forward after l + 1 blocks, jodo_debug_fetch copies the
    packed internal arrays out (molecules in descending-size order, dense n x n edge tiles)."""
    from jodo_amd import capi
    fx = load_fixture(fname)
    cfg = make_config(str(fx['cfg_name']), kernel_layout=layout)
    model = make_model(cfg, int(fx['seed']), DEV)
    hp = O.Hyper.from_config(cfg)
    n_nodes = fx['n_nodes'].tolist()
    nm, em = masks(n_nodes, DEV)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    args = (t('noise_level'), t('xh'), nm, em)
    kw = dict(edge_x=t('edge_x'), cond_x=t('out1_x'), cond_edge_x=t('out1_e'), noise_level=t('noise_level'))
    with torch.no_grad():
        o = model(*args, **kw)
    close(o[0], t('out2_x'))
    close(o[1], t('out2_e'))
    order = sorted(range(len(n_nodes)), key=lambda b: -n_nodes[b])           # the plan's order: descending n, stable
    Nn, rows, D, De = sum(n_nodes), sum(n * n for n in n_nodes), hp.nf, hp.de
    handle = model._last_plan['handle']
    worst = dict(h=0.0, e=0.0, pos=0.0)
    try:
        for l in range(hp.n_layers):
            capi.check(capi.lib().jodo_debug_set_max_blocks(handle, l + 1), 'set_max_blocks')
            with torch.no_grad():
                model(*args, **kw)
            assert model._last_plan['handle'] is handle                         # same plan (same mask tensors)
            h = debug_fetch(model, 0, Nn * D).reshape(Nn, D)
            e = debug_fetch(model, 1, rows * De).reshape(rows, De)
            pos = debug_fetch(model, 2, Nn * 4).reshape(Nn, 4)[:, :3]
            ref = reference_blocks_dense(fx, l)
            no, eo = 0, 0
            for b in order:
                n = n_nodes[b]
                rh, re, rp = ref[b]
                offd = ~torch.eye(n, dtype=torch.bool)
                gp = pos[no:no + n] - pos[no:no + n].mean(0, keepdim=True)      # the kernels centre once, at the end
                ge = e[eo:eo + n * n].reshape(n, n, De)
                for name, got, want in (('h', h[no:no + n], rh), ('e', ge[offd], re[offd]), ('pos', gp, rp)):
                    err = (got - want).abs().max().item() if want.numel() else 0.0
                    worst[name] = max(worst[name], err)
                    assert err < 1e-4, "block %d molecule %d %s: %.3e" % (l, b, name, err)
                no += n
                eo += n * n
    finally:
        capi.check(capi.lib().jodo_debug_set_max_blocks(handle, -1), 'set_max_blocks')
    print("per-block worst |err|:", worst)


@pytest.mark.parametrize("cfg_name,info,B,over,n_sub", [
    ('vpsde_qm9_uncond_jodo', 'qm9_with_h', 2500, {}, 64),                     # BASELINE configs[1]
    ('vpsde_geom_uncond_jodo', 'geom_with_h_1', 512, {}, 64),                  # BASELINE configs[2] (the config file's L = 10)
    ('vpsde_geom_uncond_jodo', 'geom_with_h_1', 512, dict(n_layers=8), 64),    # BASELINE configs[2] as worded (8 layers)
    ('vpsde_geom_uncond_jodo', 'geom_with_h_1', 1250, dict(nf=384), 64),       # per-GPU share of BASELINE configs[3]
    # BASELINE configs[4], conditional model with per-molecule context (mol_gnn.py:728-734): no shared modulation row,
    # so the un-folded pair update and the four-block row GEMM run at the real batch (1250 = one round per GPU when the
    # molecules are dealt to the ranks first; 313 = a quarter round)
    ('vpsde_qm9_cond_jodo', 'qm9_second_half', 1250, {}, 64),
    ('vpsde_qm9_cond_jodo', 'qm9_second_half', 313, {}, 64),
    # ~1 100 node strips: one full round of k_node_post + a remainder of < 256 strips, i.e. the four-wave form of the merged
    # remainder launch (k_node_mix<., 4>; B = 2500 takes the two-wave form), 24 molecules re-evaluated
    ('vpsde_qm9_uncond_jodo', 'qm9_with_h', 1950, {}, 24),
    ('vpsde_geom_uncond_jodo', 'geom_with_h_1', 256, dict(nf=128, n_layers=6), 24),      # the README's GEOM Base model at a real batch
])
def test_full_size_batches_match_oracle_on_sampled_molecules(cfg_name, info, B, over, n_sub):
    """The batch sizes the bench numbers are quoted on: a first-step and a self-conditioned evaluation of the FULL
    batch by the kernels; n_sub whole molecules spread over the size range (always including the largest and the
    smallest) are then re-evaluated by the dense oracle as a sub-batch (outputs are batch-independent,
    SURVEY.md §4) and compared at the single-forward tolerance."""
    from jodo_amd.models import load_dataset_info, get_node_dist
    cfg = make_config(cfg_name, **over)
    model = make_model(cfg, 8, DEV)
    hp = O.Hyper.from_config(cfg)
    sd = state_dict_cpu(model)
    torch.manual_seed(42)
    n_nodes = get_node_dist(load_dataset_info(info)).sample(B).tolist()
    if info.startswith('geom') and B >= 512:
        # the GEOM histogram reaches 181 atoms (datasets/datasets_config.py:58) but a draw of 512 rarely does: force the maximum
        # and one more molecule above an attention group (n > 128: directed-mode items inside the persistent pair launch)
        n_nodes[3], n_nodes[B // 2] = 181, 150
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=7)
    xh[:, :, :3] -= xh[:, :, :3].sum(1, keepdim=True) / nm.sum(1, keepdim=True) * nm
    nl[:] = 0.5                                                              # sampling: one noise level per batch
    shared = 0 if hp.cond_ch else 1                          # conditional: the context makes every modulation row different
    # masks (the plan key, _DGTBase._plan) and inputs go to the device ONCE: every call below runs on the same plan.  The module-level
    # `run` moves the masks on every call — a new address, hence a new unpinned plan on zeroed scratch each time — which is how this
    # test used to compare the flag-dispatched path with itself.
    batch = DeviceBatch(xh, ex, nl, nm, em, ctx, DEV)
    x1, e1 = batch(model)
    fl = model.last_flags.cpu().tolist()
    assert (fl[0], fl[2], fl[3], fl[4]) == (0, shared, 0, 0)      # no NaN, shared time row, first-step branch (:544), pair path
    x2, e2 = batch(model, x1, e1)
    fl = model.last_flags.cpu().tolist()
    assert (fl[0], fl[2], fl[3], fl[4]) == (0, shared, 1, 0)      # self-conditioned branch
    assert len(model._plans) == 1
    # launches per forward: profile_read() counts BRACKETS (one per class and block: 2 + 4 L with or without pins, asserted below);
    # profile_read_kernels() counts the kernel launches issued inside them, which is what a pin takes away
    model.profile_enable(1)
    model.profile_read(), model.profile_read_kernels()
    batch(model, x1, e1)
    brackets_flag, launches_flag = sum(model.profile_read()[1]), sum(model.profile_read_kernels())
    # The configuration the samplers (and bench.py's timed region) run: pin_paths() after the first self-conditioned evaluation —
    # half rows, merged heads, only the launches the flags leave.  Same kernels on the same values: bit-identical at the full
    # batch (k_node_mix, straddled attention groups, the merged heads' second round only exist at this size), and it is the
    # PINNED outputs that go to the oracle below.
    pinned_plan = batch.pin(model)
    p2x, p2e = batch(model, x1, e1)                               # (every call under the pin asserts AFTER it ran that it ran on the pinned plan)
    brackets_pin, launches_pin = sum(model.profile_read()[1]), sum(model.profile_read_kernels())
    model.profile_enable(0)
    p1x, p1e = batch(model)
    assert model._last_plan.get('pinned') and model._last_plan is pinned_plan and len(model._plans) == 1
    assert model.take_nan_count() == 0                            # (also raises if a pin was violated)
    # fewer launches under the pin: the idle variants are gone ("24 per forward at 8 blocks", pin_paths' docstring, is the expectation
    # the printed numbers are to be compared with; the difference itself is not hard-coded)
    print("%s B=%d %r: launches per self-conditioned forward flag-dispatched %d, pinned %d (difference %d, %d blocks; brackets %d / %d)" % (
        cfg_name, B, over, launches_flag, launches_pin, launches_flag - launches_pin, hp.n_layers, brackets_flag, brackets_pin))
    assert brackets_flag == brackets_pin == 2 + 4 * hp.n_layers
    assert 0 < launches_pin < launches_flag
    for name, a, b in (('x1', x1, p1x), ('e1', e1, p1e), ('x2', x2, p2x), ('e2', e2, p2e)):
        assert torch.equal(a, b), "pinned != flag-dispatched on %s: max |diff| %.3e" % (name, (a - b).abs().max().item())
    batch.unpin(model)
    x1, e1, x2, e2 = p1x, p1e, p2x, p2e
    N = max(n_nodes)
    for x, e in ((x1, e1), (x2, e2)):
        assert torch.isfinite(x).all() and torch.isfinite(e).all()
        assert torch.equal(e, e.transpose(1, 2))
        assert (x * (1 - nm)).abs().max() == 0 and (e * (1 - em.reshape(B, N, N, 1))).abs().max() == 0
    by_size = sorted(range(B), key=lambda b: (n_nodes[b], b))
    sub = sorted(set(by_size[int(round(i * (B - 1) / (n_sub - 1.0)))] for i in range(n_sub)), key=lambda b: (n_nodes[b], b))
    sn = [n_nodes[b] for b in sub]
    assert max(sn) == max(n_nodes) and min(sn) == min(n_nodes) and len(sub) >= n_sub - 4
    # the oracle takes them in four size-sorted chunks: a dense sub-batch is padded to its largest molecule (181 atoms at
    # GEOM), and outputs do not depend on the batch
    for lo in range(0, len(sub), 16):
        part = sub[lo:lo + 16]
        pn = [n_nodes[b] for b in part]
        Ns = max(pn)
        nms, ems = masks(pn)
        cut = lambda a, k: a[part][:, :Ns] if k == 1 else a[part][:, :Ns, :Ns]
        cp = ctx[part] if ctx is not None else None
        check64((cut(x1, 1), cut(e1, 2)), sd, hp, cut(xh, 1), nms, ems, cut(ex, 2), None, None, nl[part], cp, 'B=%d first step, molecules %d..' % (B, lo))
        check64((cut(x2, 1), cut(e2, 2)), sd, hp, cut(xh, 1), nms, ems, cut(ex, 2), cut(x1, 1), cut(e1, 2), nl[part], cp,
                'B=%d self-conditioned, molecules %d..' % (B, lo))


def test_full_size_batch_properties():
    """BASELINE config 2 shape (QM9, B = 2500): no oracle at this size; check structure, determinism and
    that a slice of the batch equals the same molecules run alone."""
    from jodo_amd.models import load_dataset_info, get_node_dist
    cfg = make_config('vpsde_qm9_uncond_jodo')
    model = make_model(cfg, 8, DEV)
    hp = O.Hyper.from_config(cfg)
    torch.manual_seed(42)
    n_nodes = get_node_dist(load_dataset_info('qm9_with_h')).sample(2500).tolist()
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=7)
    nl[:] = 0.5
    x1, e1 = run(model, xh, ex, nl, nm, em)
    assert torch.isfinite(x1).all() and torch.isfinite(e1).all()
    assert torch.equal(e1, e1.transpose(1, 2))
    B, N = len(n_nodes), max(n_nodes)
    assert (x1 * (1 - nm)).abs().max() == 0 and (e1 * (1 - em.reshape(B, N, N, 1))).abs().max() == 0
    sub = list(range(100, 108))
    sn = [n_nodes[i] for i in sub]
    Ns = max(sn)
    nms, ems = masks(sn)
    x2, e2 = run(model, xh[sub][:, :Ns], ex[sub][:, :Ns, :Ns], nl[sub], nms, ems)
    close(x2, x1[sub][:, :Ns], atol=2e-5)
    close(e2, e1[sub][:, :Ns, :Ns], atol=2e-5)


def test_cpu_tensor_and_input_grad_are_rejected_loudly():
    cfg = make_config('vpsde_qm9_uncond_jodo')
    model = make_model(cfg, 4, DEV)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, [4, 6], seed=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(nl, xh, nm, em, edge_x=ex, cond_x=None, cond_edge_x=None, noise_level=nl)
    d = lambda x: x.to(DEV)
    # since round 4 a grad-enabled call runs the training path (parameter gradients, tests/test_train_gpu.py); what it does
    # not provide — gradients with respect to the INPUTS — is refused, not silently dropped
    with pytest.raises(RuntimeError, match="parameter gradients only"):
        model(d(nl), d(xh).requires_grad_(True), d(nm), d(em), edge_x=d(ex), cond_x=None, cond_edge_x=None, noise_level=d(nl))
    out = model(d(nl), d(xh), d(nm), d(em), edge_x=d(ex), cond_x=None, cond_edge_x=None, noise_level=d(nl))
    assert out[0].requires_grad and out[1].requires_grad


@pytest.mark.parametrize("cfg_name,n_nodes,over", [
    ('vpsde_qm9_uncond_jodo', [1, 2, 3, 4, 9, 10, 18, 29, 28], {}),       # odd/even sizes, n = 1, 2
    ('vpsde_geom_uncond_jodo', [44, 45, 7], {}),
    ('vpsde_geom_uncond_jodo', [44, 45, 7, 1, 2], dict(nf=384)),             # width-generic pair kernels
    ('vpsde_qm9_uncond_jodo', [1, 2, 3, 4, 9, 10, 18, 29, 28], dict(kernel_layout='wide')),
])
def test_pair_path_equals_directed_path(cfg_name, n_nodes, over):
    """Symmetric inputs take the pair kernels (decided on the device); forcing the directed kernels on the
    same inputs must give the same result (and both match the oracle)."""
    cfg = make_config(cfg_name, **over)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=11)
    m_pair = make_model(cfg, 3, DEV, gain=1.5, coord_scale=0.05)
    m_dir = make_model(cfg, 3, DEV, gain=1.5, coord_scale=0.05)
    m_dir.force_directed = True
    sd = state_dict_cpu(m_pair)
    cx = cex = None
    for step in (1, 2):
        a = run(m_pair, xh, ex, nl, nm, em, cx, cex)
        assert m_pair.last_flags.cpu().tolist()[4] == 0          # pair path taken
        b = run(m_dir, xh, ex, nl, nm, em, cx, cex)
        assert m_dir.last_flags.cpu().tolist()[4] == 1           # directed path taken
        r32 = check64(a, sd, hp, xh, nm, em, ex, cx, cex, nl, None, 'pair path, step %d' % step)
        check64(b, sd, hp, xh, nm, em, ex, cx, cex, nl, None, 'directed path, step %d' % step)
        close(a[0], b[0], atol=1e-5)
        close(a[1], b[1], atol=1e-5)
        cx, cex = r32


# ---- caller-side kernels: fused ancestral update and fused decode ----------------
@pytest.mark.parametrize("cfg_name,n_nodes", [('vpsde_qm9_uncond_jodo', [9, 1, 29, 17, 2]), ('vpsde_geom_uncond_jodo', [44, 7, 61])])
def test_fused_sampler_step_equals_framework_step(cfg_name, n_nodes):
    """Same seed -> same normal draws in the same order -> the HIP update must reproduce the op-by-op update."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.sampling import AncestralSampler
    from jodo_amd.models.utils import sample_combined_position_feature_noise, sample_symmetric_edge_feature_noise
    cfg = make_config(cfg_name)
    hp = O.Hyper.from_config(cfg)
    nm, em = masks(n_nodes, DEV)
    B, N = len(n_nodes), max(n_nodes)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    ts = torch.linspace(ns.T, 1e-3, 6)

    class Fake(torch.nn.Module):                       # deterministic stand-in for the score network
        def forward(self, t, x, node_mask, edge_mask, edge_x=None, noise_level=None, cond_x=None, cond_edge_x=None, context=None):
            e = torch.tanh(edge_x * 0.7 + 0.1)
            return torch.tanh(x * 0.5 + 0.2) * node_mask, (e + e.transpose(1, 2)) * edge_mask.reshape(edge_x.shape[0], edge_x.shape[1], edge_x.shape[2], 1)

    outs = []
    for fused in (False, True):
        torch.manual_seed(123)
        z = sample_combined_position_feature_noise(B, N, hp.in_node_dim, nm)
        ez = sample_symmetric_edge_feature_noise(B, N, hp.edge_ch, em)
        smp = AncestralSampler(ns, ts, True, True, True, lambda a, b: (a, b), fused=fused)
        st = smp.init_state(z, ez)
        hist = []
        for i in range(len(ts)):
            st = smp.step(Fake(), i, st, nm, em)
            hist.append([st[k].clone() for k in ('x', 'edge_x', 'x_mean', 'edge_x_mean')])
        outs.append(hist)
    for ha, hb in zip(*outs):
        for a, b in zip(ha, hb):
            assert (a - b).abs().max().item() < 2e-6
    xa, ea = outs[1][-1][0], outs[1][-1][1]
    assert torch.equal(ea, ea.transpose(1, 2))                                   # symmetric edge state
    assert float((xa * (1 - nm)).abs().max()) == 0.0                             # padding stays exactly zero


@pytest.mark.parametrize("method,order,nfe", [('singlestep_fixed', 2, 6), ('singlestep_fixed', 3, 6), ('singlestep_fixed', 1, 3),
                                              ('multistep', 2, 5)])
def test_fused_dpm_update_equals_framework_update(method, order, nfe):
    """Hybrid DPM-solver: the fused update kernel (jodo_dpm_update) against the op-by-op framework update on the same
    seed (same position-noise draws), for every solver variant of mix_dpm_solver.py:61-265."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.mix_dpm_solver import DPM_Solver_hybrid
    from jodo_amd.models.utils import sample_combined_position_feature_noise, sample_symmetric_edge_feature_noise
    cfg = make_config('vpsde_qm9_uncond_jodo')
    cfg.sampling.steps, cfg.sampling.method = nfe, 'fast'
    cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = method, order
    hp = O.Hyper.from_config(cfg)
    n_nodes = [9, 1, 29, 17, 2]
    nm, em = masks(n_nodes, DEV)
    B, N = len(n_nodes), max(n_nodes)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)

    class Fake(torch.nn.Module):                       # deterministic stand-in for the score network
        def forward(self, t, x, node_mask, edge_mask, edge_x=None, noise_level=None, cond_x=None, cond_edge_x=None, context=None):
            e = torch.tanh(edge_x * 0.7 + 0.1 * noise_level.reshape(-1, 1, 1, 1))
            out = torch.tanh(x * 0.5 + 0.2) * node_mask
            if cond_x is not None:
                out = out + 0.1 * cond_x
            pos = out[:, :, :3] - out[:, :, :3].sum(1, keepdim=True) / node_mask.sum(1, keepdim=True) * node_mask
            return torch.cat([pos, out[:, :, 3:]], 2), (e + e.transpose(1, 2)) * edge_mask.reshape(edge_x.shape[0], edge_x.shape[1], edge_x.shape[2], 1)

    outs = []
    for fused_on in (False, True):
        torch.manual_seed(321)
        z = sample_combined_position_feature_noise(B, N, hp.in_node_dim, nm)
        ez = sample_symmetric_edge_feature_noise(B, N, hp.edge_ch, em)
        solver = DPM_Solver_hybrid(ns, cfg, fused=fused_on)
        outs.append(solver.sampling(Fake(), z, nm, em, ez, None))
        assert solver._noise_calls == solver.noise_draws_per_round()
    for a, b in zip(*outs):
        assert (a - b).abs().max().item() < 2e-6
    assert float((outs[1][0] * (1 - nm)).abs().max()) == 0.0                     # padding stays exactly zero


def test_graph_replayed_dpm_round_equals_eager_solver():
    """BASELINE config 5 path (conditional model, single-step order 2): the captured outer step replayed K - 2 times
    against the eager solver.  Position noise is switched off on both sides (sigma columns of the table zeroed / a
    zero noise_fn), which makes the two runs comparable sample for sample."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.graphed import GraphedDPMRound
    from jodo_amd.mix_dpm_solver import DPM_Solver_hybrid
    from jodo_amd.models.utils import sample_combined_position_feature_noise, sample_symmetric_edge_feature_noise
    cfg = make_config('vpsde_qm9_cond_jodo')
    cfg.sampling.steps, cfg.sampling.method = 10, 'fast'
    cfg.sampling['dpm_solver_method'], cfg.sampling['dpm_solver_order'] = 'singlestep_fixed', 2
    hp = O.Hyper.from_config(cfg)
    n_nodes = [9, 1, 27, 17, 2, 12]
    nm, em = masks(n_nodes, DEV)
    B, N = len(n_nodes), max(n_nodes)
    model = make_model(cfg, 4, DEV, head_gain=10.0)
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    torch.manual_seed(5)
    z = sample_combined_position_feature_noise(B, N, hp.in_node_dim, nm)
    ez = sample_symmetric_edge_feature_noise(B, N, hp.edge_ch, em)
    ctx = torch.randn(B, 1, device=DEV)
    eager = DPM_Solver_hybrid(ns, cfg, noise_fn=lambda i, kind, like: torch.zeros_like(like))
    want = eager.sampling(model, z, nm, em, ez, ctx)
    rnd = GraphedDPMRound(DPM_Solver_hybrid(ns, cfg), model, nm, em, ctx)
    rnd.tab_host[:, 2] = 0.0
    rnd.tab_host[:, 10] = 0.0
    rnd.solver.position_coefficients = (lambda f: (lambda a, b: f(a, b)[:2] + (torch.zeros(()),)))(rnd.solver.position_coefficients)
    with torch.no_grad():
        got = rnd.run(z, ez)
    torch.cuda.synchronize()
    assert rnd.K == 5 and int(rnd.step.item()) == 5                # outer steps 0 (eager), 1 (warm-up), 2-4 (replays)
    close(got[0], want[0], atol=2e-4, rtol=0)
    close(got[1], want[1], atol=2e-4, rtol=0)


@pytest.mark.parametrize("cfg_name", ['vpsde_qm9_uncond_jodo', 'vpsde_geom_uncond_jodo'])
def test_fused_decode_equals_post_process(cfg_name):
    from jodo_amd import fused
    from jodo_amd.sampling import mol_process, post_process
    from jodo_amd.utils import get_data_inverse_scaler
    cfg = make_config(cfg_name)
    hp = O.Hyper.from_config(cfg)
    n_nodes = [9, 1, 23, 17, 2, 23]
    nm, em = masks(n_nodes, DEV)
    B, N = len(n_nodes), max(n_nodes)
    g = torch.Generator().manual_seed(5)
    xh = (torch.randn(B, N, 3 + hp.in_node_dim, generator=g) * 1.5).to(DEV) * nm
    ex = torch.randn(B, N, N, hp.edge_ch, generator=g)
    ex = ((ex + ex.transpose(1, 2)) * 0.6).to(DEV) * em.reshape(B, N, N, 1)
    # exact threshold case: bond channels exactly on the decision boundaries
    ex[0, 0, 1] = 0.0; ex[0, 1, 0] = 0.0                  # (0 + 1) / 2 = 0.5 -> exists
    inv = get_data_inverse_scaler(cfg)
    pos, one_hot, fc, et = post_process(xh.clone(), cfg.data.atom_types, cfg.model.include_fc_charge, nm, inv, ex.clone(), em,
                                        cfg.data.compress_edge)
    want = mol_process(one_hot, pos, fc, n_nodes, et)
    got = fused.mols_from_decoded(*fused.decode(cfg, xh, ex, fused.n_nodes_from_mask(nm)), n_nodes)
    assert len(want) == len(got)
    for w, g_ in zip(want, got):
        assert torch.equal(w[0].cpu(), g_[0]) and torch.equal(w[1].cpu(), g_[1])
        assert torch.equal(w[2].cpu().float(), g_[2]) and torch.equal(w[3].cpu().long(), g_[3])
        assert g_[1].dtype == torch.int64 and g_[3].dtype == torch.int64
    with pytest.raises(TypeError):
        fused.decode(cfg, xh.cpu(), ex, fused.n_nodes_from_mask(nm))


@pytest.mark.parametrize("split", [False, True])
def test_graph_replayed_sampling_round(split):
    """HIP-graph replay of the ancestral loop: every replayed step must (a) have evaluated the score network on
    the state the previous step produced and (b) apply the reference update to its own recorded noise draws.
    split: the captured step holds the opt-in split-bf16 kernels (the round pins its paths before the capture); the eager re-evaluation
    under the same pins reproduces it bit for bit, the exact-fp32 kernels (paths unpinned) to the stated tolerance."""
    from jodo_amd.diffusion import NoiseScheduleVP
    from jodo_amd.graphed import GraphedAncestralRound
    from jodo_amd.sampling import AncestralSampler, posterior_coefficients
    from jodo_amd.models.utils import sample_combined_position_feature_noise, sample_symmetric_edge_feature_noise
    from jodo_amd.utils import get_self_cond_fn
    cfg = make_config('vpsde_qm9_uncond_jodo')
    hp = O.Hyper.from_config(cfg)
    n_nodes = [9, 1, 29, 17, 2, 12]
    nm, em = masks(n_nodes, DEV)
    B, N = len(n_nodes), max(n_nodes)
    model = make_model(cfg, 4, DEV, head_gain=10.0)
    model.split_bf16 = split
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    ts = torch.linspace(ns.T, 1e-3, 7)
    smp = AncestralSampler(ns, ts, True, True, True, get_self_cond_fn(cfg))
    torch.manual_seed(5)
    z = sample_combined_position_feature_noise(B, N, hp.in_node_dim, nm)
    ez = sample_symmetric_edge_feature_noise(B, N, hp.edge_ch, em)
    rnd = GraphedAncestralRound(smp, model, nm, em, record=True)
    with torch.no_grad():
        x_mean, e_mean = rnd.run(z, ez)
    torch.cuda.synchronize()
    assert [h['step'] for h in rnd.history] == list(range(1, len(ts)))           # steps 1..6 ran exactly once each
    prev_pred = None
    for h in rnd.history:
        i = h['step']
        c_x, c_pred, sigma, alpha_t, sigma_t, _, _ = posterior_coefficients(ns, ts[i], smp.s_array[i])
        zx = h['eps_pos'] * nm
        zx = zx - zx.sum(1, keepdim=True) / nm.sum(1, keepdim=True) * nm
        eps_n = torch.cat([zx, h['eps_feat'] * nm], 2)
        ze = torch.tril(h['eps_edge'], -1)
        ze = (ze + ze.transpose(-1, -2)).permute(0, 2, 3, 1) * em.reshape(B, N, N, 1)
        want_mean, want_emean = float(c_x) * h['x_prev'] + float(c_pred) * h['pred_keep'], float(c_x) * h['e_prev'] + float(c_pred) * h['epred_keep']
        assert (h['x_mean'] - want_mean).abs().max().item() < 2e-6 and (h['e_mean'] - want_emean).abs().max().item() < 2e-6
        assert (h['x'] - (want_mean + float(sigma) * eps_n)).abs().max().item() < 2e-6
        assert (h['e'] - (want_emean + float(sigma) * ze)).abs().max().item() < 2e-6
        if prev_pred is not None:                                  # (a): same forward, eagerly, on the recorded inputs
            nl = torch.full((B,), float(torch.log(alpha_t ** 2 / sigma_t ** 2)), device=DEV)
            with torch.no_grad():
                px, pe = model(nl, h['x_prev'], nm, em, edge_x=h['e_prev'], noise_level=nl, cond_x=prev_pred[0], cond_edge_x=prev_pred[1])
            assert torch.equal(px, h['pred_keep']) and torch.equal(pe, h['epred_keep'])
            assert torch.equal(h['x_prev'], prev_state[0]) and torch.equal(h['e_prev'], prev_state[1])
        prev_pred, prev_state = (h['pred_keep'], h['epred_keep']), (h['x'], h['e'])
    assert torch.equal(x_mean, rnd.history[-1]['x_mean']) and not bool(torch.isnan(x_mean).any())
    if split:                                                      # the split kernels really were what the graph replayed: the plan holds their
        assert model._last_plan.get('split_tape') is not None      # tape, and the exact kernels (paths unpinned) give the last bits differently
        model.unpin_paths()
        h = rnd.history[-1]
        nl = torch.full((B,), float(torch.log(alpha_t ** 2 / sigma_t ** 2)), device=DEV)
        with torch.no_grad():
            px, pe = model(nl, h['x_prev'], nm, em, edge_x=h['e_prev'], noise_level=nl, cond_x=rnd.history[-2]['pred_keep'], cond_edge_x=rnd.history[-2]['epred_keep'])
        assert not (torch.equal(px, h['pred_keep']) and torch.equal(pe, h['epred_keep']))
        for got, want in ((h['pred_keep'], px), (h['epred_keep'], pe)):
            assert bool(((got - want).abs() <= 2e-5 + 1e-4 * want.abs()).all())


@pytest.mark.parametrize("cfg_name,info,B,over", [
    ('vpsde_qm9_uncond_jodo', 'qm9_with_h', 230, {}),        # ~130 strips (4-wave node_post), pair items just above one round
    ('vpsde_qm9_uncond_jodo', 'qm9_with_h', 700, {}),        # ~395 strips (2-wave node_post), 3 full rounds + split remainder
    ('vpsde_geom_uncond_jodo', 'geom_with_h_1', 60, dict(nf=384)),
])
def test_medium_batches_cross_the_decomposition_boundaries(cfg_name, info, B, over):
    """Batch sizes chosen so that the launches mix their variants (full rounds + cooperative / direction-split
    remainders, automatic chunk sizes): the pair path must equal the directed path, and the first molecules must
    equal the same molecules evaluated alone (batch independence)."""
    from jodo_amd.models import load_dataset_info, get_node_dist
    cfg = make_config(cfg_name, **over)
    hp = O.Hyper.from_config(cfg)
    torch.manual_seed(B)
    n_nodes = get_node_dist(load_dataset_info(info)).sample(B).tolist()
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=B)
    nl[:] = 0.3
    m_pair = make_model(cfg, 6, DEV, gain=1.2, coord_scale=0.05)
    m_dir = make_model(cfg, 6, DEV, gain=1.2, coord_scale=0.05)
    m_dir.force_directed = True
    a = run(m_pair, xh, ex, nl, nm, em)
    b = run(m_dir, xh, ex, nl, nm, em)
    assert m_pair.last_flags.cpu().tolist()[4] == 0 and m_dir.last_flags.cpu().tolist()[4] == 1
    close(a[0], b[0], atol=2e-5)
    close(a[1], b[1], atol=2e-5)
    assert torch.isfinite(a[0]).all() and torch.equal(a[1], a[1].transpose(1, 2))
    k = 12
    sub = n_nodes[:k]
    Ns = max(sub)
    nm2, em2 = masks(sub)
    c = run(m_pair, xh[:k, :Ns], ex[:k, :Ns, :Ns], nl[:k], nm2, em2)
    close(c[0], a[0][:k, :Ns], atol=2e-5)
    close(c[1], a[1][:k, :Ns, :Ns], atol=2e-5)


@pytest.mark.parametrize("cfg_name,n_nodes,uniform,over", [
    ('vpsde_qm9_uncond_jodo', [6, 11, 20, 29, 1, 2] * 3, True, {}),
    ('vpsde_qm9_uncond_jodo', [6, 11, 20, 29, 1, 2], False, {}),
    ('vpsde_qm9_cond_jodo', [9, 9, 14, 27], True, {}),
    ('vpsde_geom_uncond_jodo', [140, 33, 12], True, {}),                 # n > 128: directed attention items stay, both edge rows kept
    # the width-generic kernel set under pins (half rows, merged heads): nf 384, nf 128 / 6 blocks, nf 256 'wide'; even and odd n
    ('vpsde_geom_uncond_jodo', [44, 33, 12, 2, 1], True, dict(nf=384)),
    ('vpsde_geom_uncond_jodo', [40, 33, 131, 7], True, dict(nf=128, n_layers=6)),
    ('vpsde_qm9_uncond_jodo', [6, 11, 20, 29, 1, 2], True, dict(kernel_layout='wide')),
])
def test_pinned_paths_equal_flag_dispatch(cfg_name, n_nodes, uniform, over):
    """pin_paths() (what the samplers do after the first self-conditioned evaluation of a round) makes the launcher leave
    out the kernel variants the device flags rule out; the variants that do run are the same kernels on the same inputs, so
    outputs are bit-identical.  A call that breaks the pinned structure is reported, not silently mis-computed."""
    cfg = make_config(cfg_name, **over)
    hp = O.Hyper.from_config(cfg)
    model = make_model(cfg, 9, DEV, gain=1.3, coord_scale=0.05)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=5)
    if uniform:
        nl[:] = 0.4
    d = lambda x: None if x is None else x.to(DEV)
    nmd, emd = d(nm), d(em)

    def call(cx=None, cex=None, edge=None):
        with torch.no_grad():
            o = model(d(nl), d(xh), nmd, emd, edge_x=d(ex if edge is None else edge), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(nl),
                      context=d(ctx))
        torch.cuda.synchronize()
        return o[0].cpu(), o[1].cpu()

    a1 = call()
    a2 = call(a1[0], a1[1])
    flags = model.last_flags.cpu().tolist()
    assert flags[4] == 0 and flags[2] == (1 if uniform and not hp.cond_ch else 0)
    model.pin_paths()
    assert model._last_plan.get('pinned')
    pinned = list(model._last_plans)
    b2 = call(a1[0], a1[1])
    assert_pinned_call(model, pinned)                        # AFTER the call: it ran on the plan that was pinned, not on a new one
    b1 = call()
    assert_pinned_call(model, pinned)
    assert len(model._plans) == 1
    assert torch.equal(a1[0], b1[0]) and torch.equal(a1[1], b1[1]) and torch.equal(a2[0], b2[0]) and torch.equal(a2[1], b2[1])
    assert model.take_nan_count() == 0
    bad = ex.clone()
    bad[0, 0, 1, 0] += 1.0                                   # asymmetric input under a symmetric pin
    call(edge=bad)
    with pytest.raises(RuntimeError, match="pinned"):
        model.take_nan_count()
    assert model.take_nan_count() == 0                       # cleared by the read


@pytest.mark.parametrize("cfg_name,n_nodes,k", [('vpsde_qm9_uncond_jodo', [6, 11, 20, 29, 1, 2, 18, 18, 7, 23, 12], 2),
                                                ('vpsde_qm9_uncond_jodo', [6, 11, 20, 29, 1, 2, 18, 18, 7, 23, 12], 3),
                                                ('vpsde_qm9_cond_jodo', [9, 9, 14, 27, 5], 2),
                                                ('vpsde_geom_uncond_jodo', [70, 33, 12, 44], 2)])
def test_stream_interleaved_sub_batches_equal_single_stream(cfg_name, n_nodes, k):
    """model.n_streams = k evaluates k contiguous sub-batches concurrently on k HIP streams (molecules are independent):
    the result must equal the single-stream evaluation of the whole batch within the batch-independence tolerance and
    match the oracle; a NaN in one sub-batch resets the positions of the WHOLE batch like the reference's batch-global guard."""
    cfg = make_config(cfg_name)
    hp = O.Hyper.from_config(cfg)
    xh, ex, nl, ctx, nm, em = random_inputs(hp, n_nodes, seed=17)
    nl[:] = -0.3
    one = make_model(cfg, 4, DEV, gain=1.3, coord_scale=0.05)
    many = make_model(cfg, 4, DEV, gain=1.3, coord_scale=0.05)
    many.n_streams = k
    sd = state_dict_cpu(one)
    a1 = run(one, xh, ex, nl, nm, em, None, None, ctx)
    nmd, emd = nm.to(DEV), em.to(DEV)
    d = lambda x: None if x is None else x.to(DEV)

    def split_call(cx=None, cex=None, x_in=xh):
        with torch.no_grad():
            o = many(d(nl), d(x_in), nmd, emd, edge_x=d(ex), cond_x=d(cx), cond_edge_x=d(cex), noise_level=d(nl), context=d(ctx))
        torch.cuda.synchronize()
        return o[0].cpu(), o[1].cpu()

    b1 = split_call()
    assert len(many._last_plans) == k
    check64(b1, sd, hp, xh, nm, em, ex, None, None, nl, ctx, '%d streams' % k)
    close(b1[0], a1[0], atol=2e-5)
    close(b1[1], a1[1], atol=2e-5)
    a2 = run(one, xh, ex, nl, nm, em, a1[0], a1[1], ctx)
    b2 = split_call(a1[0], a1[1])
    many.pin_paths()
    pinned = list(many._last_plans)
    assert len(pinned) == k and all(p.get('pinned') for p in pinned)
    b3 = split_call(a1[0], a1[1])
    assert_pinned_call(many, pinned)                         # AFTER the call: every sub-batch ran on its pinned plan
    close(b2[0], a2[0], atol=2e-5)
    close(b2[1], a2[1], atol=2e-5)
    assert torch.equal(b2[0], b3[0]) and torch.equal(b2[1], b3[1]) and many.take_nan_count() == 0
    xn = xh.clone()
    xn[len(n_nodes) - 1, 0, 0] = float('nan')                # last molecule: last sub-batch
    c = split_call(x_in=xn)
    assert many.nan_guard_fired() and float(c[0][:, :, :3].abs().max()) == 0.0 and many.take_nan_count() == 1

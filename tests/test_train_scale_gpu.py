"""The 3-D training backward (csrc/dgt_train.hip, train_ops.h, train_fused.hip, train_gemm.hip) at the batch sizes where its reductions
and its attention change form BY SIZE, held to an absolute yardstick: float64 autograd through the CPU oracle where the oracle is
affordable, the op-by-op form of the same kernels where it is not.  Linearity and bit-identical replay (tests/test_train_gpu.py's
full-batch test) cannot see a reduction that drops a chunk, a ragged tail or a whole second level: such a reduction is still linear and
still deterministic.

Cases, inputs and yardsticks: tests/train_scale_common.py (shared with the host emulation build, tests/test_train_emul.py); the switch
table with the test that covers each row: DESIGN.md 9a.  TrainEngine is driven directly so that one forward serves several backwards.

Bounds are the project's own: against float64 3e-4 of the tensor's scale, widened to 16 x the float32-autograd distance
(helpers.compare_grads); between two kernel forms 2e-4 of scale, 1e-3 for dist_layer / time_mlp names
(test_fused_forward_chains_equal_the_op_by_op_forward); forward 2e-5 + 1e-4 |x|."""
import time

import pytest
import torch

import train_scale_common as S
from helpers import compare_grads, masks, oracle_param_grads

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def d(x):
    return None if x is None else x.to(DEV)


def fwd_close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    assert bool((err <= 2e-5 + 1e-4 * want.abs()).all()), "%s: max |err| %.3e (max |want| %.3e)" % (what, err.max().item(), want.abs().max().item())


def forward(eng, params, n_nodes):
    xh, ex, nl = S.batch(n_nodes)[:3]
    ox, oe = eng.forward(params, d(xh), d(ex), None, None, d(nl), None, 0.0, 0)
    flags = eng.flags.tolist()
    assert flags[0] == 0 and flags[3] == 0 and bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oe).all())
    return ox, oe


def backward(eng, params, n_nodes, local=None):
    d_x, d_e = S.out_grads(n_nodes, local)
    grads = eng.backward(params, d(S.batch(n_nodes)[2]), d(d_x), d(d_e), 0.0, 0)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    return grads


def oracle_pass(eng, names, params, n_nodes, local, what):
    """One backward on the engine's current activations against the float64 yardstick of (case, pass) by the gradient rule; a pass confined
    to one molecule also asserts what train_scale_common.UNWIDENED says of the widened bounds."""
    grads = [g.clone() for g in backward(eng, params, n_nodes, local)]
    want = S.yardstick(n_nodes, local)[2]
    want32 = S.yardstick(n_nodes, local, torch.float32)[2]
    S.assert_reduced_nonzero(want, what)
    ratio, widened = compare_grads(zip(names, grads), want, S.GRAD_REL, want32, S.K32, what=what)
    S.check_widening(n_nodes, local, widened, what)
    return grads


def forms_close(names, got, ref, what):
    """Two forms of the same kernels: 2e-4 of the tensor's scale, 1e-3 for the Gaussian-layer and time-path gradients."""
    bad, worst = [], 0.0
    for name, a, b in zip(names, got, ref):
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        tol = (1e-3 if ('dist_layer' in name or 'time_mlp' in name) else 2e-4) * max(scale, 1e-12) + 1e-9
        worst = max(worst, err / tol)
        if not err <= tol:
            bad.append("%s: %.3e of %.3e" % (name, err, scale))
    print("%s: worst err / bound %.4f" % (what, worst))
    assert not bad, what + " differ in the gradients of:\n  " + "\n  ".join(bad[:20])


def test_above_65536_rows_every_gradient_matches_the_oracle():
    """(a) n_nodes = [181, 181, 46, 5], R = 67 663 edge rows (no multiple of 32).  colsum's deferred form has n = 2 115 first-level
    chunks for coord_norm.scale — above 2 048, so the second level's chunk is c2 = 34 rows instead of 32 — and the Gaussian layer's
    d means / d stds (2 115 chunk rows -> 67 partial rows) gain their second level (FIN_COLPART) at all.  Three backwards on one forward:
    a random output gradient everywhere; the same confined to the LAST molecule (5 atoms: the final, ragged rows beyond row 65 536);
    confined to the FIRST molecule (the first chunks).  The bulk pass takes the rule's widening where float32 autograd itself is far from
    float64 (measured on the CPU at this size: 4.4e-4 of scale on e_block_0's coord_norm.scale, 3.2e-3 on its dist_layer.time_mlp.1.bias,
    2e-5 to 6e-4 on 26 tensors in all).  Confined to the 5-atom molecule float32 autograd is at most 2.5e-6 of scale from float64 on any
    tensor and the widening must be active on none; confined to the 181-atom one it is not that quiet (3.0e-3 on e_block_0's
    coord_norm.scale, 30 tensors above 3e-4 / 16), so that pass follows the rule and must leave e_block_1's coord_norm.scale un-widened
    (train_scale_common.UNWIDENED).
    Measured on the MI355X, worst err / bound and tensors with a widened bound: everywhere 0.51 (23), last molecule 0.0083 (0), first
    molecule 0.38 (22); through the emulation build 0.12 (26), 0.0087 (0), 0.12 (30).  3.6 s, nearly all of it the oracle."""
    t0 = time.time()
    n_nodes = S.ABOVE_64K
    assert S.rows(n_nodes) == 67663 and S.rows(n_nodes) % 32 and (S.rows(n_nodes) + 31) // 32 > 2048
    eng, names, params = S.make_engine(n_nodes, DEV)
    ox, oe = forward(eng, params, n_nodes)
    px, pe, _ = S.yardstick(n_nodes, None)
    fwd_close(ox, px, 'positions and atom features')
    fwd_close(oe, pe, 'edge features')
    oracle_pass(eng, names, params, n_nodes, None, '(a) 67 663 rows, output gradient everywhere')
    oracle_pass(eng, names, params, n_nodes, 3, '(a) 67 663 rows, output gradient on the last molecule (5 atoms)')
    oracle_pass(eng, names, params, n_nodes, 0, '(a) 67 663 rows, output gradient on the first molecule (181 atoms)')
    print('(a) wall time %.1f s' % (time.time() - t0))


@pytest.mark.parametrize("case,pinned", [('GBF_BY_SIZE', 0), ('GBF_BELOW', 2)])
def test_gaussian_chunk_pass_on_both_sides_of_its_threshold(case, pinned):
    """(b) The Gaussian layer's backward as the wave-per-chunk pass (train_fused.hip k_gbf_bwd_chunk) is the default from nch = 4 096
    chunk rows: [181, 181, 181, 181] (R = 131 044, nch = 4 096) takes it by size, [181, 181, 181, 180] (R = 130 683, nch = 4 084) does not.
    Each batch at default options against the same batch with option 5 pinned the other way (0 = never, resp. 2 = always): outputs
    bit for bit, gradients within the rule for two forms of the same kernels.  Behind either form runs the two-level colsum.
    Measured on the MI355X: the two forms' gradients are bit-equal at both sizes (both sum in double and round once); 0.04 s each."""
    t0 = time.time()
    from jodo_amd.train import TrainEngine
    n_nodes = getattr(S, case)
    assert ((S.rows(n_nodes) + 31) // 32 >= 4096) == (case == 'GBF_BY_SIZE')
    pool = TrainEngine.new_pool()
    res = []
    for options in (None, {5: pinned}):
        eng, names, params = S.make_engine(n_nodes, DEV, options=options, pool=pool)
        ox, oe = forward(eng, params, n_nodes)
        res.append((ox.cpu(), oe.cpu(), [g.cpu() for g in backward(eng, params, n_nodes)]))
        del eng
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    forms_close(names, res[0][2], res[1][2], '(b) %s: default options and option 5 = %d' % (case, pinned))
    print('(b) %s forms: wall time %.1f s' % (case, time.time() - t0))


def test_gaussian_chunk_pass_by_size_matches_the_oracle_and_replays():
    """(b) [181, 181, 181, 181], R = 131 044: the chunk pass selected by size, together with the two-level colsum behind it (4 096 chunk
    rows -> 128 -> 4 partial rows; coord_norm.scale: 4 096 first-level chunks, c2 = 64), against float64 autograd through the oracle —
    the output gradient everywhere, and confined to the last molecule (181 atoms: the rule with its widening, e_block_1's coord_norm.scale
    un-widened; float32 autograd's worst distance there 2.5e-4 of scale, on e_block_0's dist_layer.stds) — and a replay of the backward bit for bit.
    Measured on the MI355X, worst err / bound and tensors with a widened bound: everywhere 0.091 (24), last molecule 0.15 (27); the last
    molecule through the emulation build 0.15 (19).  3.0 s."""
    t0 = time.time()
    n_nodes = S.GBF_BY_SIZE
    eng, names, params = S.make_engine(n_nodes, DEV)
    ox, oe = forward(eng, params, n_nodes)
    px, pe, _ = S.yardstick(n_nodes, None)
    fwd_close(ox, px, 'positions and atom features')
    fwd_close(oe, pe, 'edge features')
    g1 = oracle_pass(eng, names, params, n_nodes, None, '(b) 131 044 rows, output gradient everywhere')
    oracle_pass(eng, names, params, n_nodes, 3, '(b) 131 044 rows, output gradient on the last molecule')
    assert all(torch.equal(a, b) for a, b in zip(g1, backward(eng, params, n_nodes)))
    print('(b) oracle: wall time %.1f s' % (time.time() - t0))


@pytest.mark.parametrize("total", [16383, 16384])
def test_attention_across_the_one_wave_switch(total):
    """(c) Attention forward / backward with one wave per atom instead of 2 - 4 (train_fused.hip fused_attn_fwd / fused_attn_bwd) from
    Nn = 16 384 atoms: molecules of 3 .. 6 atoms (softmax rows of 2 .. 5 sources), Nn = 16 383 and 16 384.  The oracle cannot afford the
    batch (3 700 such molecules: 433 s in float64), so: default options against option 4 = 0 (op-by-op attention) — outputs bit for bit,
    gradients within the rule for two forms; at 16 383 also against option 4 = 2 (the one-wave form forced); and, because molecules do
    not interact, the backward of an output gradient confined to the first six (resp. the last six) molecules IS the gradient of those
    six evaluated alone, which float64 autograd through the oracle checks by the gradient rule — as is the forward of the first six.
    These batches are also the ones whose queued weight-gradient products do not fit one grouped launch: 16 k node rows against 79 k edge
    rows at nf = 128 make the 13 products queued up to a block's attention overflow the grouped launch's scratch (6 x one product's
    plan), so gemm_dw_group cuts the group there (train_scale_common.dw_group_launches restates it).  Grouped against one launch per
    product (option 3 = 0): every gradient bit for bit.
    Measured on the MI355X, worst err / bound: default against op-by-op attention 0.0015 (Nn = 16 383) and 0.0019 (16 384), against the
    forced one-wave form 0.0013; the six molecules against float64 0.078 (first) and 0.042 / 0.046 (last), 4 tensors widened.  0.4 s each."""
    t0 = time.time()
    from jodo_amd.train import TrainEngine
    n_nodes = S.attention_nodes(total)
    B = len(n_nodes)
    xh, ex, nl, nm, em, d_x, d_e = S.batch(n_nodes)
    pool = TrainEngine.new_pool()
    k = 6
    sel = {'first': torch.arange(B) < k, 'last': torch.arange(B) >= B - k}
    conf = {w: ((d_x * m.view(-1, 1, 1)).contiguous(), (d_e * m.view(-1, 1, 1, 1)).contiguous()) for w, m in sel.items()}
    res = {}
    cuts = [g for g in S.dw_group_launches(n_nodes) if g[2] > 1]
    assert cuts and all(g[3] == 'scratch' for g in cuts), cuts
    for form, options in (('default', None), ('op-by-op', {4: 0}), ('one launch per product', {3: 0})) + ((('one wave', {4: 2}),) if total < 16384 else ()):
        eng, names, params = S.make_engine(n_nodes, DEV, options=options, pool=pool)
        ox, oe = forward(eng, params, n_nodes)
        grads = [g.cpu() for g in backward(eng, params, n_nodes)]
        part = {w: [g.cpu() for g in eng.backward(params, d(nl), d(dx), d(de), 0.0, 0)] for w, (dx, de) in conf.items()} if form == 'default' else None
        res[form] = (ox.cpu(), oe.cpu(), grads, part)
        del eng
    for form in res:
        if form == 'one launch per product':
            diff = [k for k, a, b in zip(names, res['default'][2], res[form][2]) if not torch.equal(a, b)]
            assert not diff, "grouped (cut at the scratch) and one-by-one weight gradients differ: %s" % diff[:20]
        elif form != 'default':
            assert torch.equal(res[form][0], res['default'][0]) and torch.equal(res[form][1], res['default'][1]), form
            forms_close(names, res['default'][2], res[form][2], '(c) Nn = %d: default and %s attention' % (total, form))
    # the six molecules alone: forward and every gradient against float64 (and float32) autograd through the oracle
    model, hp = S.model_and_hp()
    for w, m in sel.items():
        idx = m.nonzero()[:, 0].tolist()
        sub = [n_nodes[i] for i in idx]
        Ns = max(sub)
        nm_s, em_s = masks(sub)
        cut = lambda t: t[idx][:, :Ns].contiguous()
        cut2 = lambda t: t[idx][:, :Ns, :Ns].contiguous()
        args = (model, hp, cut(xh) * nm_s, nm_s, em_s, cut2(ex) * em_s.reshape(k, Ns, Ns, 1), None, None, nl[idx].contiguous(), None, cut(d_x), cut2(d_e))
        px, pe, want = oracle_param_grads(*args)
        want32 = oracle_param_grads(*args, dtype=torch.float32)[2]
        fwd_close(cut(res['default'][0]) * nm_s, px, 'the %s six molecules, positions and atom features' % w)
        fwd_close(cut2(res['default'][1]) * em_s.reshape(k, Ns, Ns, 1), pe, 'the %s six molecules, edge features' % w)
        compare_grads(zip(names, res['default'][3][w]), want, S.GRAD_REL, want32, S.K32, what='(c) Nn = %d, output gradient on the %s six molecules' % (total, w))
    print('(c) Nn = %d (%d molecules, %d rows): wall time %.1f s' % (total, B, S.rows(n_nodes), time.time() - t0))


def test_edge_chunk_lengths_on_either_side_of_32_rows():
    """(d) Per-molecule edge chunks are max(32, ceil(n^2 / 64)) rows long: [46, 45, 64, 1] has n^2 = 2 116 (chunks of 34 rows, the last
    one 8), 2 025 (32 rows, the last one 9), 4 096 (64 rows, none ragged) and 1 (one row).
    Measured on the MI355X: worst err / bound 0.048, 19 tensors widened (emulation build: 0.062, 19).  0.2 s."""
    t0 = time.time()
    n_nodes = S.CHUNK_EDGES
    assert [max(32, (n * n + 63) // 64) for n in n_nodes] == [34, 32, 64, 32]
    eng, names, params = S.make_engine(n_nodes, DEV)
    ox, oe = forward(eng, params, n_nodes)
    px, pe, _ = S.yardstick(n_nodes, None)
    fwd_close(ox, px, 'positions and atom features')
    fwd_close(oe, pe, 'edge features')
    oracle_pass(eng, names, params, n_nodes, None, '(d) [46, 45, 64, 1], output gradient everywhere')
    print('(d) wall time %.1f s' % (time.time() - t0))

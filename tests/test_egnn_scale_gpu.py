"""GPU tests of the property classifier (jodo_amd.cond_gen.EGNN, csrc/egnn_forward.hip) at evaluation batch sizes and at its size edges,
against tests/oracle_egnn.py in float32 and float64 (helpers.close64 at its defaults everywhere; tests/test_egnn_host.py holds the
oracle to the reference's recorded outputs).  tests/test_egnn_gpu.py drives one batch of 262 atoms; here:

  1. three trips of kegnn_edge's persistent loop in each of its four instantiations (4 986 atoms > 2 x 512 x 4);
  2. the molecule-level GEMM (graph_dec.0, 64-row blocks) at B = 64, 65, 129;
  3. molecules of 255, 181 and 224 atoms at padded width 255, in_node_nf = 16, real-valued inputs;
  4. in_node_nf 1 and 16 with and without node_attr;
  5. a saturated attention gate and saturated SiLUs (att_mlp.0.weight x 64; positions 20 randn);
  6. NaN and +inf on the padding atoms;
  7. the plan cache: eviction, re-entry, alternation at one (B, N)."""
import pytest
import torch

import egnn_scale_common as C
from egnn_scale_common import call, hidden
from helpers import close64

pytestmark = pytest.mark.gpu


def _check(model, sd, st, h0, x, n_nodes, N, chunk, what, finite=False):
    """Output and first-layer hidden state against the chunked oracle; returns the output."""
    (o32, h32), (o64, h64) = C.yardsticks(sd, st, h0, x, n_nodes, chunk)
    out = call(model, h0, x, n_nodes, N)
    hid = hidden(model, h0, x, n_nodes, N)
    assert out.shape == o64.shape and hid.shape == h64[0].shape == (sum(n_nodes), st['hidden_nf'])
    if finite:
        assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(h32[0]).all()), "%s: the float32 oracle is not finite" % what
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(hid).all()), "%s: non-finite values" % what
    print("%s output: err %.3e, oracle fp32 %.3e" % ((what,) + close64(out, o32, o64, '%s output' % what)))
    print("%s hidden 1: err %.3e, oracle fp32 %.3e" % ((what,) + close64(hid, h32[0], h64[0], '%s hidden 1' % what)))
    return out


# ---- 1. three trips of the persistent edge kernel ---------------------------------------------------------------------------------------
def _trip_picks(n_nodes):
    """About a dozen molecules: first, last, those holding atoms 2048 and 4096 (straddling a trip boundary), and per trip the first
    molecule of 1 atom and the first of 33 that begins in it."""
    off, picks, seen = 0, {0, len(n_nodes) - 1}, set()
    for b, n in enumerate(n_nodes):
        for edge in (C.TRIP, 2 * C.TRIP):
            if off <= edge < off + n:
                picks.add(b)
        if n in (1, 33) and (n, off // C.TRIP) not in seen:
            seen.add((n, off // C.TRIP))
            picks.add(b)
        off += n
    assert seen == {(n, t) for n in (1, 33) for t in range(3)}
    return sorted(picks)


@pytest.mark.parametrize("tag", list(C.TRIP_CASES))
def test_three_trips_of_the_persistent_edge_kernel(tag):
    """272 molecules, 4 986 atoms: every wave of the capped grid walks two atoms and some walk three, with 1-atom molecules (the early
    `continue`) and 33-atom molecules (two source chunks) in every trip.  Output and first-layer hidden state against the oracle (a
    failure names the worst error per trip t // 2048); a molecule alone, the reversed batch and a second run are bit-identical."""
    st, model, sd, h0, x, n_nodes, (o32, h32), (o64, h64) = C.trip_case(tag)
    B, N, Nn = len(n_nodes), h0.shape[1], sum(n_nodes)
    # csrc/egnn_forward.hip edge_launch: at most 512 workgroups; kegnn_edge: 4 waves each, wave w walks atoms w, w + 2048, ...
    assert Nn > 2 * 512 * 4 and C.TRIP == 512 * 4, "the batch no longer gives any wave a third trip"
    hid = hidden(model, h0, x, n_nodes, N)                    # first: its rows are atoms, so a failure can be laid out by trip
    assert hid.shape == h64[0].shape == (Nn, st['hidden_nf'])
    try:
        print("%s hidden 1: err %.3e, oracle fp32 %.3e" % ((tag,) + close64(hid, h32[0], h64[0], 'egnn trips %s hidden 1' % tag)))
    except AssertionError as e:
        raise AssertionError("%s; worst error per trip of the edge kernel (t // %d = 0, 1, 2): %s; float32 oracle: %s" % (
            e, C.TRIP, ["%.3e" % v for v in C.per_trip_errors(hid, h64[0])], ["%.3e" % v for v in C.per_trip_errors(h32[0], h64[0])]))
    out = call(model, h0, x, n_nodes, N)
    assert out.shape == (B,)
    print("%s output: err %.3e, oracle fp32 %.3e" % ((tag,) + close64(out, o32, o64, 'egnn trips %s output' % tag)))
    for b in _trip_picks(n_nodes):
        alone = call(model, h0[b:b + 1], x[b:b + 1], [n_nodes[b]], N, edges=False)
        assert torch.equal(alone, out[b:b + 1]), "molecule %d (%d atoms) alone differs from the batch" % (b, n_nodes[b])
    # reversal moves every atom to another wave and trip
    assert torch.equal(call(model, h0.flip(0), x.flip(0), n_nodes[::-1], N), out.flip(0))
    assert torch.equal(call(model, h0, x, n_nodes, N), out)
    assert torch.equal(hidden(model, h0, x, n_nodes, N), hid)


# ---- 2. row counts of the molecule-level GEMM -------------------------------------------------------------------------------------------
def test_molecule_level_gemm_row_counts():
    """graph_dec.0 is a row GEMM over rows = B in 64-row blocks with clamped reads: one full block, one block plus a row, two blocks
    plus a row.  The leading 64 molecules give the same bits whatever follows them."""
    st = C.settings(64, 1, 1, 1)
    model, sd = C.make_model(st, 23)
    N = 3
    n_all = [1 + b % 3 for b in range(129)]
    h0, x = C.batch(n_all, N, 29, 5, True)
    outs = {}
    for B in (64, 65, 129):
        n = n_all[:B]
        o32, _ = C.oracle_chunked(sd, st, h0[:B], x[:B], n, torch.float32, B)
        o64, _ = C.oracle_chunked(sd, st, h0[:B], x[:B], n, torch.float64, B)
        outs[B] = call(model, h0[:B], x[:B], n, N)
        assert outs[B].shape == (B,)
        print("B = %d: err %.3e, oracle fp32 %.3e" % ((B,) + close64(outs[B], o32, o64, 'egnn rows B=%d' % B)))
    assert torch.equal(outs[65][:64], outs[64]) and torch.equal(outs[129][:64], outs[64])
    assert float((outs[129][:64] - outs[129][64:128]).abs().max()) > 1e-4         # the second block holds other molecules' results


# ---- 3. wide molecules ------------------------------------------------------------------------------------------------------------------
WIDE = [255, 181, 224, 1, 2]


@pytest.mark.parametrize("nf,layers", [(128, 2), (256, 1)])
def test_wide_molecules(nf, layers):
    """n = 255 (eight source chunks, the last with 31 sources; atom slot 254), 181, 224 (seven full chunks) beside 1 and 2, with 16
    real-valued input channels and node_attr: LDS weights (nf 128) and streamed (nf 256).  The reversed batch gives the same bits."""
    st = C.settings(nf, layers, 1, 1, in_nf=16)
    model, sd = C.make_model(st, 37)
    N = 255
    h0, x = C.batch(WIDE, N, 41, 16, False, scale=3.0)
    out = _check(model, sd, st, h0, x, WIDE, N, 1, 'egnn wide nf%d' % nf)
    assert torch.equal(call(model, h0.flip(0), x.flip(0), WIDE[::-1], N), out.flip(0))


def test_padded_width_256_is_refused():
    from jodo_amd import capi
    st = C.settings(64, 1, 0, 0)
    model, _ = C.make_model(st, 1)
    h0, x = C.batch([3], 256, 1, 5, True)
    with pytest.raises(capi.JodoHipError, match="padded width"):
        call(model, h0, x, [3], 256)
    h0, x = C.batch([3], 255, 1, 5, True)
    assert bool(torch.isfinite(call(model, h0, x, [3], 255)).all())


# ---- 4. input channel counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node_attr", [0, 1])
@pytest.mark.parametrize("in_nf", [1, 16])
def test_input_channel_counts(in_nf, node_attr):
    """kegnn_gather zero-pads h0 to a 64-wide K chunk: the embedding's only chunk and, with node_attr, the third K range of node_mlp.0
    (the tail of a 2 nf + in column matrix).  Real-valued inputs at both ends of the accepted range."""
    st = C.settings(64, 1, 0, node_attr, in_nf=in_nf)
    model, sd = C.make_model(st, 43)
    n_nodes = [1, 2, 33, 40]
    h0, x = C.batch(n_nodes, 40, 47, in_nf, False)
    _check(model, sd, st, h0, x, n_nodes, 40, 4, 'egnn in%d attr%d' % (in_nf, node_attr))


# ---- 5. saturating gate and activations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.5, 20.0])
@pytest.mark.parametrize("nf", [128, 192])
def test_saturating_gate_and_activations(nf, scale):
    """att_mlp.0.weight x 64: the gate rcp(1 + exp(-g)) goes to exactly 0 and 1 through exp2 -> inf -> rcp -> 0.  At positions 20 randn
    the radial terms are in the thousands and the first edge layer's SiLU saturates both ways.  Everything stays finite."""
    st = C.settings(nf, 2, 1, 0)
    model, sd = C.make_model(st, 21, att_gain=64.0)
    n_nodes = [1, 2, 5, 29, 33, 64, 65]
    h0, x = C.batch(n_nodes, 65, 53, 5, True, scale=scale)
    _check(model, sd, st, h0, x, n_nodes, 65, 7, 'egnn saturated nf%d x%g' % (nf, scale), finite=True)


# ---- 6. padding is not read -------------------------------------------------------------------------------------------------------------
def test_padding_atoms_are_never_read():
    """The fixture batch at width 80 with NaN, then +inf, on every padding atom of h0 and x: bit-identical to width 65.  (A kernel that
    read a padded row and multiplied it by zero would pass finite junk and fail here.)  The masks are the correct prefix masks."""
    from test_egnn_gpu import CASES, _case, _inputs
    fx, _, st, model, _ = _case(CASES[0])
    h0, x, n_nodes = _inputs(fx)
    B = h0.shape[0]
    base = call(model, h0, x, n_nodes, h0.shape[1])
    assert bool(torch.isfinite(base).all())
    for junk in (float('nan'), float('inf')):
        h0w, xw = torch.full((B, 80, h0.shape[2]), junk), torch.full((B, 80, 3), junk)
        for b, n in enumerate(n_nodes):
            h0w[b, :n], xw[b, :n] = h0[b, :n], x[b, :n]
        assert not bool(torch.isfinite(h0w[0, n_nodes[0]:]).any()) and not bool(torch.isfinite(xw[-1, n_nodes[-1]:]).any())
        assert torch.equal(call(model, h0w, xw, n_nodes, 80), base), "padding filled with %r" % junk


# ---- 7. plan cache ----------------------------------------------------------------------------------------------------------------------
def test_plan_cache_eviction_reentry_and_alternation():
    """_plan keeps eight plans keyed on (device, B, N, atom counts): ten count lists at one (B, N) evict the first two; an evicted key
    re-enters and two lists alternate with the results of their first call."""
    st = C.settings(64, 1, 1, 0)
    model, _ = C.make_model(st, 59)
    B, N = 4, 12
    lists = [[1 + (k + 3 * b) % N for b in range(B)] for k in range(10)]
    assert len({tuple(n) for n in lists}) == 10
    h0, x = C.batch([N] * B, N, 61, 5, True)
    first = [call(model, h0, x, n, N) for n in lists]
    assert len(model._plans) <= 8
    assert not any(k[3] == torch.tensor(lists[0], dtype=torch.int32).numpy().tobytes() for k in model._plans), "the first plan was not evicted"
    for _ in range(2):
        for k in (0, 9):
            assert torch.equal(call(model, h0, x, lists[k], N), first[k]), "list %d" % k
            assert len(model._plans) <= 8
    assert not torch.equal(first[0], first[1])                # different atom counts, different results: the comparison is not vacuous

"""Python plumbing for the caller-side HIP kernels (csrc/sampler_kernels.hip): the fused ancestral update, the fused DPM-Solver++
update and the fused decode, for the 3-D + edge models and (the *_2d functions) the 2-D ones.  Device tensors in, device tensors out; raises (no CPU fallback) on CPU tensors —
the callers in sampling.py pick the framework path themselves when they run on the CPU (host-logic tests).
"""
import ctypes

import torch

from . import capi
from .utils import _norm_factors


def _f32c(t, name):
    if not t.is_cuda or t.dtype != torch.float32:
        raise TypeError("%s must be a float32 GPU tensor" % name)
    return t if t.is_contiguous() else t.contiguous()


def n_nodes_from_mask(node_mask):
    """int32 [B] atom counts on the mask's device (masks are prefix masks, sampling.py:193-201)."""
    B = node_mask.shape[0]
    return node_mask.reshape(B, -1).sum(1).round().to(torch.int32).contiguous()


class StepBuffers:
    """Ping-pong state buffers of one sampling round (allocated once, reused every step)."""

    def __init__(self, x, edge_x):
        # explicit row-major buffers: empty_like would inherit the permuted strides of the reference's
        # edge-noise expression (z.permute(0, 2, 3, 1) * mask), which the kernels do not follow
        new = lambda t: torch.empty(t.shape, dtype=torch.float32, device=t.device)
        self.x = [new(x), new(x)]
        self.e = [new(edge_x), new(edge_x)]
        self.x_mean = new(x)
        self.e_mean = new(edge_x)
        self.cur = 0


def mix64(*words):
    """splitmix64 finaliser chained over integer words -> one 64-bit value: distinct (seed, rank, round) triples give
    unrelated keys whatever their sizes (no shifting, no truncation: seeds above 2^32 and ranks above 2^16 stay distinct)."""
    M = 0xFFFFFFFFFFFFFFFF
    z = 0x9E3779B97F4A7C15
    for w in words:
        w = int(w)
        while True:                                           # every 64-bit limb of the word, at least one
            z = (z + (w & M) + 0x9E3779B97F4A7C15) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            w >>= 64
            if w <= 0:
                break
    return z


class DeviceNoise:
    """In-kernel normal draws (jodo_sampler_step_rng / jodo_dpm_update_rng, include/jodo_hip.h): Philox4x32-10 keyed by a
    64-bit seed; the draw index counts the updates of a round.  `for_rank` hashes (seed, rank, round) into the key
    (mix64), so the streams of different triples are unrelated."""

    def __init__(self, seed, draw=0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.draw = int(draw)

    @classmethod
    def for_rank(cls, seed, rank=0, round_index=0):
        return cls(mix64(seed, rank, round_index))

    def next_draw(self):
        d = self.draw
        self.draw += 1
        return d


PROP_CONTEXT_TAG = 0x70726F70                                 # 'prop': sampling.py keys a run's context draws by mix64(seed, this)


class PropTables:
    """The property prior's tables on one device (jodo_prop_sample, include/jodo_hip.h), uploaded once from
    DistributionProperty.host_tables(): cum int32 [P, S, K] (the kernel's uint32), minmax f32 [P, S, 2], norm f32 [P, 2].
    `PropTables.uploads` counts the uploads of the process (tests: a second draw from an unchanged prior uploads nothing)."""
    uploads = 0

    def __init__(self, host, device):
        cum, minmax, norm = host['cum'], host['minmax'], host['norm']
        self.n_prop, self.n_slots, self.n_bins = (int(v) for v in cum.shape)
        if cum.dtype != torch.int32 or minmax.shape != (self.n_prop, self.n_slots, 2) or norm.shape != (self.n_prop, 2):
            raise ValueError("PropTables: cum int32 [P,S,K], minmax f32 [P,S,2], norm f32 [P,2]")
        self.device = torch.device(device)
        self.cum = cum.contiguous().to(self.device)
        self.minmax = minmax.to(torch.float32).contiguous().to(self.device)
        self.norm = norm.to(torch.float32).contiguous().to(self.device)
        PropTables.uploads += 1


def prop_sample(tables, slots, seed, first_index=0, indices=None, words=None, out=None):
    """jodo_prop_sample: [B, n_prop] float32 conditioning targets on tables.device, one launch.  slots: CPU int32 [B] table slots (checked
    by the host entry, then uploaded); molecule i has global index indices[i] (CPU integers [B], uploaded as int64) when given, else
    first_index + i.  words (tests): uint32 [B, n_prop, 2] as a CPU or device int32 / int64 tensor, taken instead of Philox's first two
    words.  out: a contiguous float32 [B, n_prop] tensor on the device to write into."""
    if not isinstance(tables, PropTables):
        raise TypeError("prop_sample: tables is a fused.PropTables")
    slots = torch.as_tensor(slots)
    if slots.is_cuda or slots.dtype != torch.int32 or slots.dim() != 1:
        raise TypeError("prop_sample: slots is a CPU int32 [B] tensor")
    slots = slots.contiguous()
    B, P, dev = int(slots.shape[0]), tables.n_prop, tables.device
    if out is None:
        out = torch.empty(B, P, dtype=torch.float32, device=dev)
    elif out.shape != (B, P) or out.device != dev or _f32c(out, 'out') is not out:
        raise ValueError("prop_sample: out is a contiguous float32 [B, n_prop] tensor on the tables' device")
    if B == 0:
        return out
    idx_dev = None
    if indices is not None:
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        if idx.shape[0] != B:
            raise ValueError("prop_sample: %d indices for %d molecules" % (idx.shape[0], B))
        idx_dev = idx.to(dev)
    words_dev = None
    if words is not None:
        words = torch.as_tensor(words)
        if tuple(words.shape) != (B, P, 2):
            raise ValueError("prop_sample: words is [B, n_prop, 2]")
        if words.dtype != torch.int32:                        # uint32 values held in a wider integer: keep the low 32 bits
            w = words.to(torch.int64) & 0xFFFFFFFF
            words = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
        words_dev = words.contiguous().to(dev)
    slots_dev = slots.to(dev)
    with torch.cuda.device(dev):
        capi.check(capi.lib().jodo_prop_sample(
            B, P, tables.n_bins, tables.n_slots, capi.ptr(tables.cum), capi.ptr(tables.minmax), capi.ptr(tables.norm), capi.ptr(slots),
            capi.ptr(slots_dev), capi.ptr(idx_dev), int(first_index) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF,
            capi.ptr(words_dev), capi.ptr(out), capi.current_stream_ptr()), 'jodo_prop_sample')
    # slots_dev / idx_dev / words_dev were allocated and are read on the current stream: the caching allocator hands their memory out
    # again only to work queued behind this launch
    return out


def split_replayed_noise(node_noise, edge_noise):
    """Recorded reference noise (node [B,N,3+nd] masked + CoM-free, edge [B,N,N,ch] symmetric + masked) as the RAW draws the
    kernels take: masking, centre-of-mass removal and lower-triangle mirroring are idempotent on them."""
    return (node_noise[:, :, :3].contiguous(), node_noise[:, :, 3:].contiguous(),
            edge_noise.permute(0, 3, 1, 2).contiguous())


def sampler_step(bufs, n_nodes_dev, c_x, c_pred, sigma, x, edge_x, pred, edge_pred, eps_pos=None, eps_feat=None, eps_edge=None,
                 rng=None):
    """x_mean = c_x x + c_pred pred; x_next = x_mean + sigma * eps (both tensors), eps from RAW normal draws
    in the reference's shapes (see include/jodo_hip.h) or, with rng = DeviceNoise, drawn inside the kernel.
    Returns (x_next, edge_next, x_mean, edge_mean); the returned tensors live in `bufs` and stay valid until the
    call after next."""
    B, N, F = x.shape
    ch = edge_x.shape[-1]
    x, edge_x = _f32c(x, 'x'), _f32c(edge_x, 'edge_x')
    pred, edge_pred = _f32c(pred, 'pred'), _f32c(edge_pred, 'edge_pred')
    nxt = bufs.cur ^ 1
    xn, en = bufs.x[nxt], bufs.e[nxt]
    if xn.data_ptr() == x.data_ptr() or en.data_ptr() == edge_x.data_ptr():
        raise RuntimeError("sampler_step: output buffer aliases the input state")
    cf = lambda v: ctypes.c_float(float(v))
    if rng is not None:
        capi.check(capi.lib().jodo_sampler_step_rng(
            B, N, F, ch, capi.ptr(n_nodes_dev), cf(c_x), cf(c_pred), cf(sigma), None, None, ctypes.c_uint64(rng.seed),
            ctypes.c_uint32(rng.next_draw()), capi.ptr(x), capi.ptr(edge_x), capi.ptr(pred), capi.ptr(edge_pred), capi.ptr(xn),
            capi.ptr(en), capi.ptr(bufs.x_mean), capi.ptr(bufs.e_mean), capi.current_stream_ptr()), 'jodo_sampler_step_rng')
    else:
        eps_pos, eps_feat, eps_edge = _f32c(eps_pos, 'eps_pos'), _f32c(eps_feat, 'eps_feat'), _f32c(eps_edge, 'eps_edge')
        if eps_pos.shape != (B, N, 3) or eps_feat.shape != (B, N, F - 3) or eps_edge.shape != (B, ch, N, N):
            raise ValueError("noise draws must have the reference's shapes [B,N,3], [B,N,nd], [B,ch,N,N]")
        capi.check(capi.lib().jodo_sampler_step(
            B, N, F, ch, capi.ptr(n_nodes_dev), cf(c_x), cf(c_pred), cf(sigma), capi.ptr(x), capi.ptr(edge_x), capi.ptr(pred),
            capi.ptr(edge_pred), capi.ptr(eps_pos), capi.ptr(eps_feat), capi.ptr(eps_edge), capi.ptr(xn), capi.ptr(en),
            capi.ptr(bufs.x_mean), capi.ptr(bufs.e_mean), capi.current_stream_ptr()), 'jodo_sampler_step')
    bufs.cur = nxt
    return xn, en, bufs.x_mean, bufs.e_mean


def sampler_step_2d(n_nodes_dev, c_x, c_pred, sigma, x, edge_x, pred, edge_pred, eps_node, eps_edge):
    """The 2-D sampler's ancestral update as one kernel (jodo_sampler_step_2d): no position channels, node noise masked to the
    real atoms, edge noise [B,N,N,ch] read from its strict lower triangle for both orientations of a pair.
    Returns (x_next, edge_next, x_mean, edge_mean), freshly allocated."""
    x, edge_x, pred, edge_pred = _f32c(x, 'x'), _f32c(edge_x, 'edge_x'), _f32c(pred, 'pred'), _f32c(edge_pred, 'edge_pred')
    eps_node, eps_edge = _f32c(eps_node, 'eps_node'), _f32c(eps_edge, 'eps_edge')
    B, N, nd = x.shape
    ch = edge_x.shape[-1]
    if edge_x.shape != (B, N, N, ch) or eps_edge.shape != edge_x.shape or eps_node.shape != x.shape or pred.shape != x.shape \
            or edge_pred.shape != edge_x.shape:
        raise ValueError("sampler_step_2d: shape mismatch")
    new = lambda t: torch.empty(t.shape, dtype=torch.float32, device=t.device)
    x_next, e_next, x_mean, e_mean = new(x), new(edge_x), new(x), new(edge_x)
    capi.check(capi.lib().jodo_sampler_step_2d(B, N, nd, ch, capi.ptr(n_nodes_dev), ctypes.c_float(c_x), ctypes.c_float(c_pred),
                                               ctypes.c_float(sigma), capi.ptr(x), capi.ptr(edge_x), capi.ptr(pred), capi.ptr(edge_pred),
                                               capi.ptr(eps_node), capi.ptr(eps_edge), capi.ptr(x_next), capi.ptr(e_next), capi.ptr(x_mean),
                                               capi.ptr(e_mean), capi.current_stream_ptr()), 'jodo_sampler_step_2d')
    return x_next, e_next, x_mean, e_mean


def sampler_step_2d_rng(bufs, n_nodes_dev, c_x, c_pred, sigma, x, edge_x, pred, edge_pred, rng):
    """The 2-D ancestral update with both draws generated inside the kernel (jodo_sampler_step_2d_rng, host-scalar form; rng = DeviceNoise,
    one draw index per call) on the ping-pong `bufs` (StepBuffers): nothing is allocated per step.  Returns (x_next, edge_next, x_mean,
    edge_mean); the returned tensors live in `bufs` and stay valid until the call after next."""
    x, edge_x, pred, edge_pred = _f32c(x, 'x'), _f32c(edge_x, 'edge_x'), _f32c(pred, 'pred'), _f32c(edge_pred, 'edge_pred')
    B, N, nd = x.shape
    ch = edge_x.shape[-1]
    if edge_x.shape != (B, N, N, ch) or pred.shape != x.shape or edge_pred.shape != edge_x.shape or bufs.x[0].shape != x.shape \
            or bufs.e[0].shape != edge_x.shape:
        raise ValueError("sampler_step_2d_rng: shape mismatch")
    nxt = bufs.cur ^ 1
    xn, en = bufs.x[nxt], bufs.e[nxt]
    if xn.data_ptr() == x.data_ptr() or en.data_ptr() == edge_x.data_ptr():
        raise RuntimeError("sampler_step_2d_rng: output buffer aliases the input state")
    capi.check(capi.lib().jodo_sampler_step_2d_rng(
        B, N, nd, ch, capi.ptr(n_nodes_dev), float(c_x), float(c_pred), float(sigma), None, None, rng.seed, rng.next_draw(),
        capi.ptr(x), capi.ptr(edge_x), capi.ptr(pred), capi.ptr(edge_pred), capi.ptr(xn), capi.ptr(en), capi.ptr(bufs.x_mean),
        capi.ptr(bufs.e_mean), capi.current_stream_ptr()), 'jodo_sampler_step_2d_rng')
    bufs.cur = nxt
    return xn, en, bufs.x_mean, bufs.e_mean


def decode(config, xh, edge_x, n_nodes_dev):
    """post_process + inverse scaling on the device.  Returns compact device tensors
    (pos f32 [B,N,3], atom_type u8 [B,N], fc i8 [B,N], edge_type u8 [B,N,N])."""
    xh, edge_x = _f32c(xh, 'xh'), _f32c(edge_x, 'edge_x')
    B, N, F = xh.shape
    atom_types = int(config.data.atom_types)
    include_fc = int(bool(config.model.include_fc_charge))
    if F != 3 + atom_types + include_fc:
        raise ValueError("xh has %d features, config says %d" % (F, 3 + atom_types + include_fc))
    nf = _norm_factors(config)
    edge_norm = nf[3] if len(nf) > 3 else 1
    dev = xh.device
    pos = torch.empty(B, N, 3, device=dev)
    at = torch.empty(B, N, dtype=torch.uint8, device=dev)
    fc = torch.empty(B, N, dtype=torch.int8, device=dev)
    et = torch.empty(B, N, N, dtype=torch.uint8, device=dev)
    capi.check(capi.lib().jodo_decode(
        B, N, atom_types, include_fc, int(edge_x.shape[-1]), int(bool(config.data.compress_edge)),
        int(bool(config.data.centered)), ctypes.c_float(float(nf[0])), ctypes.c_float(float(nf[1])),
        ctypes.c_float(float(nf[2])), ctypes.c_float(float(edge_norm)), capi.ptr(n_nodes_dev), capi.ptr(xh),
        capi.ptr(edge_x), capi.ptr(pos), capi.ptr(at), capi.ptr(fc), capi.ptr(et), capi.current_stream_ptr()),
        'jodo_decode')
    return pos, at, fc, et


def mols_from_decoded(pos, at, fc, et, n_nodes):
    """One device->host copy per tensor, then per-molecule views in the reference's tuple format
    (pos[n,3] f32, atom_type[n] i64, edge_type[n,n] f32, fc[n] i64) — sampling.py:12-32."""
    pos, at, fc, et = pos.cpu(), at.cpu().long(), fc.cpu().long(), et.cpu().float()
    mols = []
    for i, n in enumerate(n_nodes):
        n = int(n)
        mols.append((pos[i, :n], at[i, :n], et[i, :n, :n], fc[i, :n]))
    return mols


def decode_2d(config, xh, edge_x, n_nodes_dev):
    """post_process_2D + inverse scaling on the device (jodo_decode_2d).  Returns compact device tensors
    (atom_type u8 [B,N], fc i8 [B,N] — zeros when the config has no charge channel —, edge_type u8 [B,N,N])."""
    xh, edge_x = _f32c(xh, 'xh'), _f32c(edge_x, 'edge_x')
    B, N, F = xh.shape
    atom_types = int(config.data.atom_types)
    include_fc = int(bool(config.model.include_fc_charge))
    if F != atom_types + include_fc or edge_x.shape[:3] != (B, N, N):
        raise ValueError("xh has %d features, config says %d (edge_x %s)" % (F, atom_types + include_fc, tuple(edge_x.shape)))
    nf = _norm_factors(config)
    edge_norm = nf[3] if len(nf) > 3 else 1
    dev = xh.device
    at = torch.empty(B, N, dtype=torch.uint8, device=dev)
    fc = torch.empty(B, N, dtype=torch.int8, device=dev)
    et = torch.empty(B, N, N, dtype=torch.uint8, device=dev)
    capi.check(capi.lib().jodo_decode_2d(
        B, N, atom_types, include_fc, int(edge_x.shape[-1]), int(bool(config.data.compress_edge)), int(bool(config.data.centered)),
        float(nf[1]), float(nf[2]), float(edge_norm), capi.ptr(n_nodes_dev), capi.ptr(xh), capi.ptr(edge_x), capi.ptr(at), capi.ptr(fc),
        capi.ptr(et), capi.current_stream_ptr()), 'jodo_decode_2d')
    return at, fc, et


def mols_from_decoded_2d(at, fc, et, n_nodes, include_fc=True):
    """One device->host copy per tensor, then per-molecule views in mol_process_2D's tuple format (None, atom_type[n] i64,
    edge_type[n,n] f32, fc[n] i64) — sampling.py:35-50; without a charge channel fc is mol_process_2D's empty-charge form, a float32
    [n, 0] (what post_process_2D makes of the empty charge tensor)."""
    at, fc, et = at.cpu().long(), fc.cpu().long(), et.cpu().float()
    mols = []
    for i, n in enumerate(n_nodes):
        n = int(n)
        mols.append((None, at[i, :n], et[i, :n, :n], fc[i, :n] if include_fc else torch.zeros(n, 0)))
    return mols


class _DpmBuffers:
    """Output buffers of the fused solver updates: a small ring, so that an update never writes a tensor that the
    solver still holds (state at the start of the outer step, intermediate states, the previous output)."""

    def __init__(self, x, edge_x, depth=4):
        new = lambda t: torch.empty(t.shape, dtype=torch.float32, device=t.device)
        self.x = [new(x) for _ in range(depth)]
        self.e = [new(edge_x) for _ in range(depth)]
        self.eps = torch.empty(x.shape[0], x.shape[1], 3, dtype=torch.float32, device=x.device)
        self.cur = 0


def dpm_update(solver, coef, x_pos, x_base, edge_base, P, DA, DB, PP, n_nodes_dev, eps=None, rng=None):
    """jodo_dpm_update (include/jodo_hip.h): coef = [cx, cp, sigma, a, b, c, c2, 0]; P / DA / DB / PP are
    (node prediction, edge prediction) pairs; n_nodes_dev = int32 [B] atom counts of THIS round (the solver computes them
    once per `sampling` call).  Position noise: `eps` (a replayed draw [B,N,3]; masking / CoM removal are idempotent),
    in-kernel draws with rng = DeviceNoise, otherwise a raw N(0,1) [B,N,3] draw (the reference's shape and draw,
    mix_dpm_solver.py:56); nothing is drawn when sigma == 0 (last update of a round).  Returns (x_out, edge_out)."""
    B, N, F = x_base.shape
    ch = edge_base.shape[-1]
    if n_nodes_dev.shape[0] != B or n_nodes_dev.device != x_base.device:
        raise ValueError("dpm_update: n_nodes_dev does not belong to this batch")
    bufs = getattr(solver, '_dpm_bufs', None)
    if bufs is None or bufs.x[0].shape != x_base.shape or bufs.e[0].shape != edge_base.shape or bufs.x[0].device != x_base.device:
        bufs = solver._dpm_bufs = _DpmBuffers(x_base, edge_base)
    live = {t.data_ptr() for t in (x_pos, x_base, edge_base, P[0], P[1], DA[0], DA[1], DB[0], DB[1], PP[0])}
    for _ in range(len(bufs.x)):
        bufs.cur = (bufs.cur + 1) % len(bufs.x)
        if bufs.x[bufs.cur].data_ptr() not in live and bufs.e[bufs.cur].data_ptr() not in live:
            break
    else:
        raise RuntimeError("dpm_update: no free output buffer")
    xo, eo = bufs.x[bufs.cur], bufs.e[bufs.cur]
    if rng is None:
        if eps is not None:
            bufs.eps.copy_(eps)
        elif coef[2] != 0.0:
            bufs.eps.normal_()
    c8 = (ctypes.c_float * 8)(*coef)
    # contiguous fp32 views are bound to names until the launch is enqueued: a temporary freed earlier could be handed
    # out again by the caching allocator for the next temporary and be overwritten before the kernel reads it
    t = [_f32c(v, n) for v, n in ((x_pos, 'x_pos'), (x_base, 'x_base'), (edge_base, 'edge_base'), (P[0], 'P'), (P[1], 'eP'),
                                  (DA[0], 'DA'), (DA[1], 'eDA'), (DB[0], 'DB'), (DB[1], 'eDB'), (PP[0], 'PP'))]
    if rng is not None:
        draw = rng.next_draw() if coef[2] != 0.0 else 0
        capi.check(capi.lib().jodo_dpm_update_rng(
            B, N, F, ch, capi.ptr(n_nodes_dev), c8, None, None, 0, 0, ctypes.c_uint64(rng.seed), ctypes.c_uint32(draw),
            ctypes.c_uint32(0), *[capi.ptr(v) for v in t], capi.ptr(xo), capi.ptr(eo), capi.current_stream_ptr()),
            'jodo_dpm_update_rng')
    else:
        capi.check(capi.lib().jodo_dpm_update(
            B, N, F, ch, capi.ptr(n_nodes_dev), c8, None, None, 0, 0, *[capi.ptr(v) for v in t],
            capi.ptr(bufs.eps), capi.ptr(xo), capi.ptr(eo), capi.current_stream_ptr()), 'jodo_dpm_update')
    del t
    return xo, eo


class _DpmBuffers2D:
    """_DpmBuffers for the 2-D solver: the same ring of output buffers, no position-noise buffer (nothing is drawn)."""

    def __init__(self, x, edge_x, depth=4):
        new = lambda t: torch.empty(t.shape, dtype=torch.float32, device=t.device)
        self.x = [new(x) for _ in range(depth)]
        self.e = [new(edge_x) for _ in range(depth)]
        self.cur = 0


def dpm_update_2d(solver, coef, x_base, edge_base, P, DA, DB, n_nodes_dev):
    """jodo_dpm_update_2d (include/jodo_hip.h) in its host-scalar form: coef = [a, b, c, c2, 0, 0, 0, 0]; P / DA / DB are (node prediction,
    edge prediction) pairs; node tensors [B,N,nd] without position channels, edge tensors [B,N,N,ch]; n_nodes_dev = int32 [B] atom counts
    of THIS round.  The outputs come from a ring on `solver` (never a tensor the call reads) and are symmetric, with zero padding and
    diagonal, whatever the inputs hold there.  Returns (x_out, edge_out)."""
    if x_base.dim() != 3 or edge_base.dim() != 4:
        raise ValueError("dpm_update_2d: node tensors are [B,N,nd], edge tensors [B,N,N,ch]")
    B, N, nd = x_base.shape
    ch = edge_base.shape[-1]
    if edge_base.shape != (B, N, N, ch) or any(t[0].shape != x_base.shape or t[1].shape != edge_base.shape for t in (P, DA, DB)):
        raise ValueError("dpm_update_2d: shape mismatch")
    if len(coef) != 8:
        raise ValueError("dpm_update_2d: coef holds 8 floats [a, b, c, c2, 0, 0, 0, noise_level]")
    if n_nodes_dev.shape[0] != B or n_nodes_dev.device != x_base.device or n_nodes_dev.dtype != torch.int32:
        raise ValueError("dpm_update_2d: n_nodes_dev does not belong to this batch")
    bufs = getattr(solver, '_dpm_bufs', None)
    if bufs is None or bufs.x[0].shape != x_base.shape or bufs.e[0].shape != edge_base.shape or bufs.x[0].device != x_base.device:
        bufs = solver._dpm_bufs = _DpmBuffers2D(x_base, edge_base)
    live = {t.data_ptr() for t in (x_base, edge_base, P[0], P[1], DA[0], DA[1], DB[0], DB[1])}
    for _ in range(len(bufs.x)):
        bufs.cur = (bufs.cur + 1) % len(bufs.x)
        if bufs.x[bufs.cur].data_ptr() not in live and bufs.e[bufs.cur].data_ptr() not in live:
            break
    else:
        raise RuntimeError("dpm_update_2d: no free output buffer")
    xo, eo = bufs.x[bufs.cur], bufs.e[bufs.cur]
    c8 = (ctypes.c_float * 8)(*coef)
    # contiguous fp32 views stay bound to names until the launch is enqueued (see dpm_update)
    t = [_f32c(v, n) for v, n in ((x_base, 'x_base'), (edge_base, 'edge_base'), (P[0], 'P'), (P[1], 'eP'), (DA[0], 'DA'), (DA[1], 'eDA'),
                                  (DB[0], 'DB'), (DB[1], 'eDB'))]
    capi.check(capi.lib().jodo_dpm_update_2d(B, N, nd, ch, capi.ptr(n_nodes_dev), c8, None, None, 0, 0, *[capi.ptr(v) for v in t],
                                             capi.ptr(xo), capi.ptr(eo), capi.current_stream_ptr()), 'jodo_dpm_update_2d')
    del t
    return xo, eo


class _DataBuffers2D:
    """Output buffers of eps_to_data_2d: a ring of data predictions.  The solver holds at most three at a time (single-step order 3:
    the predictions at t, s1 and s2 of one outer step; multistep order 2: the newest and the one before), so with depth 4 a conversion
    never writes a prediction that an update still reads."""

    def __init__(self, x, edge_x, depth=4):
        new = lambda t: torch.empty(t.shape, dtype=torch.float32, device=t.device)
        self.x = [new(x) for _ in range(depth)]
        self.e = [new(edge_x) for _ in range(depth)]
        self.cur = 0


def eps_to_data_2d(solver, alpha, sigma, x, edge_x, eps_x, eps_e, n_nodes_dev, out=None):
    """jodo_eps_to_data_2d (include/jodo_hip.h) in its host-scalar form: d = (x - sigma * eps) / alpha on the node tensor [B,N,nd] and the
    edge tensor [B,N,N,ch], the noise prediction of a 2-D network turned into the data prediction that DPM-Solver++ updates.  alpha / sigma
    are floats; n_nodes_dev = int32 [B] atom counts of THIS round.  The outputs come from a ring of their own on `solver` (_DataBuffers2D),
    or are `out` = (d_x, d_e), which may be the (x, edge_x) or (eps_x, eps_e) pair itself; they are symmetric, with zero padding and
    diagonal, whatever the inputs hold there.  Returns (d_x, d_e)."""
    if x.dim() != 3 or edge_x.dim() != 4:
        raise ValueError("eps_to_data_2d: node tensors are [B,N,nd], edge tensors [B,N,N,ch]")
    B, N, nd = x.shape
    ch = edge_x.shape[-1]
    if edge_x.shape != (B, N, N, ch) or eps_x.shape != x.shape or eps_e.shape != edge_x.shape:
        raise ValueError("eps_to_data_2d: shape mismatch")
    if n_nodes_dev.shape[0] != B or n_nodes_dev.device != x.device or n_nodes_dev.dtype != torch.int32:
        raise ValueError("eps_to_data_2d: n_nodes_dev does not belong to this batch")
    # contiguous fp32 views stay bound to names until the launch is enqueued (see dpm_update)
    t = [_f32c(v, n) for v, n in ((x, 'x'), (edge_x, 'edge_x'), (eps_x, 'eps_x'), (eps_e, 'eps_e'))]
    if out is None:
        bufs = getattr(solver, '_data_bufs', None)
        if bufs is None or bufs.x[0].shape != x.shape or bufs.e[0].shape != edge_x.shape or bufs.x[0].device != x.device:
            bufs = solver._data_bufs = _DataBuffers2D(x, edge_x)
        bufs.cur = (bufs.cur + 1) % len(bufs.x)
        dx, de = bufs.x[bufs.cur], bufs.e[bufs.cur]
    else:
        dx, de = out
        if dx.shape != x.shape or de.shape != edge_x.shape or _f32c(dx, 'd_x') is not dx or _f32c(de, 'd_e') is not de:
            raise ValueError("eps_to_data_2d: out = (d_x, d_e), contiguous float32 GPU tensors of the inputs' shapes")
    capi.check(capi.lib().jodo_eps_to_data_2d(B, N, nd, ch, capi.ptr(n_nodes_dev), float(alpha), float(sigma), None, None, 0, 0,
                                              *[capi.ptr(v) for v in t], capi.ptr(dx), capi.ptr(de), capi.current_stream_ptr()),
               'jodo_eps_to_data_2d')
    del t
    return dx, de

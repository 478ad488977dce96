"""MI355X-native Diffusion Graph Transformer score networks, registered under the reference's names.

`DGT_concat` / `Cond_DGT_concat` / `DGT_concat_sim` are drop-in replacements for the classes of the same registry name
in /root/reference/models/mol_gnn.py (:410-594, :597-794, :949-1124):

  * same constructor argument (`config`) and the same config keys are read;
  * same parameter names, shapes and registration order (state_dict keys, EMA shadow-list order,
    `strict=True` checkpoint loading) — the parameter tree below is built from stock torch containers
    in the reference's construction order, so even `torch.manual_seed(s); Model(config)` yields the
    same initial weights;
  * same call: `model(t, xh, node_mask, edge_mask, context=None, edge_x=..., cond_x=..., cond_edge_x=...,
    noise_level=...)` -> `(xh_pred [B,N,3+nd], edge_pred [B,N,N,ch])`, inputs untouched.

The arithmetic is NOT done by these torch modules: `forward` packs the weights once (MFMA operand
order, csrc/dgt_pack.cpp), builds a plan per batch of atom counts, and calls
`jodo_dgt_forward` in libjodo_hip.so on the current HIP stream.  There is no CPU or eager fallback:
on a non-GPU tensor, with an unsupported config, or — DGT_concat_sim without its `hip_training` opt-in — with gradients enabled,
forward raises; a grad-enabled call otherwise runs the HIP training path (csrc/dgt_train.hip, jodo_amd/train.py).
"""
import ctypes

import torch
from torch import nn

from .. import capi
from .dims import ModelDims
from . import utils
from ._runtime import HostRuntime


# ---------------------------------------------------------------------------------------------
# parameter containers (hold weights only; mirror the reference's module tree)
# ---------------------------------------------------------------------------------------------
def _time_seq(time_dim, out_dim):
    return nn.Sequential(nn.SiLU(), nn.Linear(time_dim, out_dim))


class _SinusoidParams(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.weights = nn.Parameter(torch.randn(dim // 2))


class _GaussianParams(nn.Module):
    def __init__(self, K, time_dim):
        super().__init__()
        self.means = nn.Embedding(1, K - 1)
        self.stds = nn.Embedding(1, K - 1)
        self.time_mlp = _time_seq(time_dim, 2)
        nn.init.uniform_(self.means.weight, 0, 3)
        nn.init.uniform_(self.stds.weight, 0, 3)


class _CoorsNormParams(nn.Module):
    def __init__(self, scale_init):
        super().__init__()
        self.scale = nn.Parameter(torch.zeros(1).fill_(scale_init))


class _AttnParams(nn.Module):
    def __init__(self, node_dim, head_ch, n_extra, n_heads, edge_dim):
        super().__init__()
        sub_heads = n_heads - n_extra
        sub_ch = (n_heads * head_ch) // sub_heads
        self.lin_key = nn.Linear(node_dim, sub_heads * sub_ch)
        self.lin_query = nn.Linear(node_dim, sub_heads * sub_ch)
        self.lin_value = nn.Linear(node_dim, n_heads * head_ch)
        self.lin_edge0 = nn.Linear(edge_dim, sub_heads * sub_ch, bias=False)
        self.lin_edge1 = nn.Linear(edge_dim, n_heads * head_ch, bias=False)
        for m in (self.lin_key, self.lin_query, self.lin_value, self.lin_edge0, self.lin_edge1):
            m.reset_parameters()          # the reference layer re-initialises after construction


class _EquiUpdateParams(nn.Module):
    def __init__(self, hidden, edge_dim, dist_dim, time_dim, n_extra):
        super().__init__()
        self.coord_norm = _CoorsNormParams(1e-2)
        self.time_mlp = _time_seq(time_dim, hidden * 2)
        self.input_lin = nn.Linear(hidden * 2 + edge_dim + dist_dim, hidden)
        self.coord_mlp = nn.Sequential(nn.Linear(hidden, hidden), nn.SiLU(), nn.Linear(hidden, 1 + n_extra, bias=False))


class _BlockParams(nn.Module):
    def __init__(self, node_dim, edge_dim, time_dim, n_extra, n_heads, mlp_ratio):
        super().__init__()
        self.edge_emb = nn.Linear(edge_dim * 2, edge_dim)
        self.node2edge_lin = nn.Linear(node_dim, edge_dim)
        self.attn_mpnn = _AttnParams(node_dim, node_dim // n_heads, n_extra, n_heads, edge_dim)
        self.ff_linear1 = nn.Linear(node_dim, node_dim * mlp_ratio)
        self.ff_linear2 = nn.Linear(node_dim * mlp_ratio, node_dim)
        self.ff_linear3 = nn.Linear(edge_dim, edge_dim * mlp_ratio)
        self.ff_linear4 = nn.Linear(edge_dim * mlp_ratio, edge_dim)
        self.equi_update = _EquiUpdateParams(node_dim, edge_dim, edge_dim, time_dim, n_extra)
        self.node_time_mlp = _time_seq(time_dim, node_dim * 6)
        self.edge_time_mlp = _time_seq(time_dim, edge_dim * 6)
        self.dist_layer = _GaussianParams(edge_dim, time_dim)


def _mlp3(i, h, m, o):
    return nn.Sequential(nn.Linear(i, h), nn.SiLU(), nn.Linear(h, m), nn.SiLU(), nn.Linear(m, o))


_UNSUPPORTED = (('dist_gbf', True), ('cond_time', True), ('pred_data', True), ('gbf_name', 'CondGaussianLayer'),
                ('CoM', True), ('softmax_inf', True))


class _DGTBase(HostRuntime, nn.Module):
    conditional = False
    extra_heads = None                # None: config.model.n_extra_heads (2); 0: the class never reads the key (DGT_concat_sim)
    _derived = ('_split_tape',)       # (pack generation, device uint8 tensor): the split form's static weight tape

    def __init__(self, config):
        super().__init__()
        m = config.model
        sim = self.extra_heads is not None        # no adjacency heads: softmax_inf, trans_name, n_extra_heads, edge_quan_th are never read
        for key, want in _UNSUPPORTED:
            if sim and key == 'softmax_inf':
                continue
            if getattr(m, key) != want:
                raise NotImplementedError(
                    "config.model.%s=%r: the HIP path implements %r only (the JODO configs' setting)"
                    % (key, getattr(m, key), want))
        if not self.conditional and not sim and getattr(m, 'trans_name', 'TransMixLayer') != 'TransMixLayer':
            raise NotImplementedError("config.model.trans_name=%r: only TransMixLayer is implemented" % m.trans_name)
        in_node_dim = config.data.atom_types + int(m.include_fc_charge)
        D, De, L = m.nf, m.nf // 4, m.n_layers
        T = D * 4
        cond_ch = int(m.cond_ch) if self.conditional else 0
        n_extra = self.extra_heads if sim else m.n_extra_heads
        if D not in (128, 256, 384) or m.n_heads != 16 or n_extra != (0 if sim else 2) or m.mlp_ratio not in (2, 4):
            raise NotImplementedError("HIP kernels are built for nf in {128, 256, 384}, n_heads=16, n_extra_heads=2, "
                                      "mlp_ratio in {2,4} (got nf=%d heads=%d/%d ratio=%d)" %
                                      (D, m.n_heads, n_extra, m.mlp_ratio))
        # kernel_layout (not a reference key): 'wide' runs the width-generic kernel set at nf=256 too (tests)
        wide = getattr(m, 'kernel_layout', 'auto') == 'wide'
        self.dims = ModelDims(D, L, m.n_heads, n_extra, m.mlp_ratio, in_node_dim, m.edge_ch, cond_ch, wide=wide)
        if n_extra == 0 and self.dims.wide:
            raise NotImplementedError("DGT_concat_sim at nf=%d, n_layers=%d, kernel_layout=%r: the kernels without adjacency heads are built "
                                      "for the tuned nf=256 set only (nf=256, n_layers >= 8, the default layout)"
                                      % (D, L, getattr(m, 'kernel_layout', 'auto')))
        if self.dims.cep > 32 or self.dims.KEH % 32 or not 3 <= self.dims.KEH // 32 <= 15 or self.dims.KEH // 32 == 14 or L > 16:
            raise NotImplementedError("n_layers=%d at nf=%d: the edge head input (De + n_layers x %d = %d) must be a multiple of 32 in "
                                      "[96, 480] and the per-block edge readout (%d) at most 32 wide" %
                                      (L, D, self.dims.cep, self.dims.KEH, self.dims.ce))
        # (without adjacency heads both thresholds only feed an adjacency nobody reads: constants, so that the keys have no effect)
        self.edge_th = 0.0 if sim else float(m.edge_quan_th)
        self.spatial_cut_off = 0.0 if sim else float(m.spatial_cut_off)
        self.n_layers = L
        self.dropout_p = m.dropout           # identity at inference; kept for config parity

        # ---- parameter tree, reference construction/registration order ----
        self.node_emb = nn.Linear(in_node_dim * 2, D)
        self.edge_emb = nn.Linear(m.edge_ch * 2 + De, De)
        self.dist_layer = _GaussianParams(De, T)
        cat_node, cat_edge = (D * 2) // L, (De * 2) // L
        for i in range(L):
            self.add_module("e_block_%d" % i, _BlockParams(D, De, T, n_extra, m.n_heads, m.mlp_ratio))
            self.add_module("node_%d" % i, nn.Linear(D, cat_node))
            self.add_module("edge_%d" % i, nn.Linear(De, cat_edge))
        self.node_pred_mlp = _mlp3(cat_node * L + D, D, D // 2, in_node_dim)
        self.edge_type_mlp = _mlp3(cat_edge * L + De, De, De // 2, m.edge_ch - 1)
        self.edge_exist_mlp = _mlp3(cat_edge * L + De, De, De // 2, 1)
        self.time_mlp = nn.Sequential(_SinusoidParams(16), nn.Linear(17, T), nn.GELU(), nn.Linear(T, T))
        if self.conditional:
            self.cond_mlp = nn.Sequential(nn.Linear(1, D), nn.GELU(), nn.Linear(D, D))
            self.cond_lin = nn.Linear(cond_ch * D, T)

        # ---- runtime state (not part of state_dict) ----
        self._init_runtime()          # _packed, _plans (plan cache keyed by the mask storage, see _plan), _split_tape
        self._pack_gen = 0            # pack generation: +1 on every re-pack of the blob (the split tape and the plans' tapes key on it)
        self._splits = {}             # sub-batch splits of n_streams > 1, keyed likewise (node and edge mask storage, k), see _split_of
        self.n_streams = 1            # > 1: sub-batches evaluated concurrently on that many HIP streams (_forward_split)
        self._cfg_struct = None
        self.last_flags = None        # device int32[8] of the last call (NaN guard etc.)
        self.warn_nan = True
        # OPT-IN (default off): under pinned paths (pin_paths: what the samplers do after a round's first self-conditioned evaluation)
        # the pair update runs its projections in the split-bf16 form — three bf16 terms per operand, six bf16 MFMAs per K = 16
        # step, fp32 accumulation: fp32-equivalent arithmetic, not bit-identical to the default (csrc/dgt_kernels_split.h,
        # JODO_OPT_SPLIT_BF16).  Unconditional models: nf 256 (folded pair update + node kernel) and nf 384 (folded pair update) under a
        # shared noise level.  The conditional model at nf 256: the un-folded pair update (csrc/dgt_kernels_split_cond.h; per-molecule
        # noise levels allowed).  Ignored elsewhere (nf 128, asymmetric inputs).  The default path and every headline number stay exact fp32.
        self.split_bf16 = False       # True: pair update + node kernel; 'attention': also the attention kernel (experiments: measured slower)

    # -- C structs ---------------------------------------------------------------------------
    class _Cfg(ctypes.Structure):
        _fields_ = [('nf', ctypes.c_int32), ('n_layers', ctypes.c_int32), ('n_heads', ctypes.c_int32),
                    ('n_extra', ctypes.c_int32), ('mlp_ratio', ctypes.c_int32), ('in_node_dim', ctypes.c_int32),
                    ('edge_ch', ctypes.c_int32), ('cond_ch', ctypes.c_int32),
                    ('spatial_cut_off', ctypes.c_float), ('edge_quan_th', ctypes.c_float), ('layout', ctypes.c_int32)]

    def _cfg(self):
        if self._cfg_struct is None:
            d = self.dims
            self._cfg_struct = self._Cfg(d.D, d.L, d.H, d.XH, d.r, d.nd, d.ch, d.cond_ch, self.spatial_cut_off,
                                         self.edge_th, 1 if d.wide else 0)
        return self._cfg_struct

    # -- weights (cache, fingerprint and invalidation: _runtime.HostRuntime) ---------------------------
    def _pack(self, device):
        # C-side packer (csrc/dgt_pack.cpp, jodo_dgt_pack_weights): the state_dict goes through the C ABI as named
        # fp32 tensors; tests/py_packing_model.py is an independent Python packer kept for tests (blob equality)
        return capi.pack_weights(self._cfg(), self.state_dict(), device)

    def _repacked(self, device, blob):
        # a `.data` write re-packs under the SAME key (versions and addresses unchanged): what follows the blob — the split tape and
        # the tape handed to each pinned plan — compares this generation, not the key
        self._pack_gen += 1

    # -- plans ---------------------------------------------------------------------------------
    def _plan(self, node_mask, edge_mask, device, validate=True):
        destroy = lambda plan: capi.lib().jodo_plan_destroy(plan['handle'])
        return self._cached_plan(node_mask, edge_mask, validate, lambda n_host, B, N: self._build_plan(n_host, B, N, device), destroy)

    def _build_plan(self, n_host, B, N, device):
        L = capi.lib()
        handle = ctypes.c_void_p()
        capi.check(L.jodo_plan_create(ctypes.byref(self._cfg()), B, N, n_host.ctypes.data_as(ctypes.c_void_p),
                                      int(getattr(self, 'max_chunk', 0)) | (int(getattr(self, 'pair_chunk', 0)) << 16)
                                      | (int(getattr(self, 'spair_chunk', 0)) << 24),
                                      ctypes.byref(handle)), 'jodo_plan_create')
        L.jodo_plan_desc_bytes.restype = ctypes.c_size_t
        L.jodo_plan_workspace_bytes.restype = ctypes.c_size_t
        desc = torch.empty(L.jodo_plan_desc_bytes(handle), dtype=torch.uint8, device=device)
        # zero-filled once: rows the kernels never write (diagonal edge rows of the two edge-state copies on the pair path) must stay
        # FINITE; their values do not matter (include/jodo_hip.h, jodo_dgt_forward; tests/test_forms_gpu.py runs on poisoned scratch)
        ws = torch.zeros(L.jodo_plan_workspace_bytes(handle), dtype=torch.uint8, device=device)
        if getattr(self, 'force_directed', False):       # tests: never use the symmetric pair kernels
            capi.check(L.jodo_debug_set_force_directed(handle, 1), 'jodo_debug_set_force_directed')
        for opt, val in getattr(self, 'plan_options', {}).items():     # {jodo_plan_option: value}, experiments only
            capi.check(L.jodo_plan_set_option(handle, int(opt), int(val)), 'jodo_plan_set_option')
        capi.check(L.jodo_plan_upload(handle, capi.ptr(desc), capi.current_stream_ptr()), 'jodo_plan_upload')
        torch.cuda.current_stream().synchronize()        # host staging buffer lives in the plan; be safe
        return dict(handle=handle, desc=desc, ws=ws, n_nodes=n_host, B=B, N=N, flags=torch.zeros(8, dtype=torch.int32, device=device))

    def __del__(self):
        try:
            L = capi.lib()
            for p in self._plans.values():
                L.jodo_plan_destroy(p['handle'])
        except Exception:
            pass

    # -- forward -------------------------------------------------------------------------------
    def forward(self, t, xh, node_mask, edge_mask, context=None, *args, **kwargs):
        edge_x, cond_x, cond_edge_x = kwargs['edge_x'], kwargs.get('cond_x'), kwargs.get('cond_edge_x')
        noise_level = kwargs['noise_level']
        if not xh.is_cuda:
            raise RuntimeError("jodo_amd DGT runs on an MI355X only (got a %s tensor); there is no CPU fallback — "
                               "use oracle/dgt_oracle.py for CPU checks" % xh.device)
        if self.conditional and context is None:
            raise ValueError("cond_DGT_concat needs `context`")
        if torch.is_grad_enabled() and any(t_ is not None and t_.requires_grad for t_ in (xh, edge_x, cond_x, cond_edge_x, noise_level, context)):
            raise RuntimeError("the HIP DGT returns parameter gradients only: detach the inputs (the reference's loss detaches the "
                               "self-conditioning inputs, losses.py:339, and needs no input gradient)")
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if wants_grad or (self.training and self.dropout_p > 0):
            # training path (csrc/dgt_train.hip): activations kept for loss.backward(); under model.train() dropout is active
            # in the no-grad self-conditioning forward too (losses.py:335-339), which is why that call comes here as well
            return self._forward_train(xh, edge_x, cond_x, cond_edge_x, noise_level, context, node_mask, edge_mask, wants_grad)
        dev = xh.device
        d = self.dims
        B, N, dims = xh.shape
        if dims != 3 + d.nd or edge_x.shape != (B, N, N, d.ch):
            raise ValueError("shape mismatch: xh %s edge_x %s" % (tuple(xh.shape), tuple(edge_x.shape)))
        f32 = lambda x: None if x is None else x.detach().to(torch.float32).contiguous()
        xh_, ex_, cx_, cex_, nl_ = f32(xh), f32(edge_x), f32(cond_x), f32(cond_edge_x), f32(noise_level)
        ctx_ = f32(context) if self.conditional else None
        streams = min(int(getattr(self, 'n_streams', 1)), 4)     # the plan cache holds 8 plans: every sub-batch plan of a call stays alive
        if streams > 1 and B >= 2 * streams:
            return self._forward_split(streams, node_mask, edge_mask, xh_, ex_, cx_, cex_, nl_, ctx_, dev)
        # plan first: building a plan for a new batch re-checks the weight fingerprint (`.data` updates such as the
        # reference's EMA copy_to / restore) and drops a stale blob BEFORE this call fetches it
        plan = self._plan(node_mask, edge_mask, dev)
        _, blob, woff_c, n_woff = self._weights(dev)
        self._follow_weights([plan])
        out_x = torch.empty_like(xh_)
        out_e = torch.empty_like(ex_)
        self._launch(plan, blob, woff_c, n_woff, xh_, ex_, cx_, cex_, nl_, ctx_, out_x, out_e)
        self.last_flags = plan['flags']
        self._last_plan = plan
        self._last_plans = [plan]
        return out_x, out_e

    # -- training path ---------------------------------------------------------------------------
    def _train_engine(self, node_mask, edge_mask, device):
        """One TrainEngine (jodo_train handle + device tables) per batch of atom counts, in the module's bounded cache
        (_runtime.HostRuntime._engine_for_masks).  model.validate_masks = False skips the mask checks."""
        from ..train import TrainEngine
        opts = tuple(sorted((getattr(self, 'train_options', None) or {}).items()))   # {jodo_train_set_option: value}, e.g. {0: 0}: op-by-op forward (tests)
        return self._engine_for_masks(TrainEngine, self._cfg(), node_mask, edge_mask, device, opts, getattr(self, 'validate_masks', True))

    def _forward_train(self, xh, edge_x, cond_x, cond_edge_x, noise_level, context, node_mask, edge_mask, wants_grad):
        from ..train import dgt_autograd
        d = self.dims
        B, N, dims = xh.shape
        if dims != 3 + d.nd or edge_x.shape != (B, N, N, d.ch):
            raise ValueError("shape mismatch: xh %s edge_x %s" % (tuple(xh.shape), tuple(edge_x.shape)))
        f32 = lambda x: None if x is None else x.detach().to(torch.float32).contiguous()
        eng = self._train_engine(node_mask, edge_mask, xh.device)
        p, seed = self._dropout_draw()
        ctx_ = f32(context) if self.conditional else None
        # parameters in state_dict order = the order the engine was created with (parameters() of this tree, no buffers)
        params = list(self.parameters())
        args = (eng, p, seed, f32(xh), f32(edge_x), f32(cond_x), f32(cond_edge_x), f32(noise_level), ctx_)
        if wants_grad:
            out_x, out_e = dgt_autograd(*args, params)
        else:
            # (nobody differentiates this call — the self-conditioning forward of a training step: backward-only stores are skipped)
            out_x, out_e = eng.forward([q.detach().contiguous() for q in params], *args[3:], p, seed,
                                       save_activations=bool(getattr(self, 'train_save_always', False)))      # (True: A/B runs of tools/train_bench.py)
        self.last_flags = eng.flags
        return out_x, out_e

    def _launch(self, plan, blob, woff_c, n_woff, xh_, ex_, cx_, cex_, nl_, ctx_, out_x, out_e):
        capi.check(capi.lib().jodo_dgt_forward(plan['handle'], capi.ptr(plan['desc']), capi.ptr(blob), woff_c, n_woff,
                                               capi.ptr(xh_), capi.ptr(ex_), capi.ptr(cx_), capi.ptr(cex_), capi.ptr(nl_),
                                               capi.ptr(ctx_), capi.ptr(out_x), capi.ptr(out_e), capi.ptr(plan['flags']),
                                               capi.ptr(plan['ws']), capi.current_stream_ptr()), 'jodo_dgt_forward')

    # -- stream-interleaved evaluation -----------------------------------------------------------
    def _split_of(self, node_mask, edge_mask, k):
        """Contiguous split of the batch into k sub-batches of about equal pair work (sum n^2), cached per mask tensor:
        [(lo, hi, node_mask[lo:hi], edge_mask rows of lo..hi)] — the sub-mask tensors are kept so that their plans stay cached.
        Keyed like _plan, by the masks' storage address, shape, stride and device (the single-device DataParallel wrap hands over a
        fresh view of the same masks on every call) and checked against their version counters; the entry keeps both masks alive,
        so their storage cannot be recycled for other masks while it is cached."""
        key = (node_mask.data_ptr(), tuple(node_mask.shape), tuple(node_mask.stride()), str(node_mask.device),
               edge_mask.data_ptr(), tuple(edge_mask.shape), tuple(edge_mask.stride()), k)
        ent = self._splits.get(key)
        if ent is not None and ent[1] == node_mask._version and ent[4] == edge_mask._version:
            return ent[2]
        B, N = node_mask.shape[0], node_mask.shape[1]
        n = node_mask.reshape(B, N).sum(1).round().long().cpu()                 # one sync per new batch
        cum = torch.cumsum(n.double() ** 2, 0)
        cuts = [0]
        for j in range(1, k):
            c = int(torch.searchsorted(cum, cum[-1] * j / k).item()) + 1
            cuts.append(min(max(c, cuts[-1] + 1), B - (k - j)))
        cuts.append(B)
        em = edge_mask.reshape(B, N * N, -1)
        parts = [(lo, hi, node_mask[lo:hi], em[lo:hi].reshape((hi - lo) * N * N, -1)) for lo, hi in zip(cuts[:-1], cuts[1:])]
        self._splits.pop(key, None)
        if len(self._splits) >= 4:
            self._splits.pop(next(iter(self._splits)))
        self._splits[key] = (node_mask, node_mask._version, parts, edge_mask, edge_mask._version)
        return parts

    def _forward_split(self, k, node_mask, edge_mask, xh_, ex_, cx_, cex_, nl_, ctx_, dev):
        """n_streams = k > 1: the batch is cut into k contiguous sub-batches (molecules are independent) that are evaluated
        concurrently, sub-batch j on HIP stream j (stream 0 = the caller's).  Every launch of this path is one wave per SIMD
        with item counts that are not multiples of the chip (1409 node strips, 12 666 pair items at QM9 B = 2500), so a
        single stream leaves the tail round of every launch partly idle and serialises the latency-bound prologue /
        epilogue chains; with two streams the other sub-batch's workgroups fill those slots.  The C library still only ever
        sees the stream it is handed; the side streams belong to this module, fork from and join the caller's stream (works
        under HIP-graph capture).  Batch-global semantics of the reference: the NaN guard (mol_gnn.py:587-589) is applied
        across sub-batches below; the first-step switch (:544) is decided per sub-batch (identical unless a whole
        sub-batch's self-conditioning positions coincide — the same caveat as sharding over GPUs)."""
        parts = self._split_of(node_mask, edge_mask, k)
        plans = [self._plan(nm, em, dev) for _, _, nm, em in parts]
        _, blob, woff_c, n_woff = self._weights(dev)
        self._follow_weights(plans)
        out_x = torch.empty_like(xh_)
        out_e = torch.empty_like(ex_)
        if getattr(self, '_side_streams', None) is None or len(self._side_streams) < k - 1:
            self._side_streams = [torch.cuda.Stream(device=dev) for _ in range(k - 1)]
        cur = torch.cuda.current_stream()
        cut = lambda t, lo, hi: None if t is None else t[lo:hi]
        for j, ((lo, hi, _, _), plan) in enumerate(zip(parts, plans)):
            args = (plan, blob, woff_c, n_woff, xh_[lo:hi], ex_[lo:hi], cut(cx_, lo, hi), cut(cex_, lo, hi), nl_[lo:hi],
                    cut(ctx_, lo, hi), out_x[lo:hi], out_e[lo:hi])
            if j == 0:
                self._launch(*args)
            else:
                side = self._side_streams[j - 1]
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    self._launch(*args)
        for side in self._side_streams[:k - 1]:
            cur.wait_stream(side)
        flags = torch.stack([p['flags'] for p in plans]).amax(0)
        out_x[:, :, :3] *= (flags[0] == 0).to(out_x.dtype)           # NaN guard is batch-global: any sub-batch resets all positions
        self.last_flags = flags
        self._last_plan = plans[0]
        self._last_plans = plans
        return out_x, out_e

    def take_nan_count(self):
        """Number of evaluations since the last call in which the NaN guard fired (sticky device counter, flags[5] of
        every cached plan); one host sync, so call it once per sampling round, not per step."""
        plans = list(self._plans.values())
        if not plans:
            return 0
        both = torch.stack([p['flags'][5:7] for p in plans]).sum(0).tolist()        # one host sync for all cached plans
        total, violated = int(both[0]), int(both[1])
        if total or violated:
            for p in plans:
                p['flags'][5:7] = 0
        if violated:
            raise RuntimeError("a call on a plan with pinned kernel paths (pin_paths) had inputs that take another path "
                               "(asymmetric edge tensors or per-molecule noise levels): its outputs are invalid")
        return total

    def pin_paths(self):
        """Pin the kernel variants of the plan of the last call to the ones that call used (device flags [2] shared
        modulation row, [4] asymmetric inputs; one host sync): later calls on the same masks launch only those variants
        instead of every variant + device-side early exits (24 idle dispatches per forward at 8 blocks).  For callers that
        know the inputs keep their structure — the samplers inside one round, which unpin when the round ends
        (unpin_paths).  A violating call is detected on the device and reported by take_nan_count(); a state that went NaN
        is not a violation (k_check_sym counts NaN == NaN), it ends in the NaN guard like the reference's."""
        plans = [p for p in getattr(self, '_last_plans', []) if not p.get('pinned')]
        if not plans:
            return
        fl = torch.stack([p['flags'] for p in plans]).cpu().tolist()
        L = capi.lib()
        for plan, f in zip(plans, fl):
            capi.check(L.jodo_plan_set_option(plan['handle'], 4, 2 if f[4] else 1), 'jodo_plan_set_option')
            capi.check(L.jodo_plan_set_option(plan['handle'], 5, 1 if f[2] else 2), 'jodo_plan_set_option')
            plan['pinned'] = True
            # unconditional: the folded kernels (need the shared modulation row, f[2]); conditional: the un-folded kernel (nf 256, any rows)
            fits = (self.dims.D == 256) if self.conditional else (self.dims.D in (256, 384) and f[2])
            if self.split_bf16 and fits and not f[4]:
                self._hand_over_split(plan)
                capi.check(L.jodo_plan_set_option(plan['handle'], 13, 2 if self.split_bf16 == 'attention' else 1), 'jodo_plan_set_option')

    def _hand_over_split(self, plan):
        """The split-bf16 weight tape of the CURRENT parameters -> this plan."""
        tape = self._split_weights(plan['ws'].device)
        capi.check(capi.lib().jodo_plan_set_split_weights(plan['handle'], capi.ptr(tape), ctypes.c_size_t(tape.numel())), 'jodo_plan_set_split_weights')
        plan['split_tape'] = tape                             # keeps the device copy alive as long as the plan may use it
        plan['split_key'] = self._split_tape[0]

    def _follow_weights(self, plans):
        """Called by every forward after it fetched the packed blob: a pinned split plan whose tape predates the blob's last re-pack
        (an optimiser step, load_state_dict, a `.data` write caught by the fingerprint or invalidate_packed_weights() between two
        calls on the same masks) gets the current tape, so that no kernel of the call reads other weights than the rest."""
        for plan in plans:
            if plan.get('split_tape') is not None and plan.get('split_key') != self._pack_gen:
                self._hand_over_split(plan)

    def _split_weights(self, device):
        """Device copy of the split-bf16 weight tape of the current parameters (re-packed when the packed blob is: same generation)."""
        self._weights(device)
        gen = self._pack_gen
        if self._split_tape is None or self._split_tape[0] != gen:
            pack = capi.pack_split_cond_tape if self.conditional else capi.pack_split_tape
            self._split_tape = (gen, pack(self._cfg(), self.state_dict(), device))
        return self._split_tape[1]

    def unpin_paths(self):
        """End of the scope of pin_paths(): every cached plan goes back to launching all kernel variants and letting the device
        flags decide.  The samplers call it when a round ends (also when it ends in an exception), so a later caller that
        reuses the same mask tensors with other inputs — asymmetric edge tensors, per-molecule noise levels: a likelihood or
        loss evaluation — gets the right kernels instead of a pin violation."""
        L = capi.lib()
        for plan in self._plans.values():
            if plan.get('pinned'):
                capi.check(L.jodo_plan_set_option(plan['handle'], 4, 0), 'jodo_plan_set_option')
                capi.check(L.jodo_plan_set_option(plan['handle'], 5, 0), 'jodo_plan_set_option')
                capi.check(L.jodo_plan_set_option(plan['handle'], 13, 0), 'jodo_plan_set_option')
                plan['pinned'] = False

    # -- measurement plumbing (bench.py): HIP-event class timers and the executed-work model of the last call's plan(s) --
    def profile_enable(self, mode):
        for p in self._last_plans:
            capi.check(capi.lib().jodo_profile_enable(p['handle'], int(mode)), 'jodo_profile_enable')

    def profile_read(self):
        """Summed milliseconds and launch counts per class (8 each) since the last read, over the last call's plans."""
        ms_t, cnt_t = [0.0] * 8, [0] * 8
        for p in self._last_plans:
            ms, cnt = (ctypes.c_float * 8)(), (ctypes.c_int32 * 8)()
            capi.check(capi.lib().jodo_profile_read(p['handle'], ms, cnt), 'jodo_profile_read')
            ms_t = [a + b for a, b in zip(ms_t, ms)]
            cnt_t = [a + b for a, b in zip(cnt_t, cnt)]
        return ms_t, cnt_t

    def profile_read_kernels(self):
        """Kernel launches per class (8) issued inside the profiling brackets since the last read, over the last call's plans:
        profile_read's counts are brackets (one per class and block); these are the dispatches that pins and plan options change."""
        tot = [0] * 8
        for p in self._last_plans:
            k = (ctypes.c_int32 * 8)()
            capi.check(capi.lib().jodo_profile_read_kernels(p['handle'], k), 'jodo_profile_read_kernels')
            tot = [a + b for a, b in zip(tot, k)]
        return tot

    def work_model(self):
        """Executed MFMA flops per launch class of ONE evaluation like the last one (jodo_plan_work, summed over its plans)."""
        tot = [0.0] * 8
        for p, f in zip(self._last_plans, torch.stack([p['flags'] for p in self._last_plans]).cpu().tolist()):
            w = (ctypes.c_double * 8)()
            capi.check(capi.lib().jodo_plan_work(p['handle'], int(f[2]), int(not f[4]), w), 'jodo_plan_work')
            tot = [a + b for a, b in zip(tot, w)]
        return tot

    def nan_guard_fired(self):
        """Lazy read of the device NaN-guard flag of the last call (the reference prints a warning and
        zeroes all positions, mol_gnn.py:587-589; the zeroing already happened on the device)."""
        return self.last_flags is not None and bool(self.last_flags[0].item())


@utils.register_model(name='DGT_concat')
class DGT_concat(_DGTBase):
    """Diffusion Graph Transformer with self-conditioning (HIP)."""
    conditional = False


@utils.register_model(name='cond_DGT_concat')
class Cond_DGT_concat(_DGTBase):
    """Conditional Diffusion Graph Transformer with self-conditioning (HIP)."""
    conditional = True


@utils.register_model(name='DGT_concat_sim')
class DGT_concat_sim(_DGTBase):
    """Diffusion Graph Transformer with self-conditioning, without extra attention heads (HIP): the reference's EquivariantBlock /
    Trans_Layer / CondEquiUpdate (mol_gnn.py:949-1124, :97-208, :16-48; layers.py:13-89).  16 learned heads of nf / 16 channels, softmax over
    the real incoming edges, one coordinate head; `n_extra_heads`, `trans_name`, `softmax_inf` and `edge_quan_th` are never read and
    `spatial_cut_off` has no effect.  Built for nf = 256 (both 3-D JODO configs), exact fp32.

    Training is opt-in: with `model.hip_training = True` (jodo_amd.losses.get_step_fn sets it when asked for a training step) a
    grad-enabled call — and, under model.train() with dropout > 0, the no-grad self-conditioning call too — runs csrc/dgt_train.hip
    through jodo_amd.train.TrainEngine like DGT_concat's (dropout in the two feed-forwards; the reference builds this block's Trans_Layer
    without a dropout argument, mol_gnn.py:116), and `loss.backward()` fills every parameter's gradient; a default module keeps refusing
    such calls."""
    conditional = False
    extra_heads = 0

    def __init__(self, config):
        super().__init__(config)
        self.hip_training = False     # opt-in: grad-enabled calls go through the HIP training path (csrc/dgt_train.hip with n_extra = 0)

    def forward(self, t, xh, node_mask, edge_mask, context=None, *args, **kwargs):
        if self.split_bf16:
            raise NotImplementedError("DGT_concat_sim has no split-bf16 form: leave model.split_bf16 = False (the exact-fp32 kernels)")
        if not self.hip_training and ((torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))
                                      or (self.training and self.dropout_p > 0)):
            raise NotImplementedError("DGT_concat_sim is built for inference by default: call it under torch.no_grad() in eval() mode, or set "
                                      "model.hip_training = True for the HIP training path (jodo_amd.losses.get_step_fn does)")
        return super().forward(t, xh, node_mask, edge_mask, context, *args, **kwargs)

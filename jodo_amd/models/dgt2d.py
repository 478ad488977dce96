"""MI355X-native score network for 2-D graphs, registered under the reference's name 'DGT_concat_2D'
(reference: models/mol_gnn.py:797-946; the ZINC250k and MOSES experiments).

Same constructor argument, parameter names / shapes / registration order (state_dict keys, EMA order, `strict=True` loading) and
the same call as the reference class:
    model(t, xh, node_mask, edge_mask, context=None, edge_x=..., cond_x=..., cond_edge_x=..., noise_level=...)
        -> (atom_pred [B,N,nd], edge_pred [B,N,N,ch])
The arithmetic runs in libjodo_hip.so (csrc/dgt2d_forward.hip, `jodo_dgt2d_forward`) on the current HIP stream: the weights are
packed once (csrc/dgt2d_pack.cpp), a descriptor and a workspace are built per batch of atom counts.  There is no CPU or eager
fallback, and the 3-D models' `split_bf16` switch is not taken by this model — those raise.

`model.bf16x3 = True` (opt-in, runtime state) selects the three-term bf16 form of the node GEMMs and of the pair update
(`jodo_dgt2d_forward_split`, kernels k2d_gemm_s / k2d_pair_s) from a weight tape derived from the packed blob; attention, the edge
heads and the one-row time / modulation GEMMs stay exact fp32.  `model.last_flags[3]` tells which form ran.

`model.pair_attention = True` (opt-in, runtime state) selects the pair-symmetric attention walk (`jodo_dgt2d_forward_walk`, kernel
k2d_attn_pair): with symmetric inputs every unordered pair is evaluated once; `model.last_flags[2]` tells which walk ran.

Training is opt-in: with `model.hip_training = True` (jodo_amd.losses.get_step_fn sets it when asked for a training step) a
grad-enabled call runs csrc/dgt2d_train.hip through jodo_amd.train.TrainEngine2D and `loss.backward()` fills every parameter's
gradient; a default module keeps refusing grad-enabled calls ("inference only").
"""
import ctypes

import torch
from torch import nn

from .. import capi
from . import utils
from ._runtime import TapeRuntime
from .dgt import _SinusoidParams, _mlp3, _time_seq, _AttnParams

# (key, the one supported value) — the settings of configs/vpsde_zinc_2d_jodo.py and vpsde_moses_2d_jodo.py
_SUPPORTED_2D = (('nf', 256), ('n_heads', 16), ('n_extra_heads', 1), ('mlp_ratio', 2), ('n_layers', 8), ('cond_time', True),
                 ('pred_data', True), ('softmax_inf', True), ('trans_name', 'TransMixLayer'))


class _Block2DParams(nn.Module):
    """EquivariantMixBlock_2D (mol_gnn.py:325-362): parameters only, reference registration order."""

    def __init__(self, node_dim, edge_dim, time_dim, n_extra, n_heads, mlp_ratio):
        super().__init__()
        self.node2edge_lin = nn.Linear(node_dim, edge_dim)
        self.attn_mpnn = _AttnParams(node_dim, node_dim // n_heads, n_extra, n_heads, edge_dim)
        self.ff_linear1 = nn.Linear(node_dim, node_dim * mlp_ratio)
        self.ff_linear2 = nn.Linear(node_dim * mlp_ratio, node_dim)
        self.ff_linear3 = nn.Linear(edge_dim, edge_dim * mlp_ratio)
        self.ff_linear4 = nn.Linear(edge_dim * mlp_ratio, edge_dim)
        self.node_time_mlp = _time_seq(time_dim, node_dim * 6)
        self.edge_time_mlp = _time_seq(time_dim, edge_dim * 6)


class _Cfg2D(ctypes.Structure):                 # jodo_cfg2d (include/jodo_hip.h)
    _fields_ = [('nf', ctypes.c_int32), ('n_layers', ctypes.c_int32), ('n_heads', ctypes.c_int32), ('n_extra', ctypes.c_int32),
                ('mlp_ratio', ctypes.c_int32), ('in_node_dim', ctypes.c_int32), ('edge_ch', ctypes.c_int32),
                ('edge_quan_th', ctypes.c_float)]


@utils.register_model(name='DGT_concat_2D')
class DGT_concat_2D(TapeRuntime, nn.Module):
    """Diffusion Graph Transformer with self-conditioning for 2-D graphs (HIP)."""

    def __init__(self, config):
        super().__init__()
        m = config.model
        for key, want in _SUPPORTED_2D:
            got = getattr(m, key, want if key == 'trans_name' else None)
            if got != want:
                raise NotImplementedError("config.model.%s=%r: the 2-D HIP path implements %r only (the ZINC250k / MOSES configs' setting)"
                                          % (key, got, want))
        if hasattr(m, 'time_dim') and m.time_dim != 4 * m.nf:
            raise NotImplementedError("config.model.time_dim=%r: the 2-D HIP path implements 4 * nf = %d only" % (m.time_dim, 4 * m.nf))
        in_node_dim = config.data.atom_types + int(m.include_fc_charge)
        if not 1 <= in_node_dim <= 16:
            raise NotImplementedError("config.data.atom_types + include_fc_charge = %d: the 2-D HIP path takes 1..16 node channels" % in_node_dim)
        if m.edge_ch not in (2, 3):
            raise NotImplementedError("config.model.edge_ch=%r: the 2-D HIP path implements 2 and 3" % (m.edge_ch,))
        D, De, L, T = m.nf, m.nf // 4, m.n_layers, 4 * m.nf
        self.in_node_dim, self.edge_ch = in_node_dim, int(m.edge_ch)
        self.edge_th = float(m.edge_quan_th)
        self.n_layers = L
        self.pred_data = m.pred_data
        self.cond_time = m.cond_time
        self.dropout_p = m.dropout               # identity at inference; kept for config parity
        self._cfg_struct = _Cfg2D(D, L, m.n_heads, m.n_extra_heads, m.mlp_ratio, in_node_dim, self.edge_ch, self.edge_th)

        # ---- parameter tree, reference construction / registration order (mol_gnn.py:823-866) ----
        self.node_emb = nn.Linear(in_node_dim * 2, D)
        self.edge_emb = nn.Linear(m.edge_ch * 2, De)
        cat_node, cat_edge = (D * 2) // L, (De * 2) // L
        for i in range(L):
            self.add_module("e_block_%d" % i, _Block2DParams(D, De, T, m.n_extra_heads, m.n_heads, m.mlp_ratio))
            self.add_module("node_%d" % i, nn.Linear(D, cat_node))
            self.add_module("edge_%d" % i, nn.Linear(De, cat_edge))
        self.node_pred_mlp = _mlp3(cat_node * L + D, D, D // 2, in_node_dim)
        self.edge_type_mlp = _mlp3(cat_edge * L + De, De, De // 2, m.edge_ch - 1)
        self.edge_exist_mlp = _mlp3(cat_edge * L + De, De, De // 2, 1)
        self.time_mlp = nn.Sequential(_SinusoidParams(16), nn.Linear(17, T), nn.GELU(), nn.Linear(T, T))

        # ---- runtime state (not part of state_dict) ----
        self._init_runtime()          # _packed, _tape, _plans (per batch of atom counts: descriptor + workspace, see _plan)
        self.split_bf16 = False       # the 3-D models' opt-in form; not built for this model (forward raises when set)
        self.force_directed = False   # tests: always the directed fallback
        self.max_blocks = -1          # tests: stop after this many blocks (the workspace then holds h and e of that block)
        self.last_flags = None
        self.hip_training = False     # opt-in: grad-enabled calls go through the HIP training path (csrc/dgt2d_train.hip)
        self.pair_attention = False   # opt-in: the pair-symmetric attention walk (k2d_attn_pair) when the inputs are symmetric;
                                      # last_flags[2] tells which walk ran (1 = pair, 0 = directed).  The training path ignores it.
        self.bf16x3 = False           # opt-in, read per call: the split-bf16 (three-term) form of the node GEMMs and the pair update
                                      # (k2d_gemm_s, k2d_pair_s); last_flags[3] tells which form ran (1 = split, 0 = exact fp32).
                                      # Combines with pair_attention / force_directed / max_blocks.  The training path ignores it.

    # -- weights (cache, fingerprint, invalidation and the derived tape: _runtime.TapeRuntime) -----------
    def _pack(self, device):
        return capi.pack_weights_2d(self._cfg_struct, self.state_dict(), None)

    def _pack_tape(self, blob_host, woff_c, n_woff, device):
        return capi.split_tape_2d(self._cfg_struct, blob_host, woff_c, n_woff, device)

    # -- per-batch descriptor and workspace -----------------------------------------------------------
    def _plan(self, node_mask, edge_mask, device, validate=True):
        return self._cached_plan(node_mask, edge_mask, validate, lambda n_host, B, N: self._build_plan(n_host, B, N, device))

    def _build_plan(self, n_host, B, N, device):
        L = capi.lib()
        lay = (ctypes.c_int64 * 8)()
        n_ptr = n_host.ctypes.data_as(ctypes.c_void_p)
        capi.check(L.jodo_dgt2d_layout(ctypes.byref(self._cfg_struct), B, N, n_ptr, lay), 'jodo_dgt2d_layout')
        desc_host = torch.empty(int(lay[0]), dtype=torch.int32)
        capi.check(L.jodo_dgt2d_fill_desc(ctypes.byref(self._cfg_struct), B, N, n_ptr, ctypes.c_void_p(desc_host.data_ptr()),
                                          ctypes.c_int64(int(lay[0]))), 'jodo_dgt2d_fill_desc')
        plan = dict(desc=desc_host.to(device), ws=torch.zeros(int(lay[1]), dtype=torch.uint8, device=device), n_nodes=n_host, B=B, N=N,
                    Nn=int(lay[2]), rows=int(lay[3]), h_off=int(lay[4]), e_off=int(lay[5]), pairs=int(lay[6]),
                    flags=torch.zeros(8, dtype=torch.int32, device=device))
        if self.pair_attention:
            self._pair_desc(plan, device)
        return plan

    def _pair_desc(self, plan, device):
        """The group descriptor of the pair walk (jodo_dgt2d_pair_fill_desc), built once per plan from its host-side atom counts."""
        desc = plan.get('pair_desc')
        if desc is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("pair_attention was switched on under graph capture for a batch planned without it: run one eager "
                                   "call with pair_attention = True first")
            L = capi.lib()
            lay = (ctypes.c_int64 * 8)()
            n_ptr = plan['n_nodes'].ctypes.data_as(ctypes.c_void_p)
            capi.check(L.jodo_dgt2d_pair_layout(ctypes.byref(self._cfg_struct), plan['B'], plan['N'], n_ptr, lay), 'jodo_dgt2d_pair_layout')
            host = torch.empty(int(lay[0]), dtype=torch.int32)
            capi.check(L.jodo_dgt2d_pair_fill_desc(ctypes.byref(self._cfg_struct), plan['B'], plan['N'], n_ptr,
                                                   ctypes.c_void_p(host.data_ptr()), ctypes.c_int64(int(lay[0]))), 'jodo_dgt2d_pair_fill_desc')
            desc = plan['pair_desc'] = host.to(device)
            plan['pair_groups'] = int(lay[1])
        return desc

    # -- forward -------------------------------------------------------------------------------
    def forward(self, t, xh, node_mask, edge_mask, context=None, *args, **kwargs):
        edge_x, cond_x, cond_edge_x = kwargs['edge_x'], kwargs.get('cond_x'), kwargs.get('cond_edge_x')
        noise_level = kwargs['noise_level']
        if not xh.is_cuda:
            raise RuntimeError("jodo_amd DGT_concat_2D runs on an MI355X only (got a %s tensor); there is no CPU fallback — "
                               "use tests/oracle2d.py for CPU checks" % xh.device)
        if self.split_bf16:
            raise NotImplementedError("split_bf16 is not implemented for DGT_concat_2D (exact fp32 only)")
        inputs_want_grad = any(t_ is not None and t_.requires_grad for t_ in (xh, edge_x, cond_x, cond_edge_x, noise_level))
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if not self.hip_training and torch.is_grad_enabled() and (wants_grad or inputs_want_grad):
            raise NotImplementedError("DGT_concat_2D is inference only: call it under torch.no_grad() (training / backward for the 2-D "
                                      "model is not implemented)")
        if self.hip_training and torch.is_grad_enabled() and inputs_want_grad:
            raise RuntimeError("the HIP DGT returns parameter gradients only: detach the inputs (the reference's loss detaches the "
                               "self-conditioning inputs, losses.py:250, and needs no input gradient)")
        if (cond_x is None) != (cond_edge_x is None):
            raise ValueError("cond_x and cond_edge_x must both be given or both be None")
        B, N, dims = xh.shape
        if dims != self.in_node_dim or edge_x.shape != (B, N, N, self.edge_ch):
            raise ValueError("shape mismatch: xh %s edge_x %s" % (tuple(xh.shape), tuple(edge_x.shape)))
        if self.hip_training and (wants_grad or (self.training and self.dropout_p > 0)):
            # training path (csrc/dgt2d_train.hip): activations kept for loss.backward(); under model.train() dropout is active in the
            # no-grad self-conditioning forward too (losses.py:246-250 of the reference), which is why that call comes here as well
            return self._forward_train(xh, edge_x, cond_x, cond_edge_x, noise_level, node_mask, edge_mask, wants_grad)
        dev = xh.device
        f32 = lambda x: None if x is None else x.detach().to(torch.float32).contiguous()
        xh_, ex_, cx_, cex_, nl_ = f32(xh), f32(edge_x), f32(cond_x), f32(cond_edge_x), f32(noise_level)
        plan = self._plan(node_mask, edge_mask, dev)     # first: a new batch re-checks the weight fingerprint
        _, blob, woff_c, n_woff = self._weights(dev)
        out_x = torch.empty_like(xh_)
        out_e = torch.empty_like(ex_)
        n_ptr = plan['n_nodes'].ctypes.data_as(ctypes.c_void_p)
        wts = (capi.ptr(blob), woff_c, n_woff)
        tail = (capi.ptr(xh_), capi.ptr(ex_), capi.ptr(cx_), capi.ptr(cex_), capi.ptr(nl_), capi.ptr(out_x),
                capi.ptr(out_e), capi.ptr(plan['flags']), capi.ptr(plan['ws']), int(bool(self.force_directed)), int(self.max_blocks),
                capi.current_stream_ptr())
        if not self.pair_attention and plan.get('walk_slot_used'):   # flags[2] still holds an earlier pair-walk call's record
            plan['flags'][2:3].zero_()
            plan['walk_slot_used'] = False
        if self.bf16x3:
            tape, toff = self._split_tape(dev)
            pair = self.pair_attention
            capi.check(capi.lib().jodo_dgt2d_forward_split(ctypes.byref(self._cfg_struct), B, N, n_ptr, capi.ptr(plan['desc']),
                                                           capi.ptr(self._pair_desc(plan, dev)) if pair else None,
                                                           capi.WALK_PAIR if pair else capi.WALK_DIRECTED, *wts, capi.ptr(tape), toff, *tail),
                       'jodo_dgt2d_forward_split')
            if pair:
                plan['walk_slot_used'] = True
        elif self.pair_attention:
            capi.check(capi.lib().jodo_dgt2d_forward_walk(ctypes.byref(self._cfg_struct), B, N, n_ptr, capi.ptr(plan['desc']),
                                                          capi.ptr(self._pair_desc(plan, dev)), capi.WALK_PAIR, *wts, *tail),
                       'jodo_dgt2d_forward_walk')
            plan['walk_slot_used'] = True
        else:
            capi.check(capi.lib().jodo_dgt2d_forward(ctypes.byref(self._cfg_struct), B, N, n_ptr, capi.ptr(plan['desc']), *wts, *tail),
                       'jodo_dgt2d_forward')
        self.last_flags = plan['flags']
        self._last_plan = plan
        return out_x, out_e

    # -- training path (opt-in: hip_training) ------------------------------------------------------------
    def _train_engine(self, node_mask, edge_mask, device):
        """One TrainEngine2D (jodo_train2d handle + device tables) per batch of atom counts, in the module's bounded cache
        (_runtime.HostRuntime._engine_for_masks)."""
        from ..train import TrainEngine2D
        opts = tuple(sorted((getattr(self, 'train_options', None) or {}).items()))
        return self._engine_for_masks(TrainEngine2D, self._cfg_struct, node_mask, edge_mask, device, opts)

    def _forward_train(self, xh, edge_x, cond_x, cond_edge_x, noise_level, node_mask, edge_mask, wants_grad):
        from ..train import dgt2d_autograd
        f32 = lambda x: None if x is None else x.detach().to(torch.float32).contiguous()
        eng = self._train_engine(node_mask, edge_mask, xh.device)
        p, seed = self._dropout_draw()
        params = list(self.parameters())                         # state_dict order: this tree has no buffers
        args = (eng, p, seed, f32(xh), f32(edge_x), f32(cond_x), f32(cond_edge_x), f32(noise_level))
        if wants_grad:
            out_x, out_e = dgt2d_autograd(*args, params)
        else:                                                    # the no-grad self-conditioning forward of a training step
            out_x, out_e = eng.forward([q.detach().contiguous() for q in params], *args[3:], None, p, seed, save_activations=False)
        self.last_flags = eng.flags
        return out_x, out_e

    # -- tests: the state inside the workspace after the last call ------------------------------------
    def debug_state(self):
        """(h [Nn, nf], e [sum n^2, nf / 4]) of the last call as the kernels left them: h compact over real atoms; e row
        eoff_b + r n_b + c, with only the rows r < c live when the inputs were symmetric (flags[0])."""
        p = self._last_plan
        D = self._cfg_struct.nf
        ws = p['ws']
        h = ws[p['h_off']:p['h_off'] + p['Nn'] * D * 4].view(torch.float32).reshape(p['Nn'], D)
        e = ws[p['e_off']:p['e_off'] + p['rows'] * (D // 4) * 4].view(torch.float32).reshape(p['rows'], D // 4)
        return h.clone(), e.clone()

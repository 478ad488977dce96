"""MI355X-native noise-prediction network for 2-D graphs, registered under the reference's name 'CDGS'
(reference: models/cdgs.py; the configs vpsde_qm9_2d_cdgs and vpsde_geom_2d_cdgs).

Same constructor argument, parameter names / shapes / registration order (one `all_modules` list: state_dict keys, EMA order,
`strict=True` loading, the 4-D conv weights and the GINE `eps` buffers included) and the same call as the reference class:
    model(t, x, node_mask, edge_mask, context=None, edge_x=...) -> (atom_score [B,N,atom_types], bond_score [B,N,N,edge_ch])
The arithmetic runs in libjodo_hip.so (csrc/cdgs_forward.hip, `jodo_cdgs_forward`) on the current HIP stream: the weights are packed
once (csrc/cdgs_pack.cpp), a descriptor and a workspace are built per batch of atom counts.  Exact fp32 by default; there is no CPU or
eager fallback, and the 3-D models' `split_bf16` switch is not taken by this model — those raise.  The forward can be captured into a
HIP graph once an eager call has built the batch's plan and packed the weights (GraphedDPMRound2D does, for sampling.method 'dpm_2d');
the ancestral round has no graph replay.

`model.bf16x3 = True` (opt-in, runtime state, read per call) selects the three-term bf16 form of every row GEMM over node rows and edge
rows (`jodo_cdgs_forward_split`, kernel kc_gemm_s) from a weight tape derived from the packed blob; the time-embedding GEMMs, GINE,
attention, the GroupNorms and the random-walk features stay exact fp32.  `model.last_flags[3]` tells that the split form ran (after a
default call `last_flags` is None).  Sample quality under the split form is untested: no trained weights exist here.

Training is opt-in: with `hip_training = True` (set by
jodo_amd.losses.get_step_fn) a grad-enabled call runs csrc/cdgs_train.hip on the live parameters, keeps the activations, and
loss.backward() returns every parameter's gradient (jodo_amd/train.py TrainEngineCDGS); unset, a grad-enabled call raises.
`model.train_bf16x3 = True` (opt-in, runtime state, read per training-path call) runs the forward and data-gradient GEMMs of the training
path — mask 3; an int 0..7 selects forms itself, 4 = the weight-gradient GEMMs, which measured no faster — in the split-bf16 form (csrc/train_gemm.hip k_gemm_s); `model.last_train_form` reports the
mask the last training forward ran with.  `bf16x3` alone never changes training: that stays exact fp32.

The edge GroupNorm of the reference normalises the dense padded tensor, so a molecule's scores depend on the width N the caller
padded the batch to; the kernels reproduce that from the tensors' N.
"""
import ctypes
import math

import torch
from torch import nn

from .. import capi
from . import utils
from ._runtime import TapeRuntime

MAX_N = 181                                     # JODO_CDGS_MAX_N (include/jodo_hip.h): the GEOM config's max_node


class _Cfg(ctypes.Structure):                   # jodo_cdgs_cfg (include/jodo_hip.h)
    _fields_ = [('nf', ctypes.c_int32), ('n_layers', ctypes.c_int32), ('n_heads', ctypes.c_int32), ('atom_ch', ctypes.c_int32),
                ('edge_ch', ctypes.c_int32), ('rw_depth', ctypes.c_int32)]


class _GINEParams(nn.Module):
    """GINEConv(nn, train_eps=False): the two PyG Linears of `nn` and the `eps` buffer [1]."""

    def __init__(self, dim):
        super().__init__()
        self.nn = nn.Sequential(nn.Linear(dim, dim), nn.ReLU(), nn.Linear(dim, dim))
        self.register_buffer('eps', torch.zeros(1))


class _GateTransParams(nn.Module):
    """EdgeGateTransLayer (models/layers.py): parameters only, reference registration order."""

    def __init__(self, dim):
        super().__init__()
        self.lin_key = nn.Linear(dim, dim)
        self.lin_query = nn.Linear(dim, dim)
        self.lin_value = nn.Linear(dim, dim)
        self.lin_edge0 = nn.Linear(dim, dim, bias=False)
        self.lin_edge1 = nn.Linear(dim, dim, bias=False)


class _HybridBlockParams(nn.Module):
    """HybridMPBlock(dim, 'GINE', 'FullTrans_1'): parameters only, reference registration order."""

    def __init__(self, dim):
        super().__init__()
        groups = min(dim // 4, 32)
        self.t_node = nn.Linear(dim, dim)
        self.t_edge = nn.Linear(dim, dim)
        self.local_model = _GINEParams(dim)
        self.self_attn = _GateTransParams(dim)
        self.norm1_local = nn.GroupNorm(groups, dim, eps=1e-6)
        self.norm1_attn = nn.GroupNorm(groups, dim, eps=1e-6)
        self.ff_linear1 = nn.Linear(dim, dim * 2)
        self.ff_linear2 = nn.Linear(dim * 2, dim)
        self.norm2_node = nn.GroupNorm(groups, dim, eps=1e-6)
        self.ff_linear3 = nn.Linear(dim, dim * 2)
        self.ff_linear4 = nn.Linear(dim * 2, dim)
        self.norm2_edge = nn.GroupNorm(groups, dim, eps=1e-6)


def _conv1x1(cin, cout):
    return nn.Conv2d(cin, cout, kernel_size=1)


@utils.register_model(name='CDGS')
class CDGS(TapeRuntime, nn.Module):
    """Graph noise-prediction model: GINE + edge-gated full attention blocks over random-walk features (HIP)."""

    depends_on_padded_width = True    # the dense edge GroupNorm: read by the sampling function's parity shards (jodo_amd/sampling.py)

    def __init__(self, config):
        super().__init__()
        m, d = config.model, config.data
        for key, want in (('nf', 256), ('n_heads', 16), ('cond_time', True)):
            if getattr(m, key, None) != want:
                raise NotImplementedError("config.model.%s=%r: the CDGS HIP path implements %r only" % (key, getattr(m, key, None), want))
        if not getattr(d, 'centered', False):
            raise NotImplementedError("config.data.centered=%r: the CDGS HIP path implements True only" % (getattr(d, 'centered', None),))
        if m.edge_ch not in (2, 3):
            raise NotImplementedError("config.model.edge_ch=%r: the CDGS HIP path implements 2 and 3" % (m.edge_ch,))
        if not 1 <= d.atom_types <= 16:
            raise NotImplementedError("config.data.atom_types=%r: the CDGS HIP path takes 1..16 atom channels" % (d.atom_types,))
        if not 1 <= m.rw_depth <= 16:
            raise NotImplementedError("config.model.rw_depth=%r: the CDGS HIP path implements 1..16" % (m.rw_depth,))
        if not 1 <= m.n_layers <= 16:
            raise NotImplementedError("config.model.n_layers=%r: the CDGS HIP path implements 1..16" % (m.n_layers,))
        nf, L, rw = m.nf, m.n_layers, m.rw_depth
        self.nf, self.n_layers, self.rw_depth = nf, L, rw
        self.atom_ch, self.edge_ch = int(d.atom_types), int(m.edge_ch)
        self.dropout_p = m.dropout                # identity at inference; active in the training path under model.train()
        self.hip_training = False                 # opt-in: a grad-enabled call goes to csrc/cdgs_train.hip (get_step_fn sets it)
        self._cfg_struct = _Cfg(nf, L, m.n_heads, self.atom_ch, self.edge_ch, rw)

        # ---- parameter tree: one list, reference construction order ----
        bond_se, atom_se = int(nf * 0.4), int(nf * 0.2)
        bond_type, atom_type = int(0.5 * (nf - bond_se)), nf - 2 * atom_se
        cat = (nf * 2) // L
        mods = [nn.Linear(nf, nf * 2), nn.Linear(nf * 2, nf),
                _conv1x1(self.edge_ch - 1, bond_type), _conv1x1(1, bond_type), _conv1x1(rw + 1, bond_se),
                nn.Linear(bond_se + 2 * bond_type, nf),
                nn.Linear(self.edge_ch, atom_se), nn.Linear(self.atom_ch, atom_type), nn.Linear(rw, atom_se),
                nn.Linear(atom_type + 2 * atom_se, nf)]
        for _ in range(L):
            mods += [_HybridBlockParams(nf), nn.Linear(nf, cat), nn.Linear(nf, cat)]
        mods += [nn.Linear(cat * L + atom_type, nf), nn.Linear(nf, nf // 2), nn.Linear(nf // 2, self.atom_ch)]
        mods += [_conv1x1(cat * L + bond_type, nf), _conv1x1(nf, nf // 2), _conv1x1(nf // 2, self.edge_ch - 1)]
        mods += [_conv1x1(cat * L + bond_type, nf), _conv1x1(nf, nf // 2), _conv1x1(nf // 2, 1)]
        self.all_modules = nn.ModuleList(mods)

        # ---- runtime state (not part of state_dict) ----
        self._init_runtime()          # _packed, _tape, _plans (per batch of atom counts: descriptor + workspace, see _plan)
        self.max_blocks = -1          # tests: stop after this many blocks (the workspace then holds h and e of that block)
        self.last_flags = None        # after a bf16x3 call: the 4 int32 words jodo_cdgs_forward_split wrote ([3] = 1); else None
        self.split_bf16 = False       # the 3-D models' opt-in form; not built for this model (forward raises when set)
        self.bf16x3 = False           # opt-in, read per call: the split-bf16 (three-term) form of the node-row and edge-row GEMMs
                                      # (kc_gemm_s).  Combines with max_blocks.  The training path ignores it.
        self.train_bf16x3 = False     # opt-in, read per training-path call: the split-bf16 form of the training products (True = the forms
                                      # measured faster, mask 3; or a mask 0..7: 1 forward products, 2 data gradients, 4 weight gradients; train.split_mask).
                                      # Inference calls ignore it; get_step_fn does not set it.
        self.last_train_form = None   # the mask the last training-path forward ran with, read back from its engine

    # -- weights (cache, fingerprint, invalidation and the derived tape: _runtime.TapeRuntime) -----------
    def _key_tensors(self):
        return list(self.parameters()) + list(self.buffers())       # the GINE `eps` buffers are packed and read like the weights

    def _time_freq(self):
        half = self.nf // 2                       # the reference's sinusoid table, fp32 as it computes it
        return torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1)))

    def _pack(self, device):
        sd = dict(self.state_dict())
        sd['time_freq'] = self._time_freq()
        return capi.pack_weights_cdgs(self._cfg_struct, sd, None)

    def _pack_tape(self, blob_host, woff_c, n_woff, device):
        return capi.split_tape_cdgs(self._cfg_struct, blob_host, woff_c, n_woff, device)

    # -- per-batch descriptor and workspace -----------------------------------------------------------
    def _plan(self, node_mask, edge_mask, device, validate=True):
        if node_mask.shape[1] > MAX_N:
            raise NotImplementedError("CDGS: padded width N = %d above the limit of %d atoms" % (node_mask.shape[1], MAX_N))
        return self._cached_plan(node_mask, edge_mask, validate, lambda n_host, B, N: self._build_plan(n_host, B, N, device))

    def _build_plan(self, n_host, B, N, device):
        L = capi.lib()
        lay = (ctypes.c_int64 * 8)()
        n_ptr = n_host.ctypes.data_as(ctypes.c_void_p)
        capi.check(L.jodo_cdgs_layout(ctypes.byref(self._cfg_struct), B, N, n_ptr, lay), 'jodo_cdgs_layout')
        desc_host = torch.empty(int(lay[0]), dtype=torch.int32)
        capi.check(L.jodo_cdgs_fill_desc(ctypes.byref(self._cfg_struct), B, N, n_ptr, ctypes.c_void_p(desc_host.data_ptr()),
                                         ctypes.c_int64(int(lay[0]))), 'jodo_cdgs_fill_desc')
        return dict(desc=desc_host.to(device), ws=torch.zeros(int(lay[1]), dtype=torch.uint8, device=device),
                    flags=torch.zeros(4, dtype=torch.int32, device=device), n_nodes=n_host, B=B, N=N,
                    Nn=int(lay[2]), rows=int(lay[3]), h_off=int(lay[4]), e_off=int(lay[5]), code_off=int(lay[6]), land_off=int(lay[7]))

    # -- forward -------------------------------------------------------------------------------
    def forward(self, t, x, node_mask, edge_mask, context=None, *args, **kwargs):
        edge_x = kwargs['edge_x']
        if not x.is_cuda:
            raise RuntimeError("jodo_amd CDGS runs on an MI355X only (got a %s tensor); there is no CPU fallback — "
                               "use tests/oracle_cdgs.py for CPU checks" % x.device)
        if self.split_bf16:
            raise NotImplementedError("split_bf16 is not implemented for CDGS (exact fp32 only)")
        inputs_want_grad = any(t_ is not None and t_.requires_grad for t_ in (x, edge_x, t))
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if not self.hip_training and torch.is_grad_enabled() and (wants_grad or inputs_want_grad):
            raise NotImplementedError("CDGS is inference only: call it under torch.no_grad(), or set model.hip_training = True for the HIP "
                                      "training path (jodo_amd.losses.get_step_fn does)")
        if self.hip_training and torch.is_grad_enabled() and inputs_want_grad:
            raise RuntimeError("the HIP CDGS returns parameter gradients only: detach the inputs (the reference's loss needs no input "
                               "gradient)")
        B, N, dims = x.shape
        if dims != self.atom_ch or edge_x.shape != (B, N, N, self.edge_ch) or t.shape != (B,):
            raise ValueError("shape mismatch: x %s edge_x %s t %s" % (tuple(x.shape), tuple(edge_x.shape), tuple(t.shape)))
        if self.hip_training and (wants_grad or (self.training and self.dropout_p > 0)):
            # training path (csrc/cdgs_train.hip): activations kept for loss.backward(); under model.train() dropout is active in a
            # no-grad call too, as in the reference
            return self._forward_train(t, x, edge_x, node_mask, edge_mask, wants_grad)
        dev = x.device
        f32 = lambda v: v.detach().to(torch.float32).contiguous()
        x_, ex_, t_ = f32(x), f32(edge_x), f32(t)
        plan = self._plan(node_mask, edge_mask, dev)     # first: a new batch re-checks the weight fingerprint
        _, blob, woff_c, n_woff = self._weights(dev)
        out_x = torch.empty_like(x_)
        out_e = torch.empty_like(ex_)
        n_ptr = plan['n_nodes'].ctypes.data_as(ctypes.c_void_p)
        args = (ctypes.byref(self._cfg_struct), B, N, n_ptr, capi.ptr(plan['desc']), capi.ptr(blob), woff_c, n_woff, capi.ptr(t_),
                capi.ptr(x_), capi.ptr(ex_), capi.ptr(out_x), capi.ptr(out_e), capi.ptr(plan['ws']), int(self.max_blocks),
                capi.current_stream_ptr())
        if self.bf16x3:
            tape, toff = self._split_tape(dev)
            capi.check(capi.lib().jodo_cdgs_forward_split(*args, capi.ptr(tape), toff, capi.ptr(plan['flags'])), 'jodo_cdgs_forward_split')
            self.last_flags = plan['flags']
        else:
            capi.check(capi.lib().jodo_cdgs_forward(*args), 'jodo_cdgs_forward')
            self.last_flags = None
        self._last_plan = plan
        return out_x, out_e

    # -- training path (opt-in: hip_training) ------------------------------------------------------------
    def _train_engine(self, node_mask, edge_mask, device):
        """One TrainEngineCDGS (jodo_cdgs_train handle + device table) per batch of atom counts and padded width, in the module's
        bounded cache (_runtime.HostRuntime._engine_for_masks); an engine taken up again re-checks the device's free memory."""
        from ..train import TrainEngineCDGS
        return self._engine_for_masks(TrainEngineCDGS, self._cfg_struct, node_mask, edge_mask, device)

    def _forward_train(self, t, x, edge_x, node_mask, edge_mask, wants_grad):
        from ..train import cdgs_autograd, split_mask
        f32 = lambda v: v.detach().to(torch.float32).contiguous()
        mask = split_mask(self.train_bf16x3)
        eng = self._train_engine(node_mask, edge_mask, x.device)
        eng.set_form(mask)                                   # every call: the engine may be a cached one that last ran another form
        self.last_train_form = eng.form
        p, seed = self._dropout_draw()
        freq = self.__dict__.get('_train_freq')
        if freq is None or freq.device != x.device:
            freq = self.__dict__['_train_freq'] = self._time_freq().to(x.device)
        # the live tensors on every call, state_dict order: parameters and the GINE eps buffers (inputs without a gradient)
        tensors = list(self.state_dict(keep_vars=True).values())
        if wants_grad:
            return cdgs_autograd(eng, p, seed, freq, f32(t), f32(x), f32(edge_x), tensors)
        return eng.forward([q.detach().contiguous() for q in tensors], freq, f32(t), f32(x), f32(edge_x), p, seed)

    # -- tests: the state inside the workspace after the last call ------------------------------------
    def debug_state(self):
        """(h [Nn, nf], e [sum n^2, nf]) of the last call as the kernels left them: h compact over real atoms; e row
        eoff_b + r n_b + c, every ordered pair its own row, diagonal rows zero."""
        p = self._last_plan
        D, ws = self.nf, p['ws']
        h = ws[p['h_off']:p['h_off'] + p['Nn'] * D * 4].view(torch.float32).reshape(p['Nn'], D)
        e = ws[p['e_off']:p['e_off'] + p['rows'] * D * 4].view(torch.float32).reshape(p['rows'], D)
        return h.clone(), e.clone()

    def debug_rw(self):
        """(distance code int32 [sum n^2], landing probabilities [Nn, rw_depth]) of the last call's random-walk features, rows as in
        debug_state."""
        p = self._last_plan
        ws = p['ws']
        code = ws[p['code_off']:p['code_off'] + p['rows'] * 4].view(torch.int32)
        land = ws[p['land_off']:p['land_off'] + p['Nn'] * 16 * 4].view(torch.float32).reshape(p['Nn'], 16)
        return code.clone(), land[:, :self.rw_depth].clone()

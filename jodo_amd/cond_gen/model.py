"""MI355X-native property classifier of the conditional evaluation: the masked EGNN of the reference's cond_gen/model.py (the published
EDM classifier layout), under the reference's names `EGNN`, `get_model`, `get_classifier`.

Same constructor signature, parameter names / shapes / registration order (state_dict keys, `strict=True` loading, with or without a
leading `module.`) and the same call as the reference class:
    classifier(h0 [B*N, in_node_nf], x [B*N, 3], edges, edge_attr=None, node_mask [B*N, 1], edge_mask [B*N*N, 1], n_nodes=N) -> [B]
which is the call jodo_amd.sampling.get_cond_sampling_eval_fn / get_cond_multi_sampling_eval_fn make.  The arithmetic runs in
libjodo_hip.so (csrc/egnn_forward.hip, `jodo_egnn_forward`) on the current HIP stream: the first edge layer is hoisted to the atoms, the
per-edge message lives in registers only, and real atoms are compact (the result on real atoms does not depend on padding).  There is
no CPU or eager fallback: tests/oracle_egnn.py is the CPU checker.

Training is opt-in: with `classifier.hip_training = True` (jodo_amd.cond_gen.get_classifier_step_fn sets it) a grad-enabled call runs
csrc/egnn_train.hip through jodo_amd.train.TrainEngineEGNN and `loss.backward()` fills every parameter's gradient; a default module keeps
refusing grad-enabled calls.
"""
import ctypes
import pickle

import torch
from torch import nn

from .. import capi
from ..models._runtime import HostRuntime, lru_put, mask_counts


class _CfgEGNN(ctypes.Structure):               # jodo_egnn_cfg (include/jodo_hip.h)
    _fields_ = [('hidden_nf', ctypes.c_int32), ('n_layers', ctypes.c_int32), ('in_node_nf', ctypes.c_int32), ('attention', ctypes.c_int32),
                ('node_attr', ctypes.c_int32)]


class _GCLParams(nn.Module):
    """E_GCL_mask (cond_gen/model.py:181-197): parameters only, reference registration order (coord_mlp is deleted there)."""

    def __init__(self, nf, n_node_attr, attention):
        super().__init__()
        self.edge_mlp = nn.Sequential(nn.Linear(2 * nf + 1, nf), nn.SiLU(), nn.Linear(nf, nf), nn.SiLU())
        self.node_mlp = nn.Sequential(nn.Linear(2 * nf + n_node_attr, nf), nn.SiLU(), nn.Linear(nf, nf))
        if attention:
            self.att_mlp = nn.Sequential(nn.Linear(nf, 1), nn.Sigmoid())


class EGNN(HostRuntime, nn.Module):
    """The reference's EGNN property classifier (HIP)."""

    _engine_bound = 8

    def __init__(self, in_node_nf, in_edge_nf, hidden_nf, device='cpu', act_fn=nn.SiLU(), n_layers=4, coords_weight=1.0, attention=False,
                 node_attr=1):
        super().__init__()
        if in_edge_nf != 0:
            raise NotImplementedError("in_edge_nf=%r: the HIP classifier takes no edge attributes (in_edge_nf = 0)" % (in_edge_nf,))
        if not isinstance(act_fn, nn.SiLU):
            raise NotImplementedError("act_fn=%r: the HIP classifier implements SiLU only" % (act_fn,))
        if not 1 <= in_node_nf <= 16:
            raise NotImplementedError("in_node_nf=%r: the HIP classifier takes 1..16 node channels" % (in_node_nf,))
        if hidden_nf % 64 or not 64 <= hidden_nf <= 256:
            raise NotImplementedError("hidden_nf=%r: the HIP classifier is built for multiples of 64 in [64, 256]" % (hidden_nf,))
        if not 1 <= n_layers <= 16:
            raise NotImplementedError("n_layers=%r: the HIP classifier takes 1..16 layers" % (n_layers,))
        self.hidden_nf, self.device, self.n_layers = hidden_nf, device, n_layers
        self.in_node_nf, self.attention, self.node_attr = in_node_nf, bool(attention), node_attr
        self.coords_weight = coords_weight       # positions are never updated by the masked layer: kept for signature parity
        self._cfg_struct = _CfgEGNN(hidden_nf, n_layers, in_node_nf, int(bool(attention)), int(bool(node_attr)))
        # ---- parameter tree, reference construction / registration order (cond_gen/model.py:34-52) ----
        self.embedding = nn.Linear(in_node_nf, hidden_nf)
        for i in range(n_layers):
            self.add_module("gcl_%d" % i, _GCLParams(hidden_nf, in_node_nf if node_attr else 0, attention))
        self.node_dec = nn.Sequential(nn.Linear(hidden_nf, hidden_nf), nn.SiLU(), nn.Linear(hidden_nf, hidden_nf))
        self.graph_dec = nn.Sequential(nn.Linear(hidden_nf, hidden_nf), nn.SiLU(), nn.Linear(hidden_nf, 1))
        # ---- runtime state (not part of state_dict) ----
        self._init_runtime()          # _packed, _plans (here per (B, N, atom counts): descriptor + workspace)
        self.validate_masks = True    # one device pass per call: prefix node_mask, edge_mask = its off-diagonal outer product
        self.max_layers = -1          # tests: stop after this many layers; forward then returns the hidden state [Nn, hidden_nf]
        self.hip_training = False     # opt-in: grad-enabled calls go through the HIP training path (csrc/egnn_train.hip)
        self.to(self.device)

    # -- weights (cache, fingerprint and invalidation: models/_runtime.HostRuntime; _recheck_weights is never called here: the plan
    # lookup happens per call, and a recheck there would add a launch and a sync to every evaluation batch) -----------------------
    def _pack(self, device):
        return capi.pack_weights_egnn(self._cfg_struct, self.state_dict(), None)

    def load_state_dict(self, state_dict, strict=True, **kw):
        if state_dict and all(k.startswith('module.') for k in state_dict):      # a checkpoint saved from a DataParallel wrap
            state_dict = type(state_dict)((k[7:], v) for k, v in state_dict.items())
        return super().load_state_dict(state_dict, strict=strict, **kw)

    # -- per-batch descriptor and workspace -----------------------------------------------------------
    def _plan(self, node_mask, edge_mask, B, N, device):
        n_host = mask_counts(node_mask, edge_mask, B, N, self.validate_masks)
        key = (str(device), B, N, n_host.tobytes())
        plan = self._plans.get(key)
        if plan is None:
            L = capi.lib()
            lay = (ctypes.c_int64 * 8)()
            n_ptr = n_host.ctypes.data_as(ctypes.c_void_p)
            capi.check(L.jodo_egnn_layout(ctypes.byref(self._cfg_struct), B, N, n_ptr, lay), 'jodo_egnn_layout')
            desc_host = torch.empty(int(lay[0]), dtype=torch.int32)
            capi.check(L.jodo_egnn_fill_desc(ctypes.byref(self._cfg_struct), B, N, n_ptr, ctypes.c_void_p(desc_host.data_ptr()),
                                             ctypes.c_int64(int(lay[0]))), 'jodo_egnn_fill_desc')
            plan = dict(desc=desc_host.to(device), ws=torch.zeros(int(lay[1]), dtype=torch.uint8, device=device), n_nodes=n_host,
                        Nn=int(lay[2]), h_off=int(lay[3]))
        lru_put(self._plans, key, plan, 8)               # most recently used last
        return plan

    # -- forward -------------------------------------------------------------------------------
    def forward(self, h0, x, edges, edge_attr, node_mask, edge_mask, n_nodes):
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        inputs_want_grad = torch.is_grad_enabled() and (h0.requires_grad or x.requires_grad)
        if not self.hip_training and (wants_grad or inputs_want_grad):
            raise NotImplementedError("jodo_amd EGNN is inference only by default: call it under torch.no_grad().  Training is opt-in: "
                                      "set `hip_training = True` (jodo_amd.cond_gen.get_classifier_step_fn does) for parameter gradients")
        if inputs_want_grad:
            raise NotImplementedError("the HIP classifier returns parameter gradients only: input gradients (with respect to h0 or x) "
                                      "are not computed; detach the inputs")
        if edge_attr is not None:
            raise NotImplementedError("edge_attr must be None: the HIP classifier takes no edge attributes (in_edge_nf = 0)")
        N = int(n_nodes)
        if h0.dim() != 2 or h0.shape[1] != self.in_node_nf or h0.shape[0] % N or x.shape != (h0.shape[0], 3):
            raise ValueError("shape mismatch: h0 %s x %s n_nodes %d" % (tuple(h0.shape), tuple(x.shape), N))
        B = h0.shape[0] // N
        if edges is not None and edges[0].numel() != B * N * N:
            raise NotImplementedError("edges holds %d entries: the HIP classifier evaluates fully connected molecules (B * N * N = %d "
                                      "entries, as get_adj_matrix builds them) only" % (edges[0].numel(), B * N * N))
        if node_mask.numel() != B * N or (edge_mask is not None and edge_mask.numel() != B * N * N):
            raise ValueError("node_mask / edge_mask do not have B * N / B * N * N entries")
        if not h0.is_cuda:
            raise NotImplementedError("jodo_amd EGNN runs on an MI355X only (got a %s tensor); there is no CPU fallback — use "
                                      "tests/oracle_egnn.py for CPU checks, or move the module and its inputs to the GPU" % h0.device)
        dev = h0.device
        if wants_grad:
            return self._forward_train(h0, x, node_mask, edge_mask, B, N, dev)
        plan = self._plan(node_mask, edge_mask, B, N, dev)
        _, blob, woff_c, n_woff = self._weights(dev)
        h0_ = h0.detach().to(torch.float32).contiguous()
        x_ = x.detach().to(torch.float32).contiguous()
        out = torch.empty(B, dtype=torch.float32, device=dev)
        capi.check(capi.lib().jodo_egnn_forward(ctypes.byref(self._cfg_struct), B, N, plan['n_nodes'].ctypes.data_as(ctypes.c_void_p),
                                            capi.ptr(plan['desc']), capi.ptr(blob), woff_c, n_woff, capi.ptr(h0_), capi.ptr(x_),
                                            capi.ptr(out), capi.ptr(plan['ws']), int(self.max_layers), capi.current_stream_ptr()),
                   'jodo_egnn_forward')
        if self.max_layers >= 0:                         # tests: the hidden state on real atoms as the kernels left it
            nf = self.hidden_nf
            return plan['ws'][plan['h_off']:plan['h_off'] + plan['Nn'] * nf * 4].view(torch.float32).reshape(plan['Nn'], nf).clone()
        return out

    # -- training path (opt-in: hip_training) ------------------------------------------------------------
    def _train_engine(self, node_mask, edge_mask, B, N, device):
        """One TrainEngineEGNN (jodo_egnn_train handle + device tables) per set of atom counts, in the module's bounded cache
        (models/_runtime.HostRuntime._engine_for_counts)."""
        from ..train import TrainEngineEGNN
        n_host = mask_counts(node_mask, edge_mask, B, N, self.validate_masks)
        return self._engine_for_counts(TrainEngineEGNN, self._cfg_struct, n_host, N, device)

    def _forward_train(self, h0, x, node_mask, edge_mask, B, N, dev):
        from ..train import egnn_autograd
        if self.max_layers >= 0:
            raise NotImplementedError("max_layers is a switch of the inference forward")
        eng = self._train_engine(node_mask, edge_mask, B, N, dev)
        return egnn_autograd(eng, h0.detach().to(torch.float32).contiguous(), x.detach().to(torch.float32).contiguous(),
                             list(self.parameters()))


def get_model(args):
    """cond_gen/model.py:6-13."""
    if args.model_name == 'egnn':
        return EGNN(in_node_nf=5, in_edge_nf=0, hidden_nf=args.nf, device=args.device, n_layers=args.n_layers, coords_weight=1.0,
                    attention=args.attention, node_attr=args.node_attr)
    raise Exception('Wrong model name %s' % args.model_name)


def get_classifier(classifier_path, args_classifier_path, device='cpu'):
    """cond_gen/model.py:15-23: the published classifier layout — a pickled args object (nf, n_layers, attention, node_attr) plus a
    state_dict file, loaded with strict=True."""
    with open(args_classifier_path, 'rb') as f:
        args_classifier = pickle.load(f)
    args_classifier.device = device
    args_classifier.model_name = 'egnn'
    classifier = get_model(args_classifier)
    classifier.load_state_dict(torch.load(classifier_path, map_location=torch.device('cpu')), strict=True)
    return classifier

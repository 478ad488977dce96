"""Python plumbing of the training side behind the C ABI; device tensors in, device tensors out, no CPU
fallback.

  TrainEngineCDGS / cdgs_autograd  the same for CDGS (csrc/cdgs_train.hip), behind models/cdgs.py when `hip_training` is set
  TrainEngineEGNN / egnn_autograd  the same for the property classifier (csrc/egnn_train.hip), behind cond_gen/model.py when `hip_training` is set
  TrainEngine2D / dgt2d_autograd   the same for DGT_concat_2D (csrc/dgt2d_train.hip), behind models/dgt2d.py when `hip_training` is set
  TrainEngine / dgt_autograd   the whole score network under autograd: jodo_train_forward keeps the activations,
                               jodo_train_backward returns the gradient of every parameter (csrc/dgt_train.hip, train_ops.h,
                               train_gemm.hip) — what loss.backward() does in /root/reference/losses.py:286-385.  models/dgt.py
                               routes a grad-enabled forward here, so `loss.backward()` works on the registered module.

Checked by tests/test_train_gpu.py against torch.autograd through the CPU oracle, whose gradients are pinned by the reference's
own loss.backward() (tests/golden/grad_qm9.npz)."""
import ctypes

import numpy as np
import torch

from . import capi


class TrainEngine:
    """One batch shape (atom counts) of the training path: owns the jodo_train handle, its device tables and the workspace that
    carries the activations from forward to backward.  `lib` / `stream_ptr` exist for the build container's CPU suite, which
    drives the host-emulation build of the same sources (tests/emul/) with host tensors; the product path (models/dgt.py) never
    passes them and always runs libjodo_hip.so on the current HIP stream.

    The pool / slot / pinned-ring code is shared by every engine class: a subclass names its family of C entry points in `_abi`
    (TrainEngine2D and TrainEngineEGNN below: jodo_train2d_* / jodo_egnn_train_*, which mirror jodo_train_* one for one)."""

    _abi = 'jodo_train'

    def _fn(self, name):
        return getattr(self.L, '%s_%s' % (self._abi, name))

    @staticmethod
    def named_table(named_shapes):
        """The jodo_tensor array (names + shapes, no data) that jodo_train_create reads: built once per module."""
        n = len(named_shapes)
        arr = (capi.JodoTensor * n)()
        keep = []
        for i, (name, shape) in enumerate(named_shapes):
            shp = (ctypes.c_int64 * max(len(shape), 1))(*shape)
            nm = name.encode()
            keep.append((shp, nm))
            arr[i] = capi.JodoTensor(nm, None, shp, len(shape))
        return dict(arr=arr, keep=keep, n=n)

    @staticmethod
    def new_pool(slots=2):
        """Activation workspaces shared by the engines of one module.  A forward takes a slot that no pending backward needs; with
        `slots` = 2 two grad-enabled forwards may precede their backwards (gradient accumulation over two micro-batches, two loss
        terms — the reference's module allows any number).  When every slot is waiting for a backward the oldest is
        reused and ITS backward raises."""
        return {'slots': [{'buf': None, 'stamp': 0, 'live': False} for _ in range(slots)], 'stamp': 0}

    def __init__(self, cfg_struct, n_nodes, N, named_shapes, device, lib=None, stream_ptr=None, pool=None, options=None):
        self.L = lib if lib is not None else capi.lib()
        self._check = capi.check if lib is None else self._check_foreign
        self._stream = stream_ptr if stream_ptr is not None else capi.current_stream_ptr
        self.device = device
        named = named_shapes if isinstance(named_shapes, dict) else self.named_table(named_shapes)
        self._named = named                                      # keeps the ctypes name / shape storage alive
        self.n_params = named['n']
        n_host = np.ascontiguousarray(np.asarray(n_nodes, dtype=np.int32))
        self.B, self.N = int(n_host.shape[0]), int(N)
        self.handle = ctypes.c_void_p()
        self._check(self._fn('create')(ctypes.byref(cfg_struct), self.B, self.N, n_host.ctypes.data_as(ctypes.c_void_p), named['arr'],
                                             self.n_params, ctypes.byref(self.handle)), self._abi + '_create')
        self._fn('desc_bytes').restype = ctypes.c_size_t
        self._fn('workspace_bytes').restype = ctypes.c_size_t
        self._fn('desc_bytes').argtypes = [ctypes.c_void_p]
        self._fn('workspace_bytes').argtypes = [ctypes.c_void_p]
        for opt, val in (options or {}).items():                 # jodo_train_set_option, e.g. {0: 0} = op-by-op forward (tests)
            self._check(self._fn('set_option')(self.handle, int(opt), int(val)), self._abi + '_set_option')
        self.desc = torch.empty(self._fn('desc_bytes')(self.handle), dtype=torch.uint8, device=device)
        # The activation workspace (2.6 GB at QM9 batch 128) is shared by every engine of a module through `pool`: data loaders
        # produce a new set of atom counts every step, so handles come and go while the pool's buffers, grown to the largest request,
        # serve them all.  A slot's stamp names the forward whose activations it holds.
        self.ws_bytes = int(self._fn('workspace_bytes')(self.handle))
        self.pool = pool if pool is not None else self.new_pool()
        self._upload_tables()
        self.flags = torch.zeros(8, dtype=torch.int32, device=device)
        self._slot = None

    def _check_foreign(self, code, what=''):
        if code != 0:
            self.L.jodo_last_error.restype = ctypes.c_char_p
            raise capi.JodoHipError("%s failed (%d): %s" % (what, code, (self.L.jodo_last_error() or b'').decode()))

    def __del__(self):
        try:
            self._fn('destroy').argtypes = [ctypes.c_void_p]
            self._fn('destroy')(self.handle)
        except Exception:
            pass

    def _upload_tables(self):
        """Index tables -> device without a stream synchronisation: the handle's host image is staged through one of the pool's pinned
        buffers (a ring of four; a buffer is reused only after the copy that last read it has completed) and copied asynchronously on
        the current stream.  (jodo_train_upload, the plain C entry, synchronises instead: a shuffling loader creates an engine per
        step, and that synchronisation was the last one left in a training step.)"""
        n = int(self.desc.numel())
        if self._stream is not capi.current_stream_ptr:          # a caller-chosen stream: the plain (synchronising) upload on that stream
            self._check(self._fn('upload')(self.handle, capi.ptr(self.desc), self._stream()), self._abi + '_upload')
            return
        ring = self.pool.setdefault('pin', {'bufs': [None] * 4, 'events': [None] * 4, 'next': 0})
        i = ring['next']
        ring['next'] = (i + 1) % len(ring['bufs'])
        if ring['events'][i] is not None:
            ring['events'][i].synchronize()
        if ring['bufs'][i] is None or ring['bufs'][i].numel() < n:
            ring['bufs'][i] = torch.empty(int(n * 1.25) + 4096, dtype=torch.uint8, pin_memory=True)
        self._fn('desc_host').restype = ctypes.c_void_p
        self._fn('desc_host').argtypes = [ctypes.c_void_p]
        src = self._fn('desc_host')(self.handle)
        if not src:
            raise capi.JodoHipError(self._abi + "_desc_host returned NULL")
        ctypes.memmove(ring['bufs'][i].data_ptr(), src, n)
        self.desc.copy_(ring['bufs'][i][:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ring['events'][i] = ev

    @staticmethod
    def _ptrs(tensors):
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def _take_slot(self, device, keep):
        """A workspace slot for a forward: one that no pending backward needs (the most recently used of those first, so that a
        plain forward / backward loop stays in one buffer), else the oldest.  keep: this forward's backward will need it."""
        pool = self.pool
        free = [s_ for s_ in pool['slots'] if not s_['live']]
        slot = max(free, key=lambda s_: s_['stamp']) if free else min(pool['slots'], key=lambda s_: s_['stamp'])
        if slot['buf'] is None or slot['buf'].numel() < self.ws_bytes or slot['buf'].device != device:
            want = self._grown_bytes(slot['buf'], device)
            slot['buf'] = None                                   # release before growing
            slot['buf'] = torch.zeros(want, dtype=torch.uint8, device=device)
        pool['stamp'] += 1
        slot['stamp'], slot['live'] = pool['stamp'], bool(keep)
        return slot

    def _grown_bytes(self, buf, device):
        """The size of the workspace that replaces `buf` (None: the slot's first).  Grown with headroom: a shuffling loader's batches
        differ by a few per cent in sum n^2, and re-allocating gigabytes whenever a slightly larger one arrives stalls the step
        (batch 2 048: 440 ms per step instead of 190 while the maximum was still being found)."""
        return self.ws_bytes if buf is None else int(self.ws_bytes * 1.2)

    def check_free(self):
        """Called when a cached engine is taken up again.  Nothing to check here: TrainEngineCDGS, whose workspace grows with the padded
        width, looks at the device's free memory."""

    def _slot_or_raise(self, stamp):
        slot = self.slot_of(self.stamp if stamp is None else stamp)
        if slot is None:
            raise RuntimeError("the activations of this forward were overwritten by later training-path forwards of the same module "
                               "(%d activation workspaces per module, INTEGRATION.md §5); call backward earlier" % len(self.pool['slots']))
        return slot

    def _grad_buffer(self, params):
        """Gradient tensors like `params`, carved from one allocation (the library then zeroes them with a single fill), every slice on
        a 16-byte boundary — the layout of jodo_amd/optim.py slice_offsets, which the flat optimiser's parameter buffer has too.  The
        layout is computed once per engine."""
        from .optim import carve, slice_offsets
        lay = self.__dict__.get('_grad_layout')
        if lay is None:
            offs, total = slice_offsets([p.numel() for p in params])
            lay = self._grad_layout = ([tuple(p.shape) for p in params], offs, total)
        flat = torch.empty(lay[2], dtype=torch.float32, device=params[0].device)
        tail = lay[1][-1] + params[-1].numel()
        if tail != lay[2]:                                       # padding behind the LAST slice: no gradient buffer follows it, so the
            flat[tail:].zero_()                                  # library's fill does not reach it, and the norm of `flat` reads it
        return carve(flat, lay[0], lay[1])

    def forward(self, params, xh, edge_x, cond_x, cond_edge_x, noise_level, context, dropout_p, seed, keep=False, save_activations=True):
        """params: contiguous float32 tensors in the order of `named_shapes`.  Returns (out_xh, out_edge); the activations stay
        in a workspace slot of the pool (self.stamp names it) — until the next forward, or, with keep=True, until `backward` /
        `release` has been called for that stamp."""
        assert len(params) == self.n_params
        slot = self._take_slot(xh.device, keep)
        self._slot, self.stamp = slot, slot['stamp']
        out_x, out_e = torch.empty_like(xh), torch.empty_like(edge_x)
        if bool(save_activations) != getattr(self, '_saving', True):    # option 2: a forward nobody differentiates skips backward-only stores
            self._check(self._fn('set_option')(self.handle, 2, 1 if save_activations else 0), self._abi + '_set_option')
            self._saving = bool(save_activations)
        self._check(self._fn('forward')(
            self.handle, capi.ptr(self.desc), self._ptrs(params), self.n_params, capi.ptr(xh), capi.ptr(edge_x), capi.ptr(cond_x),
            capi.ptr(cond_edge_x), capi.ptr(noise_level), capi.ptr(context), ctypes.c_float(dropout_p), ctypes.c_uint64(seed),
            capi.ptr(out_x), capi.ptr(out_e), capi.ptr(self.flags), capi.ptr(slot['buf']), self._stream()), self._abi + '_forward')
        return out_x, out_e

    def release(self, stamp):
        """The activations of forward `stamp` are no longer needed (its backward ran, or never will): its slot may serve the next
        forward.  Called by `backward`, and by the autograd node's guard when a graph is dropped without a backward (an exception
        between forward and backward, a train-mode forward run for logging) — without it the slot stayed live forever and the
        following forward / backward loop allocated, and kept, a second workspace (gigabytes, see above)."""
        release_slot(self.pool, stamp)

    def slot_of(self, stamp):
        for s_ in self.pool['slots']:
            if s_['stamp'] == stamp and s_['buf'] is not None:
                return s_
        return None

    def debug_fetch(self, what, layer):
        """tests: a kept activation of the last forward (jodo_train_debug_locate) of block `layer`: 0 = hhat [Nn, D], 1 = alpha [R, H],
        2 = f1 [Nn, r D], 3 = a1 = SiLU(f1) x dropout, 4 = f2 [Nn, D], 5 = f3 [R, r De], 6 = a3 = SiLU(f3) x dropout, 7 = f4 [R, De]
        (f2, f4 before their dropout); flat float32."""
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        self._fn('debug_locate').argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self._check(self._fn('debug_locate')(self.handle, int(what), int(layer), ctypes.byref(off), ctypes.byref(cnt)), self._abi + '_debug_locate')
        buf = self._slot['buf']
        return buf[off.value:off.value + 4 * cnt.value].view(torch.float32).clone()

    def backward(self, params, noise_level, d_out_x, d_out_e, dropout_p, seed, stamp=None):
        """Gradients of every parameter for the forward `stamp` (default: this engine's last forward)."""
        slot = self._slot_or_raise(stamp)
        grads = self._grad_buffer(params)
        self._check(self._fn('backward')(
            self.handle, capi.ptr(self.desc), self._ptrs(params), self._ptrs(grads), self.n_params, capi.ptr(noise_level),
            capi.ptr(d_out_x), capi.ptr(d_out_e), ctypes.c_float(dropout_p), ctypes.c_uint64(seed), capi.ptr(slot['buf']),
            self._stream()), self._abi + '_backward')
        slot['live'] = False                                     # = release(stamp); a second backward over the same activations still works until a forward takes the slot
        return grads


class TrainEngine2D(TrainEngine):
    """The same for DGT_concat_2D (csrc/dgt2d_train.hip): `cfg_struct` is a jodo_cfg2d, xh has no position channels, and there is no
    context.  Pool, slots and the pinned staging ring are TrainEngine's.  debug_fetch knows five more selectors: 8 = xhat of the
    edges' LayerNorm1 [R, De], 9 = its rstd [R], 10 = et [R, De], 11 = t0 [R, QK], 12 = t1 [R, D]."""

    _abi = 'jodo_train2d'


class TrainEngineEGNN(TrainEngine):
    """The same for the property classifier (cond_gen EGNN, csrc/egnn_train.hip): `cfg_struct` is a jodo_egnn_cfg, the inputs are
    h0 [B, N, in_node_nf] and x [B, N, 3], the output is one float per molecule.  Pool, slots and the pinned staging ring are
    TrainEngine's.  debug_fetch selectors: 0 = h_layer [Nn, nf] (layer 0 .. n_layers), 1 = P [Nn, 2 nf], 2 = agg [Nn, nf],
    3 = SiLU(node_mlp.0 .) [Nn, nf]."""

    _abi = 'jodo_egnn_train'

    def forward(self, params, h0, x, keep=False):
        """params: contiguous float32 tensors in the order of `named_shapes`; h0, x: contiguous float32.  Returns out [B]; the kept
        tensors stay in a workspace slot of the pool (self.stamp names it)."""
        assert len(params) == self.n_params
        slot = self._take_slot(h0.device, keep)
        self._slot, self.stamp = slot, slot['stamp']
        out = torch.empty(self.B, dtype=torch.float32, device=h0.device)
        self._check(self._fn('forward')(self.handle, capi.ptr(self.desc), self._ptrs(params), self.n_params, capi.ptr(h0), capi.ptr(x),
                                        capi.ptr(out), capi.ptr(slot['buf']), self._stream()), self._abi + '_forward')
        return out

    def backward(self, params, d_out, stamp=None):
        """Gradients of every parameter for d_out [B] and the forward `stamp` (default: this engine's last forward)."""
        slot = self._slot_or_raise(stamp)
        grads = self._grad_buffer(params)
        self._check(self._fn('backward')(self.handle, capi.ptr(self.desc), self._ptrs(params), self._ptrs(grads), self.n_params,
                                         capi.ptr(d_out), capi.ptr(slot['buf']), self._stream()), self._abi + '_backward')
        slot['live'] = False
        return grads


TRAIN_BF16X3_ALL = 3      # what `train_bf16x3 = True` selects: forward products | data gradients.  Not the weight gradients (4): measured
                          # on MI355X their split form is not faster than the fp32 one; mask 7 or 4 still selects them


def split_mask(value):
    """`CDGS.train_bf16x3` -> the mask of jodo_cdgs_train_set_option 3: False / None 0, True TRAIN_BF16X3_ALL, an int 0..7 itself
    (1 forward products, 2 data gradients, 4 weight gradients); anything else raises."""
    if value is None or value is False:
        return 0
    if value is True:
        return TRAIN_BF16X3_ALL
    if isinstance(value, (int, np.integer)) and 0 <= int(value) <= 7:
        return int(value)
    raise ValueError("train_bf16x3 = %r: expected a bool or a mask 0..7 (1 forward products, 2 data gradients, 4 weight gradients)" % (value,))


class TrainEngineCDGS(TrainEngine):
    """The same for CDGS (csrc/cdgs_train.hip): `cfg_struct` is a jodo_cdgs_cfg, `named_shapes` lists every tensor of the state_dict
    (the GINE `local_model.eps` buffers included: inputs without a gradient), the inputs are t [B], x [B, N, atom_ch] and
    edge_x [B, N, N, edge_ch] plus the sinusoid's frequency table.  The workspace holds the reference's dense padded tensors (B N^2
    edge rows); `check_free` refuses a workspace larger than the device has free before anything is allocated.  Pool, slots and the
    pinned staging ring are TrainEngine's.  debug_fetch selectors: 0 = h after `layer` blocks [B N, nf], 1 = e after `layer` blocks
    [B N^2, nf], 2 = alpha of block `layer` [B N^2, n_heads], 3 = xhat of its norm2_edge [B N^2, nf].

    Option 3 (`options={3: mask}`, or `set_form(mask)` on an engine that exists — a cached one included) selects the product forms that
    run in split-bf16 (include/jodo_hip.h; 0 = exact fp32, the default); `form` reads the mask back from the handle.  The forward and the
    backward read it when they run; the autograd node re-sets its forward's mask before its backward."""

    _abi = 'jodo_cdgs_train'

    def set_form(self, mask):
        self._check(self._fn('set_option')(self.handle, 3, int(mask)), self._abi + '_set_option')

    @property
    def form(self):
        v = ctypes.c_int(-1)
        self._check(self._fn('get_option')(self.handle, 3, ctypes.byref(v)), self._abi + '_get_option')
        return int(v.value)

    def __init__(self, *args, **kwargs):
        if kwargs.get('lib') is not None:
            capi.bind_cdgs_train(kwargs['lib'])
        super().__init__(*args, **kwargs)
        names =[self._named['arr'][i].name.decode() for i in range(self.n_params)]
        self.is_buffer = [n.endswith('local_model.eps') for n in names]
        self.check_free()

    def _available(self, dev, releasing=0):
        """Bytes a new allocation on `dev` can get: what the driver reports free, what torch's allocator holds without using, and
        `releasing`, the size of a buffer that is dropped before the allocation."""
        return int(torch.cuda.mem_get_info(dev)[0]) + int(torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)) + int(releasing)

    def _refuse(self, avail):
        raise RuntimeError("CDGS training: the activation workspace of this batch (B = %d, N = %d: %d dense tile rows) needs %d bytes, "
                           "the device has %d bytes free; use a smaller batch" % (self.B, self.N, self.B * self.N * self.N, self.ws_bytes, avail))

    def check_free(self):
        """Raise at creation when no slot of the pool could ever hold this batch (no recompute or checkpointing form exists to fall back
        to).  The allocation itself is checked again, at its real size, in _take_slot."""
        dev = torch.device(self.device)
        if dev.type != 'cuda':
            return
        bufs = [s_['buf'].numel() for s_ in self.pool['slots'] if s_['buf'] is not None and s_['buf'].device == dev]
        if bufs and max(bufs) >= self.ws_bytes:
            return
        avail = self._available(dev, min(bufs) if len(bufs) == len(self.pool['slots']) else 0)     # a full pool grows by replacing a buffer
        if self.ws_bytes > avail:
            self._refuse(avail)

    def _grown_bytes(self, buf, device):
        """TrainEngine._grown_bytes checked against the device's free memory: the 20 % headroom when that fits, the exact size when
        only that fits, refused (bytes wanted, bytes free) when neither does."""
        want = super()._grown_bytes(buf, device)
        dev = torch.device(device)
        if dev.type == 'cuda':
            avail = self._available(dev, buf.numel() if buf is not None and buf.device == dev else 0)
            if want > avail:
                want = self.ws_bytes
            if want > avail:
                self._refuse(avail)
        return want

    def forward(self, tensors, time_freq, t, x, edge_x, dropout_p, seed, keep=False):
        """tensors: contiguous float32 tensors in the order of `named_shapes` (parameters and buffers).  Returns (atom_score, bond_score);
        the kept tensors stay in a workspace slot of the pool (self.stamp names it)."""
        assert len(tensors) == self.n_params
        slot = self._take_slot(x.device, keep)
        self._slot, self.stamp = slot, slot['stamp']
        out_x, out_e = torch.empty_like(x), torch.empty_like(edge_x)
        self._check(self._fn('forward')(
            self.handle, capi.ptr(self.desc), self._ptrs(tensors), self.n_params, capi.ptr(time_freq), capi.ptr(t), capi.ptr(x), capi.ptr(edge_x),
            ctypes.c_float(dropout_p), ctypes.c_uint64(seed), capi.ptr(out_x), capi.ptr(out_e), capi.ptr(slot['buf']), self._stream()),
            self._abi + '_forward')
        return out_x, out_e

    def backward(self, tensors, x, edge_x, d_out_x, d_out_e, dropout_p, seed, stamp=None):
        """Gradients of every PARAMETER of `tensors` (state_dict order, the buffers skipped) for the forward `stamp` (default: this
        engine's last forward)."""
        slot = self._slot_or_raise(stamp)
        grads = self._grad_buffer([p for p, buf in zip(tensors, self.is_buffer) if not buf])
        it = iter(grads)
        slots = (ctypes.c_void_p * self.n_params)(*[None if buf else next(it).data_ptr() for buf in self.is_buffer])
        self._check(self._fn('backward')(
            self.handle, capi.ptr(self.desc), self._ptrs(tensors), slots, self.n_params, capi.ptr(x), capi.ptr(edge_x), capi.ptr(d_out_x),
            capi.ptr(d_out_e), ctypes.c_float(dropout_p), ctypes.c_uint64(seed), capi.ptr(slot['buf']), self._stream()), self._abi + '_backward')
        slot['live'] = False
        return grads


def release_slot(pool, stamp):
    for s_ in pool['slots']:
        if s_['stamp'] == stamp:
            s_['live'] = False


class _SlotGuard:
    """Lives on the autograd context of one training-path forward; when the context dies (backward done and graph freed, or the
    graph dropped without a backward) the forward's workspace slot is released."""

    def __init__(self, pool, stamp):
        self.pool, self.stamp = pool, stamp

    def __del__(self):
        try:
            release_slot(self.pool, self.stamp)
        except Exception:
            pass


class _DGTTrainFn(torch.autograd.Function):
    """The score network as one autograd node: inputs need no gradient (the self-conditioning inputs are detached,
    losses.py:339); the parameters get theirs from jodo_train_backward."""

    @staticmethod
    def forward(ctx, engine, dropout_p, seed, xh, edge_x, cond_x, cond_edge_x, noise_level, context, *params):
        ps = [p.detach().contiguous() for p in params]
        out_x, out_e = engine.forward(ps, xh, edge_x, cond_x, cond_edge_x, noise_level, context, dropout_p, seed, keep=True)
        ctx.engine, ctx.dropout_p, ctx.seed, ctx.ps, ctx.nl = engine, dropout_p, seed, ps, noise_level
        ctx.stamp = engine.stamp
        ctx.slot_guard = _SlotGuard(engine.pool, engine.stamp)       # releases the slot when this context is dropped, backward or not
        return out_x, out_e

    @staticmethod
    def backward(ctx, d_out_x, d_out_e):
        grads = ctx.engine.backward(ctx.ps, ctx.nl, d_out_x.contiguous(), d_out_e.contiguous(), ctx.dropout_p, ctx.seed, stamp=ctx.stamp)
        return (None,) * 9 + tuple(grads)


def dgt_autograd(engine, dropout_p, seed, xh, edge_x, cond_x, cond_edge_x, noise_level, context, params):
    return _DGTTrainFn.apply(engine, dropout_p, seed, xh, edge_x, cond_x, cond_edge_x, noise_level, context, *params)


def dgt2d_autograd(engine, dropout_p, seed, xh, edge_x, cond_x, cond_edge_x, noise_level, params):
    """The 2-D score network (a TrainEngine2D) as the same autograd node: no context."""
    return _DGTTrainFn.apply(engine, dropout_p, seed, xh, edge_x, cond_x, cond_edge_x, noise_level, None, *params)


class _CDGSTrainFn(torch.autograd.Function):
    """CDGS as one autograd node: (atom_score, bond_score) from t, x, edge_x (no gradient) and the parameters; `is_param` tells the
    parameters from the buffers among `tensors` (state_dict order), whose gradients come from jodo_cdgs_train_backward."""

    @staticmethod
    def forward(ctx, engine, dropout_p, seed, time_freq, t, x, edge_x, *tensors):
        ts = [p.detach().contiguous() for p in tensors]
        out_x, out_e = engine.forward(ts, time_freq, t, x, edge_x, dropout_p, seed, keep=True)
        ctx.engine, ctx.dropout_p, ctx.seed, ctx.ts, ctx.x, ctx.edge_x = engine, dropout_p, seed, ts, x, edge_x
        ctx.stamp, ctx.form = engine.stamp, engine.form
        ctx.slot_guard = _SlotGuard(engine.pool, engine.stamp)
        return out_x, out_e

    @staticmethod
    def backward(ctx, d_out_x, d_out_e):
        ctx.engine.set_form(ctx.form)                        # the forms this forward ran with, whatever the engine served since
        grads = iter(ctx.engine.backward(ctx.ts, ctx.x, ctx.edge_x, d_out_x.contiguous(), d_out_e.contiguous(), ctx.dropout_p, ctx.seed,
                                         stamp=ctx.stamp))
        return (None,) * 7 + tuple(None if buf else next(grads) for buf in ctx.engine.is_buffer)


def cdgs_autograd(engine, dropout_p, seed, time_freq, t, x, edge_x, tensors):
    """(atom_score, bond_score) of a TrainEngineCDGS under autograd; tensors: the module's parameters and buffers in state_dict order."""
    return _CDGSTrainFn.apply(engine, dropout_p, seed, time_freq, t, x, edge_x, *tensors)


class _EGNNTrainFn(torch.autograd.Function):
    """The property classifier as one autograd node: out [B] from h0, x (no gradient) and the parameters, whose gradients come from
    jodo_egnn_train_backward."""

    @staticmethod
    def forward(ctx, engine, h0, x, *params):
        ps = [p.detach().contiguous() for p in params]
        out = engine.forward(ps, h0, x, keep=True)
        ctx.engine, ctx.ps, ctx.stamp = engine, ps, engine.stamp
        ctx.slot_guard = _SlotGuard(engine.pool, engine.stamp)
        return out

    @staticmethod
    def backward(ctx, d_out):
        grads = ctx.engine.backward(ctx.ps, d_out.to(torch.float32).contiguous(), stamp=ctx.stamp)
        return (None,) * 3 + tuple(grads)


def egnn_autograd(engine, h0, x, params):
    """out [B] of a TrainEngineEGNN under autograd; h0 [B, N, in_node_nf], x [B, N, 3] contiguous float32 device tensors."""
    return _EGNNTrainFn.apply(engine, h0, x, *params)

"""The host bookkeeping shared by the HIP model wrappers (models/dgt.py, dgt2d.py, cdgs.py, cond_gen/model.py): which weights a
kernel reads (the packed blob and what is derived from it), which plan a batch gets, which training engine a backward finds.  Nothing
here knows a model: a class supplies its packing call, its plan builder and its engine class."""
import numpy as np
import torch


def drop_packed_after_load(module, incompatible_keys):
    """load_state_dict post hook (module-level so that the module stays picklable)."""
    module.invalidate_packed_weights()


def mask_counts(node_mask, edge_mask, B, N, validate=True):
    """Atom counts on the host (contiguous int32 [B]).  With `validate`, node_mask must be a prefix mask and edge_mask (unless None) its
    off-diagonal outer product; the counts and both checks reach the host in ONE transfer (one stream sync per new batch).
    validate=False drops the comparison kernels as well (a loader that is known to build prefix masks, like the samplers'
    build_masks).  Counts that the caller already has on the host (`node_mask._jodo_counts`, jodo_amd/losses.py: the loader's batch is a
    CPU dict, so counts and the mask check cost nothing there) are taken as they are: no device round trip, and a training step then
    runs without any host synchronisation."""
    hint = getattr(node_mask, '_jodo_counts', None)
    if hint is not None and len(hint) == B:
        return np.ascontiguousarray(hint, dtype=np.int32)
    nm = node_mask.reshape(B, N)
    n_nodes = nm.sum(1).round().to(torch.int32)
    if not validate:
        return np.ascontiguousarray(n_nodes.cpu().numpy(), dtype=np.int32)
    prefix = torch.arange(N, device=nm.device).unsqueeze(0) < n_nodes.unsqueeze(1)
    ok = [(prefix.to(nm.dtype) == nm).all()]
    if edge_mask is not None:
        em = edge_mask.reshape(B, N, N)
        want = prefix.unsqueeze(1) & prefix.unsqueeze(2) & (~torch.eye(N, dtype=torch.bool, device=nm.device))
        ok.append((want.to(em.dtype) == em).all())
    host = torch.cat([n_nodes, torch.stack(ok).to(torch.int32)]).cpu().numpy()
    if not host[B]:
        raise ValueError("node_mask must be a prefix mask (real atoms first), as the samplers build it")
    if edge_mask is not None and not host[B + 1]:
        raise ValueError("edge_mask must be node_mask x node_mask with the diagonal removed")
    return np.ascontiguousarray(host[:B], dtype=np.int32)


def lru_put(cache, key, value, bound, evicted=None):
    """cache[key] = value as the most recently used entry of a dict that holds at most `bound`; `evicted` sees every entry that leaves
    (the oldest ones, and another value that was stored under `key`)."""
    old = cache.pop(key, None)
    if old is not None and old is not value and evicted is not None:
        evicted(old)
    while len(cache) >= bound:
        old = cache.pop(next(iter(cache)))
        if evicted is not None:
            evicted(old)
    cache[key] = value


class HostRuntime:
    """Mixin of the wrapper classes, in front of nn.Module.  A class provides `_pack(device)` and calls `_init_runtime()` at the end
    of its constructor."""

    _derived = ()                     # names of the attributes that hold something derived from `_packed`
    _engine_bound = 16                # training engines kept per module: handles are small (index tables); the workspace is shared

    def _init_runtime(self):
        self._plans = {}              # per batch: what the kernels need beside the weights, see _cached_plan
        self.invalidate_packed_weights()
        self.register_load_state_dict_post_hook(drop_packed_after_load)

    # -- weights -----------------------------------------------------------------------------
    def _key_tensors(self):
        """The tensors the kernels read: they enter the cache key and the fingerprint."""
        return list(self.parameters())

    def _repacked(self, device, blob):
        """What follows a re-pack; `blob` is what `_pack` returned (on the host unless the class packs on the device)."""

    def _weights(self, device):
        """`_packed` = (key, device blob, woff ctypes array, n_woff) of the current weights."""
        # cheap key checked on every call: tensor versions (bumped by optimizer steps, load_state_dict, p.copy_) and
        # storage addresses (model.to(...)).  In-place writes through `.data` (the reference's EMA copy_to / restore,
        # models/ema.py:44-66) bump neither: a content fingerprint is compared whenever a new plan is built (once per
        # sampling round, _cached_plan below), and invalidate_packed_weights() forces a re-pack explicitly.
        ts = self._key_tensors()
        key = (str(device),) + tuple(p._version for p in ts) + tuple(p.data_ptr() for p in ts)
        if self._packed is None or self._packed[0] != key:
            self.invalidate_packed_weights()
            blob, woff_c, n_woff = self._pack(device)
            self._packed = (key, blob.to(device), woff_c, n_woff)
            self._packed_fingerprint = self._fingerprint()
            self._repacked(device, blob)
        return self._packed

    def _fingerprint(self):
        """Content fingerprint of the key tensors: one fused norm launch + one reduction, one host sync."""
        norms = torch._foreach_norm([p.detach() for p in self._key_tensors()])
        w = torch.arange(1, len(norms) + 1, device=norms[0].device, dtype=torch.float64)
        return float((torch.stack([n.double() for n in norms]) * (1.0 + 1e-3 * w)).sum().item())

    def _recheck_weights(self):
        if self._packed is not None and self._fingerprint() != self._packed_fingerprint:
            self.invalidate_packed_weights()

    def invalidate_packed_weights(self):
        """Drop the packed kernel weights; the next forward re-packs from the current parameters.  Needed after
        in-place updates that do not bump tensor versions (`param.data.copy_(...)`, e.g. the reference's
        ExponentialMovingAverage.copy_to / restore, models/ema.py:44-66).  Everything derived from the blob goes with it: this is
        the only place that drops `_packed`."""
        self._packed = None
        for name in self._derived:
            setattr(self, name, None)

    # -- plans ---------------------------------------------------------------------------------
    def _cached_plan(self, node_mask, edge_mask, validate, build, evicted=None):
        """The plan of this batch: build(n_host, B, N) -> dict, once per mask."""
        # keyed by the mask's storage address, shape and version counter; the entry keeps the mask alive, so its storage cannot be
        # recycled for a different mask while the plan is cached (data_ptr alone would not be a safe key).  Not by tensor identity:
        # torch.nn.DataParallel — how the reference's create_model wraps the model (models/utils.py:27) — scatters every call's
        # arguments, and with one device that hands the module a fresh VIEW of the same mask on every call (same storage, same
        # version counter); identity would rebuild the plan on each of a round's 1000 calls.
        key = (node_mask.data_ptr(), tuple(node_mask.shape), tuple(node_mask.stride()), str(node_mask.device))
        plan = self._plans.get(key)
        if plan is not None and plan['mask_version'] == node_mask._version:
            return plan
        self._recheck_weights()                          # new batch (= new sampling round): catch `.data` weight updates
        B, N = node_mask.shape[0], node_mask.shape[1]
        plan = build(mask_counts(node_mask, edge_mask, B, N, validate), B, N)
        plan['mask'], plan['mask_version'] = node_mask, node_mask._version
        lru_put(self._plans, key, plan, 8, evicted)
        return plan

    # -- training engines ------------------------------------------------------------------------
    def _engine_for_masks(self, engine_cls, cfg, node_mask, edge_mask, device, opts=(), validate=True):
        """One engine (a handle + device tables) per batch of atom counts.  A shuffling loader practically never repeats a batch, so a
        real training step CREATES its engine (host tables of ~4 R ints, one upload): tools/train_bench.py times that case
        (`fresh_batches`) as its headline; the cache only serves repeated evaluation of one batch (tests, the self-conditioning
        double forward of a step).  opts: the sorted items of {set_option: value}."""
        # the same mask tensors as the previous call (the two forwards of a self-conditioned training step): the same engine, no host work
        last = self.__dict__.get('_train_last')
        if (last is not None and last[0] is node_mask and last[1] == node_mask._version and last[2] is edge_mask
                and last[3] == edge_mask._version and last[4] == opts):
            return last[5]
        B, N = node_mask.shape[0], node_mask.shape[1]
        eng = self._engine_for_counts(engine_cls, cfg, mask_counts(node_mask, edge_mask, B, N, validate), N, device, opts)
        self.__dict__['_train_last'] = (node_mask, node_mask._version, edge_mask, edge_mask._version, opts, eng)
        return eng

    def _engine_for_counts(self, engine_cls, cfg, n_host, N, device, opts=()):
        """Keyed by the counts themselves.  All engines of a module share its activation workspaces (TrainEngine.new_pool: two, so
        that a second grad-enabled forward may run before the first one's backward)."""
        key = (str(device), N, opts, n_host.tobytes())
        cache = self.__dict__.setdefault('_train_engines', {})
        eng = cache.get(key)
        if eng is None:
            # (the name / shape table of the state_dict is built once per module, not once per batch)
            named = self.__dict__.get('_train_named')
            if named is None:
                named = self.__dict__['_train_named'] = engine_cls.named_table([(k, tuple(v.shape)) for k, v in self.state_dict().items()])
            pool = self.__dict__.setdefault('_train_pool', engine_cls.new_pool())     # the activation workspace(s) of this module
            eng = engine_cls(cfg, n_host, N, named, device, pool=pool, options=dict(opts))
        else:
            eng.check_free()
        lru_put(cache, key, eng, self._engine_bound)
        return eng

    def _dropout_draw(self):
        """(p, seed) of one training-path forward.  Dropout masks are counter-based, keyed by a seed drawn from torch's generator (so
        torch.manual_seed reproduces a step)."""
        p = float(self.dropout_p) if self.training else 0.0
        return p, (int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0)

    def _replicate_for_data_parallel(self):
        """torch.nn.DataParallel with more than one device (the reference's create_model on a multi-GPU node, models/utils.py:27)
        shallow-copies the module into worker threads every forward: the copies would share this module's plan cache, ctypes
        handles and the packed weight blob on cuda:0.  Multi-GPU here is one process per GPU with the batch sharded by the sampler."""
        raise RuntimeError(
            "jodo_amd %s cannot be replicated by torch.nn.DataParallel over several devices: its plans, workspace and packed weights "
            "belong to one device.  Run one process per GPU (python -m torch.distributed.run --nproc-per-node N ...) and pass "
            "shard=(rank, world) to jodo_amd.sampling.get_sampling_fn (jodo_amd/dist.py, INTEGRATION.md section 3); "
            "DataParallel(model, device_ids=[one device]) is supported." % type(self).__name__)


class TapeRuntime(HostRuntime):
    """HostRuntime of the models whose opt-in `bf16x3` form reads a weight tape derived from the packed blob (DGT_concat_2D, CDGS).
    A class also provides `_pack_tape(blob_host, woff_c, n_woff, device)` -> (device tape, toff)."""

    _derived = ('_tape',)             # (the _packed it was derived from, device tape, toff ctypes array): valid for that _packed only

    def _repacked(self, device, blob):
        if self.bf16x3:                                  # the tape lives and dies with the blob it is derived from
            self._split_tape(device, blob)

    def _split_tape(self, device, blob_host=None):
        """(device tape, toff) of the split-bf16 form for the current `_packed`: host conversion of the packed blob + one upload, when
        the blob is re-packed with the switch on or on the first call with the switch on."""
        packed, t = self._packed, self._tape
        if t is None or t[0] is not packed:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("bf16x3 was switched on under graph capture for weights packed without it: run one eager call with "
                                   "bf16x3 = True first")
            if blob_host is None:
                blob_host = packed[1].cpu()
            tape, toff = self._pack_tape(blob_host, packed[2], packed[3], device)
            t = self._tape = (packed, tape, toff)
        return t[1], t[2]

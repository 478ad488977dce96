"""The reference's compute_mmd (evaluation/mmd.py) on the device: csrc/geometry_kernels.hip through jodo_mmd_batched.

`compute_mmd` carries the reference's name and signature and returns its float; `compute_mmd_many` evaluates any number of
(source, target) pairs in one call of three launches and returns them in order.  The value of a pair does not depend on what else is in
the call, and a call is bit-identical from run to run.  There is no CPU fallback.
"""
import numpy as np
import torch

from .. import capi

MAX_KERNEL_NUM = 8


def _check_side(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a 1-D GPU tensor of samples" % name)
    if not t.is_cuda:
        raise NotImplementedError("compute_mmd: %s is a CPU tensor; the MMD runs on the GPU only (no CPU fallback)" % name)
    if t.dim() != 1:
        raise ValueError("%s must be 1-D (one scalar per sample), got shape %s" % (name, tuple(t.shape)))
    if not t.dtype.is_floating_point:
        raise TypeError("%s must be a floating-point tensor, got %s" % (name, t.dtype))
    return t.float()


def tile_table(sizes):
    """[(n_s, n_t)] -> (tiles i32 [T,4]: segment, kind, x0, y0; tile_start i32 [S+1]) as numpy: what jodo_mmd_batched walks.  Kind 0 is
    source x source, 1 target x target (both: the tiles on and above the diagonal), 2 source x target (every tile)."""
    tile = capi.MMD_TILE
    rows, start = [], [0]
    for s, (ns, nt) in enumerate(sizes):
        count = 0
        for kind, (na, nb) in enumerate(((ns, ns), (nt, nt), (ns, nt))):
            nx, ny = -(-na // tile), -(-nb // tile)
            if nx == 0 or ny == 0:
                continue
            ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
            pick = (iy >= ix) if kind < 2 else np.ones_like(ix, dtype=bool)
            x0, y0 = ix[pick] * tile, iy[pick] * tile
            rows.append(np.stack([np.full_like(x0, s), np.full_like(x0, kind), x0, y0], 1))
            count += len(x0)
        start.append(start[-1] + count)
    tiles = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 4), np.int32)
    return tiles, np.asarray(start, np.int32)


def mmd_device(sources, targets, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """The batched call on checked device tensors -> device f64 [S].  No host synchronisation."""
    if len(sources) != len(targets) or not len(sources):
        raise ValueError("sources and targets are two lists of the same, non-zero length")
    kernel_num = int(kernel_num)
    if not 1 <= kernel_num <= MAX_KERNEL_NUM:
        raise ValueError("kernel_num is 1 .. %d, got %d" % (MAX_KERNEL_NUM, kernel_num))
    if not float(kernel_mul) > 0.:
        raise ValueError("kernel_mul must be positive")
    if fix_sigma is not None and float(fix_sigma) < 0.:
        raise ValueError("fix_sigma must not be negative")
    src = [_check_side('sources[%d]' % i, t) for i, t in enumerate(sources)]
    tgt = [_check_side('targets[%d]' % i, t) for i, t in enumerate(targets)]
    dev = src[0].device
    if any(t.device != dev for t in src + tgt):
        raise ValueError("all samples must be on one device")
    sizes = [(int(a.numel()), int(b.numel())) for a, b in zip(src, tgt)]
    pad = torch.zeros(1, dtype=torch.float32, device=dev)     # a buffer is never empty
    src_all, tgt_all = torch.cat(src + [pad]), torch.cat(tgt + [pad])
    so = np.concatenate([[0], np.cumsum([n for n, _ in sizes])])[:-1]
    to = np.concatenate([[0], np.cumsum([n for _, n in sizes])])[:-1]
    seg = np.stack([so, [n for n, _ in sizes], to, [n for _, n in sizes]], 1).astype(np.int64)
    tiles, start = tile_table(sizes)
    S, T = len(sizes), len(tiles)
    head = torch.from_numpy(np.concatenate([seg.reshape(-1).view(np.int32), start, tiles.reshape(-1)])).to(dev)      # one upload
    seg_dev, start_dev, tiles_dev = head[:8 * S].view(torch.int64), head[8 * S:9 * S + 1], head[9 * S + 1:]
    params = torch.empty(S, 12, dtype=torch.float32, device=dev)
    partials = torch.empty(max(T, 1), dtype=torch.float64, device=dev)
    out = torch.empty(S, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        capi.check(capi.lib().jodo_mmd_batched(
            S, T, capi.ptr(seg_dev), capi.ptr(tiles_dev) if T else capi.ptr(None), capi.ptr(start_dev), capi.ptr(src_all),
            capi.ptr(tgt_all), float(kernel_mul), kernel_num, float(fix_sigma) if fix_sigma else 0., capi.ptr(params), capi.ptr(partials),
            capi.ptr(out), capi.current_stream_ptr()), 'jodo_mmd_batched')
    return out


def compute_mmd_many(sources, targets, batch_size=1000, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """compute_mmd for every (sources[i], targets[i]) in one batched call -> list of floats, each bit-identical to the single call.
    `batch_size` is accepted and ignored."""
    return mmd_device(sources, targets, kernel_mul, kernel_num, fix_sigma).cpu().tolist()


def compute_mmd(source, target, batch_size=1000, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """evaluation/mmd.py:6-63 of the reference: the multi-bandwidth Gaussian MMD between two 1-D sample sets (device tensors) as a float:
    XX / n_s^2 + YY / n_t^2 - 2 XY / (n_s n_t) with the diagonals included; NaN for an empty side or all-identical samples, as there.
    `batch_size` (the reference's memory chunking) is accepted and ignored."""
    return compute_mmd_many([source], [target], batch_size, kernel_mul, kernel_num, fix_sigma)[0]

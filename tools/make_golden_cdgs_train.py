"""Training fixture of the CDGS model from the upstream reference (builders and stand-ins of tools/make_golden_cdgs.py), CPU, 8 threads.

  tests/golden/grad_cdgs_qm9.npz   one call of the reference's own 2-D loss (losses.py get_sde_2D_loss_fn, train=True, noise prediction)
                                   on the reference's own module with every block's dropout probability set to 0, on a mild batch:
                                   the loader batch's atom counts, the draws (t, node noise, edge noise), the network's inputs and
                                   outputs, the loss, d loss / d outputs, and per parameter the gradient's max-abs and sum, the full
                                   gradient for tensors of at most 4 096 entries and a seeded sample of 256 entries for the larger ones.

While recording it asserts that the reference's float32 gradients lie within a quarter of the 2e-4 bound (relative to each tensor's
largest entry) of its own float64 evaluation of the same call with the same draws, and that the file stays under 0.7 MB.

  tests/golden/train_drop_cdgs_qm9.npz   the same call under model.train() with every block's `dropout` module replaced by an object
                                   that applies the restated masks (tests/oracle_cdgs_train.drop_masks: site = 8 l + 1 .. 6, flat index of
                                   the reference's own tensor) in the reference's own call order; p, the mask seed, inputs, draws,
                                   outputs, d loss / d outputs and the same gradient summary.

Candidates (batch, seed) are tried in a fixed order and the first that meets the condition is recorded.
Run:  python tools/make_golden_cdgs_train.py
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from oracle.ref_import import load_reference                                        # noqa: E402
from make_golden_cdgs import CFG, OUT, THREADS, build_reference_model, _scheduler    # noqa: E402
from make_golden_2d import masks                                                    # noqa: E402
import oracle_cdgs_train as OCT                                                     # noqa: E402

GRAD_REF_REL, FULL_MAX, SAMPLE, MAX_BYTES = 2e-4, 4096, 256, 700_000


def loader_batch(cfg, n_nodes, seed):
    B, N = len(n_nodes), max(n_nodes)
    nm, em = masks(n_nodes)
    g = torch.Generator().manual_seed(seed)
    at = torch.randint(0, cfg.data.atom_types, (B, N), generator=g)
    bond = torch.triu(torch.randint(0, 4, (B, N, N), generator=g), 1)
    bond = bond + bond.transpose(1, 2)
    chans = [(bond > 0).float(), bond.float() / 3.] + ([(bond == 3).float()] if cfg.model.edge_ch == 3 else [])
    return dict(atom_mask=nm[..., 0], edge_mask=em, atom_one_hot=torch.nn.functional.one_hot(at, cfg.data.atom_types).float() * nm,
                edge_one_hot=torch.stack(chans, -1) * em.reshape(B, N, N, 1), formal_charges=torch.zeros(B, N, 1))


def one_call(ref, cfg, model, batch, seed, replay=None):
    """The reference's loss_fn(model, batch) under torch.manual_seed(seed); records the draws, the network's inputs and outputs and
    d loss / d outputs.  replay: the recorded draws of an earlier call, handed back (cast to the model's dtype) instead of drawn."""
    Lo = ref.losses
    dt = next(model.parameters()).dtype
    rec = {}
    orig_n, orig_e = Lo.sample_gaussian_with_mask, Lo.sample_symmetric_edge_feature_noise

    def rn(*a, **k):
        v = orig_n(*a, **k)
        rec['node_noise'] = v = v if replay is None else replay['node_noise'].to(v.dtype)
        return v

    def re_(*a, **k):
        v = orig_e(*a, **k)
        rec['edge_noise'] = v = v if replay is None else replay['edge_noise'].to(v.dtype)
        return v

    def pre(mod, args, kwargs):
        cast = lambda v: v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v
        return tuple(cast(a) for a in args), {k: cast(v) for k, v in kwargs.items()}

    def post(mod, args, kwargs, out):
        rec['t'], rec['z_t'], rec['edge_z_t'] = args[0].detach().clone(), args[1].detach().clone(), kwargs['edge_x'].detach().clone()
        out[0].retain_grad(), out[1].retain_grad()
        rec['out'] = out

    # the reference builds a few tensors in float32 whatever the module's dtype (the sinusoid, one-hot codes): every layer that owns
    # parameters gets its inputs in its own dtype, so the float64 evaluation is float64 from the first projection on
    hs = [m.register_forward_pre_hook(pre, with_kwargs=True) for m in model.modules() if list(m.parameters(recurse=False))]
    h1 = model.register_forward_pre_hook(pre, with_kwargs=True)
    h2 = model.register_forward_hook(post, with_kwargs=True)
    Lo.sample_gaussian_with_mask, Lo.sample_symmetric_edge_feature_noise = rn, re_
    try:
        loss_fn = Lo.get_sde_2D_loss_fn(_scheduler(ref, cfg), True, ref.utils.get_data_scaler(cfg), cfg)
        model.zero_grad()
        torch.manual_seed(seed)
        loss = loss_fn(model, batch)
        loss.backward()
    finally:
        Lo.sample_gaussian_with_mask, Lo.sample_symmetric_edge_feature_noise = orig_n, orig_e
        h1.remove(), h2.remove()
        for h in hs:
            h.remove()
    rec['loss'] = float(loss)
    rec['grads'] = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return rec


class MaskedDropout(torch.nn.Module):
    """Stands in for a block's nn.Dropout: the k-th call of a forward multiplies its argument by the k-th given array (the reference
    calls the module six times per block: h_local, h_attn, node FF hidden, node FF out, edge FF hidden, edge FF out)."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = masks, 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        assert m.numel() == x.numel()
        return x * m.reshape(x.shape).to(x.dtype)


def grad_fixture(ref, n_nodes=(7, 1, 6, 5), seed=7, drop=None):
    """drop: None (every block's dropout probability 0 -> grad_cdgs_qm9.npz) or (p, mask seed) -> train_drop_cdgs_qm9.npz."""
    cfg, model = build_reference_model(ref, CFG['qm9'], seed)
    cfg.device = torch.device('cpu')
    assert not cfg.model.pred_data and not cfg.model.self_cond
    fname = 'grad_cdgs_qm9.npz' if drop is None else 'train_drop_cdgs_qm9.npz'
    for l in range(cfg.model.n_layers):
        blk = model.all_modules[10 + 3 * l]
        assert isinstance(blk.dropout, torch.nn.Dropout)
        if drop is None:
            blk.dropout.p = 0.0                                # loss_fn calls model.train(): dropout off by probability, not by mode
        else:
            all_masks = OCT.drop_masks(drop[1], drop[0], len(n_nodes), max(n_nodes), cfg.model.n_layers, cfg.model.nf, dtype=torch.float32)
            blk.dropout = MaskedDropout([all_masks[(l, s)] for s in OCT.SITES])
    batch = loader_batch(cfg, list(n_nodes), seed + 1)
    r32 = one_call(ref, cfg, model, batch, seed)
    r64 = one_call(ref, cfg, copy.deepcopy(model).double(), batch, seed, replay=r32)
    worst = 0.0
    for k, g in r32['grads'].items():
        w = r64['grads'][k]
        worst = max(worst, float((g.double() - w).abs().max()) / (float(w.abs().max()) + 1e-30))
    if worst > 0.25 * GRAD_REF_REL:
        print("batch %s seed %d: the reference's float32 gradients are %.2e of their largest entry from float64: a milder batch is needed"
              % (list(n_nodes), seed, worst))
        return False
    if drop is not None:
        assert all(model.all_modules[10 + 3 * l].dropout.calls == 6 for l in range(cfg.model.n_layers))
    arrays = dict(torch_num_threads=torch.get_num_threads(), cfg_name=CFG['qm9'], seed=seed, n_nodes=np.array(n_nodes), loss=r32['loss'],
                  p=0.0 if drop is None else drop[0], drop_seed=0 if drop is None else drop[1],
                  loss64=r64['loss'], ref_f32_vs_f64=worst, t=r32['t'].numpy(), z_t=r32['z_t'].numpy(), edge_z_t=r32['edge_z_t'].numpy(),
                  node_noise=r32['node_noise'].numpy(), edge_noise=r32['edge_noise'].numpy(), out_x=r32['out'][0].detach().numpy(),
                  out_e=r32['out'][1].detach().numpy(), d_out_x=r32['out'][0].grad.numpy(), d_out_e=r32['out'][1].grad.numpy())
    names = list(r32['grads'].keys())
    arrays['grad_names'] = np.array(names)
    arrays['grad_maxabs'] = np.array([float(r32['grads'][k].abs().max()) for k in names], dtype=np.float64)
    arrays['grad_sum'] = np.array([float(r32['grads'][k].double().sum()) for k in names], dtype=np.float64)
    g = torch.Generator().manual_seed(seed)
    for i, k in enumerate(names):
        flat = r32['grads'][k].reshape(-1)
        if flat.numel() <= FULL_MAX:
            arrays['grad_%d' % i] = flat.numpy()
        else:
            idx = torch.randperm(flat.numel(), generator=g)[:SAMPLE].sort().values
            arrays['idx_%d' % i], arrays['grad_%d' % i] = idx.numpy().astype(np.int64), flat[idx].numpy()
    path = os.path.join(OUT, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, "%s is %d bytes" % (fname, size)
    print(fname + ' ok: %d parameters, loss %.6f (float64 %.6f), float32 vs float64 %.2e of the largest entry, %d bytes'
          % (len(names), r32['loss'], r64['loss'], worst, size))
    return True


if __name__ == '__main__':
    torch.set_num_threads(THREADS)
    ref_ = load_reference()
    # per file the first candidate that meets the recording condition (a ReLU argument within float32 rounding of zero breaks it by itself)
    for drop_ in [d_ for d_ in (None, (0.1, 2 ** 32 + 12345)) if not sys.argv[1:] or ('drop' if d_ else 'grad') in sys.argv[1:]]:
        for cand in ((7, 1, 6, 5), (5, 4, 6), (4, 3, 5), (3, 4), (3, 2)):
            if any(grad_fixture(ref_, cand, seed, drop_) for seed in (7, 8, 9)):
                break
        else:
            raise SystemExit("no candidate batch met the recording condition")

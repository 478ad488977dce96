"""Fixtures of the property classifier (tests/golden/egnn_*.npz), recorded from the reference's own EGNN module on the CPU.

    python tools/make_egnn_golden.py            (JODO_REFERENCE_ROOT names the reference checkout, see oracle/ref_import.py)

The reference's cond_gen/model.py is imported from its path at run time; nothing of it is kept here.  Weights are NOT stored: both
sides regenerate them with jodo_amd.models.init_utils.deterministic_init_(module, seed, gain=1.0) (gain 1.5 overflows this residual-sum
network).  Per setting two files, each under the size limit for committed files:
  egnn_<tag>.npz      settings, seed, the ordered state_dict keys and shapes, inputs (atom counts, one-hot atoms, positions), the fp32
                      and the float64 output, the fp32 hidden state after every layer on real atoms (forward hooks on gcl_<l>)
  egnn_<tag>_h64.npz  the float64 hidden state after the first and (with more than one layer) after the last layer
Inputs are drawn at a fixed width (80) and sliced to the padded width (65): torch.randn(N, 3) changes its leading values with N.
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jodo_amd.models.init_utils import deterministic_init_          # noqa: E402
from jodo_amd.sampling import build_masks, full_edge_index          # noqa: E402
from oracle.ref_import import REFERENCE_ROOT                         # noqa: E402

N_NODES = [1, 2, 5, 29, 31, 32, 33, 64, 65]
DRAW_WIDTH, WIDTH, IN_NF = 80, 65, 5
# (hidden_nf, n_layers, attention, node_attr, seed); the last one completes attention x node_attr for the state_dict test
SETTINGS = [(128, 7, 1, 0, 11), (64, 2, 0, 1, 12), (256, 1, 1, 1, 13), (192, 3, 1, 0, 14), (64, 1, 0, 0, 15)]


def tag(nf, layers, att, na):
    return 'nf%d_l%d_a%d_n%d' % (nf, layers, att, na)


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    B = len(N_NODES)
    x = 1.5 * torch.randn(B, DRAW_WIDTH, 3, generator=g)
    at = torch.randint(0, IN_NF, (B, DRAW_WIDTH), generator=g)
    nm, em = build_masks(N_NODES, WIDTH, 'cpu')
    h0 = torch.nn.functional.one_hot(at[:, :WIDTH], IN_NF).float() * nm
    return h0, x[:, :WIDTH] * nm, nm, em


def run(module, h0, x, nm, em, dtype):
    B, N = nm.shape[0], nm.shape[1]
    hidden = []
    real = nm.reshape(-1) > 0
    hooks = [module._modules['gcl_%d' % l].register_forward_hook(lambda m, i, o: hidden.append(o[0].detach()[real].clone()))
             for l in range(module.n_layers)]
    with torch.no_grad():
        out = module(h0=h0.reshape(B * N, -1).to(dtype), x=x.reshape(B * N, 3).to(dtype), edges=full_edge_index(N, B, 'cpu'), edge_attr=None,
                     node_mask=nm.reshape(B * N, 1).to(dtype), edge_mask=em.reshape(B * N * N, 1).to(dtype), n_nodes=N)
    for hk in hooks:
        hk.remove()
    return out, torch.stack(hidden)


def main():
    spec = importlib.util.spec_from_file_location('jodo_reference_cond_gen_model', os.path.join(REFERENCE_ROOT, 'cond_gen', 'model.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.set_num_threads(8)
    out_dir = os.path.join(ROOT, 'tests', 'golden')
    for nf, layers, att, na, seed in SETTINGS:
        m32 = ref.EGNN(IN_NF, 0, nf, n_layers=layers, attention=bool(att), node_attr=na)
        with torch.no_grad():
            deterministic_init_(m32, seed=seed, gain=1.0)
        m32.eval()
        m64 = copy.deepcopy(m32).double()
        h0, x, nm, em = inputs(seed)
        o32, h32 = run(m32, h0, x, nm, em, torch.float32)
        o64, h64 = run(m64, h0, x, nm, em, torch.float64)
        sd = m32.state_dict()
        keys = list(sd)
        shapes = np.zeros((len(keys), 2), dtype=np.int64)
        for i, k in enumerate(keys):
            shapes[i, :sd[k].dim()] = list(sd[k].shape)
        name = os.path.join(out_dir, 'egnn_%s.npz' % tag(nf, layers, att, na))
        np.savez_compressed(name, hidden_nf=nf, n_layers=layers, attention=att, node_attr=na, in_node_nf=IN_NF, seed=seed, gain=1.0,
                            keys=np.array(keys), shapes=shapes, n_nodes=np.array(N_NODES, dtype=np.int64), h0=h0.numpy(), x=x.numpy(),
                            out32=o32.numpy(), out64=o64.numpy(), hid32=h32.numpy(),
                            hid_e32=(h32.double() - h64).abs().amax(dim=(1, 2)).numpy())
        np.savez_compressed(name[:-4] + '_h64.npz', **({'first': h64[0].numpy()} if layers == 1 else {'first': h64[0].numpy(), 'last': h64[-1].numpy()}))
        print('%s: |out| max %.3g, fp32 - f64 %.3g (output) %.3g (hidden); %d + %d bytes' % (
            os.path.basename(name), float(o64.abs().max()), float((o32.double() - o64).abs().max()), float((h32.double() - h64).abs().max()),
            os.path.getsize(name), os.path.getsize(name[:-4] + '_h64.npz')))


if __name__ == '__main__':
    main()

"""Machine-independent deterministic weight initialisation.

Trained JODO checkpoints are external downloads and unavailable offline, so tests and benchmarks
need identical random weights in the build container (where the real reference is initialised with
them to produce fixtures) and on the GPU box (where our module is).  torch's default init depends on
construction order and generator state; this one depends only on (seed, parameter name, shape):
numpy PCG64 streams keyed by crc32(name).  Distributions follow torch's defaults for each layer kind
(U(+-1/sqrt(fan_in)) for Linear weight and bias, U(0,3) for the GBF means/stds, N(0,1) for the
sinusoid frequencies; GroupNorm scale U(0.5, 1.5) and shift U(-0.3, 0.3), GINE eps U(-0.2, 0.2),
all drawn away from their defaults so that tests see them); `gain` scales weight matrices to push activations out of the linear regime.
"""
import zlib

import numpy as np
import torch


@torch.no_grad()
def deterministic_init_(module, seed=0, gain=1.0, coord_scale=None):
    sd = module.state_dict()
    for name, t in sd.items():
        rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
        shape = tuple(t.shape)
        if name.endswith('means.weight') or name.endswith('stds.weight'):
            v = rng.uniform(0.0, 3.0, size=shape)
        elif name.endswith('coord_norm.scale'):
            v = np.full(shape, 1e-2 if coord_scale is None else coord_scale)
        elif name.endswith('.weights'):                       # learned sinusoid frequencies
            v = rng.standard_normal(size=shape)
        elif name.endswith('.weight') and len(shape) == 1:    # GroupNorm scale: away from 1, so that the affine part shows
            v = rng.uniform(0.5, 1.5, size=shape)
        elif name.endswith('.weight'):
            bound = 1.0 / np.sqrt(shape[1])
            v = rng.uniform(-bound, bound, size=shape) * gain
        elif name.endswith('.bias') and sd[name[:-4] + 'weight'].dim() == 1:    # GroupNorm shift: away from 0
            v = rng.uniform(-0.3, 0.3, size=shape)
        elif name.endswith('.bias'):
            w = sd[name[:-4] + 'weight']
            bound = 1.0 / np.sqrt(w.shape[1])
            v = rng.uniform(-bound, bound, size=shape)
        elif name.endswith('.eps'):                           # GINE's eps buffer [1]: PyG registers 0; drawn so that its use shows
            v = rng.uniform(-0.2, 0.2, size=shape)
        else:
            raise KeyError("unexpected parameter " + name)
        t.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    return module

"""Fixture of the property prior: tests/golden/prop_dist_cases.npz, recorded from the reference's own DistributionProperty on the CPU.

    python tools/make_golden_prop_dist.py       (JODO_REFERENCE_ROOT names the reference checkout, see oracle/ref_import.py)

The reference's cond_gen/property_distribution.py and cond_gen/utils.py are imported from their path at run time; nothing of them is
kept here.  Build machine only: no test, smoke() or benchmark imports this file or reads the reference.

The stand-in dataset (seeded, float32): 401 molecules with 3 .. 12 atoms, NO molecule with 7 atoms, ONE molecule with 3 atoms (range 0:
its bin is 0 whatever the value), and at 10 atoms three more molecules set to the maximum of every property (the reference's
`idx == n_bins` clamp moves them to the last bin).  y has 12 columns; prop2idx = {'alpha': 1, 'gap': 4, 'Cv': 11}, and id 11 goes through
`sub_Cv_thermo` (here: a recorded per-molecule value that differs from y[:, 11]).

prop_dist_cases.npz:
  num_atoms [M] i64, y [M, 12] f32, cv_sub [M] f32                 the inputs (cv_sub[i] = what sub_Cv_thermo returns for molecule i)
  prop_names [3] str, prop_ids [3] i64, num_bins                   prop2idx and the bin count (1000)
  counts [S] i64                                                   the atom counts that got a distribution, ascending
  probs [3, S, num_bins] f32, minmax [3, S, 2] f32                 distributions[prop][n]['probs'].probs and ['params']
  mean_mad [3, 2] f32                                              compute_mean_mad_from_dataset per property (the normalizer used below)
  sample_counts [64] i64, sample_seeds [2] i64                     the atom counts and torch.manual_seed values of the recorded draws
  samples [2, 64, 3] f32                                           sample_batch(sample_counts) under each seed
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import REFERENCE_ROOT                         # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'prop_dist_cases.npz')
PROP2IDX = {'alpha': 1, 'gap': 4, 'Cv': 11}
NUM_BINS = 1000
SEEDS = (0, 20240521)


def _load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REFERENCE_ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Data:
    def __init__(self, i, y, n):
        self.i, self.y, self.num_atom = i, y, n


class StandInDataset:
    """What the reference's prior touches of a dataset: indices(), get(i), sub_Cv_thermo(data); len / [] for its mean-mad helper."""

    def __init__(self, num_atoms, y, cv_sub):
        self.num_atoms, self.y, self.cv_sub = num_atoms, y, cv_sub

    def indices(self):
        return range(len(self.num_atoms))

    def get(self, i):
        return _Data(i, self.y[i:i + 1], self.num_atoms[i:i + 1])

    def sub_Cv_thermo(self, data):
        return self.cv_sub[data.i]

    def __len__(self):
        return len(self.num_atoms)

    def __getitem__(self, i):
        return self.get(i)


def make_inputs():
    g = torch.Generator().manual_seed(16)
    per_count = {3: 1, 4: 6, 5: 14, 6: 30, 8: 60, 9: 75, 10: 90, 11: 70, 12: 55}
    num_atoms = torch.cat([torch.full((m,), n, dtype=torch.long) for n, m in per_count.items()])
    num_atoms = num_atoms[torch.randperm(len(num_atoms), generator=g)]
    M = len(num_atoms)
    scale = torch.tensor([1., 9., 3., 0.02, 0.05, 0.03, 40., 0.1, 30., 30., 30., 4.])
    shift = torch.tensor([2., 75., -0.24, 0.01, 0.25, 1200., 0.15, -400., -400., -400., -400., 31.])
    y = (torch.randn(M, 12, generator=g) * scale + shift + num_atoms.float().unsqueeze(1) * 0.1 * scale).float()
    cv_sub = (y[:, 11] - num_atoms.float() * 2.981).float()
    ten = (num_atoms == 10).nonzero().reshape(-1)
    for col in (1, 4):                                        # three more molecules of 10 atoms at the maximum
        y[ten[:3], col] = y[ten, col].max()
    cv_sub[ten[:3]] = cv_sub[ten].max()
    return num_atoms, y, cv_sub


def main():
    ref = _load(os.path.join('cond_gen', 'property_distribution.py'), '_ref_property_distribution')
    ref_utils = _load(os.path.join('cond_gen', 'utils.py'), '_ref_cond_utils')
    torch.set_num_threads(8)
    num_atoms, y, cv_sub = make_inputs()
    ds = StandInDataset(num_atoms, y, cv_sub)
    names = list(PROP2IDX)
    mean_mad = [ref_utils.compute_mean_mad_from_dataset(ds, PROP2IDX[p]) for p in names]
    normalizer = {p: {'mean': mm[0], 'mad': mm[1]} for p, mm in zip(names, mean_mad)}
    prior = ref.DistributionProperty(ds, PROP2IDX, num_bins=NUM_BINS, normalizer=normalizer)
    counts = sorted(prior.distributions[names[0]].keys())
    assert 7 not in counts and counts[0] == 3 and all(sorted(prior.distributions[p].keys()) == counts for p in names)
    probs = torch.stack([torch.stack([prior.distributions[p][n]['probs'].probs for n in counts]) for p in names])
    minmax = torch.stack([torch.stack([torch.stack(list(prior.distributions[p][n]['params'])) for n in counts]) for p in names])
    assert float(minmax[0, 0, 0]) == float(minmax[0, 0, 1])                        # the single molecule with 3 atoms: range 0
    assert bool((probs[:, counts.index(10), NUM_BINS - 1] >= 3 / 90 - 1e-6).all())   # the tie at the maximum, clamped into the last bin
    g = torch.Generator().manual_seed(5)
    sample_counts = torch.tensor(counts)[torch.randint(0, len(counts), (64,), generator=g)]
    samples = []
    for seed in SEEDS:
        torch.manual_seed(seed)
        samples.append(prior.sample_batch(sample_counts))
    np.savez_compressed(
        GOLDEN, num_atoms=num_atoms.numpy(), y=y.numpy(), cv_sub=cv_sub.numpy(), prop_names=np.array(names),
        prop_ids=np.array([PROP2IDX[p] for p in names], np.int64), num_bins=np.int64(NUM_BINS), counts=np.array(counts, np.int64),
        probs=probs.numpy(), minmax=minmax.numpy(), mean_mad=np.array([[float(m[0]), float(m[1])] for m in mean_mad], np.float32),
        sample_counts=sample_counts.numpy(), sample_seeds=np.array(SEEDS, np.int64), samples=torch.stack(samples).numpy())
    print('wrote %s (%d bytes): %d molecules, counts %s' % (GOLDEN, os.path.getsize(GOLDEN), len(num_atoms), counts))


if __name__ == '__main__':
    main()

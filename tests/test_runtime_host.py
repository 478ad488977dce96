"""CPU: the shared host runtime of the model wrappers (jodo_amd/models/_runtime.py) — atom counts and mask validation, and the plan
cache with a fake plan builder.  The weight cache of the same module is tests/test_weight_coherence_host.py."""
import numpy as np
import pytest
import torch

from jodo_amd.models._runtime import HostRuntime, mask_counts
from jodo_amd.sampling import build_masks

COUNTS = [5, 3, 1]                    # the smallest counts with a full molecule, a padded one and a single atom
B, N = 3, 5


def _masks():
    return build_masks(COUNTS, N, 'cpu')


def test_counts_of_correct_masks():
    nm, em = _masks()
    got = mask_counts(nm, em, B, N)
    assert got.dtype == np.int32 and got.flags['C_CONTIGUOUS'] and got.tolist() == COUNTS
    assert mask_counts(nm.reshape(B * N, 1), em.reshape(B * N * N, 1), B, N).tolist() == COUNTS      # the classifier's flat masks


@pytest.mark.parametrize('case', ['hole', 'diagonal', 'padded_pair'])
def test_invalid_masks_raise(case):
    nm, em = _masks()
    em = em.reshape(B, N, N).clone()
    if case == 'hole':
        nm[1, 1] = 0.0                                            # atoms 0 and 2 real, 1 not: no prefix
        word = 'prefix'
    elif case == 'diagonal':
        em[0, 2, 2] = 1.0
        word = 'diagonal'
    else:
        em[1, 0, 4] = 1.0                                         # molecule 1 has 3 atoms: (0, 4) is a padded pair
        word = 'diagonal'
    with pytest.raises(ValueError, match=word):
        mask_counts(nm, em, B, N)


def test_node_mask_is_checked_first():
    nm, em = _masks()
    nm[1, 1] = 0.0
    em = torch.ones_like(em)
    with pytest.raises(ValueError, match='prefix'):
        mask_counts(nm, em, B, N)


def test_hint_is_returned_without_touching_the_masks():
    nm = torch.full((B, N, 1), float('nan'))                      # neither a prefix mask nor countable
    nm._jodo_counts = [4, 2, 2]
    got = mask_counts(nm, torch.full((B * N * N, 1), float('nan')), B, N)
    assert got.dtype == np.int32 and got.tolist() == [4, 2, 2]
    nm._jodo_counts = [4, 2]                                      # a hint of another batch size is not this batch's
    with pytest.raises(ValueError, match='prefix'):
        mask_counts(nm, None, B, N)


def test_no_edge_mask_skips_the_second_check():
    nm, em = _masks()
    assert mask_counts(nm, None, B, N).tolist() == COUNTS
    nm[1, 1] = 0.0
    with pytest.raises(ValueError, match='prefix'):
        mask_counts(nm, None, B, N)


def test_validate_false_counts_an_invalid_mask():
    nm, em = _masks()
    nm[1, 1] = 0.0
    em = em.reshape(B, N, N).clone()
    em[0, 2, 2] = 1.0
    assert mask_counts(nm, em, B, N, validate=False).tolist() == [5, 2, 1]


class _Cache(HostRuntime):
    """The plan cache alone: no weights (the recheck on a miss is counted), a fake builder."""

    def __init__(self):
        self._plans, self.rechecks, self.built = {}, 0, []

    def _recheck_weights(self):
        self.rechecks += 1

    def plan(self, nm, em, evicted=None, validate=True):
        def build(n_host, b, n):
            self.built.append((n_host.tolist(), b, n))
            return dict(serial=len(self.built))
        return self._cached_plan(nm, em, validate, build, evicted)


def test_plan_cache_is_keyed_on_mask_storage_and_version():
    c = _Cache()
    nm, em = _masks()
    plan = c.plan(nm, em)
    assert c.built == [(COUNTS, B, N)] and c.rechecks == 1 and plan['mask'] is nm
    assert c.plan(nm.view_as(nm), em) is plan and c.plan(nm[:], em) is plan           # a fresh view of the same mask: a hit
    assert len(c.built) == 1 and c.rechecks == 1
    other = c.plan(nm.clone(), em)                                                   # same content, other storage: a miss
    assert other is not plan and len(c.built) == 2 and c.rechecks == 2 and len(c._plans) == 2
    nm[2, 1] = 1.0                                                                   # an in-place write: the cached plan is stale
    with pytest.raises(ValueError, match='diagonal'):                                # (and the masks are validated again)
        c.plan(nm, em)
    em = build_masks([5, 3, 2], N, 'cpu')[1]
    fresh = c.plan(nm, em)
    assert fresh is not plan and c.built[-1] == ([5, 3, 2], B, N) and len(c._plans) == 2
    assert c.plan(nm, em) is fresh


@pytest.mark.parametrize('with_callback', [False, True])
def test_ninth_mask_evicts_the_oldest(with_callback):
    c = _Cache()
    seen = []
    evicted = seen.append if with_callback else None
    masks = [_masks() for _ in range(9)]
    plans = [c.plan(nm, em, evicted) for nm, em in masks[:8]]
    assert len(c._plans) == 8 and seen == []
    c.plan(*masks[8], evicted)
    assert len(c._plans) == 8 and len(c.built) == 9
    assert seen == ([plans[0]] if with_callback else [])
    assert c.plan(*masks[1], evicted) is plans[1] and len(c.built) == 9              # the second oldest is still there
    assert c.plan(*masks[0], evicted) is not plans[0] and len(c.built) == 10         # the oldest is not
    nm, em = masks[3]
    nm.mul_(1.0)                                                                     # a stale plan under its own key leaves too
    c.plan(nm, em, evicted)
    assert plans[3] in seen if with_callback else seen == []

"""CPU: the bookkeeping that decides which weights a kernel reads — the packed blob, the split-bf16 weight tape that follows it, and
the sub-batch split cache of n_streams > 1 (jodo_amd/models/dgt.py).  The C packers are replaced by counting fakes, so nothing here
needs the GPU; the GPU side of the same contract is tests/test_weight_coherence_gpu.py."""
import pytest
import torch

from jodo_amd import capi
from jodo_amd.models import get_model_class, deterministic_init_

from helpers import make_config


@pytest.fixture
def packers(monkeypatch):
    """Counting fakes of capi.pack_weights / capi.pack_split_tape.  The fake tape is derived from the state_dict it is given (its
    first value's sum), so a stale tape is told apart from a fresh one by content, not only by the counts."""
    calls = dict(blob=0, tape=0)

    def pack_weights(cfg_struct, state_dict, device=None):
        calls['blob'] += 1
        return torch.zeros(1), None, 0

    def pack_split_tape(cfg_struct, state_dict, device=None):
        calls['tape'] += 1
        return next(iter(state_dict.values())).detach().double().sum().reshape(1).clone()

    monkeypatch.setattr(capi, 'pack_weights', pack_weights)
    monkeypatch.setattr(capi, 'pack_split_tape', pack_split_tape)
    return calls


def _model():
    return deterministic_init_(get_model_class('DGT_concat')(make_config('vpsde_qm9_uncond_jodo')), seed=3).eval()


def _content(model):
    return next(iter(model.state_dict().values())).detach().double().sum()


def test_split_tape_follows_data_writes_and_invalidate(packers):
    """`param.data.copy_` / `.data.mul_` (the reference's EMA copy_to / restore) bump neither versions nor addresses: the blob is
    re-packed under the same key, and the tape must be re-packed with it — not served from the previous weights."""
    model = _model()
    tape = model._split_weights('cpu')
    assert packers == dict(blob=1, tape=1) and float(tape) == float(_content(model))
    assert model._split_weights('cpu') is tape and packers == dict(blob=1, tape=1)          # nothing changed: nothing re-packed
    versions = [p._version for p in model.parameters()]
    for p in model.parameters():
        p.data.mul_(2.0)
    assert [p._version for p in model.parameters()] == versions
    model.invalidate_packed_weights()
    tape = model._split_weights('cpu')
    assert packers == dict(blob=2, tape=2)
    assert float(tape) == float(_content(model))


def test_split_tape_follows_the_fingerprint_recheck(packers):
    """The same `.data` write caught by the content fingerprint a new sampling round checks (_recheck_weights, no explicit invalidate)."""
    model = _model()
    model._split_weights('cpu')
    model._recheck_weights()                                  # unchanged weights: the fingerprint matches, nothing is dropped
    model._split_weights('cpu')
    assert packers == dict(blob=1, tape=1)
    for p in model.parameters():
        p.data.mul_(2.0)
    model._recheck_weights()
    tape = model._split_weights('cpu')
    assert packers == dict(blob=2, tape=2)
    assert float(tape) == float(_content(model))


def test_split_tape_follows_version_bumping_writes(packers):
    model = _model()
    model._split_weights('cpu')
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(2.0)
    tape = model._split_weights('cpu')
    assert packers == dict(blob=2, tape=2)
    assert float(tape) == float(_content(model))


def test_pinned_plans_get_the_tape_of_the_current_pack(packers, monkeypatch):
    """Every plan holding a tape of an older pack generation is handed the current one; plans without a tape (not split) or with
    the current one are left alone.  Both forward paths (one stream and sub-batches) go through this."""
    model = _model()
    handed = []
    monkeypatch.setattr(type(model), '_hand_over_split', lambda self, plan: (handed.append(plan), plan.update(
        split_tape=self._split_weights('cpu'), split_key=self._split_tape[0])))
    model._split_weights('cpu')
    plans = [dict(split_tape=model._split_tape[1], split_key=model._split_tape[0]) for _ in range(2)] + [dict()]
    model._follow_weights(plans)
    assert handed == []
    for p in model.parameters():
        p.data.mul_(2.0)
    model.invalidate_packed_weights()
    model._weights('cpu')
    model._follow_weights(plans)
    assert handed == plans[:2] and packers == dict(blob=2, tape=2)
    assert all(float(p['split_tape']) == float(_content(model)) for p in plans[:2]) and 'split_tape' not in plans[2]


def test_sub_batch_split_is_keyed_on_mask_storage():
    """_split_of is cached like _plan: by the masks' storage, not their identity.  torch.nn.DataParallel over one device hands the
    module a fresh view of the same masks on every call; a fresh view must hit the cache (no recomputation, no host sync)."""
    from jodo_amd.sampling import build_masks
    model = _model()
    n_nodes = [3, 9, 17, 29, 12, 5, 1, 2, 28]
    nm, em = build_masks(n_nodes, max(n_nodes), 'cpu')
    parts = model._split_of(nm, em, 2)
    assert len(parts) == 2 and parts[0][0] == 0 and parts[-1][1] == len(n_nodes)
    assert model._split_of(nm.view_as(nm), em.view_as(em), 2) is parts
    assert model._split_of(nm[:], em[:], 2) is parts
    assert len(model._splits) == 1
    other = model._split_of(nm.clone(), em.clone(), 2)          # same content, other storage: an entry of its own
    assert other is not parts and [(lo, hi) for lo, hi, _, _ in other] == [(lo, hi) for lo, hi, _, _ in parts]
    assert len(model._splits) == 2
    assert model._split_of(nm, em, 3) is not parts and len(model._splits) == 3
    nm[-1].zero_()                                                # an in-place write to the mask: the cached split is stale
    nm[-1, :4] = 1.0
    fresh = model._split_of(nm, em, 2)
    assert fresh is not parts and len(model._splits) == 3
    assert model._split_of(nm.view_as(nm), em, 2) is fresh
    em.mul_(1.0)                                                  # the edge mask's version counts too
    assert model._split_of(nm, em, 2) is not fresh


# ---------------------------------------------------------------------------------------------
# the same contract for the models whose blob is packed on the host (jodo_amd/models/_runtime.py is the one implementation)
# ---------------------------------------------------------------------------------------------
def _build(kind):
    if kind == 'egnn':
        from jodo_amd.cond_gen.model import EGNN
        return EGNN(5, 0, 64, n_layers=2, attention=True, node_attr=1).eval()
    name, cfg = dict(dgt2d=('DGT_concat_2D', 'vpsde_zinc_2d_jodo'), cdgs=('CDGS', 'vpsde_qm9_2d_cdgs'))[kind]
    return deterministic_init_(get_model_class(name)(make_config(cfg)), seed=3).eval()


@pytest.fixture(params=['dgt2d', 'cdgs', 'egnn'])
def hosted(request, monkeypatch):
    """(model, calls): counting fakes of the model's host packer and, where the model has one, of its tape packer.  The fake blob is
    the content of the state_dict it is given and the fake tape is a copy of the blob it is derived from, so a stale blob or tape is
    told apart from a fresh one by content."""
    kind = request.param
    calls = dict(blob=0, tape=0)

    def pack(cfg_struct, state_dict, device=None):
        calls['blob'] += 1
        return next(iter(state_dict.values())).detach().double().sum().reshape(1).clone(), None, 0

    def tape(cfg_struct, blob_host, woff, n_woff, device=None):
        calls['tape'] += 1
        return blob_host.clone(), None

    monkeypatch.setattr(capi, 'pack_weights_' + dict(dgt2d='2d').get(kind, kind), pack)
    if kind != 'egnn':
        monkeypatch.setattr(capi, 'split_tape_' + dict(dgt2d='2d').get(kind, kind), tape)
        monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)      # (asks the driver: there is none here)
    model = _build(kind)
    if kind != 'egnn':
        model.bf16x3 = True
    return model, calls


def _check_repacked_once(model, calls, n):
    """The n-th pack happened exactly once, the blob holds the current weights, and the tape (where there is one) was rebuilt from it."""
    packed = model._weights('cpu')
    assert model._weights('cpu') is packed and packed is model._packed
    has_tape = hasattr(model, '_tape')
    assert calls == dict(blob=n, tape=n if has_tape else 0)
    assert float(packed[1]) == float(_content(model))
    if has_tape:
        assert model._tape[0] is model._packed
        tape, _ = model._split_tape('cpu')
        assert tape is model._tape[1] and float(tape) == float(_content(model)) and calls['tape'] == n


def _data_write(model):
    versions = [p._version for p in model.parameters()]
    for p in model.parameters():
        p.data.mul_(2.0)
    assert [p._version for p in model.parameters()] == versions


def test_hosted_blob_follows_version_bumping_writes(hosted):
    model, calls = hosted
    _check_repacked_once(model, calls, 1)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(2.0)
    _check_repacked_once(model, calls, 2)


def test_hosted_blob_follows_data_writes_and_invalidate(hosted):
    model, calls = hosted
    _check_repacked_once(model, calls, 1)
    _data_write(model)
    assert model._weights('cpu')[1] is not None and calls['blob'] == 1     # nobody told the module: the stale blob is still served
    model.invalidate_packed_weights()
    assert model._packed is None and getattr(model, '_tape', None) is None
    _check_repacked_once(model, calls, 2)


@pytest.mark.parametrize('hosted', ['dgt2d', 'cdgs'], indirect=True)
def test_hosted_blob_follows_the_fingerprint_recheck(hosted):
    """A `.data` write caught by the fingerprint: whatever drops `_packed` drops the tape derived from it.  (Not the classifier, which
    never rechecks: its plan lookup is per call, jodo_amd/cond_gen/model.py.)"""
    model, calls = hosted
    _check_repacked_once(model, calls, 1)
    model._recheck_weights()                                      # unchanged weights: the fingerprint matches, nothing is dropped
    assert model._packed is not None and model._tape[0] is model._packed
    _check_repacked_once(model, calls, 1)
    _data_write(model)
    model._recheck_weights()
    assert model._packed is None and model._tape is None
    _check_repacked_once(model, calls, 2)


def test_hosted_blob_follows_load_state_dict(hosted):
    model, calls = hosted
    _check_repacked_once(model, calls, 1)
    sd = {k: v.clone() * 2.0 for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    assert model._packed is None and getattr(model, '_tape', None) is None      # the post hook dropped both
    _check_repacked_once(model, calls, 2)

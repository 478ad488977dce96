"""Checkpoint ingestion: reference-format files (utils.py:7-30, models/ema.py:79-85)."""
import os

import pytest
import torch

from jodo_amd import configs
from jodo_amd.models import utils as mutils
from jodo_amd.models.ema import ExponentialMovingAverage
from jodo_amd.utils import load_for_sampling, restore_checkpoint, save_checkpoint


def _cfg():
    cfg = configs.get('vpsde_qm9_uncond_jodo')
    cfg.device = torch.device('cpu')
    return cfg


def test_ema_update_rule_and_positional_state():
    p = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.zeros(2), requires_grad=False),
         torch.nn.Parameter(torch.full((2,), 2.0))]
    ema = ExponentialMovingAverage(p, decay=0.999)
    assert len(ema.shadow_params) == 2                       # frozen tensors are skipped
    with torch.no_grad():
        p[0].add_(1.0)
    ema.update(p)
    d = min(0.999, 2 / 11)                                   # warm-up (1 + k) / (10 + k), k = 1
    assert torch.allclose(ema.shadow_params[0], torch.full((3,), 1.0 + (1 - d)))
    sd = ema.state_dict()
    assert set(sd) == {'decay', 'num_updates', 'shadow_params'} and sd['num_updates'] == 1
    ema.store(p)
    ema.copy_to(p)
    assert torch.allclose(p[0], ema.shadow_params[0])
    ema.restore(p)
    assert torch.allclose(p[0], torch.full((3,), 2.0))
    with pytest.raises(ValueError):
        ExponentialMovingAverage(p, decay=1.5)


def test_round_trip_and_ema_overwrite(tmp_path):
    cfg = _cfg()
    torch.manual_seed(3)
    model = mutils.create_model(cfg)
    ema = ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_decay)
    with torch.no_grad():
        for s in ema.shadow_params:
            s.mul_(0.5)
    path = str(tmp_path / 'ckpt' / 'checkpoint_7.pth')
    os.makedirs(os.path.dirname(path))
    save_checkpoint(path, dict(optimizer=None, model=model, ema=ema, step=7))
    raw = torch.load(path)
    assert all(k.startswith('module.') for k in raw['model'])  # DataParallel-style keys on disk
    model2, ema2, step = load_for_sampling(path, cfg, use_ema=True)
    assert step == 7
    for (k, a), b in zip(model.state_dict().items(), model2.parameters()):
        assert torch.equal(a * 0.5, b), k
    versions = [p._version for p in model2.parameters()]
    ema2.copy_to(model2.parameters())
    assert all(p._version > v for p, v in zip(model2.parameters(), versions))   # invalidates packed weights
    with pytest.raises(FileNotFoundError):
        load_for_sampling(str(tmp_path / 'missing.pth'), cfg)


def test_reference_written_checkpoint_loads_strict(tmp_path, golden_dir):
    """tests/golden/ckpt_ref_qm9.pth.xz: the bytes the reference's utils.save_checkpoint wrote for its own create_model(QM9)
    wrapper, EMA (one update) and Adam (oracle/make_golden.py checkpoint_fixture)."""
    import lzma
    path = str(tmp_path / 'checkpoint_ref.pth')
    with lzma.open(os.path.join(golden_dir, 'ckpt_ref_qm9.pth.xz'), 'rb') as f, open(path, 'wb') as out:
        out.write(f.read())
    raw = torch.load(path)
    ref_sd = raw['model']                                    # the reference wrapper's state_dict (`module.` keys)
    assert all(k.startswith('module.') for k in ref_sd)
    model, ema, step = load_for_sampling(path, _cfg(), use_ema=False)
    assert step == 123
    assert len(ref_sd) == len(model.state_dict())
    for (k, a), (k2, b) in zip(ref_sd.items(), model.state_dict().items()):
        assert k == k2 and torch.equal(a, b), (k, k2)
    ema.copy_to(model.parameters())
    shadow = raw['ema']['shadow_params']
    assert len(shadow) == len(list(model.parameters()))
    for s, b in zip(shadow, model.parameters()):
        assert torch.equal(s, b)
    # ... and a file written by this package restores the way the reference's utils.restore_checkpoint does it: the optimizer
    # state into an Adam over the reference's parameters, the model state with strict=True, the EMA state, the step
    path2 = str(tmp_path / 'checkpoint_ours.pth')
    save_checkpoint(path2, dict(optimizer=torch.optim.Adam(model.parameters()), model=model, ema=ema, step=5))
    ours = torch.load(path2)
    ref_params = [torch.nn.Parameter(v.clone()) for v in ref_sd.values()]        # the reference model has no buffers
    torch.optim.Adam(ref_params).load_state_dict(ours['optimizer'])
    assert list(ours['model']) == list(ref_sd)                                    # load_state_dict(strict=True): same keys ...
    for k, v in ours['model'].items():
        assert v.shape == ref_sd[k].shape, k                                      # ... and shapes
    assert set(ours['ema']) == set(raw['ema'])
    assert [s.shape for s in ours['ema']['shadow_params']] == [s.shape for s in shadow]
    assert ours['step'] == 5

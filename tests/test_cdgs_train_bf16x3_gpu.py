"""GPU: CDGS training with the products in split-bf16 (CDGS.train_bf16x3, TrainEngineCDGS option 3, csrc/train_gemm.hip k_gemm_s) at the
cases, yardsticks and unchanged bounds of tests/test_cdgs_train_gpu.py (tests/cdgs_train_common.py): forward under helpers.close64, every
parameter gradient under train2d_common.compare_grads, dropout against the masked oracle, the switch's read-back and bit equalities, three
AdamW steps through get_step_fn, refusals."""
import pytest
import torch

import cdgs_train_common as C
from helpers import FWD_RTOL, close64, make_config
from test_cdgs_train_gpu import _OracleModule, _loader_batch, _steps, d, engine_run, module_grads

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_MODELS = {}


def split_model(which):
    """One device model per config with hip_training on, this file's own (the switch is runtime state of the module)."""
    if which not in _MODELS:
        _MODELS[which] = C.fresh_model(which, device=DEV)[1]
        _MODELS[which].hip_training = True
    return _MODELS[which]


def grads_with(model, c, form):
    model.train_bf16x3 = form
    try:
        out, grads = module_grads(model, c)
        return out, grads, model.last_train_form
    finally:
        model.train_bf16x3 = False


@pytest.mark.parametrize('name', ['mixed', 'w9', 'geom', 'b65'])
def test_forward_and_all_gradients_match_the_oracle_in_the_split_form(name):
    c, (px, pe, want), (px32, pe32, want32) = C.yardsticks(name)
    model = split_model(c['which'])
    _, g32, ran32 = grads_with(model, c, False)
    (out_x, out_e), grads, ran = grads_with(model, c, 7)            # every form (True selects 3: the forms measured faster)
    assert (ran32, ran) == (0, 7)
    close64(out_x, px32, px, name + ' split x')
    close64(out_e, pe32, pe, name + ' split e')
    assert torch.equal(out_e, out_e.transpose(1, 2))
    assert len(grads) == len(want) == (254 if name == 'geom' else 326)
    w32 = C.compare_grads(g32, want, want32=want32, what=name + ' fp32 form')
    ws = C.compare_grads(grads, want, want32=want32, what=name + ' split form')
    print('%s: worst gradient error / bound: fp32 form %.4f, split form %.4f' % (name, w32, ws))


@pytest.mark.parametrize('form', [1, 2, 4])
def test_single_forms_stay_inside_the_bound_and_reach_their_products(form):
    """Masks 1 (forward products), 2 (data gradients), 4 (weight gradients) one at a time: inside the bound, and bitwise different from the
    fp32 form in at least one gradient — the option reaches that product form.  (Mask 1 also moves the outputs; 2 and 4 must not.)"""
    c, (px, pe, want), (px32, pe32, want32) = C.yardsticks('w9')
    model = split_model('qm9')
    out0, g0, _ = grads_with(model, c, 0)
    out1, g1, ran = grads_with(model, c, form)
    assert ran == form
    C.compare_grads(g1, want, want32=want32, what='w9 mask %d' % form)
    close64(out1[1], pe32, pe, 'w9 mask %d e' % form)
    differ = [k for (k, a), (_, b) in zip(g0, g1) if not torch.equal(a, b)]
    print('mask %d: %d of %d gradients differ bitwise from the fp32 form' % (form, len(differ), len(g0)))
    assert differ
    assert torch.equal(out0[1], out1[1]) == (form != 1)


def test_dropout_matches_the_masked_oracle_in_the_split_form():
    p, seed = 0.1, 12345
    c, (px, pe, want), (px32, pe32, want32) = C.drop_yardsticks('w12', p, seed)
    model = split_model('qm9')
    eng = model._train_engine(d(c['nm']), d(c['em']), torch.device(DEV))
    eng.set_form(7)
    try:
        _, _, out, grads = engine_run(model, c, p, seed)
        assert eng.form == 7
        out = (out[0].clone(), out[1].clone())
        close64(out[0], px32, px, 'w12 dropout split x')
        close64(out[1], pe32, pe, 'w12 dropout split e')
        C.compare_grads(grads, want, want32=want32, what='w12 dropout 0.1 split form')
    finally:
        eng.set_form(0)


def test_read_back_and_bit_equalities():
    c = C.yardsticks('w9')[0]
    model = split_model('qm9')
    _, never = C.fresh_model('qm9', device=DEV)
    never.hip_training = True
    assert never.train_bf16x3 is False and never.last_train_form is None
    out_n, g_n = module_grads(never, c)
    assert never.last_train_form == 0
    for form, mask in ((True, 3), (7, 7), (5, 5), (0, 0), (False, 0)):
        assert grads_with(model, c, form)[2] == mask
    # the same cached engine, back on the fp32 form: the bits of a model that never had the switch
    out_b, g_b, _ = grads_with(model, c, False)
    assert torch.equal(out_b[0], out_n[0]) and torch.equal(out_b[1], out_n[1])
    assert all(torch.equal(a[1], b[1]) for a, b in zip(g_b, g_n))
    # two backward calls with the switch on
    _, g1, _ = grads_with(model, c, 7)
    _, g2, _ = grads_with(model, c, 7)
    assert all(torch.equal(a[1], b[1]) for a, b in zip(g1, g2))
    assert not all(torch.equal(a[1], b[1]) for a, b in zip(g1, g_n))
    # bf16x3 (the inference switch) alone: training stays exact fp32
    never.bf16x3 = True
    out_i, g_i = module_grads(never, c)
    assert never.last_train_form == 0
    assert torch.equal(out_i[1], out_n[1]) and all(torch.equal(a[1], b[1]) for a, b in zip(g_i, g_n))
    # inference calls are untouched by train_bf16x3
    never.bf16x3 = False
    args = (d(c['t']), d(c['x']), d(c['nm']), d(c['em']))
    with torch.no_grad():
        plain = never(*args, edge_x=d(c['ex']))[1].clone()
        never.train_bf16x3 = True
        assert torch.equal(never(*args, edge_x=d(c['ex']))[1], plain)


def test_the_backward_runs_the_forms_of_its_forward():
    """The switch is read per forward; a backward that runs after the engine served another form re-sets its own."""
    c = C.yardsticks('w9')[0]
    model = split_model('qm9')
    _, want, _ = grads_with(model, c, 7)
    model.zero_grad(set_to_none=True)
    model.train_bf16x3 = 7
    out_x, out_e = model(d(c['t']), d(c['x']), d(c['nm']), d(c['em']), edge_x=d(c['ex']))
    model.train_bf16x3 = False
    with torch.no_grad():
        model._train_engine(d(c['nm']), d(c['em']), torch.device(DEV)).set_form(0)
    ((out_x * d(c['d_x'])).sum() + (out_e * d(c['d_e'])).sum()).backward()
    assert all(torch.equal(p.grad, w) for (_, p), (_, w) in zip(model.named_parameters(), want))


def test_three_steps_through_get_step_fn_with_the_switch_on():
    """tests/test_cdgs_train_gpu.py::test_training_steps_through_get_step_fn (a) with train_bf16x3 = True: every step's loss within
    2 x FWD_RTOL of the dense torch oracle's.  get_step_fn itself leaves the switch alone."""
    cfg = make_config('vpsde_qm9_2d_cdgs')
    cfg.device = DEV
    cfg.optim.warmup = 10
    cfg.model.dropout = 0.0
    batch = _loader_batch(cfg, [1, 2, 5, 17, 29, 9], 4)
    _, model = C.fresh_model('qm9', device=DEV)
    model.dropout_p = 0.0
    oracle = _OracleModule(model, cfg).to(DEV)
    model.train_bf16x3 = True
    _, losses, _ = _steps(cfg, model, batch, 3)
    assert model.train_bf16x3 is True and model.last_train_form == 3 and model.hip_training is True
    _, losses_o, _ = _steps(cfg, oracle, batch, 3)
    print('losses split form %s oracle %s' % (losses, losses_o))
    for a, b in zip(losses, losses_o):
        assert abs(a - b) <= 2 * FWD_RTOL * abs(b), (losses, losses_o)
    _, plain = C.fresh_model('qm9', device=DEV)
    plain.dropout_p = 0.0
    _steps(cfg, plain, batch, 1)
    assert plain.train_bf16x3 is False and plain.last_train_form == 0


def test_refusals():
    from jodo_amd import capi
    c = C.yardsticks('w9')[0]
    model = split_model('qm9')
    eng = model._train_engine(d(c['nm']), d(c['em']), torch.device(DEV))
    eng.set_form(5)
    for bad in (-1, 8, 255):
        with pytest.raises(capi.JodoHipError, match='mask 0..7'):
            eng.set_form(bad)
    assert eng.form == 5                                         # a refused value leaves the option as it was
    eng.set_form(0)
    for bad in (8, -1, 1.5, 'on'):
        model.train_bf16x3 = bad
        try:
            with pytest.raises(ValueError, match='train_bf16x3'):
                module_grads(model, c)
        finally:
            model.train_bf16x3 = False

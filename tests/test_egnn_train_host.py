"""CPU tests of the classifier's training side: the autograd-capable oracle against tests/oracle_egnn.py, its gradients on the fixture
cases, the opt-in switch, the loss and the saved layout."""
import pytest
import torch

import egnn_train_common as C
import oracle_egnn as OE
import oracle_egnn_train as OET
from jodo_amd.cond_gen import EGNN, classifier_loss, get_classifier, get_classifier_step_fn, save_classifier  # noqa: F401


@pytest.mark.parametrize("tag", C.CASES)
def test_autograd_oracle_equals_the_forward_oracle_and_no_gradient_vanishes(tag):
    _, st, sd, h0, x, n_nodes, d_out = C.case(tag)
    want, _ = OE.forward(sd, st, h0, x, n_nodes, torch.float64)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        assert torch.equal(OET.forward(sd64, st, h0.double(), x.double(), n_nodes), want)
    (out64, g64), (out32, g32) = C.yardsticks(tag)
    assert torch.equal(out64, want)
    assert set(g64) == set(sd)
    for k, g in g64.items():
        assert g.shape == sd[k].shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    # float32 autograd sits far inside the GPU test's bound (3e-4 of the tensor's scale): the widening is active on no tensor
    worst = max(float((g32[k].double() - g64[k]).abs().max()) / (3e-4 * float(g64[k].abs().max())) for k in g64)
    print("%s: float32 autograd at %.4f of the bound" % (tag, worst))
    assert 16 * worst < 1.0


def test_hip_training_is_opt_in_and_has_no_cpu_fallback():
    from jodo_amd.sampling import build_masks, full_edge_index
    m = EGNN(5, 0, 64, n_layers=1)
    assert m.hip_training is False
    nm, em = build_masks([2, 3], 3, 'cpu')
    args = dict(h0=torch.zeros(6, 5), x=torch.zeros(6, 3), edges=full_edge_index(3, 2, 'cpu'), edge_attr=None, node_mask=nm.reshape(6, 1),
                edge_mask=em, n_nodes=3)
    with pytest.raises(NotImplementedError, match="no_grad"):
        m(**args)
    m.hip_training = True
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        m(**args)
    with pytest.raises(NotImplementedError, match="input gradients"):
        m(**dict(args, x=torch.zeros(6, 3, requires_grad=True)))


def test_classifier_loss_inverts_the_evaluation_rescaling():
    g = torch.Generator().manual_seed(0)
    pred, label = torch.randn(7, generator=g), 3.0 + 2.0 * torch.randn(7, generator=g)
    mean, mad = 2.5, 1.75
    # the evaluation loops: pred * mad + mean against the property itself
    want = torch.nn.functional.l1_loss(pred * mad + mean, label) / mad
    assert abs(float(classifier_loss(pred, label, mean, mad)) - float(want)) < 1e-6
    assert float(classifier_loss((label - mean) / mad, label, mean, mad)) < 1e-7


def test_save_classifier_round_trips_through_get_classifier(tmp_path):
    st = dict(hidden_nf=64, n_layers=2, attention=1, node_attr=1, in_node_nf=5)
    m, sd = OE.init_state_dict(st, 4)
    cp, ap = str(tmp_path / 'classifier.npy'), str(tmp_path / 'args.pickle')
    save_classifier(m, cp, ap)
    back = get_classifier(cp, ap)
    assert (back.hidden_nf, back.n_layers, back.attention, back.node_attr) == (64, 2, True, 1)
    got = back.state_dict()
    assert list(got) == list(sd)
    for k in sd:
        assert torch.equal(got[k], sd[k]), k

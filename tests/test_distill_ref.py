"""CPU checks of the distillation rule (k210_yolo_framework_amd/distill.py): the numpy statement against tests/distill_ref.py's
torch autograd build, its properties, the host-side teacher check, and the figure the GPU test's absolute gradient tolerance rests on."""
import copy

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import distill, netspec
from k210_yolo_framework_amd.engine import YkError
from tests import distill_ref as R


@pytest.mark.parametrize('name', R.ALL_PARITY)
def test_autograd_equals_the_analytic_gradient(name):
    q, p, kw = R.parity_case(name)
    assert q.shape == p.shape and (np.abs(q).max() <= 4 or name == 'saturated')
    ta, ga = R.autograd(q, p, **kw)
    tn, gn = R.analytic(q, p, **kw)
    for term in R.TERMS:
        assert abs(ta[term] - tn[term]) <= 1e-12 * max(1.0, abs(tn[term])), (term, ta[term], tn[term])
        assert tn[term] >= 0
    assert abs(tn['total'] - (tn['obj'] + tn['cls'] + tn['box'])) <= 1e-12 * max(1.0, tn['total'])
    assert np.abs(ga - gn).max() <= 1e-12, np.abs(ga - gn).max()
    assert tn['total'] > 0 and np.abs(gn).max() > 0


@pytest.mark.parametrize('name', R.ALL_PARITY)
def test_every_elementwise_term_is_not_negative(name):
    q, p, _ = R.parity_case(name)
    assert (distill.kl(q, p) >= 0).all()


def test_kl_has_the_stated_derivative():
    """d kl / dp = sigmoid(p) - sigmoid(q), by central differences in float64."""
    rng = np.random.default_rng(0)
    q, p = rng.uniform(-4, 4, 200), rng.uniform(-4, 4, 200)
    num = (distill.kl(q, p + 1e-6) - distill.kl(q, p - 1e-6)) / 2e-6
    assert np.abs(num - (distill.sigmoid(p) - distill.sigmoid(q))).max() <= 1e-8


@pytest.mark.parametrize('name', ('head_7x10', 'saturated'))
def test_equal_outputs_give_exactly_zero(name):
    q, _, kw = R.parity_case(name)
    terms, grad = R.analytic(q, q.copy(), **kw)
    assert all(v == 0.0 for v in terms.values())
    assert (grad == 0).all()
    ta, ga = R.autograd(q, q.copy(), **kw)
    assert all(v == 0.0 for v in ta.values())
    assert np.abs(ga).max() <= 1e-16                                    # (autograd adds sigmoid(q) (-sigmoid(-p)) and (1 - sigmoid(q)) sigmoid(p))


def test_saturated_is_finite():
    q, p, kw = R.parity_case('saturated')
    assert set(np.unique(np.abs(q))) == {80.0} and set(np.unique(np.abs(p))) == {80.0}
    assert (q != p).any() and (q == p).any()
    for build in (R.analytic, R.autograd):
        terms, grad = build(q, p, **kw)
        assert all(np.isfinite(v) for v in terms.values()) and np.isfinite(grad).all()
    assert np.isfinite(distill.softplus(np.array([-80.0, 80.0, -745.0, 745.0]))).all()


def test_shapes_that_are_not_one_layer_are_refused():
    with pytest.raises(ValueError):
        distill.loss_and_grad(np.zeros((1, 4, 6)), np.zeros((1, 4, 7)))
    with pytest.raises(ValueError):
        distill.loss_and_grad(np.zeros((1, 4, 5)), np.zeros((1, 4, 5)))            # no class


def _spec(hw=(64, 96), anchors=3, classes=20, net='yolo_mobilev1', alpha=0.5):
    return netspec.NETWORKS[net]([hw[0], hw[1], 3], anchors, classes, alpha=alpha)


def test_check_teacher_accepts_another_network_of_the_zoo_and_names_each_difference():
    anchors = np.zeros((2, 3, 2), np.float32)
    student = _spec()
    distill.check_teacher(student, _spec(net='yolo_mobilev2', alpha=1.0), anchors)
    distill.check_teacher(student, _spec(alpha=1.0), anchors)
    with pytest.raises(YkError, match='class count.*teacher has 3 classes.*student 20'):
        distill.check_teacher(student, _spec(classes=3), anchors)
    with pytest.raises(YkError, match='output size: output 0 of the teacher is 3 x 4.*student 2 x 3'):
        other = copy.deepcopy(student)                                  # the same input size, another grid on output 0
        other.tensors[other.outputs[0]] = (3, 4, other.tensors[other.outputs[0]][2])
        distill.check_teacher(student, other, anchors)
    with pytest.raises(YkError, match='input size: the teacher takes 96 x 128.*student 64 x 96'):
        distill.check_teacher(student, _spec(hw=(96, 128)), anchors)
    with pytest.raises(YkError, match='anchor count: the teacher has 5 anchors per layer.*student 3'):
        distill.check_teacher(student, _spec(anchors=5), anchors)
    with pytest.raises(YkError, match='anchor count.*anchor table 4'):
        distill.check_teacher(student, _spec(), np.zeros((2, 4, 2), np.float32))
    one = _spec()
    one.outputs = one.outputs[:1]
    with pytest.raises(YkError, match='output count: the teacher has 1 output layers.*student 2'):
        distill.check_teacher(student, one, anchors)


def test_float32_build_of_the_reference_meets_the_recorded_atol():
    """What the GPU test's absolute gradient tolerance rests on: (a) in torch float32 against (a) in float64 at rtol 2e-5."""
    worst = 0.0
    for name in R.ALL_PARITY:
        q, p, kw = R.parity_case(name)
        _, g64 = R.autograd(q, p, **kw)
        t32, g32 = R.autograd(q, p, dtype=torch.float32, **kw)
        assert all(np.isfinite(v) for v in t32.values()) and np.isfinite(g32).all()
        a = R.atol_needed(g32, g64)
        print(name, 'float32 build needs atol', a)
        worst = max(worst, a)
    print('largest', worst, 'recorded', R.F32_ATOL_MEASURED)
    assert 0 < worst <= R.F32_ATOL_MEASURED

"""GPU parity of the distillation kernel (yk_distill_loss_f32, csrc/yk_distill.hip) against tests/distill_ref.py's float64
autograd build, and its way up to the Trainer.

Tolerances.  Loss entries: tests/test_gpu_loss.py's, 2e-5 of max(1, |reference|).  Gradient: rtol 2e-5 as there; the absolute term is
measured, not guessed: the reference evaluated in torch float32 on the CPU on these inputs needs atol 1.871e-8 against float64 at that rtol
(distill_ref.F32_ATOL_MEASURED, the largest over the parity cases; measured again by tests/test_distill_ref.py), and the kernel, another
fp32 evaluation of the same expression, is given twice that.  Where the kernel adds into a preloaded gradient g0 the stored sum is rounded
to fp32 once more: half an ulp of the result, 2^-24 |result|, is added to the bound there."""
import functools

import numpy as np
import pytest
import torch

from tests import distill_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2 * R.F32_ATOL_MEASURED
YK_ERR_ARG = -10


@functools.lru_cache(maxsize=None)
def _ref(name):
    q, p, kw = R.parity_case(name)
    return R.autograd(q, p, **kw)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(q, p, weight, batch_size, grad0=None, want_grad=True):
    """engine.distill_loss -> (loss[4], gradient buffer after the call | None)."""
    from k210_yolo_framework_amd import engine
    g = None
    if want_grad:
        g = torch.zeros(p.shape, dtype=torch.float32, device='cuda') if grad0 is None else _cu(grad0)
    loss = engine.distill_loss(_cu(q), _cu(p), weight, batch_size or p.shape[0], grad=g)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), None if g is None else g.cpu().numpy()


@pytest.mark.parametrize('name', R.ALL_PARITY)
def test_loss_and_gradient_vs_float64_autograd(name):
    """One row; the 7x10 head with batch_size 16 for 4 images; 255, 256 and 257 rows per image; 85 floats per row; every logit +-80."""
    q, p, kw = R.parity_case(name)
    ref_l, ref_g = _ref(name)
    loss, grad = _run(q, p, **kw)
    assert loss.shape == (4,) and grad.shape == p.shape
    for k, term in enumerate(R.TERMS):
        print(name, term, loss[k], ref_l[term], abs(loss[k] - ref_l[term]) / max(1.0, abs(ref_l[term])))
    print(name, 'grad: atol needed at rtol 2e-5:', R.atol_needed(grad, ref_g, RTOL), 'allowed', ATOL)
    for k, term in enumerate(R.TERMS):
        assert abs(loss[k] - ref_l[term]) <= 2e-5 * max(1.0, abs(ref_l[term])), (term, loss[k], ref_l[term])
    np.testing.assert_allclose(grad, ref_g, rtol=RTOL, atol=ATOL)
    # the same into a preloaded gradient: it accumulates
    g0 = np.random.default_rng(11).normal(0, 1, p.shape).astype(np.float32)
    loss_acc, acc = _run(q, p, grad0=g0, **kw)
    assert np.array_equal(_bits(loss_acc), _bits(loss))
    err = np.abs((acc.astype(np.float64) - g0) - ref_g)
    bound = RTOL * np.abs(ref_g) + ATOL + 2.0 ** -24 * np.abs(acc)
    print(name, 'accumulated: worst error / bound', float((err / bound).max()))
    assert (err <= bound).all()
    # without a gradient the loss entries keep their bits
    loss_only, none = _run(q, p, want_grad=False, **kw)
    assert none is None and np.array_equal(_bits(loss_only), _bits(loss))


@pytest.mark.parametrize('name', ('head_7x10', 'p257', 'saturated'))
def test_equal_outputs_give_zero_bits(name):
    q, _, kw = R.parity_case(name)
    loss, grad = _run(q, q.copy(), **kw)
    assert (_bits(loss) == 0).all(), loss                               # +0.0, all four
    assert (_bits(grad) == 0).all()                                     # a zero gradient stays all-zero bits
    g0 = np.random.default_rng(12).normal(0, 1, q.shape).astype(np.float32)
    _, acc = _run(q, q.copy(), grad0=g0, **kw)
    assert np.array_equal(_bits(acc), _bits(g0))


def test_saturated_logits_stay_finite():
    q, p, kw = R.parity_case('saturated')
    loss, grad = _run(q, p, **kw)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert loss[0] > 0 and (grad != 0).any()


@pytest.mark.parametrize('name', ('head_7x10', 'p257'))
def test_two_calls_give_identical_bits(name):
    q, p, kw = R.parity_case(name)
    a, b = _run(q, p, **kw), _run(q, p, **kw)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_argument_errors_return_yk_err_arg_without_a_launch():
    from k210_yolo_framework_amd import engine
    q, p, _ = R.parity_case('p255')
    B, rows, C = p.shape[0], p.shape[1] * p.shape[2] * p.shape[3], p.shape[4] - 5
    qd, pd = _cu(q), _cu(p)
    fn, st = engine.lib().yk_distill_loss_f32, engine._stream()

    def call(teacher=qd, pred=pd, batch=B, rows_=rows, classes=C, batch_size=B, has_loss=True):
        loss = torch.full((4,), -7.0, device='cuda')
        grad = torch.zeros_like(pd)
        rc = fn(teacher, pred, batch, rows_, classes, 1.0, batch_size, loss if has_loss else None, grad, st)
        torch.cuda.synchronize()
        return rc, loss.cpu().numpy(), grad.cpu().numpy()

    rc, loss, grad = call()
    assert rc == 0 and (loss != -7.0).all() and (grad != 0).any()
    for bad in (dict(teacher=None), dict(pred=None), dict(has_loss=False), dict(batch_size=0), dict(batch_size=-3), dict(classes=0),
                dict(classes=-1), dict(batch=0), dict(rows_=0)):
        rc, loss, grad = call(**bad)
        assert rc == YK_ERR_ARG, bad
        assert 'yk_distill_loss_f32' in engine.lib().yk_last_error().decode()
        assert (loss == -7.0).all() and (grad == 0).all(), bad          # nothing ran
    with pytest.raises(engine.YkError, match='pred'):
        engine.distill_loss(qd, pd[:, :, :40], 1.0, B)                   # another shape than the teacher's, and not contiguous
    with pytest.raises(engine.YkError, match='yk_distill_loss_f32'):
        engine.distill_loss(qd, pd, 1.0, 0)


# ---------------------------------------------------------------------------------------------------------------- the Trainer, mini networks
HYPER = dict(obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0)
TEACHER_SEED = 99


def _case(seed, B=4):
    """tests/mini_net.py::residual_zoo_spec at 32x48 with seeded weights, frames and labels (the form of tests/qat_ref.py::mini_case).  Not
    mini_spec: the teacher is an inference plan, and both plans refuse mini_spec's 8-filter stem, while the f16 plan builds and runs this
    network (tests/test_gpu_plan_zoo.py, F16_BUILDS)."""
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from tests.mini_net import residual_zoo_spec
    spec = residual_zoo_spec()
    w = spec.init_weights(seed)
    h = Helper(None, 20, VOC_ANCHORS, [[32, 48]], [list(v) for v in spec.out_hw()])
    rng = np.random.default_rng(seed)
    ys = [[] for _ in spec.outputs]
    for _ in range(B):
        n = int(rng.integers(1, 4))
        boxes = np.stack([rng.integers(0, 20, n), rng.uniform(.2, .8, n), rng.uniform(.2, .8, n), rng.uniform(.1, .6, n), rng.uniform(.1, .6, n)], 1)
        for i, lab in enumerate(h.box_to_label(boxes)):
            ys[i].append(lab)
    return spec, w, h, _cu(rng.uniform(0, 1, (B, 32, 48, 3))), [_cu(np.stack(y)) for y in ys]


def _config(spec, weight=1.0):
    """A teacher of the student's architecture with other weights: a second mini net.  precision='f16': the f16x2 plan refuses this head
    (8 channels through the upsample, tests/plan_zoo.py::refuse_residual_zoo_spec)."""
    from k210_yolo_framework_amd.distill import DistillConfig
    return DistillConfig(spec, spec.init_weights(TEACHER_SEED), weight=weight, precision='f16')


def test_replayed_steps_equal_eager_steps_with_a_different_batch_each():
    """Eager, captured + replayed, replayed, each on another batch: a capture that read a stale teacher buffer (or a stale frame) would differ
    from the eager run in the second and third step."""
    from k210_yolo_framework_amd.train import Trainer
    cases = [_case(seed) for seed in (5, 6, 7)]
    spec, w, h = cases[0][:3]
    batches = [(c[3], c[4]) for c in cases]
    runs = []
    for graph in (False, True):
        tr = Trainer(spec, w, h.anchors, 4, use_graph=graph, distill=_config(spec), **HYPER)
        outs = [tr.step(x, ys) for x, ys in batches]
        assert (tr._graph is not None) == graph
        runs.append(([o['distill'] for o in outs], [o['loss'] for o in outs], tr.P.cpu().numpy().copy()))
    print('distill per step', runs[0][0])
    assert all(np.isfinite(v) and v > 0 for v in runs[0][0])
    assert len(set(runs[0][0])) == 3                                    # three batches, three teacher outputs
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert np.array_equal(_bits(runs[0][2]), _bits(runs[1][2]))


def test_step_reports_the_rule_on_the_teachers_outputs():
    """The `distill` entry of a step is the float64 rule on (teacher buffers, student outputs) of that step, summed over the layers, and
    `loss` is detection + distillation + regulariser."""
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case(6)
    tr = Trainer(spec, w, h.anchors, 4, use_graph=False, distill=_config(spec, weight=3.0), **HYPER)
    out = tr.step(x, yt)
    e = 5 + spec.class_num
    want = 0.0
    for tq, o in zip(tr._tq, spec.outputs):
        yp = tr.T[o].view(4, *spec.tensors[o][:2], spec.anchor_num, e)
        want += R.analytic(tq.cpu().numpy(), yp.cpu().numpy(), 3.0, 4)[0]['total']
    print('distill', out['distill'], 'float64 rule', want)
    assert abs(out['distill'] - want) <= 2e-5 * max(1.0, want), (out['distill'], want)
    assert abs(out['loss'] - (out['data_loss'] + out['distill'] + out['reg_loss'])) <= 1e-5 * out['loss']


def test_thirty_steps_on_one_batch_lower_the_distillation_term():
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case(7)
    tr = Trainer(spec, w, h.anchors, 4, lr=1e-3, distill=_config(spec, weight=10.0), **HYPER)
    outs = [tr.step(x, yt) for _ in range(30)]
    print([round(o['distill'], 4) for o in outs])
    assert all(np.isfinite(o['loss']) and np.isfinite(o['distill']) for o in outs)
    assert outs[-1]['distill'] < outs[0]['distill']


def test_without_a_teacher_the_kernel_is_never_called(monkeypatch):
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.train import Trainer
    calls, real = [], engine.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(engine, 'call', counting)
    spec, w, h, x, yt = _case(8)
    tr = Trainer(spec, w, h.anchors, 4, distill=None, **HYPER)
    outs = [tr.step(x, yt) for _ in range(3)]
    assert 'yk_yolo_loss' in calls and 'yk_distill_loss_f32' not in calls and 'yk_run_f32' not in calls
    assert all('distill' not in o for o in outs)
    n = len(calls)
    tr = Trainer(spec, w, h.anchors, 4, distill=_config(spec), **HYPER)
    tr.step(x, yt)                                                      # eager: one call per output layer, one teacher run
    assert calls[n:].count('yk_distill_loss_f32') == len(spec.outputs) and calls[n:].count('yk_run_f32') == 1


def test_a_change_of_the_weight_recaptures():
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case(9)
    runs = []
    for graph in (False, True):
        tr = Trainer(spec, w, h.anchors, 4, use_graph=graph, distill=_config(spec), **HYPER)
        outs = [tr.step(x, yt) for _ in range(3)]
        tr.distill_weight = 4.0                                         # a launch argument of the capture
        outs += [tr.step(x, yt) for _ in range(3)]
        runs.append([o['distill'] for o in outs])
    assert runs[0] == runs[1]
    assert runs[0][3] > 2 * runs[0][2]


def _wide_mini_spec():
    """tests/mini_net.py::mini_spec at twice the width (a 16-filter stem, which the f16 plan takes): a larger teacher for mini_spec, with
    outputs of the same shape."""
    from k210_yolo_framework_amd import netspec as ns
    s = ns.NetSpec('mini_wide', (32, 32), anchor_num=3, class_num=20)
    x = s._new_tensor(32, 32, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    x = s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='conv_dw_1')
    x1 = s.conv(x, 32, 1, act=ns.LEAKY03, name='conv_pw_1')
    x = s.dwconv(x1, 2, ns.K210_S2_PAD, act=ns.RELU, name='conv_dw_2')
    x = s.conv(x, 64, 1, act=ns.LEAKY03, name='conv_pw_2')
    ns._head(s, x1, x, 48, 32, 32, 75, [0])
    return s


def test_one_qat_step_with_ciou_and_a_larger_teacher_runs_and_is_finite():
    """QAT (which takes mini_spec, not the residual wiring), an IoU box loss and distillation share loss_and_grads."""
    from k210_yolo_framework_amd.distill import DistillConfig
    from k210_yolo_framework_amd.qat import QatConfig
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, x, yt = mini_case(8)
    teacher = _wide_mini_spec()
    cfg = DistillConfig(teacher, teacher.init_weights(TEACHER_SEED), precision='f16')
    tr = Trainer(spec, w, h.anchors, 2, lr=1e-3, qat=QatConfig(momentum=0.9), box_loss='ciou', distill=cfg, **HYPER)
    tr.qat_observe(_cu(x))
    out = tr.step(_cu(x), [_cu(y) for y in yt])
    assert np.isfinite(out['loss']) and np.isfinite(out['box']) and out['distill'] > 0
    assert np.isfinite(tr.G.cpu().numpy()).all()


def test_a_teacher_of_another_shape_is_refused_by_name():
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.distill import DistillConfig
    from k210_yolo_framework_amd.train import Trainer
    from tests.mini_net import mini_spec
    spec, w, h, x, yt = _case(5)
    other = mini_spec(class_num=3)
    with pytest.raises(engine.YkError, match='input size: the teacher takes 32 x 32'):
        Trainer(spec, w, h.anchors, 4, distill=DistillConfig(other, other.init_weights(1), precision='f16'), **HYPER)

"""GPU parity of the IoU-family box losses (yk_yolo_loss_ex, csrc/yk_loss.hip) against tests/box_loss_ref.py's float64
autograd build (a), and their way up to the Trainer.

Tolerances.  Loss entries: tests/test_gpu_loss.py's, 2e-5 of max(1, |reference|).  Gradient: rtol 2e-5 as there; the absolute term is
measured, not guessed: (a) evaluated in torch float32 on the CPU on these inputs needs atol 2.130e-8 against (a) in float64 at that rtol
(box_loss_ref.F32_ATOL_MEASURED, the largest over the parity cases and the three modes: the wide 1x257 grid with GIoU; measured again by
tests/test_box_loss_ref.py), and the kernel, another fp32 evaluation of the same expression, is given twice that."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import box_loss_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2 * R.F32_ATOL_MEASURED


@functools.lru_cache(maxsize=None)
def _ref(name, mode):
    anc, y_true, y_pred, kw = R.parity_case(name)
    return R.autograd(y_true, y_pred, anc, box_loss=mode, **kw)


def _run(anc, y_true, y_pred, mode, ow=1.0, nw=1.0, ww=1.0, batch_size=None, box_weight=1.0, counts0=(0, 0, 0), **kw):
    from k210_yolo_framework_amd import engine
    counts = torch.tensor(counts0, dtype=torch.float32, device='cuda')
    loss, grad, ign = engine.yolo_loss(torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda(), anc, 0.7, 0.5, ow, nw, ww,
                                       batch_size=batch_size, counts=counts, box_loss=mode, box_weight=box_weight, **kw)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), None if grad is None else grad.cpu().numpy(), None if ign is None else ign.cpu().numpy(),
            tuple(int(v) for v in counts.cpu()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', R.ALL_PARITY)
def test_loss_and_gradient_vs_float64_autograd(name, mode):
    """One cell; the 7x10 head with batch_size 16 for 4 images, an image without objects and random boxes under conf 0; 255, 256 and 257
    predictions per image; the four forced geometries.  pw, ph are drawn over +-4."""
    anc, y_true, y_pred, kw = R.parity_case(name)
    edge, thr = R.min_gap(y_true, y_pred, anc)
    assert edge > 1e-6 and thr > 1e-5, (edge, thr)                      # no two compared edges closer than 1e-6: fp32 decides as float64 does
    if name == 'geometry':
        _, _, _, cells = R.geometry_case()
        box, _ = R.decode(y_pred, anc)
        assert [R.geometry_of(box[c], y_true[c][0:4].astype(np.float64)) for c in cells] == ['disjoint', 'pred_inside', 'label_inside', 'partial']
    ref_l, ref_g, ref_i = _ref(name, mode)
    loss, grad, ign, counts = _run(anc, y_true, y_pred, mode, want_ignore=True, **kw)
    assert loss.shape == (7,)
    for k, term in enumerate(R.TERMS):
        print(name, mode, term, loss[k], ref_l[term], abs(loss[k] - ref_l[term]) / max(1.0, abs(ref_l[term])))
    print(name, mode, 'grad: atol needed at rtol 2e-5:', R.atol_needed(grad, ref_g, RTOL), 'allowed', ATOL,
          '| box entries alone:', R.atol_needed(grad[..., 0:4], ref_g[..., 0:4], RTOL))
    for k, term in enumerate(R.TERMS):
        assert abs(loss[k] - ref_l[term]) <= 2e-5 * max(1.0, abs(ref_l[term])), (term, loss[k], ref_l[term])
    assert loss[1] == 0 and loss[2] == 0 and ref_l['box'] > 0
    assert np.array_equal(ign, ref_i)
    np.testing.assert_allclose(grad, ref_g, rtol=RTOL, atol=ATOL)
    ob = y_true[..., 4] > 0.7
    assert (_bits(grad[~ob][:, 0:4]) == 0).all()                        # cells without an object: +0.0f, not a product with 0
    t, p = ob, y_pred[..., 4] > 0.7
    assert counts == (int((t & p).sum()), int((~t & p).sum()), int((t & ~p).sum()))


@pytest.mark.parametrize('mode', R.MODES)
def test_image_without_objects_and_zero_labels_give_exact_zeros(mode):
    """head_7x10: image 2 has no object at all, and half of the other cells without an object hold a random box under conf 0; p256: every
    cell without an object is all zeros (atan(0 / 0), 0 * NaN if the term were multiplied away).  Nothing is NaN, and entries 0..3 of those
    cells are exactly 0."""
    for name in ('head_7x10', 'p256'):
        anc, y_true, y_pred, kw = R.parity_case(name)
        ob = y_true[..., 4] > 0.7
        if name == 'head_7x10':
            assert not ob[2].any() and ob[[0, 1, 3]].any((1, 2, 3)).all() and (y_true[~ob][:, 2] > 0).any()
        else:
            assert (y_true[~ob] == 0).all()
        loss, grad, ign, _ = _run(anc, y_true, y_pred, mode, want_ignore=True, **kw)
        assert np.isfinite(loss).all() and np.isfinite(grad).all() and np.isfinite(ign).all()
        assert (_bits(grad[~ob][:, 0:4]) == 0).all() and (grad[ob][:, 0:4] != 0).any()
        if name == 'head_7x10':
            assert (_bits(grad[2][..., 0:4]) == 0).all() and (grad[2][..., 4] != 0).all()


@pytest.mark.parametrize('mode', R.MODES)
def test_prediction_equal_to_the_label_box_to_the_last_bit(mode):
    """Every min / max of the rule is at a tie there, so no parity: finite outputs, a box loss below 1e-5 per cell, |gradient| below 1e-4.
    (tests/test_box_loss_ref.py checks on the CPU that the decoded boxes equal the labels bit for bit.)"""
    anc, y_true, y_pred = R.equal_case()
    ob = y_true[..., 4] > 0.7
    loss, grad, _, _ = _run(anc, y_true, y_pred, mode)
    per_cell = loss[6] * len(y_true) / ob.sum()
    print(mode, 'box per cell', per_cell, 'max |grad 0..3|', np.abs(grad[..., 0:4]).max())
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert 0 <= per_cell < 1e-5
    assert np.abs(grad[..., 0:4]).max() < 1e-4


def _raw(entry, cfg_cls, anc, y_true, y_pred, box=None, want=(True, True, True), batch_size=None, weights=(5, 0.5, 0.5)):
    """The C call itself.  -> (return code, loss, grad | None, ignore | None, counts | None); loss is prefilled with -7."""
    from k210_yolo_framework_amd import engine
    B, h, w, A, E = y_pred.shape
    cfg = cfg_cls()
    cfg.out_h, cfg.out_w, cfg.anchor_num, cfg.class_num = h, w, A, E - 5
    for n, (aw, ah) in enumerate(anc):
        cfg.anchors[n][0], cfg.anchors[n][1] = float(aw), float(ah)
    cfg.obj_thresh, cfg.iou_thresh = 0.7, 0.5
    cfg.obj_weight, cfg.noobj_weight, cfg.wh_weight = weights
    cfg.batch_size = batch_size or B
    if box is not None:
        cfg.box_loss, cfg.box_weight = box
    yt, yp = torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()
    loss = torch.full((7,), -7.0, device='cuda')
    grad = torch.empty_like(yp) if want[0] else None
    ign = torch.empty((B, h, w, A), device='cuda') if want[1] else None
    counts = torch.zeros(3, device='cuda') if want[2] else None
    rc = getattr(engine.lib(), entry)(C.byref(cfg), yt, yp, B, loss, grad, ign, counts, engine._stream())
    torch.cuda.synchronize()
    return (rc, loss.cpu().numpy()) + tuple(None if t is None else t.cpu().numpy() for t in (grad, ign, counts))


def test_extended_call_in_mse_mode_is_the_old_call_bit_for_bit():
    from k210_yolo_framework_amd import engine
    for name in ('head_7x10', 'p257'):
        anc, y_true, y_pred, kw = R.parity_case(name)
        old = _raw('yk_yolo_loss', engine.LossCfg, anc, y_true, y_pred, batch_size=kw['batch_size'])
        new = _raw('yk_yolo_loss_ex', engine.LossCfgEx, anc, y_true, y_pred, box=(0, 3.0), batch_size=kw['batch_size'])
        assert old[0] == 0 and new[0] == 0
        assert old[1][6] == -7.0 and new[1][6] == 0.0                   # the old call writes six entries; the new one's box term is 0
        assert old[1][1] > 0 and old[1][2] > 0
        assert np.array_equal(_bits(old[1][:6]), _bits(new[1][:6]))
        for a, b in zip(old[2:], new[2:]):
            assert np.array_equal(_bits(a), _bits(b))
        for mode in (1, 2, 3):                                          # an IoU mode: xy and wh exactly 0, mask and counters untouched
            iou = _raw('yk_yolo_loss_ex', engine.LossCfgEx, anc, y_true, y_pred, box=(mode, 1.0), batch_size=kw['batch_size'])
            assert iou[0] == 0 and (_bits(iou[1][1:3]) == 0).all() and iou[1][6] > 0
            assert np.array_equal(_bits(iou[1][3:6]), _bits(old[1][3:6]))
            assert np.array_equal(_bits(iou[3]), _bits(old[3])) and np.array_equal(_bits(iou[4]), _bits(old[4]))
            assert np.array_equal(_bits(iou[2][..., 4:]), _bits(old[2][..., 4:]))


@pytest.mark.parametrize('mode', (1, 2, 3))
def test_loss_values_do_not_depend_on_the_optional_outputs(mode):
    from k210_yolo_framework_amd import engine
    anc, y_true, y_pred, _ = R.parity_case('p255')
    full = _raw('yk_yolo_loss_ex', engine.LossCfgEx, anc, y_true, y_pred, box=(mode, 1.0))
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        part = _raw('yk_yolo_loss_ex', engine.LossCfgEx, anc, y_true, y_pred, box=(mode, 1.0), want=want)
        assert part[0] == 0 and np.array_equal(_bits(part[1]), _bits(full[1])), want
        for a, b in zip(part[2:], full[2:]):
            assert a is None or np.array_equal(_bits(a), _bits(b))


def test_unknown_mode_is_an_argument_error_without_a_launch():
    from k210_yolo_framework_amd import engine
    anc, y_true, y_pred, _ = R.parity_case('one_cell')
    for bad in (4, -1):
        rc, loss, *_ = _raw('yk_yolo_loss_ex', engine.LossCfgEx, anc, y_true, y_pred, box=(bad, 1.0))
        assert rc == -10                                                # YK_ERR_ARG
        msg = engine.lib().yk_last_error().decode()
        assert 'yk_yolo_loss_ex' in msg and 'box_loss' in msg and str(bad) in msg, msg
        assert (loss == -7.0).all()                                     # nothing ran
    with pytest.raises(ValueError, match="'mse', 'giou', 'diou', 'ciou'"):
        _run(anc, y_true, y_pred, 'iou')


def test_helper_loss_fn_passes_the_box_loss_through():
    from k210_yolo_framework_amd.helper import Helper, create_loss_fn
    anc, y_true, y_pred, kw = R.parity_case('head_7x10')
    h = Helper(None, 20, anc[None], [[224, 320]], [[7, 10]])
    h.batch_size = 16
    fn = create_loss_fn(h, 0.7, 0.5, kw['ow'], kw['nw'], kw['ww'], 0, box_loss='diou', box_weight=kw['box_weight'])
    total = float(fn(torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()))
    ref_l, ref_g, _ = _ref('head_7x10', 'diou')
    assert abs(total - ref_l['total']) <= 2e-5 * max(1.0, abs(ref_l['total']))
    assert fn.terms.shape == (7,) and abs(float(fn.terms[6]) - ref_l['box']) <= 2e-5 * max(1.0, ref_l['box'])
    np.testing.assert_allclose(fn.grad.cpu().numpy(), ref_g, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- the Trainer, mini network
HYPER = dict(obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _ref_step(spec, w, x, yt, anchors, box_loss, box_weight):
    """oracle/train_ref.loss_and_grads with the layer loss of box_loss_ref (a): the float64 network build, autograd through both."""
    from oracle import train_ref
    trainable = [k for k in w if not k.endswith(('/moving_mean', '/moving_variance'))]
    params = {k: torch.from_numpy(np.asarray(w[k], np.float64)).requires_grad_(True) for k in trainable}
    stats = {'__want_pre__': True}
    preds = train_ref.forward_train(spec, params, torch.from_numpy(np.asarray(x, np.float64)), stats)
    data = sum(R.layer_loss_torch(torch.from_numpy(np.asarray(y, np.float64)), yp, anchors[i], 0.7, 0.5, 1.0, 1.0, 1.0, x.shape[0], box_loss,
                                  box_weight)[0]['total'] for i, (y, yp) in enumerate(zip(yt, preds)))
    reg = sum(train_ref.L2_WEIGHT * (params[l.name + '/kernel'] ** 2).sum() for l in spec.layers if l.kind == 'conv' and train_ref._is_darknet_conv(l.name))
    (data + reg).backward()
    stats.pop('__want_pre__')
    return float(data.detach()), {k: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in params.items()}, stats


def test_training_step_with_ciou_all_gradients_vs_autograd():
    """tests/test_gpu_train.py::test_training_step_loss_and_all_gradients_vs_autograd on the mini network with box_loss='ciou': its
    tolerances (loss 1e-4, every gradient 2e-3 of its tensor's maximum) and its rule for seeds (compared only where no activation gate
    falls on different sides in fp32 and float64)."""
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    from tests.test_gpu_train import _gate_flips
    compared = 0
    for seed in range(5, 17):
        spec, w, h, x, yt = mini_case(seed, B=4)
        ref_data, ref_g, ref_stats = _ref_step(spec, w, x, yt, h.anchors, 'ciou', 1.5)
        tr = Trainer(spec, w, h.anchors, 4, lr=5e-4, decay=0.0, box_loss='ciou', box_weight=1.5, **HYPER)
        r = tr.loss_and_grads(_cu(x), [_cu(y) for y in yt])
        torch.cuda.synchronize()
        assert all(p.shape == (7,) for p in r['layers'])
        data = float(sum(p[0] for p in r['layers']).cpu())
        assert abs(data - ref_data) <= 1e-4 * abs(ref_data), (data, ref_data)
        flips = _gate_flips(tr, spec, ref_stats)
        if flips:
            print('seed', seed, 'gate flips', flips, '-> gradients not comparable, next seed')
            continue
        got, worst = tr.grads(), 0.0
        gmax = max(np.abs(v).max() for v in ref_g.values())
        for k, rg in ref_g.items():
            if np.abs(rg).max() < 1e-9 * gmax:
                assert np.abs(got[k]).max() <= 1e-6 * gmax, (k, np.abs(got[k]).max(), gmax)
                continue
            e = np.abs(got[k] - rg).max() / np.abs(rg).max()
            worst = max(worst, e)
            assert e <= 2e-3, (k, e)
        print('seed', seed, 'worst gradient error (relative to tensor max):', worst)
        compared += 1
        if compared == 2:
            break
    assert compared >= 1, 'no flip-free seed found'


def test_graph_replayed_ciou_step_equals_the_eager_step_and_a_change_of_box_loss_recaptures():
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, x, yt = mini_case(6, B=4)
    xs, ys = _cu(x), [_cu(y) for y in yt]
    runs = []
    for graph in (False, True):
        tr = Trainer(spec, w, h.anchors, 4, use_graph=graph, box_loss='ciou', **HYPER)
        outs = [tr.step(xs, ys) for _ in range(3)]                      # eager, captured + replayed, replayed
        assert all('box' in o and 0 < o['box'] < o['data_loss'] for o in outs)
        tr.hyper['box_loss'] = 'giou'                                   # a launch argument of the capture: invalidate and recapture
        outs += [tr.step(xs, ys) for _ in range(3)]
        tr.hyper['box_loss'] = 'mse'
        outs += [tr.step(xs, ys) for _ in range(2)]
        assert 'box' not in outs[-1]
        runs.append(([o['loss'] for o in outs], tr.G.cpu().numpy().copy(), tr.P.cpu().numpy().copy()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_twenty_adam_steps_with_ciou_lower_the_loss():
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, x, yt = mini_case(7, B=4)
    tr = Trainer(spec, w, h.anchors, 4, lr=1e-3, box_loss='ciou', **HYPER)
    xs, ys = _cu(x), [_cu(y) for y in yt]
    outs = [tr.step(xs, ys) for _ in range(20)]
    print([round(o['loss'], 4) for o in outs], [round(o['box'], 4) for o in outs])
    assert all(np.isfinite(o['loss']) for o in outs)
    assert outs[-1]['loss'] < outs[0]['loss']


def test_one_qat_step_with_ciou_runs_and_is_finite():
    from k210_yolo_framework_amd.qat import QatConfig
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, x, yt = mini_case(8)
    tr = Trainer(spec, w, h.anchors, 2, lr=1e-3, qat=QatConfig(momentum=0.9), box_loss='ciou', **HYPER)
    tr.qat_observe(_cu(x))
    out = tr.step(_cu(x), [_cu(y) for y in yt])
    assert np.isfinite(out['loss']) and np.isfinite(out['box']) and out['box'] > 0
    assert np.isfinite(tr.G.cpu().numpy()).all()

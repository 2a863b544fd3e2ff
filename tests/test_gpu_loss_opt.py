"""GPU parity of focal loss, label smoothing and the IoU objectness target (yk_yolo_loss_opt, csrc/yk_loss.hip) against
tests/loss_opt_ref.py's float64 autograd statement, the cases in which the call must give the bits of the calls without options, and the
options' way up to the Trainer.

Tolerances.  Loss entries: tests/test_gpu_loss.py's, 2e-5 of max(1, |reference|).  Gradient entries 0..3 (the box): the options do not touch
them (the IoU target is a constant), so they are held to the BITS of the call without options, which tests/test_gpu_loss.py and
tests/test_gpu_box_loss.py hold to float64.  Gradient entries 4.. (objectness, classes): rtol 2e-5 as there; the absolute term is measured,
not guessed: the statement evaluated in torch float32 on the CPU on these inputs needs atol 1.361e-7 against float64 at that rtol
(loss_opt_ref.F32_ATOL_MEASURED, the largest over the parity cases, the option sets and both box modes: the 20x20 layer with the IoU target,
whose float32 IoU is 8.4e-7 off; measured again by tests/test_loss_opt_ref.py), and the kernel, another fp32 evaluation of the same expression
with the GPU's expf / logf / powf, is given four times that: 5.444e-7.  (The kernel itself needed 1.36e-7 when measured on an MI355X, in that
same case; the loss entries were within 1.3e-7.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import loss_opt_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, R.ATOL_FACTOR * R.F32_ATOL_MEASURED


@functools.lru_cache(maxsize=None)
def _ref(name, box, oname):
    anc, y_true, y_pred, kw = R.parity_case(name)
    return R.autograd(y_true, y_pred, anc, box_loss=box, **kw, **R.options(oname))


@functools.lru_cache(maxsize=None)
def _dev(name):
    anc, y_true, y_pred, kw = R.parity_case(name)
    return torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()


def _run(name, box, opts, counts0=(0, 0, 0), **more):
    """engine.yolo_loss on a parity case -> (loss, grad, ignore, counts) as numpy."""
    from k210_yolo_framework_amd import engine
    anc, _, _, kw = R.parity_case(name)
    yt, yp = _dev(name)
    counts = torch.tensor(counts0, dtype=torch.float32, device='cuda')
    loss, grad, ign = engine.yolo_loss(yt, yp, anc, 0.7, 0.5, kw['ow'], kw['nw'], kw['ww'], batch_size=kw['batch_size'], counts=counts,
                                       box_loss=box, box_weight=kw['box_weight'], want_ignore=True, **opts, **more)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy(), ign.cpu().numpy(), tuple(int(v) for v in counts.cpu())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('box', R.BOX_MODES)
@pytest.mark.parametrize('name', R.ALL_PARITY)
def test_loss_and_gradient_vs_float64_autograd(name, box):
    """One cell; the 7x10 head with 20 classes, batch_size 16 for 4 images, an image without objects and garbage under conf 0; 255, 256 and
    257 predictions per image; 80 classes; 20x20x3 with every cell an object (1200 label boxes: the scan of global memory); logits of +-80
    on objectness and classes.  Every option set of loss_opt_ref.OPTION_SETS."""
    plain = _run(name, box, {})
    for oname in R.OPTION_SETS:
        ref_l, ref_g, ref_i, _ = _ref(name, box, oname)
        loss, grad, ign, counts = _run(name, box, R.OPTION_SETS[oname])
        assert loss.shape == (7,)
        for k, term in enumerate(R.TERMS):
            print(name, box, oname, term, loss[k], ref_l[term], abs(loss[k] - ref_l[term]) / max(1.0, abs(ref_l[term])))
        print(name, box, oname, 'grad 4..: atol needed at rtol 2e-5:', R.atol_needed(grad[..., 4:], ref_g[..., 4:], RTOL), 'allowed', ATOL)
        for k, term in enumerate(R.TERMS):
            assert abs(loss[k] - ref_l[term]) <= 2e-5 * max(1.0, abs(ref_l[term])), (oname, term, loss[k], ref_l[term])
        assert np.isfinite(grad).all()
        np.testing.assert_allclose(grad[..., 4:], ref_g[..., 4:], rtol=RTOL, atol=ATOL, err_msg=oname)
        # what the options do not touch: the box terms, gradient entries 0..3, the ignore mask, the counters
        assert np.array_equal(_bits(grad[..., 0:4]), _bits(plain[1][..., 0:4])), oname
        assert np.array_equal(_bits(loss[[1, 2]]), _bits(plain[0][[1, 2]])) and (box == 'mse' or _bits(loss[6]) == _bits(plain[0][6]))
        assert np.array_equal(ign, ref_i) and np.array_equal(_bits(ign), _bits(plain[2])) and counts == plain[3]


def _raw(entry, cfg_cls, name, box=None, opt=None, want=(True, True, True)):
    """The C call itself.  -> (return code, loss, grad | None, ignore | None, counts | None); loss is prefilled with -7."""
    from k210_yolo_framework_amd import engine
    anc, y_true, y_pred, kw = R.parity_case(name)
    B, h, w, A, E = y_pred.shape
    cfg = cfg_cls()
    cfg.out_h, cfg.out_w, cfg.anchor_num, cfg.class_num = h, w, A, E - 5
    for n, (aw, ah) in enumerate(anc):
        cfg.anchors[n][0], cfg.anchors[n][1] = float(aw), float(ah)
    cfg.obj_thresh, cfg.iou_thresh = 0.7, 0.5
    cfg.obj_weight, cfg.noobj_weight, cfg.wh_weight = 5, 0.5, 0.5
    cfg.batch_size = kw['batch_size'] or B
    if box is not None:
        cfg.box_loss, cfg.box_weight = box
    if opt is not None:
        cfg.focal, cfg.focal_gamma, cfg.focal_alpha, cfg.label_smooth, cfg.obj_target = opt
    yt, yp = _dev(name)
    loss = torch.full((7,), -7.0, device='cuda')
    grad = torch.empty_like(yp) if want[0] else None
    ign = torch.empty((B, h, w, A), device='cuda') if want[1] else None
    counts = torch.zeros(3, device='cuda') if want[2] else None
    rc = getattr(engine.lib(), entry)(C.byref(cfg), yt, yp, B, loss, grad, ign, counts, engine._stream())
    torch.cuda.synchronize()
    return (rc, loss.cpu().numpy()) + tuple(None if t is None else t.cpu().numpy() for t in (grad, ign, counts))


OPT_OFF = (0, 2.0, 0.0, 0.0, 0)


@pytest.mark.parametrize('mode', (0, 1, 2, 3))
def test_every_option_off_is_the_extended_call_bit_for_bit(mode):
    """All four box modes, with and without the optional outputs: loss, gradient, ignore mask and counts."""
    from k210_yolo_framework_amd import engine
    for name in ('head_7x10', 'p257'):
        for want in ((True, True, True), (False, False, False), (True, False, True)):
            old = _raw('yk_yolo_loss_ex', engine.LossCfgEx, name, box=(mode, 1.5), want=want)
            for off in (OPT_OFF, (0, 1.5, 0.25, 0.0, 0)):                # gamma and alpha say nothing while focal is 0
                new = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, name, box=(mode, 1.5), opt=off, want=want)
                assert old[0] == 0 and new[0] == 0
                assert np.array_equal(_bits(old[1]), _bits(new[1])) and (old[1] != -7.0).all()
                for a, b in zip(old[2:], new[2:]):
                    assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize('mode', (0, 3))
def test_focal_with_gamma_0_and_alpha_0_is_focal_off_bit_for_bit(mode):
    from k210_yolo_framework_amd import engine
    for rest in ((0.0, 0), (0.1, 1)):                                   # alone, and beside label smoothing and the IoU target
        off = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, 'head_7x10', box=(mode, 1.0), opt=(0, 2.0, 0.0) + rest)
        on = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, 'head_7x10', box=(mode, 1.0), opt=(3, 0.0, 0.0) + rest)
        assert off[0] == 0 and on[0] == 0
        for a, b in zip(off[1:], on[1:]):
            assert np.array_equal(_bits(a), _bits(b))


def test_image_without_objects_gives_the_noobj_term_alone():
    """head_7x10, image 2 alone (no object; the garbage under conf 0 stays): cls, obj, xy, wh are exactly 0 and so are gradient entries
    0..3 and 5.."""
    from k210_yolo_framework_amd import engine
    anc, y_true, y_pred, kw = R.parity_case('head_7x10')
    assert not (y_true[2, ..., 4] > 0.7).any() and (y_true[2, ..., 5:] > 0).any()
    yt, yp = torch.from_numpy(y_true[2:3]).cuda(), torch.from_numpy(y_pred[2:3]).cuda()
    for box in R.BOX_MODES:
        loss, grad, _ = engine.yolo_loss(yt, yp, anc, 0.7, 0.5, 5, 0.5, 0.5, box_loss=box, **R.OPTION_SETS['all_three'])
        loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
        assert loss[4] > 0 and loss[0] == loss[4] and (loss[[1, 2, 3, 5, 6]] == 0).all(), loss
        assert (grad[..., 0:4] == 0).all() and (grad[..., 5:] == 0).all() and (grad[..., 4] != 0).any() and np.isfinite(grad).all()


def test_iou_target_of_a_prediction_on_its_label_box_is_1():
    """box_loss_ref.equal_case: every object cell's prediction IS its label box, so IoU = I / (I + 1e-7) and the objectness target is 1 within
    1e-7 / I <= 1.34e-6 (the smallest box has area 0.075) in exact arithmetic.  In fp32 the four edges centre -+ size / 2 lie below 1.03 and
    are rounded (half an ulp of 1: 6e-8 each), so each axis' overlap is up to 1.2e-7 short of a side of at least 0.25: 2 * 4.8e-7 more; the
    clamp keeps the target at or below 1.  The objectness gradient of those cells shows it: (sigmoid(x) - z) / batch."""
    from k210_yolo_framework_amd import engine
    from tests import box_loss_ref as B
    anc, y_true, y_pred = B.equal_case()
    ob = y_true[..., 4] > 0.7
    yt, yp = torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()
    _, g_label, _ = engine.yolo_loss(yt, yp, anc, 0.7, 0.5, 1, 1, 1, label_smooth=0.1)          # (an option on: the same entry point)
    _, g_iou, _ = engine.yolo_loss(yt, yp, anc, 0.7, 0.5, 1, 1, 1, label_smooth=0.1, obj_target='iou')
    g_label, g_iou = g_label.cpu().numpy(), g_iou.cpu().numpy()
    # d/dx = (sigmoid(x) - z) / batch: the two differ by (1 - z) / 2
    dz = (g_iou[ob][:, 4] - g_label[ob][:, 4]) * len(y_true)
    print('1 - z per object cell:', dz)
    assert dz.min() >= -2e-7 and dz.max() <= 1e-7 / 0.075 + 2 * 1.2e-7 / 0.25 + 2e-7              # (+- 2e-7: fp32 rounding of two gradients of size <= 1)
    assert np.array_equal(_bits(g_iou[~ob]), _bits(g_label[~ob]))


def test_two_calls_give_the_same_bits_and_counts_add():
    a = _run('head_7x10', 'ciou', R.OPTION_SETS['all_three_g1.5'], counts0=(1, 2, 3))
    b = _run('head_7x10', 'ciou', R.OPTION_SETS['all_three_g1.5'], counts0=(1, 2, 3))
    plain = _run('head_7x10', 'ciou', {})
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(u), _bits(v))
    assert a[3] == b[3] == tuple(c + d for c, d in zip(plain[3], (1, 2, 3)))


@pytest.mark.parametrize('bad,field', [((3, 0.5, 0.0, 0.0, 0), 'focal_gamma'), ((3, 2.0, 1.0, 0.0, 0), 'focal_alpha'),
                                       ((0, 2.0, 0.0, 1.0, 0), 'label_smooth'), ((4, 2.0, 0.0, 0.0, 0), 'focal'),
                                       ((-1, 2.0, 0.0, 0.0, 0), 'focal'), ((0, 2.0, 0.0, 0.0, 2), 'obj_target')])
def test_a_field_out_of_range_is_an_argument_error_without_a_launch(bad, field):
    from k210_yolo_framework_amd import engine
    rc, loss, *_ = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, 'one_cell', box=(0, 1.0), opt=bad)
    assert rc == -10                                                    # YK_ERR_ARG
    msg = engine.lib().yk_last_error().decode()
    assert msg.startswith('yk_yolo_loss_opt: ' + field + ' '), msg
    assert (loss == -7.0).all()                                         # nothing ran
    rc, loss, *_ = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, 'one_cell', box=(7, 1.0), opt=OPT_OFF)
    assert rc == -10 and 'yk_yolo_loss_opt' in engine.lib().yk_last_error().decode() and 'box_loss' in engine.lib().yk_last_error().decode()


def test_helper_loss_fn_passes_the_options_through():
    from k210_yolo_framework_amd.helper import Helper, create_loss_fn
    anc, y_true, y_pred, kw = R.parity_case('head_7x10')
    h = Helper(None, 20, anc[None], [[224, 320]], [[7, 10]])
    h.batch_size = 16
    opts = dict(focal='all', label_smooth=0.1, obj_target='iou')
    fn = create_loss_fn(h, 0.7, 0.5, kw['ow'], kw['nw'], kw['ww'], 0, **opts)
    total = float(fn(*_dev('head_7x10')))
    ref_l, ref_g, _, _ = R.autograd(y_true, y_pred, anc, **kw, **opts)
    assert abs(total - ref_l['total']) <= 2e-5 * max(1.0, abs(ref_l['total']))
    assert fn.terms.shape == (7,)
    for k, term in enumerate(R.TERMS):
        assert abs(float(fn.terms[k]) - ref_l[term]) <= 2e-5 * max(1.0, abs(ref_l[term])), term
    np.testing.assert_allclose(fn.grad.cpu().numpy()[..., 4:], ref_g[..., 4:], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- the Trainer, mini network
HYPER = dict(obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0)
ALL_ON = dict(focal='all', label_smooth=0.1, obj_target='iou')


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _ref_step(spec, w, x, yt, anchors, box_loss, box_weight, opts):
    """tests/test_gpu_box_loss._ref_step with the layer loss of loss_opt_ref: the float64 network build, autograd through both."""
    from oracle import train_ref
    trainable = [k for k in w if not k.endswith(('/moving_mean', '/moving_variance'))]
    params = {k: torch.from_numpy(np.asarray(w[k], np.float64)).requires_grad_(True) for k in trainable}
    stats = {'__want_pre__': True}
    preds = train_ref.forward_train(spec, params, torch.from_numpy(np.asarray(x, np.float64)), stats)
    data = sum(R.layer_loss_torch(torch.from_numpy(np.asarray(y, np.float64)), yp, anchors[i], 0.7, 0.5, 1.0, 1.0, 1.0, x.shape[0], box_loss,
                                  box_weight, **opts)[0]['total'] for i, (y, yp) in enumerate(zip(yt, preds)))
    reg = sum(train_ref.L2_WEIGHT * (params[l.name + '/kernel'] ** 2).sum() for l in spec.layers if l.kind == 'conv' and train_ref._is_darknet_conv(l.name))
    (data + reg).backward()
    stats.pop('__want_pre__')
    return float(data.detach()), {k: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in params.items()}, stats


def test_training_step_with_all_three_all_gradients_vs_autograd():
    """tests/test_gpu_box_loss.py::test_training_step_with_ciou_all_gradients_vs_autograd with the three options on: its tolerances (loss
    1e-4, every gradient 2e-3 of its tensor's maximum) and its rule for seeds."""
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    from tests.test_gpu_train import _gate_flips
    compared = 0
    for seed in range(5, 17):
        spec, w, h, x, yt = mini_case(seed, B=4)
        ref_data, ref_g, ref_stats = _ref_step(spec, w, x, yt, h.anchors, 'mse', 1.0, ALL_ON)
        tr = Trainer(spec, w, h.anchors, 4, lr=5e-4, decay=0.0, **HYPER, **ALL_ON)
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


def test_graph_replayed_step_equals_the_eager_step_and_a_change_of_an_option_recaptures():
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, x, yt = mini_case(6, B=4)
    xs, ys = _cu(x), [_cu(y) for y in yt]
    runs = []
    for graph in (False, True):
        tr = Trainer(spec, w, h.anchors, 4, use_graph=graph, **HYPER, **ALL_ON)
        outs = [tr.step(xs, ys) for _ in range(3)]                      # eager, captured + replayed, replayed
        tr.hyper['focal_gamma'] = 1.5                                   # a launch argument of the capture: invalidate and recapture
        outs += [tr.step(xs, ys) for _ in range(3)]
        tr.hyper.update(focal='off', label_smooth=0.0, obj_target='label')
        outs += [tr.step(xs, ys) for _ in range(2)]
        assert all('box' not in o for o in outs)
        runs.append(([o['loss'] for o in outs], tr.G.cpu().numpy().copy(), tr.P.cpu().numpy().copy()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    # the options are in force: the same weights and batch without them give another loss
    plain = Trainer(spec, w, h.anchors, 4, use_graph=False, **HYPER).step(xs, ys)
    assert plain['loss'] != runs[0][0][0]


def test_twenty_adam_steps_with_all_three_lower_the_loss():
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, x, yt = mini_case(7, B=4)
    tr = Trainer(spec, w, h.anchors, 4, lr=1e-3, **HYPER, **ALL_ON)
    xs, ys = _cu(x), [_cu(y) for y in yt]
    outs = [tr.step(xs, ys) for _ in range(20)]
    print([round(o['loss'], 4) for o in outs])
    assert all(np.isfinite(o['loss']) for o in outs)
    assert outs[-1]['loss'] < outs[0]['loss']


def test_one_qat_step_with_the_options_and_ciou_is_finite():
    from k210_yolo_framework_amd.qat import QatConfig
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, x, yt = mini_case(8)
    tr = Trainer(spec, w, h.anchors, 2, lr=1e-3, qat=QatConfig(momentum=0.9), box_loss='ciou', **HYPER, **ALL_ON)
    tr.qat_observe(_cu(x))
    out = tr.step(_cu(x), [_cu(y) for y in yt])
    assert np.isfinite(out['loss']) and np.isfinite(out['box']) and out['box'] > 0
    assert np.isfinite(tr.G.cpu().numpy()).all()


def test_with_every_option_off_the_step_makes_the_calls_it_made(monkeypatch):
    """The names of the library calls of a step: yk_yolo_loss (or, with an IoU box loss, yk_yolo_loss_ex), never yk_yolo_loss_opt, and the
    same list whether the options are left out or passed as their defaults; with an option on, yk_yolo_loss_opt in their place, one for one."""
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    calls, real = [], engine.call

    def recording(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(engine, 'call', recording)
    spec, w, h, x, yt = mini_case(9, B=4)
    xs, ys = _cu(x), [_cu(y) for y in yt]
    seen = {}
    for key, kw in (('plain', {}), ('defaults', dict(R.OFF)), ('ciou', dict(box_loss='ciou')), ('on', dict(ALL_ON))):
        del calls[:]
        Trainer(spec, w, h.anchors, 4, use_graph=False, **HYPER, **kw).step(xs, ys)
        seen[key] = list(calls)
    loss_calls = lambda names: [n for n in names if n.startswith('yk_yolo_loss')]
    assert seen['defaults'] == seen['plain']
    assert loss_calls(seen['plain']) == ['yk_yolo_loss'] * len(yt) and loss_calls(seen['ciou']) == ['yk_yolo_loss_ex'] * len(yt)
    assert loss_calls(seen['on']) == ['yk_yolo_loss_opt'] * len(yt)
    assert [n.replace('yk_yolo_loss_opt', 'yk_yolo_loss') for n in seen['on']] == seen['plain']

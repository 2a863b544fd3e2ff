"""Every compiled instance of yolo_loss_kernel<MODE, OPT> with an option on (csrc/yk_loss.hip: 27 sets of L_* bits x 4 box modes = 108; DESIGN.md
3.25) against tests/loss_opt_ref.py's float64 autograd statement; the ends of the focal and smoothing parameters; the IoU objectness target on
box_loss_ref's forced geometries; the optional outputs with an option on; and one Trainer step on an instance no other test trains.

The tolerances are tests/test_gpu_loss_opt.py's, unchanged (its header derives them): loss entries within 2e-5 of max(1, |reference|); gradient
entries 4.. at rtol 2e-5 and atol 4 x 1.361e-7; gradient entries 0..3, the box terms, the ignore mask and the counters bit-equal to the call of
the same box mode without options, which tests/test_gpu_box_loss.py and tests/test_gpu_loss.py hold to float64 on these cases.
tests/test_loss_opt_ref.py shows on the CPU that the option sets are the 27 cases of the dispatch, that the statement in float32 stays within
1.361e-7 on every input used here, and that two instances one bit apart differ by at least 100 times these tolerances, so an instance that
runs in another's place, or not at all, cannot pass."""
import numpy as np
import pytest
import torch

from tests import box_loss_ref as B
from tests import loss_opt_ref as R
from tests.test_gpu_loss_opt import ATOL, HYPER, RTOL, _bits, _cu, _dev, _raw, _ref_step, _run

pytestmark = pytest.mark.gpu

MODE_ID = {'mse': 0, 'giou': 1, 'diou': 2, 'ciou': 3}


def _run_fresh(case, box, opts):
    """`_run` with the gradient's memory filled with NaN beforehand: the caching allocator hands engine.yolo_loss the block just freed, so an
    instance that is not launched leaves NaN and not an earlier call's gradient."""
    torch.full_like(_dev(case)[1], float('nan'))
    return _run(case, box, opts)


def _check(case, box, oname, plain):
    """One option set of loss_opt_ref.SWEEP_SETS: the assertions of test_gpu_loss_opt.test_loss_and_gradient_vs_float64_autograd.
    -> (loss, grad, reference gradient, atol needed at rtol 2e-5 on entries 4..)."""
    ref_l, ref_g, ref_i, _ = R.sweep_ref(case, box, oname)
    loss, grad, ign, counts = _run_fresh(case, box, R.SWEEP_SETS[oname])
    assert loss.shape == (7,)
    need = R.atol_needed(grad[..., 4:], ref_g[..., 4:], RTOL)
    worst = max(abs(loss[k] - ref_l[term]) / max(1.0, abs(ref_l[term])) for k, term in enumerate(R.TERMS))
    print(case, box, oname, 'worst loss term', worst, 'grad 4..: atol needed at rtol 2e-5:', need, 'allowed', ATOL)
    for k, term in enumerate(R.TERMS):
        assert abs(loss[k] - ref_l[term]) <= 2e-5 * max(1.0, abs(ref_l[term])), (oname, term, loss[k], ref_l[term])
    assert np.isfinite(loss).all() and np.isfinite(grad).all() and np.isfinite(ign).all()
    np.testing.assert_allclose(grad[..., 4:], ref_g[..., 4:], rtol=RTOL, atol=ATOL, err_msg=oname)
    # what the options do not touch: the box terms, gradient entries 0..3, the ignore mask, the counters
    assert np.array_equal(_bits(grad[..., 0:4]), _bits(plain[1][..., 0:4])), oname
    assert np.array_equal(_bits(loss[[1, 2]]), _bits(plain[0][[1, 2]])) and (box == 'mse' or _bits(loss[6]) == _bits(plain[0][6])), oname
    assert np.array_equal(ign, ref_i) and np.array_equal(_bits(ign), _bits(plain[2])) and counts == plain[3], oname
    return loss, grad, ref_g, need


# one two- or three-option set per box mode for the raw call: (focal, gamma, alpha, label_smooth, obj_target)
RAW_SET = {'mse': (2, 2.0, 0.0, 0.0, 1), 'giou': (1, 2.0, 0.0, 0.1, 0), 'diou': (0, 2.0, 0.0, 0.1, 1), 'ciou': (1, 1.5, 0.0, 0.0, 1)}


@pytest.mark.parametrize('case', R.INSTANCE_CASES)
@pytest.mark.parametrize('box', R.ALL_BOX_MODES)
def test_every_instance_vs_float64_autograd(box, case):
    """The 27 option sets of loss_opt_ref.INSTANCE_SETS, one per OPT of loss_launch_opt's switch, in one box mode on: the 7x10 head (batch_size
    16 for 4 images, an image without objects, garbage under conf 0); 257 predictions (two chunks, the second of one box); the four forced
    box relations.  Then the C call itself for one set, with the loss prefilled."""
    from k210_yolo_framework_amd import engine
    plain = _run(case, box, {})
    need = max(_check(case, box, oname, plain)[3] for oname in R.INSTANCE_SETS)
    print(case, box, 'largest atol needed over the 27 instances:', need, 'allowed', ATOL)
    rc, loss, grad, ign, counts = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, case, box=(MODE_ID[box], 1.0), opt=RAW_SET[box])
    assert rc == 0 and (loss != -7.0).all() and np.isfinite(loss).all() and np.isfinite(grad).all()


@pytest.mark.parametrize('case', R.EDGE_CASES)
@pytest.mark.parametrize('box', R.ALL_BOX_MODES)
def test_edge_parameters_vs_float64_autograd(box, case):
    """loss_opt_ref.EDGE_SETS, the ends of what loss_launch accepts: gamma 1 (powf(m, 0)) and 5; gamma 0 with alpha 0.25 (alpha-balanced bce
    through the `gamma > 0 ? .. : ..` arms of an L_POW instance); alpha 0.75 and 0.999; label_smooth 0.9 and 0.999; gamma 1 beside the IoU
    target.  On `saturated` (logits of +-80 on objectness and classes, in object cells and others) every gradient entry is finite, and under
    gamma 1 the saturated cells are looked at by themselves."""
    anc, y_true, y_pred, _ = R.parity_case(case)
    sat = np.abs(y_pred[..., 4]) == 80
    assert sat.any() == (case == 'saturated')
    plain = _run(case, box, {})
    need = 0.0
    for oname, o in R.EDGE_SETS.items():
        loss, grad, ref_g, a = _check(case, box, oname, plain)
        need = max(need, a)
        if sat.any() and o.get('focal_gamma') == 1.0:
            assert (y_true[sat][:, 4] > 0.7).any() and (y_true[sat][:, 4] <= 0.7).any() and {-80.0, 80.0} == set(y_pred[sat][:, 4])
            np.testing.assert_allclose(grad[sat][:, 4:], ref_g[sat][:, 4:], rtol=RTOL, atol=ATOL, err_msg=oname)
    print(case, box, 'largest atol needed over the 7 edge sets:', need, 'allowed', ATOL)


def test_iou_target_on_the_forced_geometries_in_all_four_modes():
    """`geometry` with label_smooth=0.1 (an option on: the same entry point), objectness target 'label' and 'iou'.  In an object cell
    d/dx = obj_weight (sigmoid(x) - z) / batch_size and conf is 1, so (g_iou - g_label) batch_size / obj_weight = 1 - z: held to the
    reference's target within ATOL batch_size / obj_weight.  The disjoint cell has the gradient of target 0, the cells without an object
    the same bits in both calls, and the four box modes the same bits in entry 4: in fp32 the MSE mode's own copy of the IoU gives the
    number l_box_loss<MODE> gives."""
    anc, y_true, y_pred, kw = R.parity_case('geometry')
    cells = B.geometry_case()[3]
    ob = y_true[..., 4] > 0.7
    scale = len(y_true) / kw['ow']
    assert kw['batch_size'] is None and (y_true[ob][:, 4] == 1).all()
    entry4 = []
    for box in R.ALL_BOX_MODES:
        zo = R.sweep_ref('geometry', box, 'smooth+iou')[3]
        assert zo[cells[0]] == 0.0
        g_label = _run('geometry', box, dict(label_smooth=0.1))[1]
        g_iou = _run_fresh('geometry', box, dict(label_smooth=0.1, obj_target='iou'))[1]
        z = 1.0 - (g_iou[ob][:, 4].astype(np.float64) - g_label[ob][:, 4]) * scale
        print(box, 'target per object cell:', z, 'largest distance from the reference', np.abs(z - zo[ob]).max(), 'allowed', ATOL * scale)
        np.testing.assert_allclose(z, zo[ob], rtol=0, atol=ATOL * scale)
        x = float(y_pred[cells[0]][4])
        np.testing.assert_allclose(g_iou[cells[0]][4], 1 / (1 + np.exp(-x)) / scale, rtol=RTOL, atol=ATOL)
        assert np.array_equal(_bits(g_iou[~ob]), _bits(g_label[~ob]))
        entry4.append(_bits(g_iou[..., 4]))
    for box, e in zip(R.ALL_BOX_MODES[1:], entry4[1:]):
        assert np.array_equal(e, entry4[0]), (box, np.flatnonzero((e != entry4[0]).ravel()), e[e != entry4[0]], entry4[0][e != entry4[0]])


def test_iou_target_of_boxes_disjoint_in_both_axes_is_0_in_all_four_modes():
    """loss_opt_ref.corner_case: the prediction lies off the label box's corner, so both overlaps are negative and their product is positive
    and smaller than the two areas.  The target is 0 - the overlaps are clamped one by one, not their product or the quotient alone - and the
    cell's objectness gradient is sigmoid(x) / batch_size.  (`geometry`'s own disjoint cell cannot tell: its product exceeds the areas, the
    quotient is negative and the clamp of the target hides it.)"""
    from k210_yolo_framework_amd import engine
    anc, y_true, y_pred, kw, cell = R.corner_case()
    yt, yp = torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()
    entry4 = []
    for box in R.ALL_BOX_MODES:
        ref_l, ref_g, ref_i, zo = R.autograd(y_true, y_pred, anc, box_loss=box, **kw, obj_target='iou')
        assert zo[cell] == 0.0
        loss, grad, ign = engine.yolo_loss(yt, yp, anc, 0.7, 0.5, kw['ow'], kw['nw'], kw['ww'], box_loss=box, want_ignore=True, obj_target='iou')
        loss, grad, ign = loss.cpu().numpy(), grad.cpu().numpy(), ign.cpu().numpy()
        for k, term in enumerate(R.TERMS):
            assert abs(loss[k] - ref_l[term]) <= 2e-5 * max(1.0, abs(ref_l[term])), (box, term, loss[k], ref_l[term])
        np.testing.assert_allclose(grad[..., 4:], ref_g[..., 4:], rtol=RTOL, atol=ATOL, err_msg=box)
        x = float(y_pred[cell][4])
        print(box, 'objectness gradient of the corner cell', grad[cell][4], 'of target 0:', kw['ow'] / (1 + np.exp(-x)) / len(y_true))
        np.testing.assert_allclose(grad[cell][4], kw['ow'] / (1 + np.exp(-x)) / len(y_true), rtol=RTOL, atol=ATOL)
        assert np.array_equal(ign, ref_i)
        entry4.append(_bits(grad[..., 4]))
    assert all(np.array_equal(e, entry4[0]) for e in entry4[1:])


@pytest.mark.parametrize('opt', ((2, 2.0, 0.0, 0.0, 1), (1, 1.5, 0.0, 0.1, 0)), ids=('FCLS|IOU', 'FOBJ|POW|SMOOTH'))
@pytest.mark.parametrize('mode', (0, 2))
def test_optional_outputs_with_an_option_on(mode, opt):
    """yk_yolo_loss_opt itself on p257 with the gradient, the ignore mask or the counters left out, one by one and all three: the loss and
    every output that is present have the bits of the call with all of them."""
    from k210_yolo_framework_amd import engine
    full = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, 'p257', box=(mode, 1.5), opt=opt)
    assert full[0] == 0 and (full[1] != -7.0).all()
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        part = _raw('yk_yolo_loss_opt', engine.LossCfgOpt, 'p257', box=(mode, 1.5), opt=opt, want=want)
        assert part[0] == 0 and np.array_equal(_bits(part[1]), _bits(full[1])), want
        for there, a, b in zip(want, part[2:], full[2:]):
            assert (a is not None and np.array_equal(_bits(a), _bits(b))) if there else a is None, want


DIOU_CLS_IOU = dict(focal='cls', obj_target='iou')


def test_training_step_with_diou_focal_cls_and_iou_target_all_gradients_vs_autograd():
    """tests/test_gpu_loss_opt.py::test_training_step_with_all_three_all_gradients_vs_autograd with box_loss='diou', focal='cls',
    obj_target='iou': its tolerances (loss 1e-4, every gradient 2e-3 of its tensor's maximum) and its rule for seeds."""
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    from tests.test_gpu_train import _gate_flips
    compared = 0
    for seed in range(5, 17):
        spec, w, h, x, yt = mini_case(seed, B=4)
        ref_data, ref_g, ref_stats = _ref_step(spec, w, x, yt, h.anchors, 'diou', 1.0, DIOU_CLS_IOU)
        tr = Trainer(spec, w, h.anchors, 4, lr=5e-4, decay=0.0, box_loss='diou', **HYPER, **DIOU_CLS_IOU)
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

"""simota.assign, the rule alone, on cases worked out by hand, and yk_assign_simota_f32's argument checks that come before the device."""
import ctypes as C
import math

import numpy as np
import pytest

from k210_yolo_framework_amd import simota


def _one_cell(anchors, class_num):
    """A 1x1 grid with all logits 0: s = 0.5, so candidate a is the box (0.5, 0.5, aw, ah) and every q_k is 0.5."""
    cfg = dict(out_hw=[(1, 1)], anchors=[anchors], class_num=class_num)
    return cfg, [np.zeros((1, 1, 1, len(anchors), 5 + class_num), np.float32)]


def test_one_box_and_one_candidate():
    cfg, preds = _one_cell([(.5, .5)], 1)
    labels, npos, status, margin = simota.assign(preds, [[0, .5, .5, .5, .5]], [0, 1], cfg)
    assert labels[0].reshape(-1).tolist() == [.5, .5, .5, .5, 1, 1] and npos.tolist() == [1]
    assert status == simota.STATUS_CLEAN and margin == math.inf


@pytest.mark.parametrize('order', [(0, 1), (1, 0)])
def test_two_boxes_contend_for_one_candidate_and_the_cheaper_one_owns_it(order):
    # IoU 1 and 0.5 with the candidate (0.5, 0.5, 0.5, 0.5); the class costs are equal, 2 ln 2 (Z = 2 ln 2, L0(.5) = L1(.5)): the costs differ
    # by the IoU terms alone, 3 (log(1 + 1e-8) - log(0.5 + 1e-8))
    cfg, preds = _one_cell([(.5, .5)], 2)
    boxes = np.array([[0, .5, .5, .5, .5], [1, .5, .5, .25, .5]])[list(order)]
    labels, npos, _, margin = simota.assign(preds, boxes, [0, 2], cfg)
    assert labels[0].reshape(-1).tolist() == [.5, .5, .5, .5, 1, 1, 0] and npos.tolist() == [1]
    assert abs(margin - 3 * (math.log(1 + 1e-8) - math.log(.5 + 1e-8))) < 1e-12


@pytest.mark.parametrize('third, k', [(.18, 2), (.14, 1)])
def test_k_goes_from_1_to_2_as_the_iou_sum_crosses_2(third, k):
    # three anchors in one cell against the box (0.5, 0.5, 0.4, 0.4): IoUs 1, 0.6 and `third` / 0.4 - 2.05 or 1.95 in sum
    cfg, preds = _one_cell([(.4, .4), (.4, .24), (.4, third)], 1)
    labels, npos, _, margin = simota.assign(preds, [[0, .5, .5, .4, .4]], [0, 1], cfg)
    assert npos.tolist() == [k] and labels[0][0, 0, 0, :, 4].tolist() == ([1, 1, 0] if k == 2 else [1, 0, 0])
    assert abs(margin - .05) < 1e-9


@pytest.mark.parametrize('field, value, names', [('topk', 0, 'cfg->topk'), ('topk', 33, 'cfg->topk'), ('radius', .5, 'cfg->radius'),
                                                 ('iou_weight', 0., 'cfg->iou_weight'), ('max_boxes', 257, 'cfg->max_boxes'),
                                                 ('class_num', 0, 'cfg->class_num'), (None, None, 'd_first is NULL')])
def test_argument_errors_come_before_the_device_and_name_the_argument(field, value, names):
    from k210_yolo_framework_amd import engine
    cfg = engine.make_ota_cfg(_one_cell([(.5, .5)], 1)[0])
    if field:
        setattr(cfg, field, value)
    with pytest.raises(engine.YkError, match='yk_assign_simota_f32: ' + names):
        engine.call('yk_assign_simota_f32', C.byref(cfg), None, 0, None, 1, None, None, None, None, None, 0, None)

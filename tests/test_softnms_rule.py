"""k210_yolo_framework_amd/softnms.py on its own (CPU): the loop against oracle/decode_ref.py's hard NMS, hand-derived answers for each rule, the
coverage of tests/softnms_cases.py and the input condition of its Gaussian cases."""
import numpy as np
import pytest

from k210_yolo_framework_amd import abi, engine, softnms
from oracle import decode_ref as dr
from tests import nms_cases as nc
from tests import softnms_cases as sc

F = np.float32


@pytest.mark.parametrize('cid', [nc.case_id(c) for c in nc.CASES])
def test_the_loop_with_a_hard_weight_selects_what_the_oracle_selects(cid):
    c = nc.by_id(cid)
    boxes, scores = nc.boxes_scores(c.name)
    for s in nc.slots(cid):
        sel, cur = softnms.soft_nms(boxes[s.image], scores[s.image, :, s.cls], c.obj, c.iou, 0.5, c.max_out, 'hard')
        assert np.array_equal(sel, s.selected), (s.image, s.cls)
        assert np.array_equal(cur, scores[s.image, sel, s.cls])                # hard never decays


def test_hard_weight_equals_decode_ref_on_plain_boxes():
    rng = np.random.default_rng(5)
    yx = rng.uniform(0, 200, (60, 2)).astype(F)
    boxes = np.concatenate([yx, yx + rng.uniform(5, 80, (60, 2)).astype(F)], 1)
    scores = rng.uniform(0.1, 1, 60).astype(F)
    sel, _ = softnms.soft_nms(boxes, scores, 0.05, 0.4, 0.5, 30, 'hard')
    assert sel.tolist() == dr.non_max_suppression(boxes, scores, 30, 0.4)
    for m in (0, 7):
        o = softnms.iou_to_all(boxes, m)[0]
        assert all(o[j] == dr.tf_iou(boxes, m, j) for j in range(60))          # the operations and order of decode_ref.tf_iou


# two boxes of IoU exactly 1/2 (the second is the left half of the first), a third far away
HALF = np.array([[0, 0, 16, 16], [0, 0, 16, 8], [100, 100, 116, 116]], F)


def test_linear_halves_a_box_of_iou_one_half():
    scores = np.array([1.0, 0.75, 0.25], F)
    sel, cur = softnms.soft_nms(HALF, scores, 0.05, 0.3, 0.5, 30, 'linear')
    assert sel.tolist() == [0, 1, 2] and cur.tolist() == [1.0, 0.375, 0.25]    # exactly half, kept at a floor of 0.05
    sel, cur = softnms.soft_nms(HALF, np.array([1.0, 0.75, 0.6], F), 0.5, 0.3, 0.5, 30, 'linear')
    assert sel.tolist() == [0, 2] and cur.tolist() == [1.0, F(0.6)]            # 0.375 < 0.5: dropped
    sel, cur = softnms.soft_nms(HALF, scores, 0.05, 0.5, 0.5, 30, 'linear')
    assert cur.tolist() == [1.0, 0.75, 0.25]                                   # an IoU of exactly Nt decays nothing (strict)


def test_linear_reorders_three_boxes():
    scores = np.array([1.0, 0.75, 0.5], F)
    sel, cur = softnms.soft_nms(HALF, scores, 0.05, 0.3, 0.5, 30, 'linear')
    assert sel.tolist() == [0, 2, 1] and cur.tolist() == [1.0, 0.5, 0.375]     # the halved box is overtaken by the third
    assert softnms.soft_nms(HALF, scores, 0.05, 0.3, 0.5, 30, 'hard')[0].tolist() == [0, 2]
    assert softnms.soft_nms(HALF, scores, 0.05, 0.3, 0.5, 2, 'linear')[0].tolist() == [0, 2]
    sel, cur = softnms.soft_nms(HALF, scores, 0.05, 0.3, 0.5, 30, 'gaussian')
    assert sel.tolist() == [0, 2, 1] and cur[0] == 1 and cur[1] == 0.5        # exp(-0) is exactly 1; 0.75 exp(-1/2) = 0.455 < 0.5
    assert cur[2] == F(F(0.75) * np.exp(F(-0.5), dtype=F))                     # exp(-(1/2)^2 / 0.5)


def test_diou_equals_hard_on_concentric_boxes_and_spares_a_distant_one():
    conc = np.array([[0, 0, 32, 32], [8, 8, 24, 24], [4, 12, 28, 20]], F)      # IoU 1/4 and 3/16 with the first, all centred at (16, 16)
    scores = np.array([1.0, 0.75, 0.5], F)
    for thr in (0.1, 0.2, 0.3):
        assert softnms.soft_nms(conc, scores, 0.05, thr, 0.5, 30, 'diou')[0].tolist() == \
            softnms.soft_nms(conc, scores, 0.05, thr, 0.5, 30, 'hard')[0].tolist()
    # [48, 80]^2 holds [48, 64]^2 at IoU 1/4, centres 8 px apart in both axes: d2 / c2 = 128 / 2048, 1/4 - 1/16 = 0.1875
    off = np.array([[48, 48, 80, 80], [48, 48, 64, 64]], F)
    w = softnms.weights(off, 0, 'diou', 0.2)
    assert w.tolist() == [0.0, 1.0] and softnms.weights(off, 0, 'hard', 0.2).tolist() == [0.0, 0.0]
    assert softnms.weights(off, 0, 'diou', 0.1875).tolist() == [0.0, 1.0] and softnms.weights(off, 0, 'diou', 0.18).tolist() == [0.0, 0.0]
    sel, cur = softnms.soft_nms(off, np.array([1.0, 0.5], F), 0.05, 0.2, 0.5, 30, 'diou')
    assert sel.tolist() == [0, 1] and cur.tolist() == [1.0, 0.5]               # scores never decay


def test_zero_area_boxes_take_no_part():
    boxes = np.array([[0, 0, 16, 16], [0, 4, 16, 4], [0, 0, 16, 16]], F)
    for method in ('linear', 'gaussian', 'diou'):
        sel, cur = softnms.soft_nms(boxes, np.array([0.5, 1.0, 0.75], F), 0.05, 0.3, 0.5, 30, method)
        assert sel.tolist()[:2] == [1, 2] and cur.tolist()[:2] == [1.0, 0.75]
        assert softnms.weights(boxes, 0, method, 0.3)[1] == 1 and (softnms.weights(boxes, 1, method, 0.3) == 1).all()


def test_the_own_head_holds_its_hand_built_classes():
    c = sc.by_id('soft1040-diou-obj0.05-iou0.2-max30')
    boxes, scores = sc.boxes_scores('soft1040')
    g = sc._g
    assert boxes[0, 1024].tolist() == [48, 48, 80, 80] and boxes[0, g(3, 3, 0)].tolist() == [48, 48, 64, 64]
    sel = softnms.soft_nms(boxes[0], scores[0, :, 0], c.obj, c.iou, c.sigma, c.max_out, 'diou')[0].tolist()
    assert sel == [1024, g(3, 3, 0), g(10, 10, 0)]
    assert softnms.soft_nms(boxes[0], scores[0, :, 0], c.obj, c.iou, c.sigma, c.max_out, 'hard')[0].tolist() == [1024, g(10, 10, 0)]
    sel, cur = softnms.soft_nms(boxes[0], scores[0, :, 1], 0.05, 0.3, 0.5, 30, 'linear')
    assert sel.tolist() == [g(2, 4, 0), g(9, 9, 0), g(2, 4, 1)] and cur[2] == F(scores[0, g(2, 4, 1), 1] * F(0.5))


def test_every_label_is_covered():
    seen = {}
    for c in sc.CASES:
        for lab in sc.case_labels(sc.case_id(c)):
            seen.setdefault(lab, set()).add(c.method)
    assert set(sc.LABELS) | {'batch_x_classes_over_256'} <= set(seen), set(sc.LABELS) - set(seen)
    for lab in ('n0', 'n1', 'n_at_capacity', 'n_over_capacity', 'n4032', 'score_at_thresh', 'zero_area', 'all_tied', 'batch_x_classes_over_256'):
        assert seen[lab] >= {'linear', 'gaussian', 'diou'} or lab == 'score_at_thresh', (lab, seen[lab])
    assert {'linear', 'gaussian'} <= seen['multi_decay'] and 'linear' in seen['dropped'] and 'linear' in seen['reorder']
    assert 'linear' in seen['iou_at_thresh'] and 'diou' in seen['diou_split']
    assert {c.max_out for c in sc.CASES} >= {1, 30, 65, 100}
    assert not [c for c in sc.CASES if c.method == 'gaussian' and c.base in ('g1040', 'giants')]      # (they miss the condition below)
    assert {c.method for c in sc.CASES if c.base in ('g1040', 'giants')} == {'linear', 'diou'}


@pytest.mark.parametrize('cid', [sc.case_id(c) for c in sc.CASES if c.method == 'gaussian'])
def test_gaussian_cases_meet_the_input_condition(cid):
    gap, floor = sc.gaussian_condition(sc.by_id(cid))
    print(f'{cid}: worst top-two gap {gap:.3g}, floor margin {floor:.3g}')
    assert gap >= sc.GAP and floor >= sc.GAP
    # and with it the float64 run of the rule selects the boxes the fp32 run selects
    for (d32, i32), (d64, i64) in zip(sc.reference(cid), sc.reference(cid, True)):
        assert np.array_equal(i32, i64) and np.array_equal(d32[:, 5], d64[:, 5])


def test_names_and_sigma_are_refused_by_name():
    with pytest.raises(ValueError, match="nms 'soft'"):
        softnms.method_id('soft')
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='nms_sigma'):
            softnms.check('gaussian', bad)
        softnms.check('linear', bad)                                           # read by the Gaussian only
    assert [softnms.method_id(m) for m in softnms.METHODS] == [0, 1, 2, 3]     # YK_NMS_HARD .. YK_NMS_DIOU
    with pytest.raises(engine.YkError, match="nms 'soft'"):
        engine._nms_method('soft', 0.5)


def test_the_header_declares_the_new_entry_points():
    text = engine.HEADER_PATH.read_text()
    sigs = abi.signatures(text)
    import ctypes as C
    assert sigs['yk_decode_py_nms'][1] == sigs['yk_decode_py_ex'][1] + [C.c_int, C.c_float]
    assert sigs['yk_decode_py_packed_nms'][1] == sigs['yk_decode_py_packed'][1] + [C.c_int, C.c_float]
    for k, name in enumerate(('HARD', 'LINEAR', 'GAUSSIAN', 'DIOU')):
        assert f'#define YK_NMS_{name} {k}\n' in text

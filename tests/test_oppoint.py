"""oppoint.py alone (CPU): the sweep's cut-list property against voc_eval.evaluate, its edge rules, hand-computed confusion matrices, and the
refusals of `make eval`'s --curves flags."""
import numpy as np
import pytest

from k210_yolo_framework_amd import oppoint, voc_eval
from tests import oppoint_cases as oc

D = lambda *rows: np.asarray(rows, np.float64).reshape(-1, 6)
EMPTY = np.zeros((0, 6))


@pytest.mark.parametrize('name', oc.CONFUSION_CASES)
def test_shared_cases_hold_their_content_conditions(name):
    oc.check_content(name)


# ---- sweep ------------------------------------------------------------------------------------------------------------------------------
def test_counts_are_those_of_the_list_cut_at_every_threshold():
    c = oc.case('mixed20')
    thr = np.arange(64) / 64
    s = oppoint.sweep(c['dets'], c['gts'], 20, thr, difficult=c['diff'])
    full = voc_eval.evaluate(c['dets'], c['gts'], 20, difficult=c['diff'])
    assert np.array_equal(s['n_gt'], full['n_gt']) and s['tp'].sum() > 0 and s['fp'].sum() > 0
    for k, t in enumerate(thr):
        cut = [d[d[:, 4].astype(np.float64) >= t] for d in c['dets']]
        e = voc_eval.evaluate(cut, c['gts'], 20, difficult=c['diff'])
        assert np.array_equal(e['tp'], s['tp'][:, k]) and np.array_equal(e['fp'], s['fp'][:, k]), k


def test_a_score_equal_to_a_threshold_is_in_and_minus_zero_is_in_at_zero():
    gt = [D([0, 0, 10, 10, 1, 0], [20, 20, 30, 30, 1, 0])]
    dets = [D([0, 0, 10, 10, 0.5, 0], [20, 20, 30, 30, -0.0, 0], [50, 50, 60, 60, 0.25, 0])]
    s = oppoint.sweep(dets, gt, 1, [0.0, 0.25, 0.5, 0.5000001])
    assert s['flags'].tolist() == [1, 1, 2]
    assert s['tp'].tolist() == [[2, 1, 1, 0]] and s['fp'].tolist() == [[1, 1, 0, 0]]
    assert s['precision'][0].tolist() == [2 / 3, 0.5, 1.0, 1.0] and s['recall'][0].tolist() == [1.0, 0.5, 0.5, 0.0]
    assert s['f1'][0, 3] == 0.0 and s['f1'][0, 0] == ((2.0 * (2 / 3)) * 1.0) / (2 / 3 + 1.0)


def test_tied_scores_keep_row_order():
    gt = [D([0, 0, 10, 10, 1, 0])]
    dets = [D([0, 0, 10, 9, 0.5, 0], [0, 0, 10, 10, 0.5, 0])]          # the first of the tie takes the box although the second fits better
    s = oppoint.sweep(dets, gt, 1, [0.5])
    assert s['flags'].tolist() == [1, 2] and s['tp'][0, 0] == 1 and s['fp'][0, 0] == 1


def test_a_class_without_ground_truth_and_no_rows_at_all():
    s = oppoint.sweep([D([0, 0, 10, 10, 0.9, 1])], [D([0, 0, 10, 10, 1, 0])], 2, [0.1, 0.5])
    assert np.isnan(s['recall'][1]).all() and np.isnan(s['f1'][1]).all() and s['best'].tolist() == [0, -1]
    assert s['precision'][1].tolist() == [0.0, 0.0] and s['fp'][1].tolist() == [1, 1]
    assert s['precision'][0].tolist() == [1.0, 1.0] and s['f1'][0].tolist() == [0.0, 0.0]            # no rows of the class: P 1, F1 0
    assert s['mean_f1'].tolist() == [0.0, 0.0] and s['best_all'] == 0                                 # class 1 is skipped, not NaN
    s = oppoint.sweep([EMPTY], [EMPTY], 3, [0.5])
    assert np.isnan(s['mean_f1']).all() and s['best_all'] == -1 and s['best'].tolist() == [-1, -1, -1] and len(s['flags']) == 0
    s = oppoint.sweep([EMPTY], [D([0, 0, 1, 1, 1, 0])], 1, [0.5])
    assert s['precision'][0, 0] == 1.0 and s['recall'][0, 0] == 0.0 and s['f1'][0, 0] == 0.0


def test_best_takes_the_lowest_index_on_ties():
    gt = [D([0, 0, 10, 10, 1, 0])]
    dets = [D([0, 0, 10, 10, 0.5, 0])]
    s = oppoint.sweep(dets, gt, 1, [0.1, 0.2, 0.5, 0.6])
    assert s['f1'][0].tolist() == [1.0, 1.0, 1.0, 0.0] and s['best'][0] == 0 and s['best_all'] == 0


def test_mean_f1_adds_the_classes_with_ground_truth_in_order():
    c = oc.case('mixed20')
    s = oc.sweep_reference('mixed20')
    have = [k for k in range(20) if s['n_gt'][k] > 0]
    assert 0 < len(have) < 20
    for k in (0, 125, 500, 999):
        acc = np.float64(0.0)
        for cl in have:
            acc = acc + s['f1'][cl, k]
        assert s['mean_f1'][k] == acc / np.float64(len(have))
    assert s['best_all'] == int(np.argmax(s['mean_f1']))


@pytest.mark.parametrize('bad, why', [([], 'empty'), ([0.5, 0.5], 'ascending'), ([0.5, 0.4], 'ascending'), ([0.1, np.nan], 'finite'),
                                      ([0.1, np.inf], 'finite'), (np.arange(4097) / 4097, '4097'), ([[0.1, 0.2]], 'dimension')])
def test_threshold_arrays_that_are_refused(bad, why):
    with pytest.raises(ValueError, match=why):
        oppoint.sweep([EMPTY], [EMPTY], 1, bad)
    assert len(oppoint.check_thresholds(np.arange(4096) / 4096)) == 4096


# ---- confusion --------------------------------------------------------------------------------------------------------------------------
def conf(dets, gts, K=2, t=0.5, diff=None, **kw):
    r = oppoint.confusion(dets, gts, K, t, difficult=diff, **kw)
    m, match = r['matrix'], r['match']
    hard = np.concatenate(diff).astype(bool) if diff is not None else np.zeros(sum(len(g) for g in gts), bool)
    pairs = int(sum(1 for v in match if v >= 0 and not hard[v]))
    free_boxes = int(sum(1 for b in range(len(hard)) if not hard[b] and b not in set(match.tolist())
                         and 0 <= int(np.concatenate(gts)[b, 5]) < K))
    assert m.sum() == pairs + int((match == -1).sum()) + free_boxes                # the identity
    return m.tolist(), match.tolist()


def test_a_row_over_two_boxes_takes_the_better_one():
    m, match = conf([D([0, 0, 10, 10, 0.9, 0])], [D([0, 0, 10, 8, 1, 0], [0, 0, 10, 9, 1, 1])])
    assert match == [1] and m == [[0, 0, 1], [1, 0, 0], [0, 0, 0]]


def test_two_rows_on_one_box_the_second_is_a_background_false_positive():
    m, match = conf([D([0, 0, 10, 9, 0.9, 0], [0, 0, 10, 10, 0.8, 0])], [D([0, 0, 10, 10, 1, 0])])
    assert match == [-1, 0] and m == [[1, 0, 0], [0, 0, 0], [1, 0, 0]]             # the larger IoU wins, not the larger score


def test_a_wrong_class_match_lands_off_the_diagonal():
    m, match = conf([D([0, 0, 10, 10, 0.9, 1])], [D([0, 0, 10, 10, 1, 0])])
    assert match == [0] and m == [[0, 1, 0], [0, 0, 0], [0, 0, 0]]


def test_difficult_boxes():
    gts = [D([0, 0, 10, 10, 1, 0], [50, 50, 60, 60, 1, 1])]
    m, match = conf([D([0, 0, 10, 10, 0.9, 0])], gts, diff=[np.array([True, False])])
    assert match == [0] and m == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]                 # the matched pair counts nowhere
    m, match = conf([D([0, 0, 10, 10, 0.9, 0])], gts, diff=[np.array([False, True])])
    assert match == [0] and m == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]                 # the unmatched difficult box is not a miss


def test_an_iou_of_exactly_one_half_counts():
    assert voc_eval.box_iou(np.array([0., 0, 2, 2]), np.array([[0., 0, 1, 2]]))[0] == 0.5
    m, match = conf([D([0, 0, 2, 2, 0.9, 0])], [D([0, 0, 1, 2, 1, 0])])
    assert match == [0] and m[0][0] == 1
    m, match = conf([D([0, 0, 2, 2, 0.9, 0])], [D([0, 0, 1, 2, 1, 0])], iou_thresh=0.5000001)
    assert match == [-1] and m == [[0, 0, 1], [0, 0, 0], [1, 0, 0]]


def test_equal_iou_ties_go_to_the_score_then_the_row_then_the_box():
    box = [0, 0, 10, 10]
    m, match = conf([D([*box, 0.7, 0], [*box, 0.9, 0])], [D([*box, 1, 0])])
    assert match == [-1, 0]                                                         # the larger score
    m, match = conf([D([*box, 0.0, 0], [*box, -0.0, 0])], [D([*box, 1, 0])], t=0.0)
    assert match == [0, -1]                                                         # -0.0 == +0.0: the lower row
    m, match = conf([D([*box, 0.9, 0], [*box, 0.9, 0])], [D([*box, 1, 0], [*box, 1, 1])])
    assert match == [0, 1]                                                          # the lower row takes the lower box


def test_rows_that_take_no_part():
    dets = [D([0, 0, 10, 10, 0.4, 0], [0, 0, 10, 10, 0.5, 0], [0, 0, 10, 10, 0.9, 2], [0, 0, 10, 10, 0.9, -1])]
    m, match = conf(dets, [D([0, 0, 10, 10, 1, 0], [0, 0, 10, 10, 1, 5])])
    assert match == [-2, 0, -2, -2] and m == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]      # the box of class 5 belongs nowhere either


def test_images_are_matched_apart_and_match_indexes_the_concatenated_boxes():
    box = D([0, 0, 10, 10, 1, 1])
    m, match = conf([EMPTY, D([0, 0, 10, 10, 0.9, 1]), D([0, 0, 10, 10, 0.9, 0])], [box, box, EMPTY])
    assert match == [1, -1] and m == [[0, 0, 0], [0, 1, 1], [1, 0, 0]]


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_parse_refusals(capsys):
    from k210_yolo_framework_amd import evaluate
    base = ['w.h5', '--synthetic', '8']
    a = evaluate.parse(base)
    assert a.curves == 'False' and a.conf_thresh == 0.6 and a.curve_steps == 1000 and a.curves_out is None
    a = evaluate.parse(base + ['--curves', 'True', '--conf_thresh', '0.3', '--curve_steps', '100', '--curves_out', 'c.npz'])
    assert a.curves == 'True' and a.conf_thresh == 0.3 and a.curve_steps == 100 and a.curves_out == 'c.npz'
    for bad, why in ((['--curves', 'True', '--conf_thresh', '0.01'], 'below --obj_thresh'),
                     (['--curves', 'True', '--obj_thresh', '0.7'], 'below --obj_thresh'),
                     (['--curves', 'True', '--curve_steps', '0'], '--curve_steps 0'),
                     (['--curves', 'True', '--curve_steps', '4096'], '--curve_steps 4096'),
                     (['--curves', 'True', '--conf_thresh', 'nan'], 'not a finite number'),
                     (['--curves_out', 'c.npz'], '--curves True')):
        with pytest.raises(SystemExit):
            evaluate.parse(base + bad)
        assert why in capsys.readouterr().err, bad


def test_curve_grid():
    from k210_yolo_framework_amd import evaluate
    g = evaluate.curve_grid(0.05, 0.6, 1000)
    assert g[0] == 0.05 and g[-1] == 0.999 and len(g) == 950 and (g == 0.6).sum() == 1 and np.all(np.diff(g) > 0)
    g = evaluate.curve_grid(0.05, 0.6125, 100)
    assert len(g) == 96 and g[g.tolist().index(0.6125) - 1] == 0.61 and np.all(np.diff(g) > 0)       # appended in its place
    assert evaluate.curve_grid(0.9999, 0.99995, 10).tolist() == [0.99995]
    oppoint.check_thresholds(evaluate.curve_grid(0.0, 1.5, 4095))

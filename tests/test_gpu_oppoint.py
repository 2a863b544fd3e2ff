"""map_gpu.MapEvaluator.sweep and .confusion (csrc/yk_map.hip) against oppoint.py on the shared cases of
tests/oppoint_cases.py.  Everything is exact: tp, fp, best, best_all, matrix and match are integers; precision, recall, f1 and mean_f1 are each
one fixed chain of float64 operations on equal integers (the library is compiled without contraction), so they are compared bit for bit,
NaNs included."""
import json
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import oppoint
from tests import oppoint_cases as oc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def evaluator(c, plus_one=False):
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    ev = MapEvaluator(c['class_num'], plus_one=plus_one)
    rows, off = oc.pack(c['dets'])
    ev.add(rows, off, c['gts'], c['diff'])
    return ev


def same_sweep(got, ref):
    for k in ('flags', 'n_gt', 'tp', 'fp', 'best'):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (k, np.argwhere(np.asarray(got[k]) != np.asarray(ref[k]))[:8])
    assert got['best_all'] == ref['best_all']
    for k in ('thresholds', 'precision', 'recall', 'f1', 'mean_f1'):
        a, b = np.ascontiguousarray(got[k], np.float64), np.ascontiguousarray(ref[k], np.float64)
        assert a.shape == b.shape
        bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        print(k, 'entries', a.size, 'different bits', len(bad))
        assert len(bad) == 0, (k, len(bad), bad[:8], a[tuple(bad[0])], b[tuple(bad[0])])


def same_confusion(got, ref):
    for k in ('matrix', 'match'):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:8])


def ref_sweep(c, grid, plus_one=False):
    return oppoint.sweep(c['dets'], c['gts'], c['class_num'], grid, 0.5, c['diff'], plus_one)


# ---- sweep ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', oc.SWEEP_CASES)
def test_sweep_of_the_shared_cases_on_the_default_grid(name):
    oc.check_content(name)                                  # at least one score equals a grid threshold
    c = oc.case(name)
    got = evaluator(c).sweep()
    same_sweep(got, oc.sweep_reference(name))
    assert got['tp'].shape == (c['class_num'], 1000) and got['tp'].sum() > 0 and got['fp'].sum() > 0


@pytest.mark.parametrize('grid', ['one', 'two', 'most'])
@pytest.mark.parametrize('name', ['mixed20', 'wide80'])
def test_sweep_with_1_2_and_4096_thresholds(name, grid):
    same_sweep(evaluator(oc.case(name)).sweep(oc.GRIDS[grid]), oc.sweep_reference(name, grid))


@pytest.mark.parametrize('n_rows', [0, 1, 255, 256, 257])
def test_sweep_row_counts_around_a_workgroup(n_rows):
    c = oc.head(oc.case('wide80'), n_rows)                  # 80 classes, some rows with a class out of range
    ev = evaluator(c)
    assert ev.n_rows == n_rows
    same_sweep(ev.sweep(), ref_sweep(c, oc.GRIDS['default']))


def test_sweep_one_class_plus_one_and_nothing_at_all():
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    c = oc.one_class()
    same_sweep(evaluator(c).sweep(), ref_sweep(c, oc.GRIDS['default']))
    c = oc.case('mixed20')
    same_sweep(evaluator(c, plus_one=True).sweep(), oc.sweep_reference('mixed20', 'default', True))
    ev = MapEvaluator(3)
    same_sweep(ev.sweep(), oppoint.sweep([], [], 3, oc.GRIDS['default']))
    ev.add(np.zeros((0, 6), np.float32), np.zeros(2, np.int32), [np.array([[0., 0, 5, 5, 1, 1]])])
    same_sweep(ev.sweep([0.5]), oppoint.sweep([np.zeros((0, 6))], [np.array([[0., 0, 5, 5, 1, 1]])], 3, [0.5]))


def test_sweep_refuses_bad_threshold_arrays_by_name():
    from k210_yolo_framework_amd import engine
    ev = evaluator(oc.case('mixed20'))
    for bad, why in ((np.arange(4097) / 4097, '4097'), ([0.5, 0.4], 'ascending'), ([0.5, 0.5], 'ascending'), ([], 'empty'),
                     ([0.1, float('nan')], 'finite')):
        with pytest.raises(engine.YkError, match=why):
            ev.sweep(bad)
    with pytest.raises(engine.YkError, match='4097 thresholds'):                   # the entry point refuses too, before any launch
        engine.call('yk_map_sweep_workspace_bytes', 10, 20, 4097, None)
    same_sweep(ev.sweep(), oc.sweep_reference('mixed20'))                          # the evaluator is still good


# ---- confusion --------------------------------------------------------------------------------------------------------------------------
def test_the_staged_bound_is_the_one_the_cases_are_built_for():
    from k210_yolo_framework_amd import map_gpu
    assert map_gpu.confusion_lds_boxes() == oc.LDS_BOXES
    c = oc.case('lds')
    sizes = [len(d) + len(g) for d, g in zip(c['dets'], c['gts'])]
    assert sizes[-2:] == [oc.LDS_BOXES, oc.LDS_BOXES + 1] and all(d[:, 4].min() >= c['conf'] for d in c['dets'][-2:])


@pytest.mark.parametrize('name', oc.CONFUSION_CASES)
def test_confusion_of_the_shared_cases(name):
    oc.check_content(name)                                  # >= 3 off-diagonal matches, >= 3 background FP, >= 3 background FN
    c = oc.case(name)
    scores = np.concatenate([d[:, 4] for d in c['dets']])
    assert (scores == np.float32(c['conf'])).any()          # conf_thresh equals a score
    got = evaluator(c).confusion(c['conf'])
    same_confusion(got, oc.confusion_reference(name))
    assert got['matrix'].shape == (c['class_num'] + 1,) * 2 and (got['match'] == -2).any() == (scores < c['conf']).any()


def test_confusion_plus_one_other_thresholds_and_nothing_at_all():
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    c = oc.case('mixed20')
    same_confusion(evaluator(c, plus_one=True).confusion(c['conf']), oc.confusion_reference('mixed20', True))
    ev = evaluator(c)
    for conf, iou in ((0.0, 0.3), (-1.0, 0.5), (0.875, 0.75), (2.0, 0.5)):
        same_confusion(ev.confusion(conf, iou), oppoint.confusion(c['dets'], c['gts'], 20, conf, iou, c['diff']))
    ev = MapEvaluator(3)
    same_confusion(ev.confusion(0.5), oppoint.confusion([], [], 3, 0.5))


# ---- both -------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes_on_any_stream_and_nothing_else_moves():
    import torch
    c = oc.case('lanes')
    ev = evaluator(c)
    before, coco_before = ev.result(), ev.coco_result()
    s1, m1 = ev.sweep(), ev.confusion(c['conf'])
    side = torch.cuda.Stream()
    s2, m2 = ev.sweep(stream=side), ev.confusion(c['conf'], stream=side)
    after, coco_after = ev.result(), ev.coco_result()
    for k in ('thresholds', 'tp', 'fp', 'n_gt', 'precision', 'recall', 'f1', 'best', 'mean_f1', 'flags'):
        assert s1[k].tobytes() == s2[k].tobytes(), k
    assert s1['best_all'] == s2['best_all']
    for k in ('matrix', 'match'):
        assert m1[k].tobytes() == m2[k].tobytes(), k
    same_sweep(s2, oc.sweep_reference('lanes'))
    same_confusion(m2, oc.confusion_reference('lanes'))
    assert np.array_equal(s1['flags'], before['flags'])
    for k in ('flags', 'n_gt', 'n_det', 'tp', 'fp', 'ap'):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert np.float64(before['map']).tobytes() == np.float64(after['map']).tobytes()
    for k in ('flags', 'npig', 'n_det', 'precision', 'recall', 'ap_class'):
        assert coco_before[k].tobytes() == coco_after[k].tobytes(), k
    assert ev.n_rows == sum(len(d) for d in c['dets']) and ev.n_img == len(c['dets'])


# ---- make eval --------------------------------------------------------------------------------------------------------------------------
VOC_KEYS = ['ckpt', 'precision', 'images', 'rows', 'obj_thresh', 'nms_iou', 'iou_thresh', 'voc07', 'note', 'map', 'ap', 'n_gt', 'n_det', 'tp', 'fp']


def test_cli_curves_adds_the_operating_object_and_nothing_else(tmp_path, capsys, monkeypatch):
    from k210_yolo_framework_amd import evaluate, netspec as ns
    monkeypatch.chdir(ROOT)
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.5)
    ck = tmp_path / 'w.npz'
    np.savez(ck, **spec.init_weights(seed=3))
    net = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--synthetic', '8', '--obj_thresh', '0.0', '--batch', '8']
    plain = evaluate.main([str(ck), '--out', str(tmp_path / 'voc.json')] + net)
    text_voc = capsys.readouterr().out
    voc_bytes = (tmp_path / 'voc.json').read_bytes()
    assert list(plain) == VOC_KEYS and voc_bytes == json.dumps(plain, indent=1).encode() and 'operating' not in text_voc
    rep = evaluate.main([str(ck), '--curves', 'True', '--conf_thresh', '0.3', '--curve_steps', '200', '--out', str(tmp_path / 'op.json'),
                         '--curves_out', str(tmp_path / 'curves.npz'), '--dump_rows', str(tmp_path / 'rows.npz')] + net)
    text = capsys.readouterr().out
    got = json.loads((tmp_path / 'op.json').read_text())
    assert list(got) == VOC_KEYS + ['operating']
    assert json.dumps({k: got[k] for k in VOC_KEYS}, indent=1).encode() == voc_bytes                 # no other key or value moved
    assert text.startswith(text_voc.split(' wrote ')[0].rsplit('\n', 1)[0])                         # the VOC lines are the same lines
    assert 'operating points' in text and 'confusion at 0.3' in text and 'best mean F1' in text and 'hard NMS scores' in text
    # the figures are oppoint.py's of the rows that were scored
    z = np.load(tmp_path / 'rows.npz')
    n_img = len(z['gt_offsets']) - 1
    off = np.searchsorted(z['image'], np.arange(n_img + 1))
    split = lambda a, o: [a[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    dets, gts = split(z['rows'], off), split(z['gt'], z['gt_offsets'])
    grid = evaluate.curve_grid(0.0, 0.3, 200)
    assert len(grid) == 200 and rep['rows'] > 0
    ref, cm = oppoint.sweep(dets, gts, 20, grid), oppoint.confusion(dets, gts, 20, 0.3)
    op, at = got['operating'], int(np.nonzero(grid == 0.3)[0][0])
    num = lambda v: None if v != v else float(v)
    assert op['conf_thresh'] == 0.3 and op['iou_thresh'] == 0.5 and op['steps'] == 200 and op['confusion'] == cm['matrix'].tolist()
    assert 'confusion[true][predicted]' in op['confusion_axes'] and 'background' in op['confusion_axes']
    for key in ('precision', 'recall', 'f1'):
        assert op[key] == [num(v) for v in ref[key][:, at]], key
    assert op['class_best_threshold'] == [None if b < 0 else float(grid[b]) for b in ref['best']]
    assert op['best_threshold'] == num(grid[ref['best_all']]) and op['best_mean_f1'] == num(ref['mean_f1'][ref['best_all']])
    c = np.load(tmp_path / 'curves.npz')
    assert sorted(c.files) == sorted(['thresholds', 'tp', 'fp', 'precision', 'recall', 'f1', 'mean_f1', 'matrix'])
    assert np.array_equal(c['tp'], ref['tp']) and np.array_equal(c['fp'], ref['fp']) and np.array_equal(c['matrix'], cm['matrix'])
    assert c['f1'].tobytes() == ref['f1'].tobytes() and c['mean_f1'].tobytes() == ref['mean_f1'].tobytes()

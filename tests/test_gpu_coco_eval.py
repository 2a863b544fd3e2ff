"""map_gpu.MapEvaluator.coco_result (csrc/yk_map.hip) against coco_eval.evaluate on the shared cases of tests/coco_cases.py:
flags, npig and n_det exactly equal; every precision and recall entry exactly equal (each is one division and a maximum of such); the
summary figures and ap_class within 1e-12 absolute, the bound tests/test_gpu_map_eval.py holds AP sums to (a mean of at most
10 * 101 * 20 values in [0, 1]: numpy adds them pairwise, the device per thread and then by a fixed tree of 256, either within
(80 + 8) * 2^-53 relative); the same absent (-1 / NaN) entries."""
import json
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import coco_eval
from tests import coco_cases as cc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-12


def pack(dets):
    dets = [np.asarray(d, np.float32).reshape(-1, 6) for d in dets]
    off = np.zeros(len(dets) + 1, np.int32)
    off[1:] = np.cumsum([len(d) for d in dets])
    return (np.concatenate(dets) if dets else np.zeros((0, 6), np.float32)), off


def evaluator(c):
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    ev = MapEvaluator(c['class_num'])
    rows, off = pack(c['dets'])
    ev.add(rows, off, c['gts'], c['diff'])
    return ev


def compare(got, ref):
    for k in ('flags', 'npig', 'n_det'):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:8])
    for k in ('precision', 'recall'):
        assert got[k].shape == ref[k].shape
        bad = np.argwhere(got[k] != ref[k])
        assert len(bad) == 0, (k, len(bad), bad[:8], got[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    for k in coco_eval.SUMMARY:
        print(k, got[k], ref[k])
        assert (np.isnan(got[k]) and np.isnan(ref[k])) or abs(got[k] - ref[k]) <= TOL, k
    assert np.array_equal(np.isnan(got['ap_class']), np.isnan(ref['ap_class']))
    have = ~np.isnan(ref['ap_class'])
    if have.any():
        assert np.abs(got['ap_class'][have] - ref['ap_class'][have]).max() <= TOL


@pytest.mark.parametrize('name', ['mixed20', 'one_class', 'lanes', 'scan', 'cut'])
def test_shared_cases_with_the_default_thresholds_and_ranges(name):
    c = cc.case(name)
    got = evaluator(c).coco_result(max_dets=c['max_dets'])
    ref = cc.reference(name)
    compare(got, ref)
    assert got['flags'].shape[:2] == (4, 10) and got['precision'].shape == (10, 101, c['class_num'], 4)


@pytest.mark.parametrize('config', ['t1a1', 't16a4', 't64a1'])
@pytest.mark.parametrize('name', ['one_class', 'lanes'])
def test_other_numbers_of_thresholds_and_ranges(name, config):
    c = cc.case(name)
    thr, area = cc.CONFIGS[config]
    got = evaluator(c).coco_result(thr, area, c['max_dets'])
    compare(got, cc.reference(name, config))
    if config == 't1a1':
        assert abs(got['ap'] - got['ap50']) <= TOL and np.isnan(got['ap75']) and np.isnan(got['ap_small'])


def test_more_than_64_pairs_is_refused_by_name():
    from k210_yolo_framework_amd import engine
    thr, area = cc.CONFIGS['t13a5']
    assert len(thr) * len(area) == 65
    ev = evaluator(cc.case('one_class'))
    with pytest.raises(engine.YkError, match='13 IoU thresholds x 5 area ranges'):
        ev.coco_result(thr, area)
    with pytest.raises(engine.YkError):
        ev.coco_result(np.zeros(0), None)
    compare(ev.coco_result(), cc.reference('one_class'))                              # the evaluator is still good


def test_edge_inputs():
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    empty = np.zeros((0, 6))
    D = lambda *rows: np.asarray(rows, np.float64).reshape(-1, 6)
    for dets, gts, K in (([empty, empty], [D([0, 0, 10, 10, 1, 0]), empty], 2),      # no detections
                         ([D([0, 0, 10, 10, .9, 0]), empty], [empty, empty], 2),      # no ground truth
                         ([], [], 2),                                                 # nothing
                         ([D([0, 0, 40, 40, .9, 0], [0, 0, 5, 5, .7, 2], [0, 0, 5, 5, .6, 7], [0, 0, 5, 5, .6, -3])],
                          [D([0, 0, 40, 40, 1, 0], [50, 50, 90, 90, 1, 1], [50, 50, 90, 90, 1, 9])], 3)):
        ev = MapEvaluator(K)
        rows, off = pack(dets)
        ev.add(rows, off, gts)
        compare(ev.coco_result(), coco_eval.evaluate(dets, gts, K))
    compare(ev.coco_result(max_dets=0), coco_eval.evaluate(dets, gts, K, max_dets=0))


def test_two_calls_give_the_same_bits_and_result_is_untouched():
    c = cc.case('mixed20')
    ev = evaluator(c)
    before = ev.result()
    a = ev.coco_result()
    after = ev.result()
    b = ev.coco_result()
    for k in ('flags', 'npig', 'n_det', 'precision', 'recall', 'ap_class'):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in coco_eval.SUMMARY:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
    for k in ('flags', 'n_gt', 'n_det', 'tp', 'fp', 'ap'):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert np.float64(before['map']).tobytes() == np.float64(after['map']).tobytes()


def test_padded_and_packed_forms_give_the_same_answer():
    import torch
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    c = cc.case('mixed20')
    dets = c['dets']
    cap = max(len(d) for d in dets) + 3
    pad = np.full((len(dets), cap, 6), 7.0, np.float32)
    cnt = np.array([len(d) for d in dets], np.int32)
    for b, d in enumerate(dets):
        pad[b, :len(d)] = d
    ev = MapEvaluator(c['class_num'])
    ev.add(torch.from_numpy(pad[:5]).cuda(), torch.from_numpy(cnt[:5]).cuda(), c['gts'][:5], c['diff'][:5])
    ev.add(pad[5:], cnt[5:], c['gts'][5:], c['diff'][5:])
    compare(ev.coco_result(), cc.reference('mixed20'))


VOC_KEYS = ['ckpt', 'precision', 'images', 'rows', 'obj_thresh', 'nms_iou', 'iou_thresh', 'voc07', 'note', 'map', 'ap', 'n_gt', 'n_det', 'tp', 'fp']


def test_cli_metric_coco_writes_the_coco_object(tmp_path, capsys, monkeypatch):
    from k210_yolo_framework_amd import evaluate, netspec as ns
    monkeypatch.chdir(ROOT)
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.5)
    ck = tmp_path / 'w.npz'
    np.savez(ck, **spec.init_weights(seed=3))
    net = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--synthetic', '8', '--obj_thresh', '0.0', '--batch', '8']
    plain = evaluate.main([str(ck), '--out', str(tmp_path / 'voc.json')] + net)
    text_voc = capsys.readouterr().out
    assert list(json.loads((tmp_path / 'voc.json').read_text())) == VOC_KEYS and 'COCO' not in text_voc
    rep = evaluate.main([str(ck), '--metric', 'coco', '--out', str(tmp_path / 'coco.json'), '--dump_rows', str(tmp_path / 'rows.npz')] + net)
    text = capsys.readouterr().out
    got = json.loads((tmp_path / 'coco.json').read_text())
    assert list(got) == VOC_KEYS + ['coco'] and {k: got[k] for k in VOC_KEYS if k != 'ckpt'} == {k: plain[k] for k in VOC_KEYS if k != 'ckpt'}
    assert text.startswith(text_voc.split(' wrote ')[0].rsplit('\n', 1)[0])           # the VOC lines are the same lines
    assert 'AP   IoU .50:.95  all' in text and 'AR   IoU .50:.95  large' in text and 'at most 30 detections per class and image' in text
    z = np.load(tmp_path / 'rows.npz')
    n_img = len(z['gt_offsets']) - 1
    off = np.searchsorted(z['image'], np.arange(n_img + 1))
    split = lambda a, o: [a[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    ref = coco_eval.evaluate(split(z['rows'], off), split(z['gt'], z['gt_offsets']), 20)
    assert rep['rows'] > 0 and got['coco']['n_det'] == ref['n_det'].tolist() and got['coco']['npig'] == ref['npig'].tolist()
    for k in coco_eval.SUMMARY:
        assert (got['coco'][k] is None and np.isnan(ref[k])) or abs(got['coco'][k] - ref[k]) <= TOL, k
    for k in range(20):
        assert (got['coco']['ap_class'][k] is None) == bool(np.isnan(ref['ap_class'][k]))
    with pytest.raises(SystemExit):
        evaluate.parse([str(ck), '--metric', 'coco', '--voc07', 'True'] + net)

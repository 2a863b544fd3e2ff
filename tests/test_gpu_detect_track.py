"""detect.run(track=True): the plain run's rows pushed through track.Tracker on the host, bit for bit, with batches that a sequence
straddles; track=False is the default run; the refused combinations; the MOTChallenge file."""
import json

import numpy as np
import pytest

from k210_yolo_framework_amd import track as tk

pytestmark = pytest.mark.gpu
F = np.float32
# seeded random weights saturate: about 400 of a frame's 600 rows score above 0.5 and about 70 above 0.95, so the thresholds sit high
KW = dict(draw=False, batch=5, depth=2, obj_thresh=0.5, iou_thresh=0.5, verbose=False)
TRACK = dict(track_thresh=0.85, track_low=0.5, track_match=0.8, track_buffer=2, track_max=1024)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """12 frames of two moving rectangles through a seeded random network: the default run, and the tracked one with its files."""
    from k210_yolo_framework_amd import detect
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.yolonet import YoloModel
    from tests.plan_zoo import residual
    spec, weights = residual()
    model = YoloModel(spec, {'weights': weights, 'precision': 'f16x2'}, False)
    h = Helper(None, 20, VOC_ANCHORS, np.array([list(spec.in_hw)]), np.array([list(x) for x in spec.out_hw()]))
    pics = []
    for t in range(12):
        p = np.full((96, 128, 3), 40, np.uint8)
        p[20:60, 10 + 6 * t:40 + 6 * t] = (220, 60, 60)
        p[50:90, 90 - 5 * t:120 - 5 * t] = (60, 200, 240)
        pics.append(p)
    out = tmp_path_factory.mktemp('tracked')
    plain = detect.run(h, model, pics, **KW)
    tracked = detect.run(h, model, pics, out_dir=out, track=True, **TRACK, **KW)
    yield h, model, pics, plain, tracked, out
    model._drop_plan()


def test_tracked_rows_are_the_plain_rows_through_the_host_tracker(runs):
    _, _, _, plain, tracked, _ = runs
    host = tk.Tracker(20, TRACK['track_thresh'], TRACK['track_low'], TRACK['track_match'], TRACK['track_buffer'], TRACK['track_max'])
    assert sum(len(d) for d in plain['detections']) > 0 and tracked['sequences'] == ['sequence']
    for rows, got, ids in zip(plain['detections'], tracked['detections'], tracked['track_ids']):
        want, want_ids = host.update(rows, cap=600)
        assert np.array_equal(ids, want_ids)
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert sum(len(i) for i in tracked['track_ids']) > 0


def test_track_false_is_the_default_run(runs):
    from k210_yolo_framework_amd import detect
    h, model, pics, plain, _, _ = runs
    off = detect.run(h, model, pics, track=False, **TRACK, **KW)
    assert sorted(off) == sorted(plain)
    assert all(a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(off['detections'], plain['detections']))


@pytest.mark.parametrize('kw, name', [(dict(tiles=(2, 2)), 'tiles'), (dict(tta='flip'), 'tta'), (dict(nms='linear'), 'nms')])
def test_track_refuses_what_it_cannot_be_combined_with(runs, kw, name):
    from k210_yolo_framework_amd import detect, engine
    h, model, pics, *_ = runs
    with pytest.raises(engine.YkError, match=f'{name}.*track|track.*{name}'):
        detect.run(h, model, pics, track=True, **kw, **KW)


def test_the_mot_file_and_the_json_parse_back_to_the_rows(runs):
    _, _, _, _, tracked, out = runs
    lines = [ln.split(',') for ln in (out / 'tracks' / 'sequence.txt').read_text().splitlines()]
    want = [(f, int(i), r) for f, (rows, ids) in enumerate(zip(tracked['detections'], tracked['track_ids']), 1) for r, i in zip(rows, ids)]
    assert len(lines) == len(want)
    for ln, (f, i, r) in zip(lines, want):
        assert (int(ln[0]), int(ln[1])) == (f, i) and ln[7:] == ['-1', '-1', '-1']
        assert [F(v) for v in ln[2:7]] == [r[1], r[0], r[3] - r[1], r[2] - r[0], r[4]]
    doc = json.loads((out / 'detections.json').read_text())
    assert [[r[6] for r in d['detections']] for d in doc] == [i.tolist() for i in tracked['track_ids']]
    assert all([F(v) for v in r[:6]] == list(w) for d, rows in zip(doc, tracked['detections']) for r, w in zip(d['detections'], rows))
    assert doc[0]['tracker'] == 'bytetrack-greedy' and doc[0]['track_buffer'] == TRACK['track_buffer'] and doc[0]['sequence'] == 'sequence'

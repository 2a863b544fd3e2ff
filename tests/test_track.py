"""track.py on the CPU: the 2 x 2-block filter against the dense 8 x 8 filter in float64, the rule on hand-built rows with known answers,
and the option checks."""
import numpy as np
import pytest

from k210_yolo_framework_amd import track as tk

F = np.float32


def row(top, left, h, w, score=0.9, cls=3):
    return [top, left, top + h, left + w, score, cls]


def ids_over(tracker, frames):
    return [tracker.update(np.asarray(f, F).reshape(-1, 6))[1].tolist() for f in frames]


def test_block_filter_equals_the_dense_filter_in_float64():
    D = np.float64
    box = lambda t: np.array([20 + 2 * t, 30 + 3 * t, 80 + 2.5 * t, 70 + 3.2 * t], D)
    mean, cov = tk.kf_open(tk.measure(box(0), D), D)
    x = mean.copy()
    P = np.diag(np.concatenate([cov[:4], cov[8:]]))
    Fm = np.eye(8)
    Fm[:4, 4:] = np.eye(4)
    H = np.eye(4, 8)
    for t in range(1, 51):
        h = x[3]
        q = np.array([h / 20, h / 20, 1e-2, h / 20, h / 160, h / 160, 1e-5, h / 160]) ** 2
        x, P = Fm @ x, Fm @ P @ Fm.T + np.diag(q)
        h = x[3]
        S = H @ P @ H.T + np.diag(np.array([h / 20, h / 20, 1e-1, h / 20]) ** 2)
        K = P @ H.T @ np.linalg.inv(S)
        z = tk.measure(box(t), D)
        x, P = x + K @ (z - H @ x), P - K @ S @ K.T
        mean, cov = tk.kf_update(*tk.kf_predict(mean, cov, D), z, D)
        np.testing.assert_allclose(mean, x, rtol=1e-9)
        np.testing.assert_allclose(cov, np.concatenate([np.diag(P)[:4], np.diag(P, 4), np.diag(P)[4:]]), rtol=1e-9)
        off = P.copy()
        for k in range(4):
            off[k, k] = off[k + 4, k + 4] = off[k, k + 4] = off[k + 4, k] = 0
        assert not off.any()


def test_a_box_moving_right_keeps_its_id():
    assert ids_over(tk.Tracker(20), [[row(10, 10 + 4 * t, 40, 30)] for t in range(8)]) == [[1]] * 8


@pytest.mark.parametrize('gap, want', [(3, 1), (4, 2)])
def test_a_lost_track_is_found_again_within_the_buffer_and_not_after(gap, want):
    t = tk.Tracker(20, track_buffer=3)
    seen = ids_over(t, [[row(10, 10, 40, 30)]] * 3 + [[]] * gap + [[row(10, 10, 40, 30)]] * 2)
    assert seen[:3] == [[1]] * 3 and seen[3:3 + gap] == [[]] * gap
    # within the buffer the old track takes the row at once; after it a NEW track opens, seen from its second frame on
    assert seen[3 + gap:] == ([[1], [1]] if want == 1 else [[], [2]])


def test_a_low_score_keeps_the_track_alive_and_opens_none():
    t = tk.Tracker(20)
    seen = ids_over(t, [[row(10, 10, 40, 30)], [row(10, 10, 40, 30, 0.3)], [row(10, 10, 40, 30, 0.3), row(100, 100, 40, 30, 0.3)]])
    assert seen == [[1], [1], [1]] and t.live == 1 and t.next_id == 2
    assert ids_over(tk.Tracker(20), [[row(10, 10, 40, 30)], [row(10, 10, 40, 30, 0.05)]]) == [[1], []]      # below low_thresh: not seen


def test_a_new_track_without_a_match_in_its_second_frame_is_gone():
    t = tk.Tracker(20)
    seen = ids_over(t, [[row(10, 10, 40, 30)], [row(10, 10, 40, 30), row(100, 100, 40, 30)], [row(10, 10, 40, 30)]])
    assert seen == [[1], [1], [1]] and t.live == 1 and t.next_id == 3
    # 0.55 is high but below track_thresh + 0.1: it opens nothing
    assert ids_over(tk.Tracker(20), [[row(10, 10, 40, 30)], [row(10, 10, 40, 30), row(100, 100, 40, 30, 0.55)]])[1] == [1]


def test_overlapping_boxes_of_two_classes_never_exchange_ids():
    t = tk.Tracker(20)
    frames = [[row(10, 10 + 2 * k, 40, 30, 0.9, 3), row(12, 8 + 2 * k, 40, 30, 0.8, 5)][::(1 if k % 2 == 0 else -1)] for k in range(6)]
    for k, f in enumerate(frames):
        rows, ids = t.update(np.asarray(f, F))
        assert ids.tolist() == [1, 2] and rows[:, 5].tolist() == [3, 5]


def test_equal_iou_ties_go_to_the_lowest_track_then_the_lowest_row():
    t = tk.Tracker(20)
    t.update(np.asarray([row(10, 10, 40, 30), row(10, 10, 40, 30)], F))                    # two identical tracks, ids 1 and 2
    rows, ids = t.update(np.asarray([row(10, 10, 40, 30, 0.7), row(10, 10, 40, 30, 0.8)], F))   # two identical rows
    assert ids.tolist() == [1, 2] and rows[:, 4].tolist() == [F(0.7), F(0.8)]


@pytest.mark.parametrize('kw, name', [(dict(track_thresh=float('nan')), 'track_thresh'), (dict(low_thresh=0.6), 'track_low'),
                                      (dict(match_thresh=0.0), 'track_match'), (dict(track_buffer=-1), 'track_buffer'),
                                      (dict(track_buffer=2.5), 'track_buffer'), (dict(max_tracks=tk.MAX_TRACKS + 1), 'track_max'),
                                      (dict(tiles=(2, 2)), 'tiles'), (dict(tta='flip'), 'tta'), (dict(nms='linear'), 'nms')])
def test_check_refuses_bad_options_by_name(kw, name):
    with pytest.raises(ValueError, match=name):
        tk.check(**kw)
    assert tk.check() == tk.DEFAULTS

"""track.Tracker(assign='lap', fuse_score=...): the optimal association against a brute force over every partial assignment, the case
that separates it from the greedy rule, and the score fusion of the first stage.  The similarities are given, not drawn as boxes:
track.iou_matrix is replaced for the frame under test."""
import itertools

import numpy as np
import pytest

from k210_yolo_framework_amd import track as tk

F = np.float32


def associate(monkeypatch, sim, scores, new=False, **opts):
    """len(sim) tracks (TRACKED; with `new`, NEW) meet len(scores) rows of their class whose IoUs are `sim` -> the row of every track, or -1."""
    sim = np.asarray(sim, F)
    t = tk.Tracker(1, **opts)
    for _ in range(2 if new else 1):                                     # tracks opened on a later frame than the first are NEW
        t.update([[100.0 * k, 0, 100.0 * k + 40, 30, 0.9, 0] for k in range(len(sim))] if t.frame or not new else [])
    monkeypatch.setattr(tk, 'iou_matrix', lambda a, b: sim)
    t.update([[0, 0, 40, 30, s, 0] for s in scores])
    hit = (t.state[:len(sim)] == tk.TRACKED) & (t.last[:len(sim)] == t.frame)
    return [scores.index(float(s)) if h else -1 for s, h in zip(t.score[:len(sim)].astype(np.float64), hit)]


def brute_force(sim, thr):
    """Every partial assignment over the allowed pairs, float64: the most pairs, then the smallest cost sum -> (best, it is the only one)."""
    n_t, n_r = sim.shape
    found = []
    for rows in itertools.product(range(-1, n_r), repeat=n_t):
        used = [r for r in rows if r >= 0]
        if len(set(used)) == len(used) and all(r < 0 or sim[t, r] >= thr for t, r in enumerate(rows)):
            found.append((-len(used), sum(1.0 - float(sim[t, r]) for t, r in enumerate(rows) if r >= 0), list(rows)))
    found.sort()
    unique = len(found) == 1 or found[1][0] != found[0][0] or found[1][1] - found[0][1] > 1e-6
    return found[0][2], unique


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('shape', [(1, 1), (2, 3), (3, 2), (4, 5), (5, 4), (5, 5)])
def test_lap_is_the_brute_force_optimum(monkeypatch, shape, seed):
    rng = np.random.default_rng([seed, *shape])
    sim = rng.uniform(0, 1, shape).astype(F)
    scores = [float(F(0.6 + 0.05 * k)) for k in range(shape[1])]         # distinct, so that a track's score names its row
    want, unique = brute_force(sim, F(0.5))
    assert unique                                                        # (no tie rule is involved: the seeds are chosen so)
    assert associate(monkeypatch, sim, scores, match_thresh=0.5, assign='lap') == want


def test_the_crossing_that_greedy_loses_and_lap_keeps(monkeypatch):
    sim, scores = [[0.9, 0.8], [0.85, 0.1]], [0.75, 0.875]
    assert associate(monkeypatch, sim, scores) == [0, -1]
    assert associate(monkeypatch, sim, scores, assign='lap') == [1, 0]


@pytest.mark.parametrize('assign', tk.ASSIGNS)
def test_fuse_score_is_the_first_stage_only(monkeypatch, assign):
    run = lambda *a, **kw: associate(monkeypatch, *a, assign=assign, **kw)
    assert run([[0.625, 0.625]], [0.75, 0.875], fuse_score=False) == [0]         # equal IoU: the lowest row
    assert run([[0.625, 0.625]], [0.75, 0.875], fuse_score=True) == [1]          # 0.625 * 0.875 is the larger
    assert run([[0.25]], [0.75], fuse_score=True) == [-1]                        # 0.1875 is below stage 1's 0.2 ...
    assert run([[0.25]], [0.75], fuse_score=False) == [0]                        # ... that the IoU alone meets
    assert run([[0.625]], [0.25], fuse_score=True) == [0]                        # stage 2 (a low row): 0.625 >= 0.5, not 0.15625
    assert run([[0.375]], [0.75], new=True, fuse_score=True) == [0]              # stage 3 (a NEW track): 0.375 >= 0.3, not 0.28125


def test_check_refuses_an_unknown_assign_by_name():
    with pytest.raises(ValueError, match="track_assign 'hungarian'"):
        tk.check(assign='hungarian')
    with pytest.raises(ValueError, match='track_fuse'):
        tk.check(fuse_score='yes')
    assert tk.check() == tk.DEFAULTS and tk.check(assign='lap', fuse_score=True) == dict(tk.DEFAULTS, assign='lap', fuse_score=True)

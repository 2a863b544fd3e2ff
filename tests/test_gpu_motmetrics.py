"""motmetrics_gpu.lap (yk_lap_f64) against motmetrics.lap, assignment for assignment, and its totals against scipy's; MotEvaluator
(yk_mot_eval) against motmetrics.evaluate: integers equal, float sums and summaries within 1e-12; make trackeval cpu against gpu."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from k210_yolo_framework_amd import motmetrics as mm

pytestmark = pytest.mark.gpu


def switch_side():
    """The largest square whose matrix still lives in LDS beside the vectors, from the header's budget."""
    from k210_yolo_framework_amd import motmetrics_gpu as mg
    k = mg.limits()
    n = 1
    while 8 * (n + 1) ** 2 + (k['LDS_PER_COL'] + k['LDS_PER_ROW']) * (n + 1) <= k['LDS_BYTES']:
        n += 1
    assert mg.lds_resident(n, n) and not mg.lds_resident(n + 1, n + 1)
    return n


def integer_costs(name):
    rng = np.random.default_rng(5)
    draw = lambda r, c: rng.integers(0, 100, (r, c)).astype(np.float64)
    if name == 'edges':                    # columns 1, 63, 64, 65, 129 against rows 1, 5, 64, 65, both orientations: one mixed batch
        return [draw(*s) for r in (1, 5, 64, 65) for c in (1, 63, 64, 65, 129) for s in ((r, c), (c, r))]
    if name == 'switch':                   # one shape on each side of the LDS / global switch, and a tall one that reads global by index
        n = switch_side()
        return [draw(n, n), draw(n + 1, n + 1), draw(n + 40, n - 20)]
    if name == 'all_equal':
        return [np.ones((7, 7)), np.full((3, 70), 2.0), np.full((70, 3), 2.0)]
    forbidden = draw(66, 66)               # 1e10 entries the optimum avoids: the diagonal and a column stay open
    forbidden[rng.random((66, 66)) < 0.6] = mm.FORBIDDEN
    forbidden[np.arange(66), np.arange(66)] = 50.0
    return [forbidden, np.where(np.eye(5, 9, 2) > 0, 1.0, mm.FORBIDDEN)]


def total(c, col):
    rows = np.flatnonzero(col >= 0)
    assert len(rows) == min(c.shape) and len(set(col[rows].tolist())) == len(rows)
    return c[rows, col[rows]].sum()


@pytest.mark.parametrize('name', ['edges', 'switch', 'all_equal', 'forbidden'])
def test_lap_integer_costs_equal_the_rule_and_scipys_total(name):
    from k210_yolo_framework_amd import motmetrics_gpu as mg
    costs = integer_costs(name)
    got = mg.lap(costs)
    assert len(got) == len(costs)
    for c, g in zip(costs, got):
        assert np.array_equal(g, mm.lap(c)), c.shape
        assert total(c, g) == c[linear_sum_assignment(c)].sum(), c.shape
        assert total(c, g) < mm.FORBIDDEN


def test_lap_float_costs_equal_the_rule_and_two_calls_agree():
    from k210_yolo_framework_amd import motmetrics_gpu as mg
    rng = np.random.default_rng(6)
    costs = [-rng.random(s) for s in ((5, 5), (64, 129), (129, 64), (65, 65), (150, 150))]
    got, again = mg.lap(costs), mg.lap(costs)
    for c, g, a in zip(costs, got, again):
        assert np.array_equal(g, mm.lap(c)) and np.array_equal(g, a), c.shape
        want = c[linear_sum_assignment(c)].sum()
        assert abs(total(c, g) - want) <= 1e-12 * abs(want), c.shape


def test_lap_refuses_non_finite_costs_by_name():
    from k210_yolo_framework_amd import engine, motmetrics_gpu as mg
    with pytest.raises(engine.YkError, match=r'costs\[1\] has a NaN'):
        mg.lap([np.ones((2, 2)), np.array([[1.0, np.nan]])])


F = 6
ONE = np.array([[f, 7, 10, 10, 20, 30] for f in range(1, 2 * F + 1)], np.float64)
NONE = np.zeros((0, 6))


def many_ids(n_gt, n_res):
    """n_gt objects in every one of 3 frames on a grid, n_res results: the objects jittered, the surplus beside the grid."""
    rng = np.random.default_rng(n_gt * 1000 + n_res)
    gt = np.array([[f, k, 40 * (k % 10), 40 * (k // 10), 30, 30] for f in (1, 2, 3) for k in range(n_gt)], np.float64)
    res = np.array([[f, 500 + (k + f) % n_res, 40 * (k % 10), 40 * (k // 10) + (2000 if k >= n_gt else 0), 30, 30]
                    for f in (1, 2, 3) for k in range(n_res)], np.float64)
    res[:, 2:6] += rng.uniform(-4, 4, (len(res), 4))
    return gt, res


def switch_case():
    res = ONE.copy()
    res[F:, 1] = 9
    return [('switch', ONE, res)]


CASES = {
    'one_object_three_frames': lambda: [('a', ONE[:3], ONE[:3] + [0, 0, 1, -1, 0.5, 0])],
    'frames_without_one_side': lambda: [('a', ONE[[0, 1, 3, 4]], (ONE + [0, 0, 1, 1, 0, 0])[[0, 2, 3, 5]])],
    'empty_between_full': lambda: (lambda s: [s[0], ('empty', NONE, NONE), s[1]])(mm.synthetic_sequences(2, 24, 5, seed=2)),
    'ids_63_65': lambda: [('wide', *many_ids(63, 65)), ('tall', *many_ids(65, 63))],
    'three_sequences': lambda: mm.synthetic_sequences(3, 30, 6, seed=1),
    'id_switch': switch_case,
    'no_results_no_truth': lambda: [('no_results', ONE, NONE), ('no_truth', NONE, ONE)],
}


def device(seqs):
    from k210_yolo_framework_amd import motmetrics_gpu as mg
    ev = mg.MotEvaluator()
    for s in seqs:
        ev.add_sequence(*s)
    return ev


def same_scores(got, want):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        if isinstance(w, (int, np.integer)) or (isinstance(w, np.ndarray) and w.dtype.kind == 'i'):
            assert np.array_equal(got[k], w), k
        else:
            assert np.allclose(got[k], w, rtol=1e-12, atol=1e-12), k


@pytest.mark.parametrize('name', sorted(CASES))
def test_evaluator_equals_the_rule(name):
    seqs = CASES[name]()
    ev = device(seqs)
    got, again, want = ev.result(), ev.result(), mm.evaluate(seqs)
    for n in want['sequences']:
        same_scores(got['sequences'][n], want['sequences'][n])
    same_scores(got['combined'], want['combined'])
    for a, b in zip(list(got['sequences'].values()) + [got['combined']], list(again['sequences'].values()) + [again['combined']]):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)          # two calls: the same bytes
    if name == 'three_sequences':                                                                # ... and the three in three calls
        for s in seqs:
            same_scores(device([s]).result()['sequences'][s[0]], want['sequences'][s[0]])
    if name == 'id_switch':
        m = got['combined']
        assert (m['IDSW'], m['Frag'], m['MT'], m['IDTP'], m['IDFN'], m['IDFP'], m['IDF1']) == (1, 0, 1, F, F, F, 0.5)
        assert m['MOTA'] == 1 - 1 / (2 * F) and (m['DetA_alpha'] == 1).all() and (m['AssA_alpha'] == 0.5).all()


def test_trackeval_prints_the_same_lines_on_cpu_and_gpu(capsys):
    import keras_trackeval
    args = ['--synthetic', '4', '--seq_frames', '30', '--seq_objects', '6']
    keras_trackeval.main(args + ['--device', 'cpu'])
    cpu = capsys.readouterr().out
    keras_trackeval.main(args + ['--device', 'gpu'])
    assert capsys.readouterr().out == cpu and cpu.count('\n') == 5

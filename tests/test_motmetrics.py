"""motmetrics.py on the CPU: lap against scipy on exact costs, the three scores on known answers, their independence of the solver, the
refusals of the module and of yk_lap_f64's host side (nothing is launched by a refused call, so no device is needed)."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from k210_yolo_framework_amd import motmetrics as mm

F = 6
ONE = np.array([[f, 7, 10, 10, 20, 30] for f in range(1, 2 * F + 1)], np.float64)      # one object over 2F frames
NONE = np.zeros((0, 6))


def scipy_solver(c):
    out = np.full(c.shape[0], -1, np.int64)
    rows, cols = linear_sum_assignment(c)
    out[rows] = cols
    return out


@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (7, 7), (20, 33), (33, 20)])
def test_lap_total_equals_scipys_on_integer_costs(shape):
    c = np.random.default_rng(shape[0] * 100 + shape[1]).integers(0, 100, shape).astype(np.float64)
    col = mm.lap(c)
    rows = np.flatnonzero(col >= 0)
    assert len(rows) == min(shape) and len(set(col[rows].tolist())) == len(rows) and col.shape == (shape[0],)
    assert c[rows, col[rows]].sum() == c[linear_sum_assignment(c)].sum()


def test_lap_tie_order_and_forbidden_entries():
    assert mm.lap(np.full((6, 6), 3.0)).tolist() == list(range(6))
    c = np.full((4, 4), mm.FORBIDDEN)
    c[np.arange(4), [2, 0, 3, 1]] = [5, 1, 7, 2]
    c[0, 0] = 0                                        # tempting, but it would force a forbidden pair elsewhere
    assert mm.lap(c).tolist() == [2, 0, 3, 1]


def test_known_answers_with_identical_boxes():
    m = mm.evaluate([('perfect', ONE, ONE)])['combined']
    assert (m['HOTA'], m['MOTA'], m['IDF1'], m['IDSW']) == (1.0, 1.0, 1.0, 0)
    res = ONE.copy()
    res[F:, 1] = 9                                     # the result id changes at frame F + 1
    m = mm.evaluate([('switch', ONE, res)])['combined']
    assert (m['IDSW'], m['Frag'], m['MT'], m['IDTP'], m['IDFN'], m['IDFP'], m['IDF1']) == (1, 0, 1, F, F, F, 0.5)
    assert m['MOTA'] == 1 - 1 / (2 * F)
    assert np.array_equal(m['DetA_alpha'], np.ones(19)) and np.array_equal(m['AssA_alpha'], np.full(19, 0.5))
    assert m['HOTA'] == pytest.approx(np.sqrt(0.5), abs=1e-15)
    m = mm.evaluate([('no_results', ONE, NONE)])['combined']
    assert (m['CLR_FN'], m['MOTA'], m['IDFN']) == (2 * F, 0.0, 2 * F) and (m['HOTA_FN'] == 2 * F).all()
    m = mm.evaluate([('no_truth', NONE, ONE)])['combined']
    assert (m['CLR_FP'], m['CLR_TP'], m['IDFP']) == (2 * F, 0, 2 * F) and (m['HOTA_FP'] == 2 * F).all()


def test_counts_do_not_depend_on_the_solver():
    """Jittered boxes leave no ties, so any optimal solver gives the same integers (seed chosen on the CPU and kept)."""
    seqs = mm.synthetic_sequences(3, 30, 6, seed=1)
    ours, theirs = mm.evaluate(seqs), mm.evaluate(seqs, solver=scipy_solver)
    for a, b in zip(list(ours['sequences'].values()) + [ours['combined']], list(theirs['sequences'].values()) + [theirs['combined']]):
        for k in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP', 'MC'):
            assert np.array_equal(a[k], b[k]), k
        assert [a[k] for k in mm.INT_FIELDS] == [b[k] for k in mm.INT_FIELDS]
    c = ours['combined']
    assert c['IDSW'] > 0 and c['CLR_FP'] > 0 and c['CLR_FN'] > 0 and 0 < c['HOTA'] < 1       # the perturbations bite


def test_several_sequences_add_up():
    seqs = mm.synthetic_sequences(2, 20, 4, seed=3) + [('empty', NONE, NONE)]
    both = mm.evaluate(seqs)
    assert both['combined']['CLR_TP'] == sum(m['CLR_TP'] for m in both['sequences'].values())
    assert both['sequences']['empty']['Frames'] == 0 and both['sequences']['empty']['LocA'] == 1.0
    alone = mm.evaluate(seqs[:1])
    assert alone['combined']['HOTA'] == alone['sequences'][seqs[0][0]]['HOTA']


@pytest.mark.parametrize('gt, res, match', [
    (np.vstack([ONE, ONE[:1]]), ONE, 'ground-truth id appears twice in frame 1'),
    (ONE, np.where(np.arange(6) == 3, np.nan, ONE), 'result row 0 has a non-finite number'),
    (ONE, np.where(np.arange(6) == 4, 0.0, ONE), 'result row 0 has a side that is not positive'),
    (np.where(np.arange(6) == 0, 0.0, ONE), ONE, 'frames are whole numbers from 1'),
])
def test_tables_are_refused_by_name(gt, res, match):
    with pytest.raises(ValueError, match=match):
        mm.evaluate([('bad', gt, res)])


def test_lap_and_loader_refusals(tmp_path):
    with pytest.raises(ValueError, match='NaN or an infinity'):
        mm.lap([[1.0, np.inf]])
    with pytest.raises(ValueError, match='expected \\[rows >= 1'):
        mm.lap(np.zeros((0, 3)))
    with pytest.raises(ValueError, match='appears twice'):
        mm.evaluate([('a', ONE, ONE), ('a', ONE, ONE)])
    p = tmp_path / 'gt.txt'
    p.write_text('1,1,10,10,20,30,1,1,1\n1,2,50,50,20,30,0,1,1\n2,1,11,10,20,30,1,1,1\n')
    assert mm.load_mot_text(p, ground_truth=True)[:, 1].tolist() == [1, 1] and len(mm.load_mot_text(p)) == 3
    p.write_text('1,1,10,10\n')
    with pytest.raises(ValueError, match='4 columns'):
        mm.load_mot_text(p)


def test_trackeval_command_line(tmp_path, capsys):
    import keras_trackeval
    seqs = mm.synthetic_sequences(2, 12, 3, seed=4)
    for name, gt, res in seqs:
        for side, t in (('gt', np.c_[gt, np.ones(len(gt))]), ('res', res)):
            (tmp_path / side).mkdir(exist_ok=True)
            np.savetxt(tmp_path / side / f'{name}.txt', t, delimiter=',', fmt='%.17g')
    got = keras_trackeval.main(['--gt', str(tmp_path / 'gt'), '--res', str(tmp_path / 'res'), '--device', 'cpu'])
    want = mm.evaluate(seqs)
    assert capsys.readouterr().out.splitlines()[:3] == [mm.line(n, m) for n, m in want['sequences'].items()] + [mm.line('COMBINED', want['combined'])]
    assert got['combined']['HOTA'] == want['combined']['HOTA'] and (tmp_path / 'trackeval.json').exists()
    (tmp_path / 'res' / f'{seqs[0][0]}.txt').unlink()
    with pytest.raises(ValueError, match=f"sequence '{seqs[0][0]}' is in .*gt only"):
        keras_trackeval.main(['--gt', str(tmp_path / 'gt'), '--res', str(tmp_path / 'res'), '--device', 'cpu'])


@pytest.mark.parametrize('table, n_cost, n_out, match', [
    ([(0, 3, 0, 0)], 9, 3, r'h_table\[0\].rows 0'),
    ([(3, -1, 0, 0)], 9, 3, r'h_table\[0\].cols -1'),
    ([(2049, 2049, 0, 0)], 2049 * 2049, 2049, 'smaller side is above YK_LAP_MAX 2048'),
    ([(1, 4097, 0, 0)], 4097, 1, 'larger side is above YK_LAP_MAX_LONG 4096'),
    ([(3, 3, 0, 0), (3, 3, 1, 3)], 9, 6, r'h_table\[1\].cost_offset 1'),
    ([(3, 3, 0, 1)], 9, 3, r'h_table\[0\].out_offset 1'),
    ([(3, 3, 0, 0), (2, 2, 0, 2)], 9, 6, r'outputs overlap at d_out\[2\]'),
    ([], 9, 3, 'n_problems 0'),
])
def test_yk_lap_f64_refuses_by_name_with_nothing_launched(table, n_cost, n_out, match):
    from k210_yolo_framework_amd import engine, motmetrics_gpu as mg
    t = (mg.LapProblem * max(1, len(table)))(*[mg.LapProblem(*row) for row in table])
    cost, out = np.zeros(16), np.zeros(16, np.int32)     # (real memory, though a refused call follows neither pointer)
    with pytest.raises(engine.YkError, match=match):
        engine.call('yk_lap_f64', cost, n_cost, t, len(table), out, n_out, None)


def test_lap_limits_and_the_lds_switch():
    from k210_yolo_framework_amd import engine, motmetrics_gpu as mg
    k = mg.limits()
    assert k['MAX'] >= 2048 and k['LDS_BYTES'] == 160 * 1024
    assert mg.lds_resident(64, 64) and not mg.lds_resident(2048, 2048)
    with pytest.raises(engine.YkError, match='which 5'):
        engine.call('yk_lap_limit', 5)


@pytest.mark.parametrize('field, value, match', [
    ('max_seq_gt_cells', (1 << 22) + 1, r"19 x G x T integers exceed"),
    ('max_seq_ids', 2049, r'\(G \+ T\)\^2 doubles exceed 2048'),
    ('max_seq_res_ids', 2049, 'ids per side exceed 2048'),
    ('max_frame_gt', 4097, "a frame's assignment exceeds"),
    ('n_seq', 0, 'n_seq 0'),
])
def test_yk_mot_sizes_above_the_limits_are_refused_by_name(field, value, match):
    from k210_yolo_framework_amd import engine, motmetrics_gpu as mg
    sh = mg.MotShape(n_seq=1, n_frames=1, n_gt_ids=1, n_res_ids=1, max_seq_gt_ids=1, max_seq_res_ids=1, max_seq_ids=2, max_frame_gt=1,
                     max_frame_res=1, n_gt_rows=1, n_res_rows=1, s_cells=1, gt_cells=1, id_cells=4, max_seq_gt_cells=1)
    setattr(sh, field, value)
    nbytes = C.c_size_t(0)
    with pytest.raises(engine.YkError, match=match):
        engine.call('yk_mot_workspace_bytes', C.byref(sh), C.byref(nbytes))
    with pytest.raises(engine.YkError, match=match):     # the same check stands in front of every launch of yk_mot_eval
        engine.call('yk_mot_eval', C.byref(sh), *[None] * 15, 0, None, None, None)

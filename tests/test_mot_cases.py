"""tests/mot_cases.py checked on its own, on the CPU: every case reaches what it claims (so tests/test_gpu_mot_edges.py cannot lose a path
without this file noticing), the hand-worked answers of the crafted cases hold for the rule, and the rule has the symmetries that the
device is then held to as well: role swap, relabel and reorder, perfect result."""
import numpy as np
import pytest

from k210_yolo_framework_amd import motmetrics as mm
from tests import mot_cases as mc


def prepared(name):
    return [mm.prepare(n, gt, res) for n, gt, res in mc.case(name)]


def frame_shapes(seq):
    return np.array([(len(g), len(t)) for g, t, _ in seq['frames']]).reshape(-1, 2)


def recording(costs):
    def solver(c):
        costs.append(np.array(c))
        return mm.lap(c)
    return solver


@pytest.mark.parametrize('name', sorted(mc.BUILDERS))
def test_tables_are_accepted_and_small(name):
    seqs = mc.case(name)
    assert len({n for n, _, _ in seqs}) == len(seqs)
    for _, gt, res in seqs:
        assert gt.shape[1] == res.shape[1] == 6 and gt.dtype == res.dtype == np.float64
    assert sorted(mc.rule(name)['sequences']) == sorted(n for n, _, _ in seqs)


@pytest.mark.parametrize('name, frames', [('long_65', 65), ('long_129', 129), ('sparse_ids_unsorted', 65)])
def test_long_cases_pass_one_and_two_strides_of_frames(name, frames):
    seqs = prepared(name)
    assert len(seqs) == 2
    for seq in seqs:
        assert seq['n_frames'] >= frames and 64 * ((frames - 1) // 64) < seq['n_frames']
        shapes = frame_shapes(seq)
        assert (shapes.min(1) > 0).sum() >= frames - 10                  # nearly every frame is a matching, not an early return
    c = mc.rule(name)['combined']
    assert c['IDSW'] > 0 and c['Frag'] > 0 and c['CLR_FN'] > 0 and c['CLR_FP'] > 0 and 0 < c['HOTA'] < 1


def test_sparse_ids_are_large_and_rows_unsorted():
    for (_, gt, res), (_, gt0, res0) in zip(mc.case('sparse_ids_unsorted'), mc.case('long_65')):
        assert res[:, 1].max() > 2.0 ** 50 and res[:, 1].max() < 2.0 ** 53 and (res[:, 1] == np.floor(res[:, 1])).all()
        assert np.unique(res[:, 1]).size == np.unique(res0[:, 1]).size and np.diff(np.unique(res[:, 1])).min() > 2.0 ** 40
        assert (np.diff(gt[:, 0]) < 0).any() and (np.diff(res[:, 0]) < 0).any()
        assert sorted(map(tuple, gt)) == sorted(map(tuple, gt0))


def test_wide_has_three_strides_of_rows_on_each_side_in_both_orientations():
    wide, tall = prepared('wide_129_133')
    for seq, (g, t) in ((wide, (129, 133)), (tall, (133, 129))):
        assert (frame_shapes(seq) == (g, t)).all() and min(g, t) >= 129 and len(seq['frames']) == 3
        assert (seq['G'], seq['T']) == (g, t) and seq['G'] + seq['T'] == 262


def test_mixed_orientation_takes_its_two_maxima_from_different_frames():
    mixed, small = prepared('mixed_orientation')
    shapes, other = frame_shapes(mixed), frame_shapes(small)
    assert [tuple(s) for s in shapes] == list(mc.MIXED_FRAMES)
    both = np.concatenate([shapes, other])                               # the batch, as _pack sees it
    assert both[:, 0].argmax() != both[:, 1].argmax()
    bound = min(both[:, 0].max(), both[:, 1].max())
    assert bound == 70 and (both.min(1) < bound).all() and other.max() < 10
    assert (shapes[:, 0] > shapes[:, 1]).any() and (shapes[:, 0] < shapes[:, 1]).any()
    assert any(g == 0 < t for g, t in shapes) and any(t == 0 < g for g, t in shapes)
    m = mc.rule('mixed_orientation')['sequences']['mixed']
    assert m['CLR_TP'] == m['HOTA_TP'][0] == 4 * 3                        # the jitter leaves every pair that a frame's 3 rows allow matched


def without_bonus(c):
    """clear()'s cost with the 1000 taken out again (a pair with the bonus is at most -1000.5, every other at least -1)"""
    return mm.lap(np.where(c <= -1000.0, c + 1000.0, c))


def test_clear_contest_known_answers_and_the_bonus_decides():
    want = mc.rule('clear_contest')['sequences']
    plain = {}
    for seq in prepared('clear_contest'):
        m = want[seq['name']]
        assert (m['CLR_TP'], m['CLR_FN'], m['CLR_FP'], m['IDSW'], m['Frag']) == mc.CONTEST[seq['name']][1], seq['name']
        plain[seq['name']] = mm.clear(seq, solver=without_bonus)
    # by hand, without the bonus: (a) 20 takes frame 2 and 10 takes frame 3 back; (e) 20 takes frame 3
    assert (plain['bonus_keeps']['IDSW'], want['bonus_keeps']['IDSW']) == (2, 0)
    assert (plain['empty_frame_inside']['IDSW'], want['empty_frame_inside']['IDSW']) == (1, 0)
    for name in ('gap_same_id', 'a_b_a', 'three_fragments'):             # no rival there: the bonus changes nothing
        assert (plain[name]['IDSW'], plain[name]['Frag']) == (want[name]['IDSW'], want[name]['Frag'])
    assert [want[n]['Frag'] for n in ('gap_same_id', 'three_fragments')] == [1, 2]
    assert [want[n]['IDSW'] for n in ('a_b_a', 'three_fragments')] == [2, 1]


def test_thresholds_sit_exactly_on_every_comparison():
    seq, = prepared('thresholds')
    S = np.concatenate([s.ravel() for _, _, s in seq['frames']])
    for v in (0.5, 0.25, 0.75):
        assert (S == v).any() and ((S < v) & (S > v - 1e-6)).any(), v
        assert v - mm.EPS in mm.ALPHAS - mm.EPS                          # each is an alpha of HOTA
    m = mc.rule('thresholds')['combined']
    assert (m['MT'], m['PT'], m['ML']) == mc.THRESHOLD_MT_PT_ML and m['CLR_TP'] == mc.THRESHOLD_CLR_TP
    # matched / seen of the four objects: 4, 0, 5 and 1 of 5 frames; 0.8 is not above 0.8 and 0.2 is not below 0.2
    assert 4 / 5 == 0.8 and 1 / 5 == 0.2
    # HOTA: 20 pairs, 5 of them just below their value.  By hand: alpha <= 0.20 counts all 20; 0.25 loses the one just below 0.25;
    # 0.30 .. 0.45 lose object 2; 0.50 also the five just below 0.5; 0.55 .. 0.70 keep object 3; 0.75 loses the one just below; none above
    assert m['HOTA_TP'].tolist() == [20] * 4 + [19] + [15] * 4 + [10] + [5] * 4 + [4] + [0] * 4
    # identity: pm counts S >= 0.5: object 1 four frames, object 3 five, object 4 one
    assert (m['IDTP'], m['IDFN'], m['IDFP']) == (10, 10, 10)


def repeated_minimum(c):
    return any((row == row.min()).sum() > 1 for row in np.asarray(c))


def test_duplicates_tie_in_the_score_matrices():
    for seq in prepared('duplicates'):
        hota_costs, clear_costs, id_costs = [], [], []
        mm.hota(seq, solver=recording(hota_costs))
        mm.clear(seq, solver=recording(clear_costs))
        mm.identity(seq, solver=recording(id_costs))
        if seq['name'] == 'uneven':                                      # ties between the rows: two objects with the same costs for every result
            assert all(np.array_equal(c[0, :seq['T']], c[1, :seq['T']]) for c in hota_costs + id_costs)
            assert not repeated_minimum(id_costs[0][:seq['G']])
            continue
        assert any(repeated_minimum(c) for c in hota_costs), seq['name']
        assert any(repeated_minimum(c) for c in clear_costs), seq['name']
        assert repeated_minimum(id_costs[0][:seq['G']]), seq['name']
    m = mc.rule('duplicates')['sequences']['copy']
    assert (m['CLR_TP'], m['CLR_FN'], m['CLR_FP'], m['IDSW'], m['IDTP']) == (16, 0, 0, 0, 16) and m['MOTA'] == m['IDF1'] == 1.0


def test_strangers_use_dummy_rows_and_columns():
    for seq in prepared('strangers'):
        G, T = seq['G'], seq['T']
        assert G != T and (G, T) in ((12, 9), (9, 12))
        overlap = np.zeros((G, T), bool)
        for g, t, S in seq['frames']:
            overlap[g[:, None], t[None, :]] |= S > 0
        assert (~overlap.any(1)).sum() * 3 == G and (~overlap.any(0)).sum() * 3 == T
        costs = []
        mm.identity(seq, solver=recording(costs))
        col = mm.lap(costs[0])
        assert (col[:G] >= T).any() and (col[G:] < T).any()               # a ground-truth id on its dummy column, a result id on its dummy row
        assert (col[:G] < T).any()
    both = mc.rule('strangers')['sequences']
    assert both['more_gt']['ML'] >= 4 and both['more_res']['IDFP'] > 0 and both['more_gt']['IDFN'] > 0


# ---- the symmetries, asserted on the rule -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', mc.GENERIC)
def test_rule_role_swap(name):
    want, swapped = mc.rule(name), mm.evaluate(mc.swap_roles(mc.case(name)))
    for w, s in zip(mc.each(want), mc.each(swapped)):
        mc.same_scores(mc.swapped_back(s), w, keys=mc.SWAP_KEYS)


@pytest.mark.parametrize('name', mc.GENERIC)
def test_rule_relabel_and_reorder(name):
    want, moved = mc.rule(name), mm.evaluate(mc.relabel_and_reorder(mc.case(name)))
    for w, s in zip(mc.each(want), mc.each(moved)):
        mc.same_scores(s, w)


@pytest.mark.parametrize('name', mc.GENERIC)
def test_rule_perfect_result(name):
    m = mm.evaluate([(n, gt, gt) for n, gt, _ in mc.case(name)])['combined']
    assert m['HOTA'] == m['DetA'] == m['AssA'] == m['IDF1'] == m['MOTA'] == 1.0
    assert (m['IDSW'], m['Frag'], m['CLR_FN'], m['CLR_FP'], m['ML'], m['PT']) == (0, 0, 0, 0, 0, 0)

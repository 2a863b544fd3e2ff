"""tests/tta_edge_cases.py checked on its own, without a GPU: tta.fuse against every answer worked out by hand, bit for bit, and every claim a
case makes about where it sits (more candidates than nmax and the cut where it says, eight clusters before the truncation, the tie at the cut,
the mirror switch at mw = +-0 and just below).

The rule for a class of more than views * max_out candidates is the kernel's (include/yolo_hip.h: "of a class's candidates only the first
views * max_out in candidate order are then read"); tta.fuse used to walk them all.  It is held here three ways: to the answer by hand on
overfull_hand, to the box-by-box restatement of tests/test_tta.py (which knows nothing of the rule) run on the rows the rule says are read,
and by showing that the rows it ignores would have changed the answer."""
import numpy as np
import pytest

from k210_yolo_framework_amd import softnms, tta
from tests import tta_edge_cases as te
from tests.test_tta import restated

F = np.float32
CASES = te.cases()
BY = {c.name: c for c in CASES}


def _fuse(case):
    return tta.fuse(case.rows, case.xforms, case.class_num, case.max_out, case.thresh)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F).reshape(-1, 6)).view(np.int32)


def _restated(case):
    return restated(case.rows, case.xforms, case.class_num, case.max_out, case.thresh)


@pytest.mark.parametrize('case', [c for c in CASES if c.want is not None], ids=lambda c: c.name)
def test_fuse_gives_the_answer_worked_out_by_hand_bit_for_bit(case):
    rows, _ = _fuse(case)
    assert rows.shape == (len(case.want), 6) and np.array_equal(_bits(rows), _bits(case.want)), (rows.tolist(), case.want)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_fuse_equals_the_restatement_on_the_rows_the_rule_reads(case):
    rows, first = _fuse(te.first_nmax_only(case))
    want, want_first = _restated(te.first_nmax_only(case))
    assert np.array_equal(_bits(rows), _bits(want)) and first.tolist() == want_first.tolist()
    assert np.array_equal(_bits(_fuse(case)[0]), _bits(want))                      # the rows past nmax change nothing
    if case.name not in te.OVERFULL:
        assert all(len(a) == len(b) for a, b in zip(te.first_nmax_only(case).rows, case.rows))   # ... and elsewhere there are none


@pytest.mark.parametrize('name', list(te.OVERFULL))
def test_overfull_classes_hold_what_they_claim_and_the_ignored_rows_would_matter(name):
    case = BY[name]
    c, total = te.OVERFULL[name]
    cap, nmax = case.class_num * case.max_out, len(case.rows) * case.max_out
    per_frame = [int((te.is_candidate(r, case.class_num) & (r[:, 5] == c)).sum()) for r in case.rows]
    assert sum(per_frame) == total > nmax and all(len(r) <= cap for r in case.rows) and max(per_frame) > case.max_out
    read = te.first_nmax_only(case)
    assert sum(int((r[:, 5] == c).sum()) for r in read.rows) == nmax
    # where the cut falls: (frame, row) of the last candidate read and of the first one left out; a row's lane in its ballot is row % 64
    order = [(f, int(i)) for f, r in enumerate(case.rows) for i in np.flatnonzero(te.is_candidate(r, case.class_num) & (r[:, 5] == c))]
    last, out = order[nmax - 1], order[nmax]
    assert (last, out) == {'overfull_hand': ((0, 5), (1, 0)), 'overfull_inside': ((1, 1), (1, 2)), 'overfull_ballot': ((0, 39), (0, 40)),
                           'overfull_three': ((0, 65), (1, 0))}[name]
    if name == 'overfull_inside':
        assert per_frame == [4, 6]                                                # the ballot that is cut starts at n = 4
    if name == 'overfull_ballot':
        assert 0 < out[1] < 64 < len(case.rows[0]) == 80                          # inside the first ballot, a whole second one behind it
    if name == 'overfull_three':
        assert last[1] // 64 == 1 and last[1] % 64 == 1 and per_frame == [66] * 3   # two lanes past a 64-lane boundary, two whole frames dropped
    got = _fuse(case)[0]
    assert not np.array_equal(_bits(got), _bits(_restated(case)[0]))              # walking all candidates gives another answer
    # the other classes are what they are without the overfull class
    alone = _fuse(te.without_class(case, c))[0]
    assert np.array_equal(_bits(got[got[:, 5] != c]), _bits(alone))
    assert 0 < (got[:, 5] == c).sum() <= case.max_out


def test_skipped_rows_are_all_there_and_each_would_have_joined():
    case = BY['skipped']
    rows = np.concatenate(case.rows)
    bad = rows[~te.is_candidate(rows, case.class_num)]
    score_ok = bad[:, 4] > 0
    assert sorted(np.signbit(s) for s in bad[bad[:, 4] == 0, 4]) == [False, True]           # 0.0 and -0.0
    assert (bad[:, 4] == F(-0.5)).sum() == 1 and np.isnan(bad[:, 4]).sum() == 1
    assert sorted(bad[score_ok & ~np.isnan(bad[:, 5]), 5].tolist()) == [-1.0, 2.5, 3.0] and np.isnan(bad[score_ok, 5]).sum() == 1
    assert len(bad) == 8 and all(0 < len(r) <= case.class_num * case.max_out for r in case.rows)
    good = rows[te.is_candidate(rows, case.class_num)]
    assert all((good[:, :4] == b[:4]).all(1).any() for b in bad)                           # each sits on a good row's box
    assert np.signbit(good[:, 5]).sum() == 1                                               # the row of class -0.0 is a candidate of class 0
    # between good rows, inside the counts
    for r in case.rows:
        ok = te.is_candidate(r, case.class_num)
        assert ok[-1] and not ok[:-1].all()
    clean = case._replace(rows=[r[te.is_candidate(r, case.class_num)] for r in case.rows])
    assert np.array_equal(_bits(_fuse(case)[0]), _bits(_fuse(clean)[0]))


def _iou_matrix(boxes):
    return np.stack([softnms.iou_to_all(boxes, m, F)[0] for m in range(len(boxes))])


def test_cut_forms_eight_clusters_and_the_tie_at_the_cut_goes_to_the_older_one():
    case = BY['cut']
    boxes = np.concatenate([tta.map_back(r, x) for r, x in zip(case.rows, case.xforms)])[:, :4]
    o = _iou_matrix(boxes)
    assert len(boxes) == 8 and not o[~np.eye(8, dtype=bool)].any()                          # pairwise disjoint: nk = 8 by construction
    rows, first = _fuse(case._replace(max_out=8))
    assert len(rows) == 8 > case.max_out
    walk = sorted(range(8), key=lambda i: (-float(np.concatenate(case.rows)[i, 4]), i))      # cluster k is opened by candidate walk[k]
    final = {i: s for i, s in zip(first.tolist(), rows[:, 4])}
    assert len({final[walk[k]].tobytes() for k in (3, 4, 5)}) == 1                          # clusters 3, 4, 5: bit-equal final scores
    assert final[walk[2]] > final[walk[3]] > final[walk[6]]
    kept, kept_first = _fuse(case)
    assert kept_first.tolist() == te.CUT_FIRST == walk[:4] and kept_first[3] == min(walk[3:6])
    one = BY['cut_one']
    rows, first = _fuse(one._replace(max_out=2))
    assert len(rows) == 2 and rows[0, 4].tobytes() == rows[1, 4].tobytes() and not _iou_matrix(rows[:, :4])[0, 1]
    assert _fuse(one)[1].tolist() == [0]


def test_mirror_switches_at_plus_and_minus_zero_and_not_just_below():
    xf = np.asarray(te.MIRROR_XFORMS, F)
    assert xf[:, 2].view(np.uint32).tolist() == [0x00000000, 0x80000000, 0x80000001]
    assert (xf[:2, 2] >= 0).all() and not xf[2, 2] >= 0 and xf[2, 2] < 0
    for f in range(3):
        got = tta.map_back(np.asarray(te.MIRROR_ROWS, F), xf[f])[:, :4]
        assert np.array_equal(got.view(np.int32), np.asarray(te.MIRROR_MAPPED[f], F).view(np.int32)), f
    assert np.signbit(np.asarray(te.MIRROR_MAPPED[1], F)[1, 1]) and not np.signbit(np.asarray(te.MIRROR_MAPPED[0], F)[1, 1])
    for name in ('mirror_fused', 'mirror_verbatim'):
        assert all(np.array_equal(r, np.asarray(te.MIRROR_ROWS, F)) for r in BY[name].rows) and BY[name].xforms.view(np.uint32).tolist() == xf.view(np.uint32).tolist()
    assert np.signbit(_fuse(BY['mirror_verbatim'])[0][:, 1]).tolist() == [False, False, True, False, True, True]
    # the switch decides the answer: frame 2 mirrored as well, all three frames would agree on two boxes
    allm = BY['mirror_fused']._replace(xforms=np.asarray([te.MIRROR_XFORMS[0]] * 3, F))
    assert len(_fuse(allm)[0]) == 2 < len(_fuse(BY['mirror_fused'])[0]) == 4


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_neighbours_are_decode_shaped_pictures_of_the_same_call(case):
    for nb in te.neighbours(case):
        assert (len(nb.rows), nb.class_num, nb.max_out, nb.thresh) == (len(case.rows), case.class_num, case.max_out, case.thresh)
        assert all(int((r[:, 5] == c).sum()) <= nb.max_out for r in nb.rows for c in range(nb.class_num))
        assert len(_fuse(nb)[0]) > 0
        assert all(len(a) == len(b) for a, b in zip(te.first_nmax_only(nb).rows, nb.rows))

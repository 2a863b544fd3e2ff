"""The rule of test-time augmentation (k210_yolo_framework_amd/tta.py) on the CPU: tta.fuse against a second statement of
Weighted Boxes Fusion written here one box at a time, and against answers worked out by hand (tests/tta_cases.py); the views, the command
line and every refusal."""
import argparse

import numpy as np
import pytest

from k210_yolo_framework_amd import tta
from tests import tta_cases

F = np.float32


# ---------------------------------------------------------------------------------------------------- a second statement, box by box
def _iou(a, b):
    """oracle/decode_ref.py::tf_iou's steps on two boxes, float32 scalars."""
    ay0, ax0, ay1, ax1 = min(a[0], a[2]), min(a[1], a[3]), max(a[0], a[2]), max(a[1], a[3])
    by0, bx0, by1, bx1 = min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])
    area_a, area_b = F(F(ay1 - ay0) * F(ax1 - ax0)), F(F(by1 - by0) * F(bx1 - bx0))
    if not (area_a > 0 and area_b > 0):
        return F(0)
    ih, iw = max(F(min(ay1, by1) - max(ay0, by0)), F(0)), max(F(min(ax1, bx1) - max(ax0, bx0)), F(0))
    inter = F(ih * iw)
    return F(inter / F(F(area_a + area_b) - inter))


def restated(rows_per_view, xforms, class_num, max_out, thresh):
    n_views = len(rows_per_view)
    cand = []
    for rows, (dy, dx, mw) in zip(rows_per_view, np.asarray(xforms, F).reshape(-1, 3)):
        for top, left, bottom, right, score, cls in np.asarray(rows, F).reshape(-1, 6):
            if mw >= 0:
                left, right = F(mw - right), F(mw - left)
            cand.append((F(top + dy), F(left + dx), F(bottom + dy), F(right + dx), score, cls))
    out, firsts = [], []
    for c in range(class_num):
        mine = [i for i, r in enumerate(cand) if r[5] == F(c) and r[4] > 0]
        mine.sort(key=lambda i: (-float(cand[i][4]), i))
        clusters = []
        for i in mine:
            box, s = cand[i][:4], cand[i][4]
            best, best_iou = None, None
            for k, cl in enumerate(clusters):
                o = _iou(box, cl['box'])
                if best is None or o > best_iou:
                    best, best_iou = k, o
            if best is not None and best_iou > F(thresh):
                cl = clusters[best]
            else:
                cl = dict(sw=F(0), sums=[F(0)] * 4, ss=F(0), cnt=0, first=i, box=None)
                clusters.append(cl)
            cl['sw'] = F(cl['sw'] + s)
            cl['sums'] = [F(acc + F(s * x)) for acc, x in zip(cl['sums'], box)]
            cl['ss'] = F(cl['ss'] + s)
            cl['cnt'] += 1
            cl['box'] = box if cl['cnt'] == 1 else tuple(F(acc / cl['sw']) for acc in cl['sums'])
        for cl in clusters:
            cl['score'] = F(F(F(cl['ss'] / F(cl['cnt'])) * F(min(cl['cnt'], n_views))) / F(n_views))
        order = sorted(range(len(clusters)), key=lambda k: (-float(clusters[k]['score']), k))[:max_out]
        out += [[*clusters[k]['box'], clusters[k]['score'], F(c)] for k in order]
        firsts += [clusters[k]['first'] for k in order]
    return np.asarray(out, F).reshape(-1, 6), np.asarray(firsts, np.int64)


def _fuse(case):
    return tta.fuse(case.rows, case.xforms, case.class_num, case.max_out, case.thresh)


HAND = tta_cases.hand_cases()
RANDOM = [tta_cases.random_case(1, 1, 40, 2, 30), tta_cases.random_case(2, 2, 25, 3, 30), tta_cases.random_case(3, 3, 12, 5, 6, thresh=0.3),
          tta_cases.random_case(4, 8, 6, 4, 4, thresh=0.7), tta_cases.random_case(5, 3, 3, 80, 5), tta_cases.one_class_counts(65, 2)]


@pytest.mark.parametrize('case', HAND + RANDOM, ids=[c.name for c in HAND + RANDOM])
def test_fuse_equals_the_box_by_box_restatement(case):
    rows, first = _fuse(case)
    want, want_first = restated(case.rows, case.xforms, case.class_num, case.max_out, case.thresh)
    assert rows.dtype == F and rows.shape == want.shape
    assert np.array_equal(rows.view(np.int32), want.view(np.int32))
    assert first.tolist() == want_first.tolist()
    if case.want is None:                                                # a seeded case must exercise the rule, not only pass rows through
        n_in = sum(len(r) for r in case.rows)
        assert 0 < len(rows) < n_in or len(case.rows) == 1


@pytest.mark.parametrize('case', HAND, ids=[c.name for c in HAND])
def test_fuse_gives_the_answer_worked_out_by_hand(case):
    rows, _ = _fuse(case)
    assert rows.tolist() == np.asarray(case.want, F).reshape(-1, 6).tolist(), case.name


def test_hand_cases_sit_where_they_claim():
    by = {c.name: c for c in HAND}
    one = by['one_view_verbatim']
    assert _fuse(one)[1].tolist() == list(range(len(one.want)))            # every row a cluster of its own, in row order
    assert float(_iou(tta_cases.A[:4], tta_cases.HALF[:4])) == 0.5         # exactly the threshold of iou_equal_to_thresh
    eq = by['equal_iou_earlier_cluster'].rows[0]
    assert _iou(eq[2, :4], eq[0, :4]) == _iou(eq[2, :4], eq[1, :4]) > F(0.25)
    assert _fuse(by['equal_scores_lower_index_first'])[1].tolist() == [0, 1]
    assert _fuse(by['two_rows_of_one_view'])[1].tolist() == [0]
    cut = by['cut_by_final_score']
    assert len(_fuse(cut._replace(max_out=30))[0]) == 4 > cut.max_out


def test_mirror_and_translate_are_exact_on_integers_and_round_trip():
    rng = np.random.default_rng(0)
    t, l = rng.integers(0, 1000, 50), rng.integers(0, 1000, 50)
    rows = np.stack([t, l, t + rng.integers(1, 500, 50), l + rng.integers(1, 500, 50), np.full(50, 0.5), np.zeros(50)], 1).astype(F)
    for oy, ox, cw, mirror in [(0, 0, 2000, False), (7, 13, 2000, False), (0, 0, 2001, True), (120, 3, 1777, True)]:
        v = np.asarray([[3000, cw, oy, ox, int(mirror)]], np.int32)
        xf = tta.xforms(v)[0]
        assert xf.tolist() == [-oy, -ox, cw if mirror else -1]
        in_canvas = rows.astype(np.float64).copy()                        # the picture's rows as the view's canvas shows them
        in_canvas[:, [0, 2]] += oy
        if mirror:
            in_canvas[:, 1], in_canvas[:, 3] = cw - (rows[:, 3] + ox), cw - (rows[:, 1] + ox)
        else:
            in_canvas[:, [1, 3]] += ox
        back = tta.map_back(in_canvas.astype(F), xf)
        assert np.array_equal(back.view(np.int32), rows.view(np.int32)), (oy, ox, cw, mirror)
    assert np.signbit(tta.xforms(np.asarray([[5, 5, 0, 0, 0]]))[0, :2]).all()            # -0.0: x + -0.0 is x, also for x = -0.0
    assert tta.map_back(np.asarray([[-0.0, -0.0, 1, 1, 0.5, 0]], F), tta.xforms(np.asarray([[5, 5, 0, 0, 0]]))[0]).view(np.int32)[0, 0] == F(-0.0).view(np.int32)


def test_views_follow_the_gain():
    assert tta.views(33, 64, ((1, False),)).tolist() == [[33, 64, 0, 0, 0]]
    assert tta.views(33, 64, 'flip').tolist() == [[33, 64, 0, 0, 0], [33, 64, 0, 0, 1]]
    v = tta.views(33, 64, 'v5')
    assert v.dtype == np.int32 and v.tolist() == [[33, 64, 0, 0, 0], [40, 78, 3, 7, 1], [50, 96, 8, 16, 0]]   # ceil(33 / .83) = 40, ceil(64 / .67) = 96
    assert tta.views(1, 1, ((0.5, True),)).tolist() == [[2, 2, 0, 0, 1]]
    for h, w, g in [(480, 640, 0.83), (7, 5, 0.67), (1000, 3, 0.1)]:
        ch, cw, oy, ox, _ = tta.views(h, w, ((g, False),))[0]
        assert ch >= h and cw >= w and 0 <= oy <= ch - h and 0 <= ox <= cw - w and abs((ch - h) - 2 * oy) <= 1 and abs((cw - w) - 2 * ox) <= 1
    rows = tta.table_rows(v, 96, 33, 64)
    assert rows.dtype == tta.VIEW_DTYPE and tta.VIEW_DTYPE.itemsize == 56
    assert rows['offset'].tolist() == [96] * 3 and rows['h'].tolist() == [33] * 3 and rows['cw'].tolist() == [64, 78, 96] and rows['mirror'].tolist() == [0, 1, 0]
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    c = tta.canvas(img, (4, 5, 1, 2, 1))
    assert c.shape == (4, 5, 3) and np.array_equal(c[1:3, 2:5], img[:, ::-1]) and not c[0].any() and not c[3].any() and not c[:, :2].any()


def test_parse_and_check_accept_the_aliases_and_refuse_by_name():
    assert tta.parse('flip') == ((1.0, False), (1.0, True)) == tta.parse('1,1f')
    assert tta.parse('v5') == ((1.0, False), (0.83, True), (0.67, False)) == tta.parse('1, 0.83F ,0.67')
    assert tta.parse('None') is None and tta.parse('') is None and tta.parse(None) is None and tta.check(None) is None and tta.check('off') is None
    assert tta.check('v5') == tta.parse('v5') and tta.check(((1, False), (0.5, True))) == ((1.0, False), (0.5, True))
    assert tta.text_of(tta.parse('v5')) == '1,0.83f,0.67' and tta.ALIASES == {'flip': '1,1f', 'v5': '1,0.83f,0.67'} and tta.MAX_VIEWS == 8
    for bad, match in [('1,x', 'not a gain'), ('1,,1f', 'not a gain'), ('1.5', 'above 1'), ('0', 'not a positive'), ('-0.5f', 'not a positive'),
                       ('nan', 'not a positive'), ('1,1', 'duplicate view'), ('0.5f,1,0.5f', 'duplicate view'),
                       (','.join(f'{1 - k / 16:g}' for k in range(9)), '9 views'), (((1, 0),), 'mirror is True or False'), ((1, 2, 3), 'pairs'),
                       ((), '0 views')]:
        with pytest.raises(ValueError, match=match):
            tta.check(bad)
    assert len(tta.check(','.join(f'{1 - k / 16:g}' for k in range(8)))) == 8
    for thresh in (float('nan'), -0.1, float('inf'), '0.5'):
        with pytest.raises(ValueError, match='tta_thresh'):
            tta.check('flip', thresh)
    with pytest.raises(ValueError, match='tta with tiles'):
        tta.check('flip', 0.55, 'hard', (2, 2))
    with pytest.raises(ValueError, match="nms 'gaussian' with tta"):
        tta.check('flip', 0.55, 'gaussian')
    with pytest.raises(ValueError, match='2\\^24'):
        tta.views(1 << 23, 10, ((0.5, False),))
    tta.views((1 << 23) - 1, 10, ((0.5, False),))
    with pytest.raises(ValueError, match='at least 1 x 1'):
        tta.views(0, 10, 'flip')
    with pytest.raises(ValueError, match='2 views, 1 transforms'):
        tta.fuse([np.zeros((0, 6)), np.zeros((0, 6))], [tta_cases.NO], 1, 3, 0.5)


def test_command_line_reads_checks_and_hands_on_the_options():
    def args(*argv, nms='hard', tiles=None):
        p = argparse.ArgumentParser()
        tta.add_arguments(p)
        a = p.parse_args(list(argv))
        a.nms, a.tiles = nms, tiles
        tta.parse_arguments(a)
        return a

    a = args()
    assert a.tta is None and a.tta_thresh == 0.55 and tta.run_options(a) == dict(tta=None, tta_thresh=0.55)
    a = args('--tta', 'v5', '--tta_thresh', '0.6')
    assert tta.run_options(a) == dict(tta=((1.0, False), (0.83, True), (0.67, False)), tta_thresh=0.6)
    assert tta.rule_of(a.tta, a.tta_thresh) == dict(tta='1,0.83f,0.67', tta_views=[[1.0, False], [0.83, True], [0.67, False]], tta_thresh=0.6)
    with pytest.raises(ValueError, match='tta with tiles'):
        args('--tta', 'flip', tiles=(2, 2))
    with pytest.raises(ValueError, match="nms 'linear' with tta"):
        args('--tta', 'flip', nms='linear')
    with pytest.raises(ValueError, match="tta '1,2'"):
        args('--tta', '1,2')
    from k210_yolo_framework_amd import detect, evaluate
    assert detect.parse(['', 'data']).tta is None and detect.parse(['', 'data', '--tta', 'flip']).tta == tta.parse('flip')
    assert evaluate.parse(['x.h5', '--tta', 'v5', '--tta_thresh', '0.5']).tta_thresh == 0.5
    for bad in (['--tta', 'flip', '--tiles', '2x2'], ['--tta', 'flip', '--nms', 'diou'], ['--tta', 'v5', '--batch', '2']):
        with pytest.raises(SystemExit):
            detect.parse(['', 'data'] + bad)


def test_makefile_passes_tta_only_when_it_is_set():
    from pathlib import Path
    text = (Path(__file__).resolve().parents[1] / 'Makefile').read_text()
    assert 'TTA           ?=\n' in text and 'TTATHRESH     ?= 0.55\n' in text
    assert 'TTA_ARGS   = $(if $(TTA),--tta $(TTA) --tta_thresh $(TTATHRESH))' in text
    targets = {name: body for name, body in zip(('eval', 'detect'), (text.split('\neval:\n')[1].split('\n\n')[0], text.split('\ndetect:\n')[1].split('\n\n')[0]))}
    assert all('$(TTA_ARGS)' in body for body in targets.values())
    assert '$(TTA_ARGS)' not in text.split('\ninference:\n')[1].split('\n\n')[0] and '$(TTA_ARGS)' not in text.split('\ntrain:\n')[1].split('\n\n')[0]

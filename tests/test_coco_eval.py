"""coco_eval.evaluate, the host statement of the COCO-style metric: hand-worked cases, the points where it parts from the
VOC rule, ignore / area / tie / truncation handling, agreement with the independent voc_eval.evaluate where the two rules must agree, edge
cases, and a check that the shared generator (tests/coco_cases.py) really contains what the GPU test relies on it for."""
import numpy as np
import pytest

from k210_yolo_framework_amd import coco_eval, voc_eval
from tests import coco_cases as cc

EPS = 2.220446049250313e-16
ALL = np.array([[0, 1e10]])


def D(*rows):
    return np.asarray(rows, np.float64).reshape(-1, 6)


def voc_flags(dets, gts, class_num, iou_thresh, difficult=None):
    """voc_eval.evaluate's matching loop, returning one flag per row in insertion order (0 ignored, 1 tp, 2 fp)."""
    dets = [np.asarray(d, np.float64).reshape(-1, 6) for d in dets]
    gts = [np.asarray(g, np.float64).reshape(-1, 6) for g in gts]
    diff = [np.zeros(len(g), bool) if difficult is None else np.asarray(difficult[i], bool) for i, g in enumerate(gts)]
    flags = [np.zeros(len(d), np.uint8) for d in dets]
    for c in range(class_num):
        sel = [g[:, -1].astype(int) == c for g in gts]
        taken = [np.zeros(int(s.sum()), bool) for s in sel]
        rows = [(d[k, 4], i, k) for i, d in enumerate(dets) for k in np.nonzero(d[:, 5].astype(int) == c)[0]]
        for k in sorted(range(len(rows)), key=lambda k: -rows[k][0]):
            _, i, r = rows[k]
            g = gts[i][sel[i], :4]
            best, j = -1.0, -1
            if len(g):
                iou = voc_eval.box_iou(dets[i][r, :4], g)
                j = int(np.argmax(iou))
                best = float(iou[j])
            if best >= iou_thresh:
                if diff[i][sel[i]][j]:
                    continue
                flags[i][r] = 2 if taken[i][j] else 1
                taken[i][j] = True
            else:
                flags[i][r] = 2
    return np.concatenate(flags) if flags else np.zeros(0, np.uint8)


# ---- hand-worked -----------------------------------------------------------------------------------------------------------------------
def test_hand_worked_curve():
    gts = [D([0, 0, 40, 40, 1, 0], [100, 100, 150, 150, 1, 0])]
    dets = [D([0, 0, 40, 40, .9, 0], [200, 200, 240, 240, .8, 0], [100, 100, 150, 150, .7, 0])]
    r = coco_eval.evaluate(dets, gts, 1)
    assert r['flags'].shape == (4, 10, 3)
    assert (r['flags'][0] == [1, 2, 1]).all()                                         # at every threshold
    first = 1.0 / (1.0 + EPS)
    for t in range(10):
        p = r['precision'][t, :, 0, 0]
        assert np.array_equal(p[:51], np.full(51, first)) and np.array_equal(p[51:], np.full(50, 2.0 / (3.0 + EPS)))
        assert r['recall'][t, 0, 0] == 1.0
    assert abs(2.0 / (3.0 + EPS) - 2.0 / 3.0) < 1e-15
    assert abs(r['ap'] - (51 * first + 50 * (2.0 / 3.0)) / 101) <= 1e-12
    assert abs(r['ap50'] - r['ap']) <= 1e-12 and abs(r['ap75'] - r['ap']) <= 1e-12 and abs(r['ap_class'][0] - r['ap']) <= 1e-12
    assert r['ar'] == 1.0 and r['n_det'].tolist() == [3] and r['npig'][0].tolist() == [2, 0, 2, 0]
    assert np.isnan(r['ap_small']) and np.isnan(r['ar_large']) and r['ar_medium'] == 1.0      # 40x40 and 50x50: both medium


def test_where_the_coco_and_the_voc_rule_part():
    # A = [0,0,10,10], B = [0,4.0625,10,14.0625]; detection 1 is A itself; detection 2 = [0,0,10,12.5]: IoU 100/125 with A, 84.375/140.625 with B
    gts = [D([0, 0, 10, 10, 1, 0], [0, 4.0625, 10, 14.0625, 1, 0])]
    dets = [D([0, 0, 10, 10, .9, 0], [0, 0, 10, 12.5, .8, 0])]
    assert voc_eval.box_iou(dets[0][1, :4], gts[0][:, :4]).tolist() == [0.8, 0.6]
    assert np.argmax(voc_eval.box_iou(dets[0][0, :4], gts[0][:, :4])) == 0
    r = coco_eval.evaluate(dets, gts, 1, [0.5, 0.65], ALL)
    assert r['flags'][0, 0].tolist() == [1, 1]                                        # falls back to the free box B
    v = voc_eval.evaluate(dets, gts, 1, 0.5)
    assert v['tp'][0] == 1 and v['fp'][0] == 1                                        # best box A is taken: false positive
    assert r['flags'][0, 1].tolist() == [1, 2]                                        # at 0.65 B no longer qualifies
    v = voc_eval.evaluate(dets, gts, 1, 0.65)
    assert v['tp'][0] == 1 and v['fp'][0] == 1


def test_ignore_handling():
    # a difficult box: the first detection on it is ignored and uses it up; the second is not matched to it again
    gts = [D([0, 0, 50, 50, 1, 0], [100, 100, 150, 150, 1, 0])]
    dets = [D([0, 0, 50, 50, .9, 0], [0, 0, 50, 50, .8, 0], [100, 100, 150, 150, .7, 0])]
    r = coco_eval.evaluate(dets, gts, 1, [0.5], ALL, difficult=[np.array([True, False])])
    assert r['flags'][0, 0].tolist() == [0, 2, 1] and r['npig'][0, 0] == 1
    # a 20x20 box counts under small, is ignored under medium and large; so is a detection matching it
    gts = [D([0, 0, 20, 20, 1, 0])]
    dets = [D([0, 0, 20, 20, .9, 0], [100, 100, 120, 120, .8, 0])]                    # the second matches nothing, area 20x20
    r = coco_eval.evaluate(dets, gts, 1, [0.5])
    assert r['npig'][0].tolist() == [1, 1, 0, 0]
    assert r['flags'][:, 0, 0].tolist() == [1, 1, 0, 0]
    assert r['flags'][:, 0, 1].tolist() == [2, 2, 0, 0]
    assert r['recall'][0, 0].tolist() == [1.0, 1.0, -1.0, -1.0] and np.isnan(r['ap_medium']) and r['ap_small'] == r['ap']
    # a non-ignored box is preferred to an ignored one with the higher IoU
    gts = [D([0, 0, 10, 10, 1, 0], [0, 1, 10, 11, 1, 0])]
    r = coco_eval.evaluate([D([0, 0, 10, 10, .9, 0])], gts, 1, [0.5], ALL, difficult=[np.array([True, False])])
    assert r['flags'][0, 0].tolist() == [1]


def test_tie_takes_the_higher_index_and_max_dets_truncates():
    gts = [D([0, 0, 2, 1, 1, 0], [0, 1, 2, 2, 1, 0])]                                 # both IoU 0.5 with the detection
    dets = [D([0, 0, 2, 2, .9, 0], [0, 1, 2, 2, .8, 0])]                              # the second is box 1 itself
    r = coco_eval.evaluate(dets, gts, 1, [0.5], ALL)
    assert r['flags'][0, 0].tolist() == [1, 2]                                        # box 1 went to the first detection
    dets = [D([0, 0, 2, 2, .9, 0], [0, 0, 2, 1, .8, 0])]                              # the second is box 0 itself
    assert coco_eval.evaluate(dets, gts, 1, [0.5], ALL)['flags'][0, 0].tolist() == [1, 1]
    gts = [D([0, 0, 10, 10, 1, 0], [20, 20, 30, 30, 1, 0], [40, 40, 50, 50, 1, 0])]
    dets = [D([40, 40, 50, 50, .1, 0], [0, 0, 10, 10, .9, 0], [20, 20, 30, 30, .8, 0])]
    r = coco_eval.evaluate(dets, gts, 1, max_dets=2)
    assert (r['flags'][:, :, 0] == 0).all() and (r['flags'][0, :, 1:] == 1).all() and r['n_det'].tolist() == [2]
    assert coco_eval.evaluate(dets, gts, 1, max_dets=3)['n_det'].tolist() == [3]


# ---- against the independent VOC code ---------------------------------------------------------------------------------------------------
def test_agrees_with_voc_eval_where_the_rules_must_agree():
    rng = np.random.default_rng(11)
    thr = coco_eval.default_iou_thresholds()
    seen = 0
    for n_img, class_num in ((3, 1), (6, 4)):
        dets, gts = [], []
        for _ in range(n_img):
            g = int(rng.integers(0, 7))
            cell = rng.permutation(12)[:g]                                            # disjoint cells of a 3 x 4 grid of 100 x 100
            tl = np.stack([cell // 4 * 100.0, cell % 4 * 100.0], 1) + rng.uniform(0, 20, (g, 2))
            gt = np.concatenate([tl, tl + rng.uniform(30, 75, (g, 2)), np.ones((g, 1)), rng.integers(0, class_num, (g, 1))], 1)
            rows = []
            for _ in range(int(rng.integers(0, 25))):
                if g and rng.random() < 0.8:
                    src = gt[int(rng.integers(0, g))]
                    rows.append([*(src[:4] + rng.normal(0, rng.choice([1.0, 4.0, 9.0]), 4)), rng.choice(cc.SCORES), src[5]])
                else:
                    t = rng.uniform(0, 300, 2)
                    rows.append([*t, *(t + rng.uniform(10, 80, 2)), rng.choice(cc.SCORES), rng.integers(0, class_num)])
            dets.append(np.asarray(rows, np.float32).reshape(-1, 6))
            gts.append(gt)
        for d, g in zip(dets, gts):                                                   # the premise, checked
            for row in d:
                same = g[g[:, 5].astype(int) == int(row[5]), :4]
                assert (voc_eval.box_iou(row[:4], same) >= 0.5).sum() <= 1
        r = coco_eval.evaluate(dets, gts, class_num, thr, ALL, max_dets=1000)
        cls = np.concatenate([d[:, 5].astype(int) for d in dets])
        for t, v in enumerate(thr):
            ref = voc_eval.evaluate(dets, gts, class_num, iou_thresh=float(v))
            assert np.array_equal(r['flags'][0, t], voc_flags(dets, gts, class_num, float(v)))
            for c in range(class_num):
                f = r['flags'][0, t][cls == c]
                assert int((f == 1).sum()) == ref['tp'][c] and int((f == 2).sum()) == ref['fp'][c]
                seen += int((f == 1).sum())
            assert np.array_equal(r['npig'][:, 0], ref['n_gt']) and np.array_equal(r['n_det'], ref['n_det'])
    assert seen > 50


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------
def test_edge_cases():
    empty = np.zeros((0, 6))
    r = coco_eval.evaluate([empty, empty], [D([0, 0, 10, 10, 1, 0]), empty], 2)      # no detections
    assert r['ap'] == 0.0 and r['ar'] == 0.0 and r['flags'].shape == (4, 10, 0) and r['ap_class'][0] == 0.0 and np.isnan(r['ap_class'][1])
    assert (r['precision'][:, :, 0, 0] == 0).all() and (r['precision'][:, :, 1, :] == -1).all() and (r['recall'][:, 0, 0] == 0).all()
    r = coco_eval.evaluate([D([0, 0, 10, 10, .9, 0]), empty], [empty, empty], 2)     # no ground truth
    assert np.isnan(r['ap']) and np.isnan(r['ar']) and np.isnan(r['ap_class']).all() and (r['precision'] == -1).all()
    assert r['flags'][0, 0].tolist() == [2] and r['n_det'].tolist() == [1, 0]
    r = coco_eval.evaluate([], [], 2)
    assert np.isnan(r['ap']) and r['flags'].shape == (4, 10, 0)
    # class 0: ground truth and a detection; class 1: ground truth only (AP 0, recall 0); class 2: detections only (absent)
    dets = [D([0, 0, 40, 40, .9, 0], [0, 0, 5, 5, .7, 2], [0, 0, 5, 5, .6, 7], [0, 0, 5, 5, .6, -3])]
    gts = [D([0, 0, 40, 40, 1, 0], [50, 50, 90, 90, 1, 1], [50, 50, 90, 90, 1, 9])]
    r = coco_eval.evaluate(dets, gts, 3)
    assert abs(r['ap_class'][0] - 1.0 / (1.0 + EPS)) < 1e-15 and r['ap_class'][1] == 0.0 and np.isnan(r['ap_class'][2])
    assert (r['recall'][:, 1, 0] == 0).all() and (r['recall'][:, 2, :] == -1).all() and (r['precision'][:, :, 2, :] == -1).all()
    assert abs(r['ap'] - 0.5) < 1e-15 and r['ar'] == 0.5
    assert (r['flags'][:, :, 2:] == 0).all() and r['n_det'].tolist() == [1, 0, 1]    # a class column outside [0, class_num): nowhere
    assert r['npig'][:, 0].tolist() == [1, 1, 0]
    r = coco_eval.evaluate(dets, gts, 3, [0.6, 0.7], ALL)                             # neither 0.5 nor 0.75 in the list
    assert np.isnan(r['ap50']) and np.isnan(r['ap75']) and np.isnan(r['ap_small'])
    with pytest.raises(ValueError):
        coco_eval.evaluate([empty], [], 1)


def test_default_thresholds_hold_the_two_named_ones():
    thr = coco_eval.default_iou_thresholds()
    assert (thr == 0.5).sum() == 1 and (thr == 0.75).sum() == 1 and len(coco_eval.REC_THRS) == 101


# ---- the shared generator holds what the GPU test relies on -----------------------------------------------------------------------------
def test_generated_cases_contain_every_situation():
    found = dict(rules_part=0, ignored_match=0, area_ignored=0, tie=0, cut=0)
    for name in ('mixed20', 'one_class', 'lanes', 'scan', 'cut'):
        c = cc.case(name)
        r = cc.reference(name)
        dets, gts, diff, K = c['dets'], c['gts'], c['diff'], c['class_num']
        assert r['flags'].shape == (4, 10, sum(len(d) for d in dets))
        t50 = r['flags'][0, 0]                                                        # range all, threshold 0.5
        found['rules_part'] += int((t50 != voc_flags(dets, gts, K, 0.5, diff)).sum()) if name != 'cut' else 0
        first = np.concatenate([[0], np.cumsum([len(d) for d in dets])])
        thr_ok = 0
        for i, (d, g, h) in enumerate(zip(dets, gts, diff)):
            dcls = d[:, 5].astype(int)
            gcls = g[:, -1].astype(int) if len(g) else np.zeros(0, int)
            for k in range(K):
                rows = np.nonzero(dcls == k)[0]
                found['cut'] += max(0, len(rows) - c['max_dets'])
                gsel = np.nonzero(gcls == k)[0]
                for row in rows:
                    iou = voc_eval.box_iou(d[row, :4], g[gsel, :4])
                    ok = iou[iou >= 0.5]
                    if len(ok) != len(np.unique(ok)):
                        found['tie'] += 1
                    f = r['flags'][:, 0, first[i] + row]
                    if f[0] == 2 and (f[1:] == 0).any():                              # unmatched, and outside some range
                        found['area_ignored'] += 1
                    # where max_dets does not bind, flag 0 under `all` for a row of a class is a match to a difficult box, or (a jittered
                    # box turned inside out) a negative area of its own, which is below every range
                    area = (float(d[row, 2]) - float(d[row, 0])) * (float(d[row, 3]) - float(d[row, 1]))
                    if name in ('mixed20', 'one_class', 'scan') and f[0] == 0:
                        assert h[gsel][iou >= 0.5].any() or area < 0
                        thr_ok += int(area >= 0)
        found['ignored_match'] += thr_ok
    print(found)
    assert all(v > 0 for v in found.values()), found
    assert (cc.reference('cut')['n_det'] <= cc.reference('mixed20')['n_det']).all()
    assert cc.reference('cut')['n_det'].sum() < cc.reference('mixed20')['n_det'].sum()
    lanes = cc.case('lanes')
    sizes = sorted({int((g[:, 5] == 0).sum()) for g in lanes['gts']})
    assert sizes == [0, 1, 64, 65, 130]
    assert any(len(d) == 0 for d in lanes['dets']) and any(len(g) == 0 for g in lanes['gts'])
    scan = cc.case('scan')
    cls = np.concatenate([d[:, 5].astype(int) for d in scan['dets']])
    assert [int((cls == k).sum()) for k in range(6)] == [0, 1, 255, 256, 257, 1000]
    assert cc.reference('scan')['n_det'].tolist() == [0, 1, 255, 256, 257, 1000]     # max_dets does not bind there
    scores = np.concatenate([d[:, 4] for d in cc.case('mixed20')['dets']])
    assert np.signbit(scores[scores == 0]).any() and (~np.signbit(scores[scores == 0])).any()

"""The cases of tests/grid_trip_cases.py checked on their own (no GPU): every size is past its cap by a PARTIAL trip under the dispatch the host
functions apply; the caps are the ones the sources state; the planted values are where the second trip reads them; the evaluator cases meet the
conditions that make a skipped group or image change an integer; dropping empty images changes no output of the references; and the tie
cases tie exactly in float64."""
import re
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import coco_eval, oppoint, voc_eval
from tests import grid_trip_cases as gt
from tests import qat_ref

CSRC = Path(__file__).resolve().parents[1] / 'k210_yolo_framework_amd' / 'csrc'
ROOT = CSRC.parents[1]


def partial_trip(items, cap, block):
    """More than one trip, fewer than two, and the last workgroup of the second trip is not full."""
    return cap < items < 2 * cap and (items - cap) % block != 0 and items - cap > block


def test_the_caps_are_the_ones_the_sources_state():
    rng_h, map_hip, qat_hip = (CSRC / 'yk_range.h').read_text(), (CSRC / 'yk_map.hip').read_text(), (CSRC / 'yk_qat.hip').read_text()
    assert int(re.search(r'constexpr int CAL_BLOCK = (\d+);', rng_h).group(1)) == gt.CAL_BLOCK
    assert int(re.search(r'constexpr unsigned CAL_MAX_GRID = (\d+);', rng_h).group(1)) == gt.CAL_MAX_GRID
    assert int(re.search(r'if \(g > (\d+)\) g = \1;', map_hip).group(1)) == gt.MAP_MAX_GRID
    assert int(re.search(r'constexpr int MAP_BLOCK = (\d+);', map_hip).group(1)) == gt.MAP_WAVES * 64 == gt.APPEND_BLOCK
    assert 'constexpr int MAP_WAVES = MAP_BLOCK / YK_WAVE;' in map_hip
    assert f'i < n_slots; i += {gt.UPDATE_BLOCK})' in qat_hip
    assert int(re.search(r'#define YK_QAT_TILE (\d+)', (ROOT / 'include' / 'yolo_hip.h').read_text()).group(1)) == gt.QAT_TILE
    assert gt.CAL_ITEMS == 524288 and gt.MAP_GROUPS == 262144 and gt.CAL_BLOCK < gt.PAST < 2 * gt.CAL_BLOCK


# ---------------------------------------------------------------------------------------------------- 1. QAT activations
@pytest.mark.parametrize('path,shift', [('vector', 0), ('vector', 1), ('vector', 2), ('vector', 3), ('scalar', 0)])
def test_activation_sizes_cross_the_cap_on_the_path_they_name_and_hold_the_edge_values_there(path, shift):
    c = gt.act_case(path, shift)
    n, head, n4, tail, x = c['n'], c['head'], c['n4'], c['tail'], c['x']
    assert head + 4 * n4 + tail == n and (head, n4, tail) == gt.act_split(n, shift, c['shift_q'])
    assert partial_trip(gt.act_items(n, shift, c['shift_q']), gt.CAL_ITEMS, gt.CAL_BLOCK)
    if path == 'vector':
        assert head == (0, 3, 2, 1)[shift] and tail == 3 and n4 == gt.CAL_ITEMS + gt.PAST and head + tail < gt.CAL_BLOCK
        assert gt.act_split(n, shift, shift + 1) == (n, 0, 0)                         # one float off: no 16-byte access at all
    else:
        assert (head, n4, tail) == (n, 0, 0) and n == gt.CAL_ITEMS + gt.PAST
    lo, hi = gt.QAT_RANGE
    s, zp = qat_ref.qparams32(lo, hi)
    assert zp == 64
    sec = x[c['second']]
    u = qat_ref.codes(sec, lo, hi)
    assert len(sec) == (4 if path == 'vector' else 1) * gt.PAST
    assert gt.is_tie(sec).sum() >= 200 and (u < 0).sum() >= 5 and (u > 255).sum() >= 5
    assert (np.signbit(sec) & (sec == 0)).any() and ((sec != 0) & (np.abs(sec) < np.finfo(np.float32).tiny)).any()
    if path == 'vector':
        last = x[n - 3:]
        ul = qat_ref.codes(last, lo, hi)
        assert gt.is_tie(last[:1]).all() and ul[1] > 255 and ul[2] < 0
        assert gt.is_tie(x[:head]).sum() >= min(head, 1) and len(gt.act_pool()[0]) > 4 * 1100     # the pool + the edge values: the last 1200 float4
    # the extremes are one value each, the maximum inside the second trip and the minimum in the last element
    e = qat_ref.extremes(x)
    assert (e[0], e[1]) == (-2e6, 2e6) and (x == e[1]).sum() == 1 and (x == e[0]).sum() == 1
    assert c['second'].start <= int(np.argmax(x)) < c['second'].stop and int(np.argmin(x)) == n - 1
    want = qat_ref.fq(x, lo, hi)
    mask = qat_ref.ste_mask(x, lo, hi)
    assert np.isfinite(want).all() and 0.5 < mask.mean() < 1.0 and not mask[c['second']].all() and mask[c['second']].any()


# ---------------------------------------------------------------------------------------------------- 2. QAT weights
def test_weight_buffer_crosses_the_cap_is_mostly_gap_and_has_segments_on_both_sides_of_the_border():
    c = gt.weights_case()
    total, border = c['total'], c['border']
    assert total % 4 == 3 and partial_trip(total // 4, gt.CAL_ITEMS, gt.CAL_BLOCK)                # the 16-byte copy: a whole allocation has head 0
    assert total > 4 * gt.CAL_ITEMS and border == 4 * gt.CAL_ITEMS
    ends = [o + len(s) for o, s in zip(c['offs'], c['segs'])]
    assert all(e < o for e, o in zip(ends[:-1], c['offs'][1:])) and c['offs'][0] > 0 and ends[-1] == total     # apart, in order, the tail covered
    assert sum(len(s) for s in c['segs']) < 0.05 * total
    assert sum(o < border < e for o, e in zip(c['offs'], ends)) == 1 and sum(o >= border for o in c['offs']) == 5
    assert any(o % 4 for o in c['offs']) and sum(e <= border for e in ends) == 3
    inside = np.zeros(total, bool)
    for o, s in zip(c['offs'], c['segs']):
        assert c['flat'][o:o + len(s)].tobytes() == s.tobytes()
        inside[o:o + len(s)] = True
    gap = c['flat'][~inside]
    z = np.nonzero((c['flat'] == 0) & np.signbit(c['flat']) & ~inside)[0]
    assert (z < gt.CAL_ITEMS).any() and ((z >= gt.CAL_ITEMS) & (z < border)).any() and (z >= border).any() and len(gap) > 0.95 * total
    first = gt.tile_first([len(s) for s in c['segs']])
    assert first[-1] == sum(-(-len(s) // gt.QAT_TILE) for s in c['segs']) and (np.diff(first) >= 1).all()


def test_bad_segments_are_the_three_kinds_and_lie_clear_of_the_good_ones():
    c = gt.bad_segment_case()
    total, offs, sizes = c['total'], c['offs'], c['sizes']
    bad = [i for i in range(len(offs)) if i not in c['good']]
    assert [(offs[i] < 0, offs[i] + sizes[i] > total, sizes[i] == 0) for i in bad] == [(True, False, False), (False, False, True), (False, True, False)]
    first = gt.tile_first(sizes)
    assert [int(first[i + 1] - first[i]) for i in bad] == [2, 0, 1]                               # size 0: no tile, as the Python side counts it
    touched = np.zeros(total, bool)
    for i in bad:
        touched[max(offs[i], 0):min(offs[i] + sizes[i], total)] = True
    for i, sg in c['good'].items():
        assert 0 <= offs[i] and offs[i] + len(sg) <= total and len(sg) == sizes[i] and not touched[offs[i]:offs[i] + len(sg)].any()
    assert touched.sum() == 4997 + 10 and bad[0] > 0 and bad[-1] < len(offs) - 1                  # good segments on both sides of the bad ones


# ---------------------------------------------------------------------------------------------------- 3. QAT range update
def test_update_table_has_every_kind_of_slot_on_both_sides_of_slot_256():
    from k210_yolo_framework_amd.qat import SLOT_NONE, SLOT_OWNER, SLOT_UNION
    c = gt.update_case()
    kind, p0, p1, data = c['kind'], c['p0'], c['p1'], c['data']
    n, B = gt.UPDATE_SLOTS, gt.UPDATE_BLOCK
    assert B < n < 2 * B and len(kind) == n
    for lo, hi in ((0, B), (B, n)):
        own = [i for i in range(lo, hi) if kind[i] == SLOT_OWNER]
        assert sum(i in data for i in own) >= 10 and sum(i not in data for i in own) >= 5
        assert any(kind[i] == SLOT_NONE and i in data for i in range(lo, hi)) and any(kind[i] == SLOT_UNION for i in range(lo, hi))
    unions = {i: (int(p0[i]), int(p1[i])) for i in range(n) if kind[i] == SLOT_UNION}
    assert unions == gt.UPDATE_UNIONS and all(a < i and b < i for i, (a, b) in unions.items())
    assert any(min(a, b) < B <= max(a, b) for a, b in unions.values())                            # parts on both sides of slot 256
    assert any(kind[a] == SLOT_UNION and a >= B for a, _ in unions.values())                       # a union of a union past slot 256
    assert all(kind[a] == SLOT_UNION and kind[b] == SLOT_UNION for a, b in [unions[299]])
    assert any(i not in data for ab in unions.values() for i in ab if kind[i] == SLOT_OWNER)       # a part the batch did not touch
    for observe in (0, 1):
        want, flags = gt.update_want(c['r0'], 0.9, observe)
        moved = (want != c['r0']).any(1)
        fed = [i for i in data if kind[i] == SLOT_OWNER and np.isfinite(data[i]).any()]
        assert moved[fed].all() if not observe else (moved[fed].sum() >= 20 and not moved[fed].all())     # a moving average always moves
        assert not moved[[i for i in range(n) if kind[i] == SLOT_NONE]].any() and not moved[gt.UPDATE_NAN_ONLY] and moved[gt.UPDATE_NAN_MIXED]
        assert flags.sum() == 2 and flags[gt.UPDATE_NAN_ONLY] == flags[gt.UPDATE_NAN_MIXED] == 1
        assert all(want[i][0] == min(want[a][0], want[b][0]) and want[i][1] == max(want[a][1], want[b][1]) for i, (a, b) in unions.items())


# ---------------------------------------------------------------------------------------------------- 4. fused calibration kernels
@pytest.mark.parametrize('path', ['vector', 'scalar'])
def test_calibration_shapes_cross_the_cap_on_the_path_they_name(path):
    M, C = gt.CALIB_SHAPES[path]
    assert gt.calib_vec(M, C) == (path == 'vector') and not gt.calib_vec(M, 20, aligned=False)
    assert partial_trip(gt.calib_items(M, C), gt.CAL_ITEMS, gt.CAL_BLOCK)
    per_row = C // 4 if path == 'vector' else C
    assert gt.CAL_ITEMS % per_row != 0 and M * per_row == gt.CAL_ITEMS + gt.PAST                  # one trip back is another channel
    z, sc, bi = gt.calib_case(path)
    assert z.shape == (M, C) and len(set(sc.tolist())) == C and len(set(bi.tolist())) == C and gt.CALIB_ACT == 3 and gt.CALIB_ALPHA != 0
    v = z * sc + bi
    assert (v < 0).mean() > 0.2 and (v > 0).mean() > 0.2                                          # the leaky slope matters


# ---------------------------------------------------------------------------------------------------- 5. matchers
def reference_flags(dets, gts, class_num, diff):
    from tests.test_gpu_map_eval import reference_flags as rf
    return rf(dets, gts, class_num, 0.5, diff)


def test_matcher_case_has_a_true_and_a_false_positive_in_every_second_trip_group():
    c = gt.match_case()
    K = c['class_num']
    assert gt.MAP_GROUPS < c['n_img'] * K < gt.MAP_GROUPS + gt.MAP_WAVES * 8 and (c['n_img'] - 1) * K < gt.MAP_GROUPS      # a few workgroups come back
    groups = gt.second_trip_groups(c)
    assert len(groups) == c['n_img'] * K - gt.MAP_GROUPS == 16 and {k for k, _ in groups} == {3} and c['full'][3] == c['n_img'] - 1
    assert sorted(cl for _, cl in groups) == list(range(4, 20))                                   # the last image: classes 0 .. 3 first trip
    flags = reference_flags(c['dets'], c['gts'], K, c['diff'])
    ref = gt.match_reference('voc')
    cat = np.concatenate(flags)
    cls = np.concatenate([d[:, 5].astype(int) for d in c['dets']])
    for k in range(K):                                                                            # the restated loop is evaluate's
        assert int((cat[cls == k] == 1).sum()) == ref['tp'][k] and int((cat[cls == k] == 2).sum()) == ref['fp'][k]
    coco = gt.match_reference('coco')
    first = np.concatenate([[0], np.cumsum([len(d) for d in c['dets']])])
    for pos, k in groups + [(p, k) for p in range(4) for k in range(K)]:                          # (and every other group with rows)
        mine = c['dets'][pos][:, 5].astype(int) == k
        assert (flags[pos][mine] == 1).sum() >= 1 and (flags[pos][mine] == 2).sum() >= 1, (pos, k)
        f = coco['flags'][0, 0, first[pos]:first[pos + 1]][mine]
        assert (f == 1).sum() >= 1 and (f == 2).sum() >= 1, (pos, k)
    assert (cat == 0).sum() >= 10 and len({float(s) for d in c['dets'] for s in d[:, 4]}) < 8     # difficult matches; score ties
    assert all(h.any() for h in c['diff'])
    dets, gts, diff = gt.spread(c)
    assert len(dets) == c['n_img'] and sum(len(d) for d in dets) == len(cat) and [i for i, d in enumerate(dets) if len(d)] == list(c['full'])


def same_dict(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_dropping_empty_images_changes_no_output_of_the_references():
    """The references are evaluated on the non-empty images only.  Here, on an instance small enough to run both ways: rich and empty images
    mixed, evaluated with and without the empty ones by all three references (and the restated VOC flags)."""
    rng = np.random.default_rng(17)
    K = 5
    rich = [gt._rich_image(rng, K) for _ in range(4)]
    full = (1, 4, 5, 8)
    small = dict(n_img=10, full=full, dets=[r[0] for r in rich], gts=[r[1] for r in rich], diff=[r[2] for r in rich])
    dets, gts, diff = gt.spread(small)
    assert [len(d) > 0 for d in dets] == [i in full for i in range(10)]
    same_dict(voc_eval.evaluate(dets, gts, K, difficult=diff), voc_eval.evaluate(small['dets'], small['gts'], K, difficult=small['diff']))
    assert np.array_equal(np.concatenate(reference_flags(dets, gts, K, diff)), np.concatenate(reference_flags(small['dets'], small['gts'], K, small['diff'])))
    same_dict(coco_eval.evaluate(dets, gts, K, difficult=diff), coco_eval.evaluate(small['dets'], small['gts'], K, difficult=small['diff']))
    same_dict(oppoint.confusion(dets, gts, K, 0.25, 0.5, diff), oppoint.confusion(small['dets'], small['gts'], K, 0.25, 0.5, small['diff']))


# ---------------------------------------------------------------------------------------------------- 6. confusion and padded append
def test_confusion_pairs_share_a_workgroup_and_stage_different_numbers_of_rows_and_boxes():
    from tests import oppoint_cases as oc
    c = gt.confusion_case()
    assert c['n_img'] == gt.MAP_MAX_GRID + 4 and c['full'] == (0, 1, 2, 3) + tuple(gt.MAP_MAX_GRID + k for k in range(4))
    assert len(set(gt.confusion_pick())) == 8
    size = [gt.confusion_sizes(d, g, c['conf'], c['class_num']) for d, g in zip(c['dets'], c['gts'])]
    for k in range(4):                                                                            # image k and image MAP_MAX_GRID + k: workgroup k
        a, b = size[k], size[4 + k]
        assert a[0] != b[0] and a[1] != b[1] and min(a + b) >= 2 and sum(a) <= oc.LDS_BOXES and sum(b) <= oc.LDS_BOXES, (k, a, b)
    assert size[4][0] > size[0][0] and size[4][1] > size[0][1] and size[5][0] < size[1][0] and size[5][1] < size[1][1]
    ref = gt.confusion_reference()
    first = np.concatenate([[0], np.cumsum([len(d) for d in c['dets']])])
    for k in range(8):
        m = ref['match'][first[k]:first[k + 1]]
        assert (m >= 0).any() and (m == -1).any(), k                                              # every image: a matched row and a free one
    assert (ref['match'] == -2).any() and ref['matrix'].sum() > 40


def test_append_counts_clamp_both_ways_and_are_non_zero_where_the_sum_is_strided():
    c = gt.append_case()
    counts, B, cap = c['counts'], gt.APPEND_BATCH, gt.APPEND_CAP
    assert B == gt.MAP_MAX_GRID + 4 and set(counts.tolist()) == {-1, 0, 1, 3, 5} and cap == 3 and gt.APPEND_BASE != 0
    assert (counts[:gt.APPEND_BLOCK] > 0).any() and (counts[gt.APPEND_BLOCK:2 * gt.APPEND_BLOCK] > 0).any() and (counts[gt.MAP_MAX_GRID:] > 0).sum() >= 2
    assert counts[B - 1] > 0                                                                      # the row a shorter n_new cuts off is the last image's
    total = int(np.clip(counts, 0, cap).sum())
    assert c['rows'].shape == (total, 6) and c['img'].shape == (total,) and c['first'][-1] == total
    assert float(c['dets'].max()) < 2 ** 24 and len(np.unique(c['dets'])) == c['dets'].size
    b = 300                                                                                       # one image by hand: count 5 clamps to the cap
    assert np.array_equal(c['rows'][c['first'][b]:c['first'][b + 1]], c['dets'][b, :3]) and (c['img'][c['first'][b]:c['first'][b + 1]] == 307).all()
    assert c['img'][-1] == gt.APPEND_BASE + B - 1 and (np.diff(c['img']) >= 0).all()


# ---------------------------------------------------------------------------------------------------- 7. ties
def test_tie_case_ties_exactly_in_float64_and_the_two_rules_break_them_their_own_way():
    c = gt.tie_case()
    d, g, h = c['dets'][0].astype(np.float64), c['gts'][0], c['diff'][0]
    assert len(g) == gt.TIE_BOXES >= 130 and np.array_equal(c['dets'][0].astype(np.float64), d)
    lane, chunk = (lambda j: j % 64), (lambda j: j // 64)
    (a0, b0), (a1, b1), (a2, b2) = gt.TIE_DUPLICATES
    assert lane(a0) != lane(b0) and chunk(a0) != chunk(b0) and lane(a1) == lane(b1) and chunk(a1) != chunk(b1) and b2 == a2 + 1 and chunk(a2) == chunk(b2)
    for p, (a, b) in enumerate(gt.TIE_DUPLICATES):
        assert np.array_equal(g[a, :4], g[b, :4]) and h[a] != h[b]
        for r in (2 * p, 2 * p + 1):
            iou = voc_eval.box_iou(d[r, :4], g[:, :4])
            assert iou[a] == iou[b] == 1.0 and (iou > 0).sum() == 2 and np.array_equal(d[r, :4], g[a, :4])
        assert d[2 * p, 4] > d[2 * p + 1, 4]
    for p, (a, b) in enumerate(gt.TIE_SPLITS):
        assert lane(a) != lane(b) or chunk(a) != chunk(b)
        whole, left = voc_eval.box_iou(d[6 + 2 * p, :4], g[:, :4]), voc_eval.box_iou(d[7 + 2 * p, :4], g[:, :4])
        assert whole[a] == whole[b] == 0.5 and (whole > 0).sum() == 2 and left[a] == 1.0 and left[b] == 0.0 and not h[a] and not h[b]
    assert chunk(gt.TIE_SPLITS[0][0]) != chunk(gt.TIE_SPLITS[0][1]) and lane(gt.TIE_SPLITS[1][0]) == lane(gt.TIE_SPLITS[1][1])
    # what the references do with them
    flags = reference_flags(c['dets'], c['gts'], 1, c['diff'])[0]
    ref = voc_eval.evaluate(c['dets'], c['gts'], 1, difficult=c['diff'])
    assert (flags == 1).sum() == ref['tp'][0] and (flags == 2).sum() == ref['fp'][0]
    assert tuple(flags[:12]) == gt.TIE_VOC_FLAGS and (flags[12:] == 1).all()
    coco = coco_eval.evaluate(c['dets'], c['gts'], 1, difficult=c['diff'])
    assert tuple(coco['flags'][0, 0, :12]) == gt.TIE_COCO_FLAGS
    assert gt.TIE_VOC_FLAGS != gt.TIE_COCO_FLAGS

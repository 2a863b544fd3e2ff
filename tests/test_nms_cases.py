"""tests/nms_cases.py checked on its own, without a GPU: the exact-head builder is exact, the label copies give the values they were written
down for, and the case table reaches every branch, boundary, radix-select exit and edge that tests/test_gpu_nms_paths.py is meant to pin - all
computed from the oracle's scores and selection alone.

The 'single keys' exit of the radix select (bins of one key and less than half a chunk taken) is absent on purpose: it cannot be reached at
any size.  A bin of one key holds at most one candidate (the box index is part of the key), so a bin can only cross the capacity when the
bins above it hold MAXC candidates already, which is the 'half full' exit."""
import numpy as np
import pytest

from oracle import decode_ref as dr
from tests import nms_cases as nc

F = np.float32
ALL = [s for c in nc.CASES for s in nc.slots(nc.case_id(c))]


def _find(**want):
    """The slots whose fields (n, tied, branch, template, detail, selp, max_out, name) all match."""
    out = []
    for s in ALL:
        c = nc.by_id(s.case)
        have = dict(n=s.n, tied=s.tied, branch=s.path.branch, template=s.path.template, detail=s.path.detail, selp=s.path.selp,
                    max_out=c.max_out, name=c.name, iou=c.iou, obj=c.obj)
        if all(have[k] == v for k, v in want.items()):
            out.append(s)
    return out


def _iou(s, i, j):
    return dr.tf_iou(nc.boxes_scores(nc.by_id(s.case).name)[0][s.image], i, j)


# ------------------------------------------------------------------------------------------------ the builder and the label copies
@pytest.mark.parametrize('name', sorted({c.name for c in nc.CASES}))
def test_exact_heads_are_exact(name):
    c = next(x for x in nc.CASES if x.name == name)
    boxes, scores = nc.boxes_scores(name)
    want = nc.boxes_f64(c.head, c.anchors)
    assert np.array_equal(want.astype(F).astype(np.float64), want)                       # every corner is an fp32 number ...
    for b in range(boxes.shape[0]):
        assert np.array_equal(boxes[b].astype(np.float64), want)                         # ... and the fp32 decode gives it, bit for bit
    cls = nc.class_logits(c).astype(np.float64)
    s64 = 1.0 / (1.0 + np.exp(-cls))
    assert np.array_equal(scores[cls == 30.0], np.ones(int((cls == 30.0).sum()), F))     # conf 30 and class 30: exactly 1.0
    assert np.array_equal(scores[cls == 0.0], np.full(int((cls == 0.0).sum()), 0.5, F))  # level 0: exactly 0.5
    on = cls != nc.OFF
    assert np.abs(scores[on] - s64[on]).max() <= 2.0 ** -24 and scores[~on].max(initial=0) < 1e-12
    for lv in nc.LEVELS:                                                                 # equal logits: bit-equal scores
        assert np.unique(scores[cls == lv]).size <= 1


def test_no_threshold_sits_near_a_level():
    lev = 1.0 / (1.0 + np.exp(-np.asarray(nc.LEVELS)))
    assert np.diff(np.sort(lev)).min() > 0.1                                             # the levels are far more than an ulp apart
    assert 0.5 in nc.THRESHOLDS
    for t in nc.THRESHOLDS:
        assert t == 0.5 or np.abs(lev - t).min() > 1e-3, t
        assert t > 1e-6                                                                  # OFF boxes (1e-13) stay out


def test_label_copies_give_the_branches_they_were_written_for():
    P = nc.nms_path
    assert P(1040, 512, 64, False).branch == 'fast' and P(1040, 513, 64, False)[:3] == (1088, 'sweep', 1024)
    assert P(1040, 1024, 30, False)[:3] == (1088, 'sweep', 1024) and P(1040, 1025, 30, False)[:2] == (1088, 'greedy')
    assert P(1088, 1088, 30, True)[:3] == (1088, 'tied', 1) and P(1089, 1089, 30, True)[:3] == (2048, 'tied', 1)
    assert P(4032, 513, 30, False)[:3] == (2048, 'sweep', 1024) and P(4032, 1025, 30, False)[:3] == (2048, 'sweep', 2048)
    assert P(4032, 2048, 64, False)[:3] == (2048, 'sweep', 2048) and P(4032, 2049, 64, False).branch == 'overflow-sweep'
    assert P(4032, 4032, 64, True)[:3] == (2048, 'tied', 2) and P(4032, 4032, 65, True)[1:] == ('overflow-greedy', None, 'selg')
    assert P(4032, 512, 65, False).branch == 'greedy' and P(4032, 2048, 65, True).branch == 'greedy'
    assert P(4032, 2049, 256, False).selp == 'selg' and P(4032, 2049, 257, False).selp == 'og'
    assert P(4032, 0, 30, False).branch == 'fast' and P(4032, 0, 65, False).branch == 'greedy'
    # the radix select on 3000 ties under 5 higher scores: the first chunk splits down to the index bits and takes 2048
    sc = np.r_[np.full(5, 0.9, F), np.full(3000, 0.7, F)]
    ch = list(nc.radix_chunks(sc, np.arange(3005), 4032, 0.05, 2048))
    assert [(c.count, c.exit, c.skip) for c in ch] == [(2048, 'half full', True), (957, 'all fits', False)] and ch[0].passes <= 5
    assert ch[0].hi == (1 << 64) - 1 and ch[1].hi == ch[0].lo and ch[0].lo == nc.key_of(F(0.7), 2047)      # boxes 0 .. 2047
    # distinct scores: one pass, the chunk ends above the bin that crosses
    ch = list(nc.radix_chunks(np.r_[np.full(1500, 0.9, F), np.full(2532, 0.3, F)], np.arange(4032), 4032, 0.05, 2048))
    assert [(c.count, c.exit, c.passes, c.skip) for c in ch] == [(1500, 'half full', 1, False), (2048, 'half full', 4, True), (484, 'all fits', 1, False)]


def test_cases_stay_small():
    for c in nc.CASES:
        B, n, C = nc.class_logits(c).shape
        assert n <= 4032 and (B <= 2 and C <= 6 or c.name == 'many'), c.name
    assert nc.class_logits(nc.by_id('many-obj0.05-iou0.3-max3')).shape == (14, 12, 20)


# ------------------------------------------------------------------------------------------------ what the table reaches
def test_fast_path_and_its_limits():
    for n in (0, 1, 64, 65, 512):
        assert _find(branch='fast', n=n, template=1088), n
    assert _find(branch='fast', n=512, template=2048)
    assert _find(branch='fast', n=512, tied=True) and _find(branch='fast', n=512, tied=False)


def test_1088_template():
    assert nc.ntot(nc.H1040) == 1040 and nc.H1040.A == 4
    for n in (513, 1024):
        assert _find(branch='sweep', detail=1024, n=n, template=1088), n
    assert _find(branch='greedy', n=1025, template=1088, max_out=30) and _find(branch='greedy', n=1040, template=1088, max_out=64)
    assert [s for s in _find(branch='tied', template=1088) if s.n > 512]
    assert not [s for s in ALL if s.path.template == 1088 and s.path.branch.startswith('overflow')]       # n <= ntot <= 1088
    # a sweep and a greedy run that visit every candidate: fewer survive than max_out
    assert [s for s in _find(branch='sweep', template=1088) if len(s.selected) < nc.by_id(s.case).max_out]
    assert [s for s in _find(branch='greedy', template=1088) if s.n > 1024 and len(s.selected) < nc.by_id(s.case).max_out] or \
        [s for s in _find(branch='greedy', template=1088) if s.n > 200 and len(s.selected) < nc.by_id(s.case).max_out]


def test_2048_template():
    assert nc.ntot(nc.H3) == 4032
    assert _find(branch='sweep', n=513, detail=1024, template=2048)
    assert _find(branch='sweep', n=1025, detail=2048, template=2048) and _find(branch='sweep', n=2048, detail=2048, template=2048)
    assert _find(branch='overflow-sweep', n=2049) and _find(branch='overflow-sweep', n=4032)
    assert [s for s in _find(branch='sweep', template=2048) if len(s.selected) < nc.by_id(s.case).max_out]
    # an overflow sweep whose selected boxes carry over into a second chunk
    assert [s for s in _find(branch='overflow-sweep') if len(nc.slot_chunks(s)) >= 2]


def test_tied_classes_across_chunks():
    full = _find(branch='tied', n=4032, detail=2)
    reached, ran_out = [], []
    for s in full:
        c = nc.by_id(s.case)
        in_first = int((s.selected < 2048).sum())                      # a tied class is taken in index order: chunk 1 is boxes [0, 2048)
        if len(s.selected) == c.max_out and in_first < c.max_out:
            reached.append(s)                                          # max_out reached inside the second chunk
        if len(s.selected) < c.max_out and in_first < len(s.selected):
            ran_out.append(s)                                          # both chunks swept, candidates exhausted
    assert reached and ran_out
    assert _find(branch='tied', n=2048, detail=1) and _find(branch='tied', n=2049, detail=2)


def test_greedy_and_the_64_65_boundary():
    assert [s for s in _find(branch='greedy', max_out=65, template=2048) if 0 < s.n <= 512] and _find(branch='greedy', max_out=65, n=2048)
    # the same inputs at max_out 64 and 65
    for name in ('giants', 'g1040'):
        ids = {(c.obj, c.iou) for c in nc.CASES if c.name == name and c.max_out == 64} & {(c.obj, c.iou) for c in nc.CASES if c.name == name and c.max_out == 65}
        assert ids, name
    assert _find(max_out=256, branch='overflow-greedy', selp='selg') and _find(max_out=257, branch='overflow-greedy', selp='og')


def _iou_many(boxes, g, others):
    """dr.tf_iou of box g with each of `others`, vectorised: the same fp32 operations in the same order (the boxes here have min <= max)."""
    b, o = boxes[g], boxes[np.asarray(others, np.int64)]
    area_g, area_o = F(b[2] - b[0]) * F(b[3] - b[1]), (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1])
    inter = np.maximum(np.minimum(b[2], o[:, 2]) - np.maximum(b[0], o[:, 0]), F(0)) * np.maximum(np.minimum(b[3], o[:, 3]) - np.maximum(b[1], o[:, 1]), F(0))
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = (inter / ((area_g + area_o) - inter)).astype(F)
    return np.where((area_g <= 0) | (area_o <= 0), F(0), iou)


def _killed_only_across_chunks(s, min_rank=0):
    """A candidate of a later chunk that no box selected in its own chunk suppresses, but one selected in an earlier chunk does (with at
    least `min_rank` boxes selected before that one): without the cross-chunk kill loop it would be kept."""
    c = nc.by_id(s.case)
    boxes, scores = nc.boxes_scores(c.name)
    boxes, sc = boxes[s.image], scores[s.image, :, s.cls]
    sel = [(nc.key_of(sc[g], g), int(g)) for g in s.selected]
    chosen = set(s.selected.tolist())
    for ch, before in nc.slot_chunks(s)[1:]:
        own = [(k, g) for k, g in sel if ch.lo <= k < ch.hi]
        earlier = [g for k, g in sel if k >= ch.hi]
        for g in s.cand.tolist():
            k = nc.key_of(sc[g], g)
            if not (ch.lo <= k < ch.hi) or g in chosen or (len(sel) == c.max_out and k < sel[-1][0]):
                continue
            mine = [o for ko, o in own if ko > k]
            if mine and (_iou_many(boxes, g, mine) > F(c.iou)).any():
                continue
            killers = np.flatnonzero(_iou_many(boxes, g, earlier) > F(c.iou))
            if killers.size and killers.min() >= min_rank:
                assert dr.tf_iou(boxes, g, earlier[killers.min()]) > F(c.iou)
                return [g]
    return []


def test_overflow_greedy_kills_across_chunks():
    for mo in (65, 256, 257):
        hit = [s for s in _find(branch='overflow-greedy', max_out=mo) if len(nc.slot_chunks(s)) >= 2 and _killed_only_across_chunks(s)]
        assert hit, mo
        if mo >= 256:                                                  # more than 256 survive: the cap is what ends the class, in the last chunk
            assert [s for s in hit if len(s.selected) == mo and nc.slot_chunks(s)[-1][1] < mo]
    # selp = og: a chunk entered with more than 256 boxes kept, with a candidate that only selections number 257 and later suppress
    deep = [s for s in _find(branch='overflow-greedy', selp='og') if nc.slot_chunks(s)[-1][1] > 256 and _killed_only_across_chunks(s, 256)]
    assert deep


def test_radix_select_exits():
    over = [s for s in ALL if s.path.branch.startswith('overflow')]
    seen = {(ch.exit, ch.skip) for s in over for ch, _ in nc.slot_chunks(s)}
    assert ('all fits', False) in seen and ('half full', False) in seen and ('half full', True) in seen
    assert not [e for e, _ in seen if e == 'single keys']              # unreachable: see the module docstring
    # the skip with candidates already taken: a few higher scores above more than 2048 ties
    s = _find(name='t2048', n=3001)[0]
    sc = nc.boxes_scores('t2048')[1][s.image, :, s.cls][s.cand]
    assert (sc == sc.min()).sum() > 2048 and 0 < (sc > sc.min()).sum() < 10
    assert [ch for sl in _find(name='t2048', n=3001) for ch, _ in nc.slot_chunks(sl) if ch.skip and ch.passes >= 3]


def _pairs_at(s, value):
    """(selected box, other candidate) pairs whose IoU is exactly `value`: a cell box and the half-width box inside it (anchors 0 and 1)."""
    an, cand, out = nc.coords(nc.by_id(s.case).head)[3], set(s.cand.tolist()), []
    for a in s.selected.tolist():
        g = a + 1 if an[a] == 0 else a - 1
        if an[a] < 2 and g in cand and _iou(s, a, g) == F(value):
            out.append((a, g))
    return out


def test_edges():
    # an IoU of exactly 1/2 at iou_thresh 0.5 (survives) and at the next float below (dies): the fast path and a sorted sweep
    for branch in ('fast', 'sweep'):
        at = [s for s in _find(branch=branch, iou=0.5) if s.n >= 64 and _pairs_at(s, 0.5)]
        below = [s for s in _find(branch=branch, iou=nc.HALF_BELOW) if s.n >= 64 and _pairs_at(s, 0.5)]
        assert at and below, branch
        # the half-width box is selected next to its cell box at 0.5 and dropped just below
        assert [s for s in at if [1 for a, g in _pairs_at(s, 0.5) if g in s.selected]]
        assert [s for s in below if [1 for a, g in _pairs_at(s, 0.5) if g not in s.selected]]
    # iou_thresh 0: touching boxes (IoU exactly 0) stay, overlapping ones go
    zero = [s for s in _find(iou=0.0) if s.n >= 512]
    assert {s.path.branch for s in zero} >= {'fast', 'sweep', 'tied'}
    assert [s for s in zero if [1 for a in s.selected[:8] for g in s.selected if g != a and _iou(s, a, g) == 0 and _touch(s, a, g)]]
    assert [s for s in zero if len(s.selected) < s.n]
    # a score equal to obj_thresh passes (>=)
    half = [s for s in _find(obj=0.5) if s.n and (nc.boxes_scores(nc.by_id(s.case).name)[1][s.image, s.selected, s.cls] == F(0.5)).any()]
    assert half
    # zero-area boxes are candidates, never suppress and are never suppressed
    z = set(np.flatnonzero(nc.coords(nc.H1040)[3] == 3).tolist())
    ran_out = [s for s in ALL if nc.by_id(s.case).name == 't1088' and len(s.selected) < min(nc.by_id(s.case).max_out, s.n)]
    assert [s for s in ran_out if len(z & set(s.cand.tolist())) >= 10]
    for s in ran_out:                                                  # where the candidates run out, every zero-area one is kept
        assert z & set(s.cand.tolist()) <= set(s.selected.tolist())
    # an empty class next to a full one
    assert [s for s in _find(n=0, name='t2048') if s.cls == 5 and [t for t in _find(n=4032, name='t2048') if t.image == s.image and t.cls == 4]]


def _touch(s, i, j):
    b = nc.boxes_scores(nc.by_id(s.case).name)[0][s.image]
    return b[i, 2] == b[j, 0] or b[j, 2] == b[i, 0] or b[i, 3] == b[j, 1] or b[j, 3] == b[i, 1]


def test_batch_times_classes_above_256_with_empty_images():
    c = nc.by_id('many-obj0.05-iou0.3-max3')
    ref = nc.reference(nc.case_id(c))
    assert len(ref) * 20 > 256 and [b for b, (d, _) in enumerate(ref) if len(d) == 0] == [2, 3, 7, 13]
    assert sum(len(d) for d, _ in ref) > 100

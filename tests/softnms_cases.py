"""The case table of the Soft-NMS / DIoU-NMS decode (csrc/yk_decode.hip: softnms_py_kernel<MAXC, METHOD>), shared by tests/test_softnms_rule.py
(CPU: the rule and the table checked on their own) and tests/test_gpu_softnms.py (the kernel).  Nothing here touches a GPU.

The heads are the EXACT heads of tests/nms_cases.py (H12, H1040, H3: dyadic boxes, a handful of logit levels), so every IoU is the same correctly
rounded quotient in k210_yolo_framework_amd/softnms.py and on the device, and with it every 1 - o, every d2 / c2 and every product: `linear` and
`diou` are compared bit for bit.  Besides nms_cases' own class logits there is one head of this module's, `soft1040`, whose classes are built for
single labels (see _cls_soft1040).

GAUSSIAN.  numpy's exp and the device's expf differ by ulps, so a Gaussian case is admitted only if, in a float64 run of the rule,
  (a) in every round, the selected score and every live score that is not bit-equal to it in the fp32 rule are at least GAP = 5e-4 apart,
      relatively (the "top-two gap": a round's selection depends on nothing else; two scores further down may come as close as they like -
      on these heads products of the same weights taken in different orders do, to 1e-16 - until one of them is the largest), and
  (b) every decayed score is at least GAP from obj_thresh, relatively
(gaussian_condition; asserted by tests/test_softnms_rule.py).  Then both sides select the same boxes and only the scores differ, within

  BOUND(R) = 11 * R * 2^-24 relative, R = the row's emission round (a class's first row is undecayed: compared exactly).

Derivation, per round a box stays live, in units of u = 2^-24 (the relative error of one correctly rounded fp32 operation), to first order:
  * the argument -(o * o) / sigma: the device's o is the float64 rule's quotient rounded once (u), so o * o carries 2u and one more for its own
    rounding, the quotient by sigma one more: 4u relative on an argument of magnitude at most 1 / sigma = 2 at the sigma in use (0.5), which
    moves exp by at most 8u relative;
  * expf itself: at most 1 ulp = 2u (the float64 yardstick contributes nothing at this scale);
  * the multiply: u.
  11u per round, summed over the R - 1 rounds before a row's emission: 11u * R bounds it.  The first estimate for this check was 16u * R
  (an expf counted on each side); the yardstick is float64, so only the device's counts, and the derived, smaller constant is the one used.
  It is derived from the formats alone, not from any output of the kernel."""
import collections
import functools

import numpy as np

from k210_yolo_framework_amd import softnms
from oracle import decode_ref as dr
from tests import nms_cases as nc

F = np.float32
GAP = 5e-4
U = 2.0 ** -24


def bound(rounds):
    return 11.0 * np.asarray(rounds, np.float64) * U


# ------------------------------------------------------------------------------------------------ this module's own head
# layer 0 as nms_cases.AN1040 (16 px cells: the cell box, its half-width twin of IoU 1/2, the 32 px box that overlaps its row neighbours by 1/3
# and holds the cell box at IoU 1/4, a zero-width box); layer 1 (128 px cells, centres 8 px off layer 0's in both axes): a 32 px box
AN_SOFT = [[(1 / 16, 1 / 16), (1 / 32, 1 / 16), (1 / 8, 1 / 8), (0.0, 1 / 16)], [(1 / 8, 1 / 8), (1 / 8, 1 / 8), (1 / 4, 1 / 4), (0.0, 1 / 16)]]


def _g(row, col, a):
    """Box index of layer 0 of H1040."""
    return (row * 16 + col) * 4 + a


def _cls_soft1040():
    """class 0  diou: two pairs of IoU exactly 1/4.  The 32 px box of layer 1's cell (0, 0), [48, 80]^2, holds the cell box of (3, 3), [48, 64]^2,
                8 px off centre in both axes: penalty 128 / 2048 = 1/16, 1/4 - 1/16 = 0.1875; the cell box of (10, 10) and its own 32 px box are
                concentric: penalty 0.  A threshold of 0.2 keeps the first and drops the second; hard NMS drops both.
       class 1  the three-box reorder: the cell box of (2, 4) at 1.0, its half-width twin at sigmoid(2) = 0.88, the cell box of (9, 9) at 0.5.
                linear at Nt 0.3 halves the twin to 0.44, below the third box: order cell, (9, 9), twin.
       class 2  zero-width boxes at the highest level on top of cell boxes and twins: they decay nothing and nothing decays them.
       class 3  one candidate.   class 4  none.   class 5  every box at one score."""
    cls = np.full((1, nc.ntot(nc.H1040), 6), nc.OFF, F)
    cls[0, 1024, 0], cls[0, _g(3, 3, 0), 0] = nc.ON, 2.0
    cls[0, _g(10, 10, 0), 0], cls[0, _g(10, 10, 2), 0] = 1.0, 0.0
    cls[0, _g(2, 4, 0), 1], cls[0, _g(2, 4, 1), 1], cls[0, _g(9, 9, 0), 1] = nc.ON, 2.0, 0.0
    for k in range(5):
        cls[0, _g(5, k, 3), 2], cls[0, _g(5, k, 0), 2], cls[0, _g(5, k, 1), 2] = nc.ON, 2.0, 1.0
    cls[0, _g(7, 7, 2), 3] = 1.0
    cls[0, :, 5] = 2.0
    return cls


# the Gaussian overflow head.  nms_cases' t2048 / AN3 misses condition (a) below whatever the levels are (two products of cross-scale weights
# come within 2.7e-5 of each other), so here only the fine scale has area - AN1040's relations on 8 px cells - and the two coarse scales are
# zero-width boxes at the lowest level: candidates that fill the score plane past the LDS capacity and never take part in a decay.
AN_SOFT3 = [[(0.0, 1 / 8)] * 3, [(0.0, 1 / 16)] * 3, [(1 / 32, 1 / 32), (1 / 64, 1 / 32), (1 / 16, 1 / 16)]]


def _cls_soft3():
    """class 0: all 4032 boxes are candidates; class 1: 2049; class 2: 2048 (the capacity); class 3: none."""
    rng = nc._rng('soft3')
    n, coarse = nc.ntot(nc.H3), (8 * 8 + 16 * 16) * 3
    cls = np.full((1, n, 4), nc.OFF, F)
    for c, k in enumerate((n, 2049, 2048)):
        g = np.sort(np.concatenate([np.arange(coarse), coarse + rng.permutation(n - coarse)[:k - coarse]]))
        cls[0, g, c] = np.where(g < coarse, F(-2.0), rng.choice(np.asarray(nc.LEVELS, F), g.size))
    return cls


OWN = {'soft1040': (nc.H1040, np.asarray(AN_SOFT, np.float64), _cls_soft1040), 'soft3': (nc.H3, np.asarray(AN_SOFT3, np.float64), _cls_soft3)}


@functools.lru_cache(maxsize=None)
def head_of(base):
    """(head, anchors) of a base: one of nms_cases' names or this module's own."""
    if base in OWN:
        return OWN[base][0], OWN[base][1]
    c = next(x for x in nc.CASES if x.name == base)
    return c.head, c.anchors


@functools.lru_cache(maxsize=None)
def preds(base):
    if base not in OWN:
        return nc.preds(base)
    p = nc.build_preds(OWN[base][0], OWN[base][2]())
    for a in p:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def boxes_scores(base):
    """decode_ref.decode_boxes_scores of every image: (boxes [B, ntot, 4], scores [B, ntot, C]), fp32, read-only."""
    if base not in OWN:
        return nc.boxes_scores(base)
    p = preds(base)
    bs = [dr.decode_boxes_scores([q[b] for q in p], OWN[base][1], (nc.S, nc.S), (nc.S, nc.S)) for b in range(p[0].shape[0])]
    out = np.stack([x[0] for x in bs]), np.stack([x[1] for x in bs])
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the case table
Case = collections.namedtuple('Case', 'base method obj iou sigma max_out')
HB = nc.HALF_BELOW

CASES = [
    # the 1088-candidate template
    Case('t1088', 'linear', 0.05, 0.3, 0.5, 30), Case('t1088', 'linear', 0.5, 0.3, 0.5, 30), Case('t1088', 'linear', 0.05, 0.5, 0.5, 65),
    Case('t1088', 'linear', 0.05, HB, 0.5, 100), Case('t1088', 'diou', 0.05, 0.3, 0.5, 30), Case('t1088', 'diou', 0.5, 0.5, 0.5, 1),
    Case('t1088', 'gaussian', 0.05, 0.5, 0.5, 30),
    Case('soft1040', 'linear', 0.05, 0.3, 0.5, 30), Case('soft1040', 'linear', 0.5, 0.3, 0.5, 30), Case('soft1040', 'diou', 0.05, 0.2, 0.5, 30),
    Case('soft1040', 'gaussian', 0.05, 0.5, 0.5, 30),
    Case('g1040', 'linear', 0.05, 0.5, 0.5, 65), Case('g1040', 'diou', 0.05, 0.3, 0.5, 30),
    # the 2048-candidate template: classes of 2048 (the capacity), 2049 and 4032 candidates run from global memory
    Case('t2048', 'linear', 0.05, 0.3, 0.5, 30), Case('t2048', 'linear', 0.05, 0.5, 0.5, 100), Case('t2048', 'diou', 0.05, 0.3, 0.5, 65),
    Case('soft3', 'gaussian', 0.05, 0.5, 0.5, 30), Case('soft3', 'linear', 0.05, 0.3, 0.5, 100),
    Case('giants', 'linear', 0.05, 0.5, 0.5, 30), Case('giants', 'diou', 0.05, 0.5, 0.5, 65),
    # batch x classes = 280
    Case('many', 'linear', 0.05, 0.3, 0.5, 3), Case('many', 'diou', 0.05, 0.3, 0.5, 3), Case('many', 'gaussian', 0.05, 0.5, 0.5, 30),
]


def case_id(c):
    return f'{c.base}-{c.method}-obj{c.obj:g}-iou{c.iou:.9g}-max{c.max_out}'


def by_id(cid):
    return next(c for c in CASES if case_id(c) == cid)


def maxc(base):
    return 1088 if nc.ntot(head_of(base)[0]) <= 1088 else 2048


@functools.lru_cache(maxsize=None)
def reference(cid, f64=False):
    """softnms.decode_image of every image of the case, computed once: [(rows [k, 6], box index [k])], read-only.  f64: the float64 run."""
    c = by_id(cid)
    boxes, scores = boxes_scores(c.base)
    out = []
    for b in range(boxes.shape[0]):
        d, i = softnms.decode_image(boxes[b], scores[b], c.obj, c.iou, c.max_out, c.method, c.sigma, np.float64 if f64 else F)
        d.setflags(write=False)
        i.setflags(write=False)
        out.append((d, i))
    return out


def rounds_of(rows):
    """The emission round (1-based, within its class) of every row of one image."""
    r = np.zeros(len(rows), np.int64)
    for k in np.unique(rows[:, 5]):
        m = rows[:, 5] == k
        r[m] = np.arange(1, int(m.sum()) + 1)
    return r


# ------------------------------------------------------------------------------------------------ labels (an instrumented copy of the loop)
LABELS = ('n0', 'n1', 'n_at_capacity', 'n_over_capacity', 'n4032', 'score_at_thresh', 'zero_area', 'all_tied', 'multi_decay', 'dropped', 'reorder',
          'iou_at_thresh', 'diou_split', 'rounds_over_64')


def slot_labels(c, boxes, scores):
    """The labels one (image, class) reaches under case c, from a run of the rule's loop with softnms.weights."""
    out = set()
    floor = F(c.obj)
    cur = np.asarray(scores, F).copy()
    live = cur >= floor
    n = int(live.sum())
    cap = maxc(c.base)
    out |= {'n0'} if n == 0 else set()
    out |= {'n1'} if n == 1 else set()
    out |= {'n_at_capacity'} if n == cap else set()
    out |= {'n_over_capacity'} if n > cap else set()
    out |= {'n4032'} if n == 4032 else set()
    if n and (cur[live] == floor).any():
        out.add('score_at_thresh')
    if n > 1 and cur[live].min() == cur[live].max():
        out.add('all_tied')
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    zero = live & (area <= 0)
    decays = np.zeros(len(cur), np.int64)
    sel, fates = [], {}
    thr = F(c.iou)
    while len(sel) < c.max_out and live.any():
        m = int(np.flatnonzero(live & (cur == cur[live].max()))[0])
        sel.append(m)
        live[m] = False
        w = softnms.weights(boxes, m, c.method, c.iou, c.sigma)
        o = softnms.iou_to_all(boxes, m)[0]
        if zero.any() and n > zero.sum():                           # zero-area boxes among others: weight 1 in both directions
            assert (w[zero & live] == 1).all() and (not zero[m] or (w[live] == 1).all())
            out.add('zero_area')
        if c.method == 'linear' and (o[live] == thr).any():
            out.add('iou_at_thresh')
        if c.method == 'diou':
            hit = live & (o > thr)
            for v, f in zip(o[hit].tolist(), w[hit].tolist()):
                fates.setdefault(v, set()).add(f)
            if any(len(f) == 2 for f in fates.values()):
                out.add('diou_split')                               # one IoU above the threshold, two fates: the centre distance decided
        decays[live & (w < 1)] += 1
        if c.method in ('linear', 'gaussian'):
            new = (cur * w).astype(F)
            if (live & (w > 0) & (w < 1) & (new < floor)).any():
                out.add('dropped')
            cur[live] = new[live]
        live &= ~((cur < floor) | (w == 0))
        if (decays[live] >= 2).any():
            out.add('multi_decay')
    s0 = np.asarray(scores, F)
    hard_order = sorted(sel, key=lambda g: (-float(s0[g]), g))
    if sel != hard_order:
        out.add('reorder')
    if len(sel) > 64:
        out.add('rounds_over_64')
    return out


@functools.lru_cache(maxsize=None)
def case_labels(cid):
    c = by_id(cid)
    boxes, scores = boxes_scores(c.base)
    out = set()
    for b in range(boxes.shape[0]):
        for k in range(scores.shape[2]):
            out |= slot_labels(c, boxes[b], scores[b, :, k])
    if scores.shape[0] * scores.shape[2] > 256:
        out.add('batch_x_classes_over_256')
    return frozenset(out)


# ------------------------------------------------------------------------------------------------ the Gaussian condition
def gaussian_condition(c):
    """-> (worst relative gap between a round's selected score and a live score not bit-equal to it in fp32, worst relative distance of a decayed
    score from obj_thresh), over every (image, class) of the case, from a float64 run of the rule in step with the fp32 run."""
    boxes, scores = boxes_scores(c.base)
    worst_gap = worst_floor = np.inf
    floor = float(F(c.obj))
    for b in range(boxes.shape[0]):
        for k in range(scores.shape[2]):
            cur64 = scores[b, :, k].astype(np.float64)
            cur32 = scores[b, :, k].astype(F)
            live = cur32 >= F(c.obj)
            sel = 0
            while sel < c.max_out and live.any():
                m = int(np.flatnonzero(live & (cur32 == cur32[live].max()))[0])
                rest = live & (cur32 != cur32[m])
                if rest.any():
                    worst_gap = min(worst_gap, float(((cur64[m] - cur64[rest]) / cur64[m]).min()))
                live[m] = False
                sel += 1
                w64 = softnms.weights(boxes[b], m, c.method, c.iou, c.sigma, np.float64)
                w32 = softnms.weights(boxes[b], m, c.method, c.iou, c.sigma, F)
                cur64[live] = cur64[live] * w64[live]
                cur32[live] = (cur32[live] * w32[live]).astype(F)
                dec = live & (w64 < 1)
                if dec.any():
                    worst_floor = min(worst_floor, float((np.abs(cur64[dec] - floor) / floor).min()))
                assert np.array_equal(cur32[live] < F(c.obj), cur64[live] < floor)
                live &= ~(cur32 < F(c.obj))
    return worst_gap, worst_floor

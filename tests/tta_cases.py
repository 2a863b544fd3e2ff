"""Inputs of the fusion of test-time augmentation (k210_yolo_framework_amd/tta.py) shared by tests/test_tta.py (the rule against a second
statement and hand-derived answers) and tests/test_gpu_tta.py (yk_fuse_views against the rule).  numpy only.

A case is one picture: rows per view, one (dy, dx, mw) per view, class_num, max_out, thresh and, for the hand cases, the answer worked out by
hand.  Every number of a hand case is a small integer or a multiple of 1/16, so every float32 step is exact and the answer can be written
down: a fused coordinate is sum(s * x) / sum(s), a fused score mean(s) * min(cnt, N) / N."""
from typing import List, NamedTuple, Optional

import numpy as np

F = np.float32
NO = (0.0, 0.0, -1.0)                       # a view that is the picture itself


class Case(NamedTuple):
    name: str
    rows: List[np.ndarray]                  # per view [k, 6]
    xforms: np.ndarray                      # [V, 3]
    class_num: int
    max_out: int
    thresh: float
    want: Optional[list]                    # the answer by hand, or None


def _case(name, rows, xforms, class_num, max_out, thresh, want=None):
    return Case(name, [np.asarray(r, F).reshape(-1, 6) for r in rows], np.asarray(xforms, F).reshape(-1, 3), class_num, max_out, thresh, want)


A = [10, 10, 20, 20, 0.5, 0]
HALF = [10, 10, 20, 15, 0.25, 0]            # inside A, half its area: IoU exactly 0.5


def hand_cases() -> List[Case]:
    nan = float('nan')
    out = []
    # one view, no same-class pair above thresh: rows, scores and order come back as they are (classes ascending, scores descending)
    apart = [[0, 0, 10, 10, 0.875, 0], [0, 20, 10, 30, 0.5, 0], [0, 5, 10, 15, 0.25, 0], [0, 0, 10, 10, 0.75, 1], [40, 40, 50, 50, 0.75, 1]]
    out.append(_case('one_view_verbatim', [apart], [NO], 2, 30, 0.375, apart))           # the overlapping pairs of class 0 are at IoU 1/3
    # two identical views: the same boxes with the same scores
    two = [[0, 0, 10, 10, 0.875, 0], [0, 20, 10, 30, 0.5, 0], [40, 40, 50, 50, 0.75, 1]]
    out.append(_case('two_identical_views', [two, two], [NO, NO], 2, 30, 0.5, two))
    # a box one of two views found keeps half its score; the one both found keeps all of it and sorts first
    out.append(_case('found_by_one_of_two', [[[0, 0, 10, 10, 0.875, 0], A], [A]], [NO, NO], 1, 30, 0.5,
                     [A, [0, 0, 10, 10, 0.4375, 0]]))
    # two rows of ONE view join (cnt 2 > N 1): mean score * min(2, 1) / 1; box (0.75 * 10 + 0.25 * 12) / 1 = 10.5 ...
    out.append(_case('two_rows_of_one_view', [[[10, 10, 20, 20, 0.75, 0], [12, 10, 22, 20, 0.25, 0]]], [NO], 1, 30, 0.5,
                     [[10.5, 10, 20.5, 20, 0.5, 0]]))
    # IoU exactly at the threshold: no join (the rule is >); N = 1 so both keep their scores
    out.append(_case('iou_equal_to_thresh', [[A, HALF]], [NO], 1, 30, 0.5, [A, HALF]))
    out.append(_case('iou_above_thresh', [[A, HALF]], [NO], 1, 30, 0.4375,
                     [[10, 10, 20, (0.5 * 20 + 0.25 * 15) / 0.75, 0.375, 0]]))
    # a candidate at IoU 1/3 with two clusters: the earlier one takes it.  left (0.75 * 0 + 0.25 * 5) / 1, right (0.75 * 10 + 0.25 * 15) / 1
    out.append(_case('equal_iou_earlier_cluster', [[[0, 0, 10, 10, 0.75, 0], [0, 10, 10, 20, 0.5, 0], [0, 5, 10, 15, 0.25, 0]]], [NO], 1, 30, 0.25,
                     [[0, 1.25, 10, 11.25, 0.5, 0], [0, 10, 10, 20, 0.5, 0]]))
    # equal scores: the lower candidate index is walked first, so it opens the first cluster and is listed first
    out.append(_case('equal_scores_lower_index_first', [[[0, 40, 10, 50, 0.5, 0]], [[0, 0, 10, 10, 0.5, 0]]], [NO, NO], 1, 30, 0.5,
                     [[0, 40, 10, 50, 0.25, 0], [0, 0, 10, 10, 0.25, 0]]))
    # more clusters than max_out: cut by FINAL score - the two boxes two of three views found beat the better-scored ones only one did
    b0, b1, b2, b3 = [0, 0, 10, 10, 0.875, 0], [0, 20, 10, 30, 0.75, 0], [0, 40, 10, 50, 0.625, 0], [0, 60, 10, 70, 0.5, 0]
    third = lambda s: float(F(F(F(2 * s) / F(2)) * F(2)) / F(3))      # (ss / cnt) * min(cnt, N) / N with cnt 2, N 3
    out.append(_case('cut_by_final_score', [[b0, b1], [b2, b3], [b2, b3]], [NO, NO, NO], 1, 2, 0.5,
                     [b2[:4] + [third(0.625), 0], b3[:4] + [third(0.5), 0]]))
    # rows that are no candidates
    odd = [[0, 0, 5, 5, nan, 0], [0, 0, 5, 5, 0.0, 0], [0, 0, 5, 5, -0.5, 0], [0, 0, 5, 5, 0.875, -1], [0, 0, 5, 5, 0.875, 2],
           [0, 0, 5, 5, 0.875, 0.5], A, [0, 0, 5, 5, nan, 1]]
    out.append(_case('dropped_rows', [odd], [NO], 2, 30, 0.5, [A]))
    # a mirrored, shifted view of one object: canvas columns [38, 52] mirrored in a canvas 72 wide are [20, 34], moved by dx -4 [16, 30]
    out.append(_case('mirror_and_shift', [[[10, 16, 20, 30, 0.5, 0]], [[18, 38, 28, 52, 0.5, 0]]], [NO, (-8.0, -4.0, 72.0)], 1, 30, 0.5,
                     [[10, 16, 20, 30, 0.5, 0]]))
    # nothing at all
    out.append(_case('no_rows', [[], [], []], [NO, NO, NO], 2, 3, 0.5, []))
    return out


def random_case(seed: int, views: int, k, class_num: int, max_out: int, thresh: float = 0.55, side: int = 96, name=None) -> Case:
    """Seeded rows around shared objects: every view sees most of `k` objects, jittered by sixteenths of a pixel, at scores from sixteen values
    (ties are common), in a canvas of its own (an integer shift; every other view mirrored).  k: the objects, or their number per class."""
    rng = np.random.default_rng(seed)
    per_class = [k] * class_num if isinstance(k, int) else list(k)
    t, l, cls = [], [], []
    for c, n in enumerate(per_class):
        t += list(rng.integers(0, side, n))
        l += list(rng.integers(0, side, n))
        cls += [c] * n
    t, l, cls = np.asarray(t, np.float64), np.asarray(l, np.float64), np.asarray(cls, np.float64)
    hh, ww = rng.integers(4, 40, len(t)).astype(np.float64), rng.integers(4, 40, len(t)).astype(np.float64)
    rows, xf = [], []
    for v in range(views):
        seen = np.flatnonzero(rng.random(len(t)) < 0.8) if views > 1 else np.arange(len(t))
        jit = lambda: rng.integers(-24, 25, len(seen)) / 16.0
        r = np.stack([t[seen] + jit(), l[seen] + jit(), t[seen] + hh[seen] + jit(), l[seen] + ww[seen] + jit(),
                      rng.integers(1, 17, len(seen)) / 16.0, cls[seen]], 1)
        r = r[np.lexsort((-r[:, 4], r[:, 5]))]                          # decode-shaped: class-major, score descending
        keep = np.concatenate([np.flatnonzero(r[:, 5] == c)[:max_out] for c in range(class_num)]).astype(np.int64)
        r = r[keep]
        oy, ox = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        cw = side + 64 + 2 * ox
        if v % 2:                                                         # into the view's canvas: shifted, then mirrored
            r[:, 0], r[:, 2] = r[:, 0] + oy, r[:, 2] + oy
            left, right = cw - (r[:, 3] + ox), cw - (r[:, 1] + ox)
            r[:, 1], r[:, 3] = left, right
            xf.append((-float(oy), -float(ox), float(cw)))
        else:
            r[:, 0], r[:, 2], r[:, 1], r[:, 3] = r[:, 0] + oy, r[:, 2] + oy, r[:, 1] + ox, r[:, 3] + ox
            xf.append((-float(oy), -float(ox), -1.0))
        rows.append(r)
    return _case(name or f'random-{seed}-v{views}-c{class_num}', rows, xf, class_num, max_out, thresh)


def one_class_counts(n: int, views: int = 1, seed: int = 0) -> Case:
    """A class of exactly n candidates (class 1 of 3; class 0 has two, class 2 none), spread over `views` views, max_out = ceil(n / views)
    or more: the wave boundaries 0, 1, 63, 64, 65."""
    per = -(-max(n, 2) // views)
    rng = np.random.default_rng(1000 * n + seed)
    rows = []
    left = n
    for v in range(views):
        m = min(per, left)
        left -= m
        t, l = rng.integers(0, 200, m).astype(np.float64), rng.integers(0, 200, m).astype(np.float64)
        r = np.stack([t, l, t + rng.integers(4, 40, m), l + rng.integers(4, 40, m), rng.integers(1, 17, m) / 16.0, np.ones(m)], 1).reshape(-1, 6)
        r = r[np.argsort(-r[:, 4], kind='stable')]
        if v == 0:
            r = np.concatenate([[[0, 0, 10, 10, 0.5, 0], [0, 2, 10, 12, 0.25, 0]], r])
        rows.append(r)
    return _case(f'class-of-{n}-in-{views}', rows, [NO] * views, 3, per, 0.55)

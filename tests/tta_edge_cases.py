"""Inputs of yk_fuse_views (csrc/yk_tta.hip) that the cases of tests/tta_cases.py do not reach, shared by tests/test_tta_edge_cases.py (CPU:
tta.fuse against the answers by hand and every claim a case makes) and tests/test_gpu_tta_edges.py (the kernels against tta.fuse).  numpy only.

  overfull_*   rows that are not decode-shaped: more candidates of one class than nmax = views * max_out.  The rule (tta.py): the first nmax in
               candidate order take part, the rest are ignored - the kernel's `pos < nmax` and `n = min(n, nmax)`;
  skipped      rows inside a frame's count that are no candidates: scores 0, -0.0, -0.5, NaN; classes -1, class_num, 2.5, NaN;
  cut, cut_one eight (two) clusters by construction against max_out 4 (1), equal final scores on both sides of the cut;
  mirror_*     the same rows under mw = 0.0, -0.0 (both mirror) and the smallest negative float32 (which does not).

Every number of a hand case is a small integer or dyadic, so every float32 step but the final division by 3 views is exact; that one is written
as the float32 quotient itself."""
from typing import Dict, List, Tuple

import numpy as np

from tests import tta_cases
from tests.tta_cases import NO, Case, _case

F = np.float32
SMALLEST_NEGATIVE = -1.4e-45                # rounds to the float32 of bits 0x80000001


def _boxes(rng, n, side):
    t, l = rng.integers(0, side, n).astype(np.float64), rng.integers(0, side, n).astype(np.float64)
    return np.stack([t, l, t + rng.integers(4, 40, n), l + rng.integers(4, 40, n)], 1)


# ---------------------------------------------------------------------------------------------------- more of a class than views * max_out
def overfull_hand() -> Case:
    """views 2, class_num 2, max_out 3: frame 0 is six rows of class 1, frame 1 four more (among two rows of class 0): 10 candidates against
    nmax = 6.  Frame 1's rows of class 1 sit on frame 0's first four boxes with score 1: were they read, those clusters would have two
    members and other scores.  Read are frame 0's six, each a cluster of its own found by one of two views: half its score, the best three."""
    s = [0.875, 0.75, 0.625, 0.5, 0.375, 0.25]
    f0 = [[0, 20 * i, 10, 20 * i + 10, s[i], 1] for i in range(6)]
    f1 = [[0, 0, 10, 10, 1.0, 1], [40, 0, 50, 10, 0.5, 0], [0, 20, 10, 30, 1.0, 1], [0, 40, 10, 50, 1.0, 1], [40, 20, 50, 30, 0.25, 0],
          [0, 60, 10, 70, 1.0, 1]]
    want = [[40, 0, 50, 10, 0.25, 0], [40, 20, 50, 30, 0.125, 0], [0, 0, 10, 10, 0.4375, 1], [0, 20, 10, 30, 0.375, 1], [0, 40, 10, 50, 0.3125, 1]]
    return _case('overfull_hand', [f0, f1], [NO, NO], 2, 3, 0.5, want)


def overfull_inside() -> Case:
    """The same call with the frames' roles exchanged: frame 0 holds four rows of class 1 among two of class 0, frame 1 six of class 1.  The
    first two of frame 1's ballot are read, its other four are not: the cut falls inside a ballot that starts at n = 4."""
    rng = np.random.default_rng(2323)
    f0 = np.concatenate([_boxes(rng, 6, 60), rng.integers(1, 17, (6, 1)) / 16.0, np.asarray([[1], [0], [1], [1], [0], [1]])], 1)
    f1 = np.concatenate([_boxes(rng, 6, 60), rng.integers(1, 17, (6, 1)) / 16.0, np.ones((6, 1))], 1)
    return _case('overfull_inside', [f0, f1], [NO, (-1.0, -2.0, 120.0)], 2, 3, 0.3)


def overfull_ballot() -> Case:
    """views 1, class_num 2, max_out 40: 80 rows of class 0 in no order.  The cut is at lane 40 of the first ballot of 64; the second ballot
    is dropped whole."""
    rng = np.random.default_rng(4040)
    rows = np.concatenate([_boxes(rng, 80, 300), rng.integers(1, 65, (80, 1)) / 64.0, np.zeros((80, 1))], 1)
    return _case('overfull_ballot', [rows], [NO], 2, 40, 0.55)


def overfull_three() -> Case:
    """views 3, class_num 3, max_out 22: every frame is 66 rows of class 2, 198 candidates against nmax = 66: frame 0's first ballot and two
    lanes of its second are read, nothing of frames 1 and 2.  Frame 0 is a mirrored, shifted view."""
    rng = np.random.default_rng(6622)
    rows = [np.concatenate([_boxes(rng, 66, 200), rng.integers(1, 65, (66, 1)) / 64.0, np.full((66, 1), 2.0)], 1) for _ in range(3)]
    return _case('overfull_three', rows, [(-3.0, -5.0, 400.0), NO, (-2.0, -1.0, -1.0)], 3, 22, 0.55)


OVERFULL: Dict[str, Tuple[int, int]] = {'overfull_hand': (1, 10), 'overfull_inside': (1, 10), 'overfull_ballot': (0, 80), 'overfull_three': (2, 198)}   # class, its candidates


def is_candidate(rows: np.ndarray, class_num: int) -> np.ndarray:
    """tta.py's sentence, not its code: the class exactly one of 0 .. class_num - 1 and the score above 0."""
    with np.errstate(invalid='ignore'):
        return np.isin(rows[:, 5], np.arange(class_num, dtype=F)) & (rows[:, 4] > 0)


def without_class(case: Case, c: int) -> Case:
    return case._replace(name=case.name + f'-without-{c}', rows=[r[~(r[:, 5] == F(c))] for r in case.rows], want=None)


def first_nmax_only(case: Case) -> Case:
    """The case with, of every class, the candidates after the first views * max_out in candidate order (frame ascending, row ascending) taken
    out: what the rule says is read, stated on the rows themselves."""
    nmax = len(case.rows) * case.max_out
    seen = np.zeros(case.class_num, np.int64)
    rows = []
    for r in case.rows:
        keep = np.ones(len(r), bool)
        for i in np.flatnonzero(is_candidate(r, case.class_num)):
            c = int(r[i, 5])
            keep[i] = seen[c] < nmax
            seen[c] += 1
        rows.append(r[keep])
    return case._replace(name=case.name + '-first-nmax', rows=rows, want=None)


# ---------------------------------------------------------------------------------------------------- rows that are no candidates
def skipped() -> Case:
    """views 2, class_num 3, max_out 4.  Every row that is no candidate sits exactly on a good row's box (with a large score where the score is
    not the defect): read, it would join that cluster.  Class -0.0 IS class 0 (-0.0 == 0).  Class 0: 0.75 and 0.25 on one box, found by both
    views: (1 / 2) * 2 / 2; class 1: one of two views: 0.5 / 2; class 2: two boxes one view each, 0.5 / 2 before 0.25 / 2."""
    nan = float('nan')
    f0 = [[0, 0, 10, 10, 0.75, 0], [0, 0, 10, 10, 0.0, 0], [0, 20, 10, 30, 0.5, 1], [0, 20, 10, 30, -0.0, 1], [0, 0, 10, 10, -0.5, 0],
          [0, 40, 10, 50, nan, 2], [0, 40, 10, 50, 0.25, 2]]
    f1 = [[0, 0, 10, 10, 0.875, -1], [0, 0, 10, 10, 0.25, -0.0], [0, 20, 10, 30, 0.875, 3], [0, 40, 10, 50, 0.875, 2.5], [0, 40, 10, 50, 0.875, nan],
          [20, 0, 30, 10, 0.5, 2]]
    want = [[0, 0, 10, 10, 0.5, 0], [0, 20, 10, 30, 0.25, 1], [20, 0, 30, 10, 0.25, 2], [0, 40, 10, 50, 0.125, 2]]
    return _case('skipped', [f0, f1], [NO, NO], 3, 4, 0.5, want)


# ---------------------------------------------------------------------------------------------------- more clusters than max_out
CUT_FIRST = [1, 4, 6, 0]                    # the candidate each kept cluster of `cut` came from


def cut() -> Case:
    """views 2, class_num 1, max_out 4: 2 x 4 pairwise disjoint boxes, eight clusters of one member, final score s / 2.  Walk order (score
    descending, ties to the lower candidate): 0.875 (candidate 1), 0.75 (4), 0.625 (6), then 0.5 three times (0, 3, 5), 0.375, 0.25.  Clusters
    3, 4 and 5 end at 0.25 alike; rank 3, the last one kept, goes to cluster 3 = candidate 0."""
    f0 = [[0, 0, 10, 10, 0.5, 0], [0, 20, 10, 30, 0.875, 0], [0, 40, 10, 50, 0.25, 0], [0, 60, 10, 70, 0.5, 0]]
    f1 = [[20, 0, 30, 10, 0.75, 0], [20, 20, 30, 30, 0.5, 0], [20, 40, 30, 50, 0.625, 0], [20, 60, 30, 70, 0.375, 0]]
    want = [[0, 20, 10, 30, 0.4375, 0], [20, 0, 30, 10, 0.375, 0], [20, 40, 30, 50, 0.3125, 0], [0, 0, 10, 10, 0.25, 0]]
    return _case('cut', [f0, f1], [NO, NO], 1, 4, 0.5, want)


def cut_one() -> Case:
    """max_out 1 (a frame is one row): two disjoint boxes of equal score, two clusters of equal final score; the older one is kept."""
    return _case('cut_one', [[[0, 0, 10, 10, 0.5, 0]], [[20, 0, 30, 10, 0.5, 0]]], [NO, NO], 1, 1, 0.5, [[0, 0, 10, 10, 0.25, 0]])


# ---------------------------------------------------------------------------------------------------- mw at the boundary of the mirror switch
MIRROR_ROWS = [[10, -30, 20, -10, 0.5, 0], [40, -20, 50, 0, 0.25, 0]]
MIRROR_XFORMS = [(-0.0, -0.0, 0.0), (-0.0, -0.0, -0.0), (-0.0, -0.0, SMALLEST_NEGATIVE)]
# the boxes of the two rows as each frame maps them: mw = 0.0 gives 0 - 0 = +0.0, mw = -0.0 gives -0.0 - 0 = -0.0 (and -0.0 + -0.0 stays -0.0);
# the third frame is not mirrored
MIRROR_MAPPED = [[[10, 10, 20, 30], [40, 0.0, 50, 20]], [[10, 10, 20, 30], [40, -0.0, 50, 20]], [[10, -30, 20, -10], [40, -20, 50, 0.0]]]


def _third(s):
    return float(F(s) / F(3))


def mirror_fused() -> Case:
    """thresh 0.5: frames 0 and 1 agree on both boxes (IoU 1), frame 2 stands alone.  Scores ((1 / 2) * 2) / 3, then 0.5 / 3 twice (cluster 1
    before cluster 2), then 0.25 / 3.  The fused left edge (0.25 * 0.0 + 0.25 * -0.0) / 0.5 is +0.0."""
    want = [[10, 10, 20, 30, _third(1.0), 0], [10, -30, 20, -10, _third(0.5), 0], [40, 0.0, 50, 20, _third(0.5), 0], [40, -20, 50, 0.0, _third(0.25), 0]]
    return _case('mirror_fused', [MIRROR_ROWS] * 3, MIRROR_XFORMS, 1, 6, 0.5, want)


def mirror_verbatim() -> Case:
    """thresh 1: no IoU is above it, every candidate stays a cluster of its own and comes back as mapped, the sign of a zero included, at a
    third of its score; equal scores in candidate order."""
    want = [[*MIRROR_MAPPED[f][r], _third(MIRROR_ROWS[r][4]), 0] for r in range(2) for f in range(3)]
    return _case('mirror_verbatim', [MIRROR_ROWS] * 3, MIRROR_XFORMS, 1, 6, 1.0, want)


# ----------------------------------------------------------------------------------------------------
def cases() -> List[Case]:
    return [overfull_hand(), overfull_inside(), overfull_ballot(), overfull_three(), skipped(), cut(), cut_one(), mirror_fused(), mirror_verbatim()]


def neighbours(case: Case, seed: int = 0) -> Tuple[Case, Case]:
    """Two seeded decode-shaped pictures of the case's views, class_num, max_out and thresh, to stand before and behind it in one call."""
    k = max(2, min(case.max_out, 6))
    return tuple(tta_cases.random_case(7000 + 10 * seed + j, len(case.rows), k, case.class_num, case.max_out, thresh=case.thresh,
                                       name=f'{case.name}-neighbour-{j}') for j in range(2))

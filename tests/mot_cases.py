"""Sequences for the tracking scores (csrc/yk_mot.hip: yk_mot_eval's seven launches) on the paths and inputs that the seven cases of
tests/test_gpu_motmetrics.py do not reach, shared by tests/test_mot_cases.py (CPU: every case proved to reach what it claims, and the
rule's own symmetries) and tests/test_gpu_mot_edges.py (the kernels held to the rule on them).  numpy only; nothing here touches a GPU.

Every builder returns [(name, gt [n, 6], res [m, 6]), ...] with the rows of motmetrics ([frame, id, left, top, width, height]).

EXACT BOXES.  The hand-built cases use boxes whose IoU is a quotient of small integers or of dyadic numbers, which iou_ltwh and the
similarity kernel both round once: a 10 x h box inside a 10 x 10 one has IoU h / 10 (IOU_BOX); a 1 x 1 inside a 2 x 1 has exactly 0.5, a
1 x 1 inside a 2 x 2 exactly 0.25, a 3 x 1 inside a 4 x 1 exactly 0.75, and a width of 1 - 2^-20 (3 - 2^-19) lands 2^-21, 2^-22 (2^-21)
below them: far above eps, so every threshold of the rule (>= 0.5, < 0.5 - eps, >= alpha - eps) sees them on its lower side."""
import functools

import numpy as np

from k210_yolo_framework_amd import motmetrics as mm
from tests.test_gpu_motmetrics import many_ids, same_scores as _same_scores

BELOW = 2.0 ** -20


def table(rows):
    return np.asarray(rows, np.float64).reshape(-1, 6)


def long_frames(n_frames):
    """Two generated sequences of n_frames frames and 6 objects: 65 is past one lane stride of frames, 129 past two.  (The generator's
    last frame is drawn; the seeds are the first at which both sequences have a row in frame n_frames, found on the CPU and kept.)"""
    return mm.synthetic_sequences(2, n_frames, 6, seed={65: 4, 129: 10}[n_frames])


def wide_129_133():
    """Three lane strides of rows on each side of a frame, both orientations in one batch, G + T = 262 for the identity matrix."""
    return [('wide', *many_ids(129, 133)), ('tall', *many_ids(133, 129))]


def grid_box(k, rng=None):
    box = np.array([40.0 * (k % 10), 40.0 * (k // 10), 30.0, 30.0])
    return box if rng is None else box + rng.uniform(-3, 3, 4)


MIXED_FRAMES = ((70, 3), (3, 70), (0, 5), (70, 3), (4, 0), (3, 70))      # (ground-truth rows, result rows) of frames 1 .. 6


def mixed_orientation():
    """One sequence whose frames alternate 70 x 3 and 3 x 70, with a frame without ground truth and one without results between them;
    object k sits on a grid, result 100 + k on it with a jitter.  A frame's few rows are picked across the whole grid, so their ids are
    not the first ones.  Batched with a small sequence: the widest ground-truth frame and the widest result frame are different frames."""
    rng = np.random.default_rng(70)
    gt, res = [], []
    for f, (g, t) in enumerate(MIXED_FRAMES, 1):
        gt += [[f, k, *grid_box(k)] for k in (range(70) if g == 70 else rng.choice(70, g, replace=False))]
        res += [[f, 100 + k, *grid_box(k, rng)] for k in (range(70) if t == 70 else rng.choice(70, t, replace=False))]
    return [('mixed', table(gt), table(res)), mm.synthetic_sequences(1, 5, 3, seed=7)[0]]


def iou_box(tenths, x=0):
    """A box whose IoU with the 10 x 10 object at (x, 0) is tenths / 10"""
    return [x, 0, 10, tenths]


FAR = [500, 500, 10, 10]
# name -> (per frame: ({gt id: box}, {result id: box}), (CLR_TP, CLR_FN, CLR_FP, IDSW, Frag) worked out by hand from clear()'s docstring).
# Object 1 is the one under test; object 2 with its result 30 is matched in every frame that has results and keeps the assignment a
# matrix.  Results 10 and 20 contend for object 1.
_O = {1: iou_box(10), 2: iou_box(10, 50)}
_R30 = {30: iou_box(10, 50)}
CONTEST = {
    # (a) frame 2: result 10, matched in frame 1, has IoU 0.6, its rival 20 has 0.9; 1000.6 beats 0.9, so 10 stays: no switch.  Without
    # the bonus 20 takes frame 2 and 10 takes frame 3 back: two switches
    'bonus_keeps': ([(_O, {10: iou_box(10), 20: FAR, **_R30}), (_O, {10: iou_box(6), 20: iou_box(9), **_R30}),
                     (_O, {10: iou_box(10), 20: FAR, **_R30})], (6, 0, 3, 0, 0)),
    # (b) frame 2: result 10 is there with IoU 0.4, unmatched, beside a matched pair: prev_t[1] resets, prev[1] stays 10; frame 3 matches
    # 10 again: a second fragment, no switch
    'gap_same_id': ([(_O, {10: iou_box(10), **_R30}), (_O, {10: iou_box(4), **_R30}), (_O, {10: iou_box(10), **_R30})], (5, 1, 1, 0, 1)),
    # (c) 10, then 20, then 10, one of them a frame: two switches, one fragment
    'a_b_a': ([(_O, {10: iou_box(10), **_R30}), (_O, {20: iou_box(10), **_R30}), (_O, {10: iou_box(10), **_R30})], (6, 0, 0, 2, 0)),
    # (d) matched in frames 1, 3, 5 and present with IoU 0.4 in frames 2 and 4: three fragments, Frag 2; frame 5 matches 20, and IDSW
    # counts it against 10, the last id ever matched (frame 3), although prev_t was none
    'three_fragments': ([(_O, {10: iou_box(10), **_R30}), (_O, {10: iou_box(4), **_R30}), (_O, {10: iou_box(10), **_R30}),
                         (_O, {10: iou_box(4), **_R30}), (_O, {20: iou_box(10), **_R30})], (8, 2, 2, 1, 2)),
    # (e) frame 2 has no results: prev_t stays, so in frame 3 the bonus still holds 10 (IoU 0.6) against 20 (0.9) and no fragment starts.
    # Had prev_t been reset, 20 would win: one switch and a second fragment
    'empty_frame_inside': ([(_O, {10: iou_box(10), 20: FAR, **_R30}), (_O, {}), (_O, {10: iou_box(6), 20: iou_box(9), **_R30})],
                           (4, 2, 2, 0, 0)),
}


def clear_contest():
    out = []
    for name, (frames, _) in CONTEST.items():
        gt = [[f, i, *b] for f, (g, _) in enumerate(frames, 1) for i, b in g.items()]
        res = [[f, i, *b] for f, (_, r) in enumerate(frames, 1) for i, b in r.items()]
        out.append((name, table(gt), table(res)))
    return out


# object -> (ground-truth box, result box with the exact IoU, its neighbour just below, the frames of 5 that carry the exact one)
THRESHOLD_OBJECTS = {
    1: ([0, 0, 2, 1], [0, 0, 1, 1], [0, 0, 1 - BELOW, 1], (1, 2, 3, 4)),            # 0.5 in 4 of 5 frames: matched / seen = 0.8, not above: PT
    2: ([100, 0, 2, 2], [100, 0, 1, 1], [100, 0, 1 - BELOW, 1], (1, 2, 4, 5)),      # 0.25: never matched by CLEAR: ML; HOTA counts it up to alpha 0.25
    3: ([200, 0, 4, 1], [200, 0, 3, 1], [200, 0, 3 - 2 * BELOW, 1], (1, 3, 4, 5)),  # 0.75 and just below: matched in 5 of 5: MT
    4: ([300, 0, 2, 1], [300, 0, 1, 1], [300, 0, 1 - BELOW, 1], (3,)),              # 0.5 in 1 of 5 frames: 0.2, PT
}
THRESHOLD_MT_PT_ML = (1, 2, 1)
THRESHOLD_CLR_TP = 4 + 0 + 5 + 1


def thresholds():
    gt = [[f, o, *g] for f in range(1, 6) for o, (g, _, _, _) in THRESHOLD_OBJECTS.items()]
    res = [[f, 10 + o, *(exact if f in on else below)] for f in range(1, 6) for o, (_, exact, below, on) in THRESHOLD_OBJECTS.items()]
    return [('exact', table(gt), table(res))]


def duplicates():
    """Equal boxes: equal S, equal gas and equal identity costs, so the first-argmin rule decides.  'pairs': two objects on one box and two
    results on another, every IoU 0.8, four frames: every row of every matrix has its minimum twice.  'uneven': the same with one result
    missing in frame 3, so the two results differ and the ties are between the rows: both objects want the same result.  'copy': three
    objects on one box and a fourth apart, the result is the ground truth row for row: S is 1 on the diagonal and 1 between the three."""
    box, shifted = [0, 0, 10, 10], [0, 0, 10, 8]
    gt = [[f, i, *box] for f in range(1, 5) for i in (1, 2)]
    res = [[f, i, *shifted] for f in range(1, 5) for i in (10, 20)]
    copy = [[f, i, *(box if i < 4 else [50, 0, 10, 10])] for f in range(1, 5) for i in (1, 2, 3, 4)]
    return [('pairs', table(gt), table(res)), ('uneven', table(gt), table([r for r in res if r[:2] != [3, 10]])),
            ('copy', table(copy), table(copy))]


def _strangers(seed, n_frames=8):
    """12 objects: 0 .. 7 are followed, 8 .. 11 overlapped by nothing.  9 results: 0 .. 3 follow objects 0 .. 3, result 4 follows object 4
    and from the middle on object 5, result 5 objects 6 and then 7, results 6 .. 8 lie apart and overlap nothing."""
    rng = np.random.default_rng(seed)
    gt = [[f, k, *grid_box(k)] for f in range(1, n_frames + 1) for k in range(12)]
    res = []
    for f in range(1, n_frames + 1):
        late = f > n_frames // 2
        follows = [0, 1, 2, 3, 5 if late else 4, 7 if late else 6]
        res += [[f, 100 + t, *grid_box(k, rng)] for t, k in enumerate(follows)]
        res += [[f, 100 + t, *(grid_box(t) + [0, 3000, 0, 0])] for t in (6, 7, 8)]
    return table(gt), table(res)


def strangers():
    """A third of the ground-truth ids overlapped by nothing, a third of the result ids overlapping nothing, G = 12 > T = 9 and, the
    roles exchanged on another draw, G = 9 < T = 12: the identity matrix's dummy rows and columns do the work."""
    return [('more_gt', *_strangers(12)), ('more_res', *_strangers(9)[::-1])]


def sparse_ids_unsorted():
    """long_65 with the result ids spread over large integers (below 2^53, so exact in the tables) and the rows of both tables shuffled."""
    rng, out = np.random.default_rng(53), []
    for name, gt, res in long_frames(65):
        res = res.copy()
        res[:, 1] = res[:, 1] * (2.0 ** 47 + 1) + 3
        assert res[:, 1].max() < 2.0 ** 53
        out.append((name, gt[rng.permutation(len(gt))], res[rng.permutation(len(res))]))
    return out


BUILDERS = {
    'long_65': functools.partial(long_frames, 65),
    'long_129': functools.partial(long_frames, 129),
    'wide_129_133': wide_129_133,
    'mixed_orientation': mixed_orientation,
    'clear_contest': clear_contest,
    'thresholds': thresholds,
    'duplicates': duplicates,
    'strangers': strangers,
    'sparse_ids_unsorted': sparse_ids_unsorted,
}
GENERIC = ('long_65', 'long_129', 'wide_129_133', 'strangers', 'sparse_ids_unsorted')       # no ties: the symmetries are asserted on these


@functools.lru_cache(maxsize=None)
def case(name):
    seqs = BUILDERS[name]()
    for _, gt, res in seqs:
        gt.setflags(write=False)
        res.setflags(write=False)
    return seqs


@functools.lru_cache(maxsize=None)
def rule(name):
    """motmetrics.evaluate of a case, computed once and shared"""
    return mm.evaluate(case(name))


# ---- the symmetries of the scores, whatever computes them ---------------------------------------------------------------------------------

SWAPPED = {'HOTA_FN': 'HOTA_FP', 'DetRe': 'DetPr', 'AssRe': 'AssPr', 'IDFN': 'IDFP', 'IDR': 'IDP'}
SWAPPED.update({v: k for k, v in list(SWAPPED.items())})
SWAPPED.update({k + '_alpha': v + '_alpha' for k, v in list(SWAPPED.items()) if k in mm.HOTA_FIELDS})
UNCHANGED = ('HOTA_TP', 'MC', 'AssA', 'DetA', 'LocA', 'HOTA', 'AssA_alpha', 'DetA_alpha', 'LocA_alpha', 'HOTA_alpha', 'Loc', 'IDTP', 'IDF1')
SWAP_KEYS = tuple(SWAPPED) + UNCHANGED


def swap_roles(seqs):
    return [(name, res, gt) for name, gt, res in seqs]


def swapped_back(m):
    """The scores of role-swapped sequences under the names they have unswapped: only the keys the swap maps (CLEAR is not symmetric,
    its bonus is per ground-truth id)."""
    return {SWAPPED.get(k, k): m[k] for k in SWAP_KEYS}


def relabel_and_reorder(seqs, seed=11):
    """Result ids permuted among themselves, the rows of both tables shuffled."""
    rng, out = np.random.default_rng(seed), []
    for name, gt, res in seqs:
        res = res.copy()
        ids = np.unique(res[:, 1])
        res[:, 1] = rng.permutation(ids)[np.searchsorted(ids, res[:, 1])]
        out.append((name, gt[rng.permutation(len(gt))], res[rng.permutation(len(res))]))
    return out


def same_scores(got, want, keys=None):
    """tests/test_gpu_motmetrics.same_scores (integers and integer arrays equal, floats within rtol = atol = 1e-12), on the keys given
    or on all of them."""
    if keys is not None:
        got, want = {k: got[k] for k in keys}, {k: want[k] for k in keys}
    _same_scores(got, want)


def each(result):
    """The score dictionaries of an evaluate() / result(): every sequence's, then the combined one."""
    return list(result['sequences'].values()) + [result['combined']]


def same_bytes(a, b):
    for x, y in zip(each(a), each(b)):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k

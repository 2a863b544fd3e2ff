"""Seeded inputs for the cross-tile merge (csrc/yk_tiles.hip: merge_tiles_kernel, merge_compact_kernel; the rule is tiles.merge) on the paths and
inputs random decode-shaped rows never reach, shared by tests/test_tile_cases.py (CPU: every claim a case makes checked from the reference alone,
and the reference against a float64 restatement) and tests/test_gpu_tiles.py (the kernels, bit for bit against the reference).  Nothing here
touches a GPU or torch.

A Case is (name, rows, origins, first, class_num, max_out, thresh, metric, claims): `rows` one float32 [k, 6] array per tile (top, left, bottom,
right, score, class), `origins` float32 [n_tiles, 2], `first` the pictures' tile ranges, `claims` what the case was built to be (read by the two
test files, not by the kernel).  No decision hangs on the last bit of a quotient: coordinates and origins are multiples of 1/4 below 2^12 and
boxes at most 32 wide, so corners, areas, intersections and unions are exact in float32 and a match is either exactly `thresh` or at least
1 / (2 * 32768) away from 0.5; the far-origin cases, whose point is that the translation rounds, keep every match above 0.9 or at 0 (or compare
with thresh 0, where only the sign of a float32 difference decides).  tests/test_tile_cases.py asserts that gap for every case."""
import collections

import numpy as np

from k210_yolo_framework_amd import tiles

F = np.float32
YK_TILES_MAXC = 2048                      # csrc/yk_tiles.hip: candidates of one (picture, class) held in LDS at most
SENTINEL = 12345.0                        # what the GPU tests fill d_out with before the call
POISON = 3e38                             # the score of a row a clamp must keep the kernel from reading: it would come out first

Case = collections.namedtuple('Case', 'name rows origins first class_num max_out thresh metric claims')


def lds_cap(n_tiles, n_pics, max_out):
    """merge_lds_candidates of csrc/yk_tiles.hip restated; the GPU test holds it to engine.merge_tiles_lds_candidates."""
    most = max(n_tiles - (n_pics - 1), 1) * max_out
    return min((most + 63) // 64 * 64, YK_TILES_MAXC)


def case_lds_cap(case):
    return lds_cap(len(case.rows), len(case.first) - 1, case.max_out)


def _case(name, rows, origins, first, class_num, max_out, thresh, metric, **claims):
    rows = [np.ascontiguousarray(np.asarray(r, F).reshape(-1, 6)) for r in rows]
    origins = np.ascontiguousarray(np.asarray(origins, F).reshape(-1, 2))
    assert len(origins) == len(rows) and first[0] == 0 and first[-1] == len(rows), name
    assert all(len(r) <= class_num * max_out for r in rows), name
    for a in rows + [origins]:
        a.setflags(write=False)
    return Case(name, rows, origins, tuple(int(v) for v in first), int(class_num), int(max_out), float(thresh), metric, claims)


def pictures(case):
    """-> per picture (rows_per_tile, origins)"""
    return [(case.rows[a:b], case.origins[a:b]) for a, b in zip(case.first[:-1], case.first[1:])]


def candidates(case):
    """Per picture, per class: the rows the rule counts (class exactly c, score above -inf)."""
    out = []
    for rows, _ in pictures(case):
        r = np.concatenate(rows, 0) if rows else np.zeros((0, 6), F)
        with np.errstate(invalid='ignore'):
            out.append([int(((r[:, 5] == F(c)) & (r[:, 4] > -np.inf)).sum()) for c in range(case.class_num)])
    return out


def over(case):
    """Per picture: the classes with more candidates than lds_cap - the ones the kernel walks in global memory."""
    cap = case_lds_cap(case)
    return [[c for c, n in enumerate(per) if n > cap] for per in candidates(case)]


_REFERENCE = {}


def reference(case):
    """tiles.merge per picture -> [(rows, candidate index)], computed once and shared (read-only)."""
    if case.name not in _REFERENCE:
        res = [tiles.merge(rows, origins, case.class_num, case.max_out, case.thresh, case.metric) for rows, origins in pictures(case)]
        for a, b in res:
            a.setflags(write=False)
            b.setflags(write=False)
        _REFERENCE[case.name] = res
    return _REFERENCE[case.name]


# ------------------------------------------------------------------------------------------------------------------------- building blocks
def _q(a):
    """onto the lattice of quarters"""
    return np.round(np.asarray(a, np.float64) * 4) / 4


def _lattice_rows(rng, k, cls, side, lo=4, hi=32, score_levels=4096):
    """k rows of class `cls` (a number or an array): lattice corners in [0, side + hi], sides lo .. hi, scores n / score_levels (ties happen)."""
    t, l = _q(rng.uniform(0, side, k)), _q(rng.uniform(0, side, k))
    h, w = _q(rng.uniform(lo, hi, k)), _q(rng.uniform(lo, hi, k))
    s = rng.integers(1, score_levels, k) / float(score_levels)
    return np.stack([t, l, t + h, l + w, s, np.broadcast_to(np.asarray(cls, np.float64), (k,))], 1).astype(F)


def _deal(rng, per_class, tile_counts):
    """Rows of several classes interleaved at random, the order inside a class kept (so position i of a class is its i-th row), cut into tiles."""
    label = np.concatenate([np.full(len(r), i) for i, r in enumerate(per_class)])
    assert len(label) == sum(tile_counts), (len(label), sum(tile_counts))
    rng.shuffle(label)
    nxt = [0] * len(per_class)
    flat = []
    for i in label:
        flat.append(per_class[i][nxt[i]])
        nxt[i] += 1
    flat = np.asarray(flat, F).reshape(-1, 6)
    cuts = np.cumsum([0] + list(tile_counts))
    return [flat[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _lattice_origins(rng, n, side):
    return _q(rng.uniform(0, side, (n, 2))).astype(F)


def _decode_shaped(rng, n_tiles, class_num, max_out, side):
    """Every tile full and as the decode leaves it: class-major, score-descending inside a class."""
    rows = []
    for _ in range(n_tiles):
        per = []
        for c in range(class_num):
            r = _lattice_rows(rng, max_out, c, side)
            per.append(r[np.argsort(-r[:, 4], kind='stable')])
        rows.append(np.concatenate(per, 0))
    return rows


# ------------------------------------------------------------------------------------------------------------------------------ the cases
def two_classes_global_small(metric='ios', seed=1):
    """3 tiles, 8 classes, max_out 8: cap 64 rows a tile and lds_cap 64.  Not decode-shaped: classes 0 and 1 have 70 candidates each, more than
    max_out in a tile, and take two segments of the one picture's list; classes 2 .. 7 share the other 52 rows and stay in LDS."""
    rng = np.random.default_rng(seed)
    small = [9, 9, 9, 9, 8, 8]
    per = [_lattice_rows(rng, 70, 0, 96), _lattice_rows(rng, 70, 1, 96)] + [_lattice_rows(rng, k, 2 + i, 96) for i, k in enumerate(small)]
    return _case(f'two_classes_global_small-{metric}', _deal(rng, per, [64, 64, 64]), _lattice_origins(rng, 3, 32), [0, 3], 8, 8, 0.5, metric,
                 lds_cap=64, over=[[0, 1]], every_class_keeps=True)


def four_classes_global_stride8(metric='ios', seed=9):
    """3 tiles, 16 classes, max_out 8: cap 128, lds_cap 64; classes 0, 1, 8 and 9 have 70 candidates each, the other twelve share 104 rows.
    One workgroup per class: a device that deals consecutive workgroups out to 8 dies, each with a cache of its own that is written back when
    the kernel ends, lets only workgroups 8 apart see each other's stores while they run - two segments that overlapped would go unnoticed
    between classes 0 and 1 there, and not between 0 and 8."""
    rng = np.random.default_rng(seed)
    big = (0, 1, 8, 9)
    small = iter([9] * 8 + [8] * 4)
    per = [_lattice_rows(rng, 70 if c in big else next(small), c, 96) for c in range(16)]
    return _case(f'four_classes_global_stride8-{metric}', _deal(rng, per, [128, 128, 128]), _lattice_origins(rng, 3, 32), [0, 3], 16, 8, 0.5, metric,
                 lds_cap=64, over=[list(big)])


def boundary(extra, metric='ios', seed=2):
    """The same geometry; class 0 has exactly lds_cap = 64 candidates (the last LDS case) or, with `extra`, 65 (the first global one).  The 65th
    is the last row of the last tile - position 64, the one `pos < lds_cap` keeps out of LDS - and has the best score of the picture."""
    rng = np.random.default_rng(seed)
    n0 = 65 if extra else 64
    rest = 192 - n0
    other = [rest // 7 + (i < rest % 7) for i in range(7)]
    c0 = _lattice_rows(rng, n0, 0, 96)
    per = [c0[:64]] + [_lattice_rows(rng, k, 1 + i, 96) for i, k in enumerate(other)]
    rows = _deal(rng, per, [64, 64, 64 - extra])
    origins = _lattice_origins(rng, 3, 32)
    claims = dict(lds_cap=64, over=[[0]] if extra else [[]], class0=n0)
    if extra:
        last = c0[64].copy()
        last[:4] = [200, 200, 210, 210]                                 # away from every other box: nothing it retires hides the mistake
        last[4] = 1.5
        rows[2] = np.concatenate([rows[2], last[None]], 0)
        claims['first_row'] = (last + np.asarray([origins[2, 0], origins[2, 1], origins[2, 0], origins[2, 1], 0, 0], F)).astype(F)
    return _case(f'boundary-{n0}-{metric}', rows, origins, [0, 3], 8, 8, 0.5, metric, **claims)


def two_classes_global_decode_shaped(metric='ios', seed=3):
    """33 full tiles of 2 classes x 64: 2112 > 2048 candidates in each class, both on the global path, two segments in one picture's list.  side
    400 leaves far more than 64 separate objects, so max_out is what ends the rounds."""
    rng = np.random.default_rng(seed)
    return _case(f'two_classes_global_decode_shaped-{metric}-{seed}', _decode_shaped(rng, 33, 2, 64, 400), _lattice_origins(rng, 33, 64), [0, 33],
                 2, 64, 0.5, metric, lds_cap=2048, over=[[0, 1]], kept_per_class=64)


def three_pictures_mixed(metric='ios', seed=4):
    """first = [0, 33, 36, 69]: two pictures like the previous case (other seeds) around a small one of 3 tiles (50, 0 and 128 rows) that stays in
    LDS.  Four global segments in two list regions, and a picture between them that must not be touched by either."""
    rng = np.random.default_rng(seed)
    a = _decode_shaped(rng, 33, 2, 64, 400)
    mid = _deal(rng, [_lattice_rows(rng, 100, 0, 24), _lattice_rows(rng, 78, 1, 24)], [50, 0, 128])
    b = _decode_shaped(rng, 33, 2, 64, 400)
    return _case(f'three_pictures_mixed-{metric}', a + mid + b, _lattice_origins(rng, 69, 64), [0, 33, 36, 69], 2, 64, 0.5, metric,
                 lds_cap=2048, over=[[0, 1], [], [0, 1]])


def dropped_rows(metric='ios', seed=5):
    """Counted rows the rule drops, among good ones, in a global-path class (0: 70 candidates) and an LDS-path class (2: 6 candidates): scores
    NaN and -inf, classes -1, C, 1.5 and NaN (with scores that would win).  A score of +inf is a score: it wins its class.  So is -0.0 - it is
    above -inf - and in class 2, where fewer than max_out separate boxes live, it comes out last with its sign."""
    rng = np.random.default_rng(seed)
    C = 8
    far = lambda i, s, c: [300 + 20 * i, 300, 310 + 20 * i, 310, s, c]                      # separate boxes away from the random ones
    c0 = np.concatenate([_lattice_rows(rng, 33, 0, 96), np.asarray([far(0, np.nan, 0), far(1, -np.inf, 0), far(2, np.inf, 0), far(3, -0.0, 0)], F),
                         _lattice_rows(rng, 35, 0, 96)], 0)
    c2 = np.asarray([far(4, 0.5, 2), far(5, np.nan, 2), far(6, -0.0, 2), far(7, 0.25, 2), far(8, -np.inf, 2), far(9, np.inf, 2), far(10, 0.75, 2),
                     far(11, 0.125, 2)], F)
    bad = np.asarray([far(12, 0.99, -1), far(13, 0.99, C), far(14, 0.99, 1.5), far(15, 0.99, np.nan), far(2, 0.99, -1), far(9, 2.0, C)], F)
    k = 192 - len(c0) - len(c2) - len(bad)
    rows = _deal(rng, [c0, c2, bad, _lattice_rows(rng, k, rng.integers(3, C, k), 96)], [64, 64, 64])
    return _case(f'dropped_rows-{metric}', rows, np.zeros((3, 2), F), [0, 3], C, 8, 0.5, metric, lds_cap=64, over=[[0]],
                 candidates0=70, candidates2=6, class2=[far(9, np.inf, 2), far(10, 0.75, 2), far(4, 0.5, 2), far(7, 0.25, 2), far(11, 0.125, 2),
                                                        far(6, -0.0, 2)])


def box_edges(metric, kind):
    """Boxes tile_match has to get right, one scenario per class so that none hides another; two tiles, origins (0, 0) and (8, 8).
    kind 'plain' (thresh 0.5): class 0 a box and the same box with both corners swapped, then with one axis swapped - both are that box and go;
    class 1 a zero-area box lying on a good box's edge and inside it - matches nothing, stays; class 2 two identical zero-area boxes - both stay.
    kind 'zero' (thresh 0): class 0 two boxes that share an edge - both stay, the rule is >; class 1 two that share one lattice cell - one goes.
    kind 'inf' (thresh +inf): 12 identical boxes and max_out 8 - nothing is ever retired but the kept one, the cap ends the rounds."""
    A = [10, 10, 20, 20]
    if kind == 'plain':
        t0 = [A + [0.875, 0], [20, 20, 10, 10, 0.75, 0], [10, 12, 10, 18, 0.5, 1], [40, 40, 40, 40, 0.5, 2], [12, 12, 12, 18, 0.25, 1]]
        t1 = [[12, 2, 2, 12, 0.625, 0], [2, 2, 12, 12, 0.75, 1], [32, 32, 32, 32, 0.5, 2], [2, 12, 12, 2, 0.5, 0]]
        want = [[0], [5 + 1, 2, 4], [3, 5 + 2]]                             # candidate indices kept, per class
        thresh, max_out = 0.5, 8
    elif kind == 'zero':
        t0 = [A + [0.875, 0], A + [0.875, 1]]
        t1 = [[2, 12, 12, 22, 0.75, 0], [11.75, 11.75, 21.75, 21.75, 0.75, 1]]       # moved by (8, 8): shares the edge x = 20 / the cell 19.75 .. 20
        want = [[0, 2], [1]]
        thresh, max_out = 0.0, 8
    else:
        assert kind == 'inf'
        t0 = [A + [0.5 + i / 64, 0] for i in range(7)]
        t1 = [[2, 2, 12, 12, 0.5 + i / 64, 0] for i in range(5)]
        want = [[6, 5, 4, 7 + 4, 3, 7 + 3, 2, 7 + 2]]                       # scores descending, equal scores: the lower candidate index
        thresh, max_out = float('inf'), 8
    C = len(want)
    return _case(f'box_edges-{kind}-{metric}', [t0, t1], [[0, 0], [8, 8]], [0, 2], C, max_out, thresh, metric, lds_cap=64, over=[[]],
                 kept=[i for w in want for i in w])


FAR_ORIGINS = [(4000.3, 2999.7), (-0.1, 1e-3), (0.0, 0.0)]


def far_origin(metric='ios', seed=6):
    """Origins that are no integers: r + origin is ONE float32 add that rounds (ulp 2^-12 at 4000).  Tile 0 holds 12 boxes in cells 40 apart with
    fractional corners; tile 1 sees nine of them again, moved by less than 1/2 (match above 0.9), tile 2 three.  The rows that come out are the
    float32 sums, and the duplicates are recognised on those."""
    rng = np.random.default_rng(seed)
    o = np.asarray(FAR_ORIGINS, F)
    cell = np.stack([40.0 * (np.arange(12) // 4), 40.0 * (np.arange(12) % 4)], 1)
    tl = cell + rng.uniform(1, 5, (12, 2))
    pic = np.concatenate([tl, tl + rng.uniform(20, 30, (12, 2))], 1) + np.tile(o[0].astype(np.float64), 2)     # where tile 0's boxes lie
    cls = np.arange(12) % 2

    def tile(which, origin, jitter, scores):
        local = pic[which] - np.tile(np.asarray(origin, np.float64), 2) + rng.uniform(-jitter, jitter, (len(which), 4))
        return np.concatenate([local, np.asarray(scores, np.float64)[:, None], cls[which][:, None].astype(np.float64)], 1).astype(F)

    s0 = rng.permutation(12) / 16.0 + 0.125
    rows = [tile(np.arange(12), o[0], 0.0, s0), tile(np.arange(9), o[1], 0.25, rng.permutation(9) / 16.0 + 0.15625),
            tile(np.arange(9, 12), o[2], 0.25, [0.9, 0.05, 0.9])]
    return _case(f'far_origin-{metric}', rows, o, [0, 3], 2, 16, 0.5, metric, lds_cap=64, over=[[]], kept_total=12)


def far_origin_touch(metric='ios'):
    """Two boxes of one class, thresh 0.  After the float32 adds B's top IS A's bottom: they touch, the intersection is 0 and both stay.  In exact
    sums B's top lies below A's bottom's value by a fraction of an ulp: a merge that translated in higher precision would retire B."""
    o = np.asarray(FAR_ORIGINS, F)
    for k in range(4000):
        ra = F(30.0 + k * 1e-4)
        T = F(ra + o[0, 0])
        rb = F(np.float64(T) - np.float64(o[1, 0]))
        for _ in range(8):
            if F(rb + o[1, 0]) == T and np.float64(rb) + np.float64(o[1, 0]) < np.float64(ra) + np.float64(o[0, 0]):
                rows = [[[10.25, 10.5, ra, 30.5, 0.875, 0]], [[rb, 3010.0, rb + F(20), 3030.0, 0.75, 0]]]
                return _case(f'far_origin_touch-{metric}', rows, o[:2], [0, 2], 1, 4, 0.0, metric, lds_cap=64, over=[[]], kept=[0, 1],
                             kept_if_exact=[0])
            rb = np.nextafter(rb, F(0))
    raise AssertionError('no touching pair found')


def ties(path, metric='ios'):
    """Every candidate of a class has the same score, so each round is decided by position alone.  3 tiles, 4 classes, max_out 32: cap 128 rows a
    tile, lds_cap 128.  Class 0: box i mod 64 of a grid of separate boxes, moved by a quarter per period - positions i and i + 64 (one lane's
    two entries, in different tiles) are the same object with equal scores, and the quarter shows in the output which of them won (identical
    rows could not: whichever wins, the same bytes come out); class 1: truly identical boxes with period 40 (different lanes).  Kept: the first
    max_out positions of each.  path 'lds': 100 candidates in each; 'global': 140 in each (two segments) and 44 of class 2 in LDS."""
    rng = np.random.default_rng(7)
    n = {'lds': 100, 'global': 140}[path]
    box = lambda b, c, d=0.0: [24.0 * (b // 8) + d, 24.0 * (b % 8) + d, 24.0 * (b // 8) + 16 + d, 24.0 * (b % 8) + 16 + d, 0.5, c]
    c0 = np.asarray([box(i % 64, 0, 0.25 * (i // 64)) for i in range(n)], F)
    c1 = np.asarray([box(i % 40, 1) for i in range(n)], F)
    per = [c0, c1, _lattice_rows(rng, 44 if path == 'global' else 60, 2, 96)]
    counts = [128, 128, 68] if path == 'global' else [100, 128, 32]
    rows = _deal(rng, per, counts)
    first0 = [t for t, r in enumerate(rows) for _ in range(int((r[:, 5] == 0).sum()))]      # the tile of each class-0 position
    return _case(f'ties-{path}-{metric}', rows, np.zeros((3, 2), F), [0, 3], 4, 32, 0.5, metric, lds_cap=128,
                 over=[[0, 1]] if path == 'global' else [[]], n=n, stride_pair_in_two_tiles=first0[0] != first0[64])


Clamps = collections.namedtuple('Clamps', 'name dets counts origins first n_tiles n_pics class_num max_out thresh metric want')


def clamps():
    """Tables the Python wrapper refuses and the kernel clamps (counts to [0, cap], first to [0, n_tiles]), for the C entry point itself: counts
    [cap + 5, -3, 7] with three `first` tables.  Every row the clamps keep out of reach holds a valid class, a separate box and the score POISON:
    read, it would come out first (a NaN there would be dropped by the rule and show nothing).  `want` is tiles.merge on what the clamps leave:
    tile 0 whole, tile 1 empty, 7 rows of tile 2; pictures [0, 3) and nothing / [0, 2) / [0, 3)."""
    rng = np.random.default_rng(8)
    C, max_out = 2, 8
    cap = C * max_out
    dets = np.zeros((3, cap, 6), F)
    for t in range(3):
        dets[t] = [[500 + 20 * t, 20 * r, 510 + 20 * t, 20 * r + 10, POISON, r % C] for r in range(cap)]
    dets[0] = _lattice_rows(rng, cap, rng.integers(0, C, cap), 48)
    dets[2, :7] = _lattice_rows(rng, 7, rng.integers(0, C, 7), 48)
    counts = np.asarray([cap + 5, -3, 7], np.int32)
    origins = np.asarray([[0, 0], [4, 4], [8.25, 12.5]], F)
    meant = [dets[0], dets[1, :0], dets[2, :7]]
    out = []
    for first, ranges in [([0, 5, 2], [(0, 3), (3, 3)]), ([-1, 2], [(0, 2)]), ([0, 3 + 4], [(0, 3)])]:
        want = [tiles.merge(meant[a:b], origins[a:b], C, max_out, 0.5, 'ios')[0] for a, b in ranges]
        out.append(Clamps('clamps-first_' + '_'.join(str(v) for v in first), dets, counts, origins, np.asarray(first, np.int32), 3, len(first) - 1, C, max_out, 0.5, 'ios', want))
    dets.setflags(write=False)
    return out


def all_cases():
    cases = []
    for m in tiles.METRICS:
        cases += [two_classes_global_small(m), four_classes_global_stride8(m), boundary(False, m), boundary(True, m), two_classes_global_decode_shaped(m), dropped_rows(m),
                  box_edges(m, 'plain'), box_edges(m, 'zero'), box_edges(m, 'inf'), far_origin(m), far_origin_touch(m), ties('lds', m),
                  ties('global', m)]
    cases.append(three_pictures_mixed('ios'))
    cases.append(three_pictures_mixed('iou'))
    return cases

"""Inputs that make a workgroup take a SECOND TRIP round a grid-stride loop, shared by tests/test_grid_trip_cases.py (CPU: the cases and the
reference side checked on their own) and tests/test_gpu_qat_trips.py, tests/test_gpu_calib_trips.py, tests/test_gpu_map_trips.py (the kernels).
Nothing here touches a GPU or the library.

The kernels launch a capped grid and walk the rest of their work in a loop; every size below is the cap plus a PARTIAL trip (PAST items: one
full workgroup and a ragged second one), so a few workgroups take a second trip, the others do not, and the end is ragged.

  csrc/yk_range.h   grid_for: at most CAL_MAX_GRID workgroups of CAL_BLOCK threads = CAL_ITEMS work items per trip (calibration and QAT)
  csrc/yk_map.hip   grid_for: at most MAP_MAX_GRID workgroups; the matchers take MAP_WAVES (image, class) groups per workgroup = MAP_GROUPS per
                    trip; confusion_kernel and append_padded_kernel take one image per workgroup

tests/test_grid_trip_cases.py reads the four constants out of the two source files and compares.

No rule is restated: the expected values come from tests/qat_ref.py, tests/calib_ref.py, voc_eval.py, coco_eval.py and oppoint.py, and the value
pools from tests/test_gpu_qat.py (`_values`, `_segment`), tests/coco_cases.py and tests/oppoint_cases.py."""
import functools

import numpy as np

CAL_BLOCK = 256                                      # csrc/yk_range.h:13  constexpr int CAL_BLOCK
CAL_MAX_GRID = 2048                                  # csrc/yk_range.h:15  constexpr unsigned CAL_MAX_GRID
CAL_ITEMS = CAL_BLOCK * CAL_MAX_GRID                 # work items of one trip (a float4 on the 16-byte paths, a float on the scalar ones)
MAP_MAX_GRID = 65536                                 # csrc/yk_map.hip:33  grid_for: `if (g > 65536) g = 65536`
MAP_WAVES = 4                                        # csrc/yk_map.hip:26-27  MAP_BLOCK / YK_WAVE = 256 / 64
MAP_GROUPS = MAP_MAX_GRID * MAP_WAVES                # (image, class) groups of one trip of match_kernel / coco_match_kernel
PAST = CAL_BLOCK + 96                                # items past a cap: the second trip of workgroup 0 in full and of workgroup 1 in part
QAT_RANGE = (-1.0, 3.0)                              # RANGES[0] of tests/test_gpu_qat.py: zero point 64
QAT_TILE = 4096                                      # YK_QAT_TILE of include/yolo_hip.h (the GPU test asserts yk_qat_tile() == this)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------- 1. QAT activations
def act_split(n, shift, shift_q):
    """(head, n4, tail) as yk_qat_act_fwd_f32 / yk_qat_act_bwd_f32 split n floats whose first element sits `shift` floats behind a 16-byte
    boundary in y (and dyq) and `shift_q` floats behind one in yq (and dy): csrc/yk_qat.hip same_phase / head_of, lines 50-54 and 287."""
    if shift % 4 != shift_q % 4:
        return n, 0, 0                                                                # no common phase: everything scalar
    head = min((4 - shift % 4) % 4, n)
    n4 = (n - head) // 4
    return head, n4, n - head - 4 * n4


def act_items(n, shift, shift_q):
    """The work items grid_for sizes the launch by: max(n4, head + tail)."""
    head, n4, tail = act_split(n, shift, shift_q)
    return max(n4, head + tail)


def act_n(path, shift=0):
    """vector: head(shift) + 4 * (CAL_ITEMS + PAST) + 3 floats - PAST float4 items take a second trip, three scalars follow.
    scalar: CAL_ITEMS + PAST floats, every one an item of its own."""
    if path == 'scalar':
        return CAL_ITEMS + PAST
    return (4 - shift % 4) % 4 + 4 * (CAL_ITEMS + PAST) + 3


@functools.lru_cache(maxsize=None)
def act_pool():
    """(the whole pool of tests/test_gpu_qat._values for QAT_RANGE, its edge values): the edge values are the pool's exact rounding ties, twenty
    values clamped at either end, both zeros and the denormals - picked by tests/qat_ref.codes, at most PAST of them."""
    from tests import qat_ref
    from tests.test_gpu_qat import _values
    lo, hi = QAT_RANGE
    pool = _values(lo, hi, 1 << 20, np.random.default_rng(2026))                      # (asks for more than there is: all of it)
    s, _ = qat_ref.qparams32(lo, hi)
    u = qat_ref.codes(pool, lo, hi)
    tie = is_tie(pool)
    den = (pool != 0) & (np.abs(pool) < np.finfo(np.float32).tiny)
    edge = np.concatenate([pool[tie], pool[u < 0][:20], pool[u > 255][:20], pool[pool == 0], pool[den]]).astype(np.float32)
    assert len(pool) > 4096 and 200 <= len(edge) <= PAST and s > 0
    return _frozen(pool), _frozen(edge)


def is_tie(x):
    """x / s (float32, as the rule divides) lies exactly half way between two codes."""
    from tests import qat_ref
    s, _ = qat_ref.qparams32(*QAT_RANGE)
    t = (np.asarray(x, np.float32) / s).astype(np.float32)
    with np.errstate(invalid='ignore'):
        return np.isfinite(t) & (np.abs(t) < 1e6) & (t - np.floor(t) == np.float32(0.5))


@functools.lru_cache(maxsize=None)
def act_case(path, shift=0):
    """-> dict(n, shift, shift_q, head, n4, tail, x, g, second): x float32 [n] drawn from the pool, the edge values planted at the end of the
    second-trip region, in the scalar head and in the scalar tail; one value above and one below everything else, each in one place only (the
    maximum inside the second trip, the minimum in the very last element); g the incoming gradient; `second` the slice of x whose items
    belong to a second trip."""
    pool, edge = act_pool()
    shift_q = shift if path == 'vector' else shift + 1
    n = act_n(path, shift)
    head, n4, tail = act_split(n, shift, shift_q)
    rng = np.random.default_rng(7000 + 10 * shift + (path == 'scalar'))
    x = pool[rng.integers(0, len(pool), n)]
    x[np.abs(x) >= 1e6] = np.float32(0.25)                                            # the pool's +-1e6: the extremes below are the only ones
    if path == 'vector':
        second = slice(head + 4 * CAL_ITEMS, head + 4 * n4)
        x[second.stop - len(edge):second.stop] = edge
        x[second.stop - len(edge) - len(pool):second.stop - len(edge)] = np.where(np.abs(pool) >= 1e6, np.float32(0.25), pool)
        x[:head] = edge[[0, -1, 40][:head]]                                           # a tie, a denormal, a tie
        x[n - 3:] = [edge[7], edge[~is_tie(edge) & (edge > 3)][0], np.float32(-2e6)]  # a tie, clamped at the top, the minimum (clamped too)
    else:
        second = slice(CAL_ITEMS, n)
        x[n - len(edge):] = edge
        x[n - 1] = np.float32(-2e6)
    x[second.start + 5] = np.float32(2e6)
    g = rng.standard_normal(n).astype(np.float32)
    return dict(n=n, shift=shift, shift_q=shift_q, head=head, n4=n4, tail=tail, x=_frozen(x), g=_frozen(g), second=second)


# ---------------------------------------------------------------------------------------------------- 2. QAT weights
def tile_first(sizes, tile=QAT_TILE):
    """d_tile_first as train.py fills it: the running sum of ceil(size / tile), [nseg + 1] int32.  A segment of size 0 has NO tile."""
    return np.concatenate([[0], np.cumsum([(int(n) + tile - 1) // tile for n in sizes])]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def weights_case():
    """A flat buffer of 4 * (CAL_ITEMS + PAST) + 3 floats, nearly all of it gap ("bias / gamma / beta": seeded values, a -0.0 planted in the
    first trip, in the second trip and in the scalar tail), nine segments of tests/test_gpu_qat._segment content at odd offsets: three in the
    first trip, one that straddles the start of the 16-byte path's second trip (element 4 * CAL_ITEMS), four inside it, the last one over the
    three tail scalars.  -> dict(flat, offs, segs, total)."""
    from tests.test_gpu_qat import _segment
    rng = np.random.default_rng(12)
    total = 4 * (CAL_ITEMS + PAST) + 3
    border = 4 * CAL_ITEMS
    layout = [(5, 216, 'normal'), (CAL_ITEMS - 2049, 4097, 'half_zero'), (1_000_003, 65537, 'normal'), (border - 101, 300, 'normal'),
              (border + 250, 1, 'equal'), (border + 263, 216, 'half_zero'), (border + 501, 333, 'zero'), (border + 900, 400, 'normal'),
              (total - 7, 7, 'normal')]
    flat = (rng.standard_normal(total) * 100).astype(np.float32)
    flat[[3, CAL_ITEMS + 5000, border + 230, border + 1350]] = -0.0
    offs, segs = [], []
    for off, n, kind in layout:
        sg = _segment(kind, n, rng)
        flat[off:off + n] = sg
        offs.append(off), segs.append(_frozen(sg))
    return dict(flat=_frozen(flat), offs=tuple(offs), segs=tuple(segs), total=total, border=border)


@functools.lru_cache(maxsize=None)
def bad_segment_case():
    """One call with four good segments and, between them, three the kernels must skip: off < 0, off + size > total, size == 0 (which has no
    tile at all: tile_first gives it none, so only the copy + reset kernel ever sees it).  -> dict(flat, offs, sizes, good, total): `good` maps
    the index of a good segment to its content."""
    from tests.test_gpu_qat import _segment
    rng = np.random.default_rng(13)
    total = 40_000
    flat = (rng.standard_normal(total) * 100).astype(np.float32)
    flat[3] = -0.0
    segs = [(6000, 216, 'normal'), (-3, 5000, None), (7001, 4097, 'half_zero'), (12_345, 0, None), (20_003, 8200, 'normal'), (total - 10, 300, None),
            (39_000, 1, 'equal')]
    good = {}
    for i, (off, n, kind) in enumerate(segs):
        if kind is not None:
            good[i] = _frozen(_segment(kind, n, rng))
            flat[off:off + n] = good[i]
    return dict(flat=_frozen(flat), offs=tuple(s[0] for s in segs), sizes=tuple(s[1] for s in segs), good=good, total=total)


# ---------------------------------------------------------------------------------------------------- 3. QAT range update
UPDATE_SLOTS = 300
UPDATE_BLOCK = 256                                   # csrc/yk_qat.hip:117  `for (int i = threadIdx.x; i < n_slots; i += 256)`
# union slot -> its two parts (both lower): both sides of slot 256, a union of a union whose inner union is >= 256, a union of two unions
UPDATE_UNIONS = {40: (3, 17), 260: (10, 258), 270: (257, 100), 280: (260, 5), 299: (280, 270)}
UPDATE_NAN_ONLY, UPDATE_NAN_MIXED = 290, 291          # owners whose batch holds nothing finite / a NaN among finite values


@functools.lru_cache(maxsize=None)
def update_case():
    """-> dict(kind, p0, p1, data, r0): 300 slots; owners with and without batch data, slots of no kind (some with batch data, which must be
    reset and change nothing), the unions above.  data: slot -> float32 values folded into the slot's batch extremes."""
    from k210_yolo_framework_amd.qat import SLOT_NONE, SLOT_OWNER, SLOT_UNION
    rng = np.random.default_rng(14)
    n = UPDATE_SLOTS
    kind = np.where(rng.random(n) < 0.8, SLOT_OWNER, SLOT_NONE).astype(np.int32)
    kind[[3, 17, 10, 258, 257, 100, 5, 255, 256, UPDATE_NAN_ONLY, UPDATE_NAN_MIXED]] = SLOT_OWNER
    kind[[0, 254, 259]] = SLOT_NONE
    p0, p1 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, (a, b) in UPDATE_UNIONS.items():
        kind[i], p0[i], p1[i] = SLOT_UNION, a, b
    data = {}
    for i in range(n):
        if kind[i] != SLOT_UNION and (rng.random() < 0.65 or i in (3, 258, 257, 255, 256, 0, 259)):
            data[i] = _frozen((rng.standard_normal(int(rng.integers(1, 9))) * rng.uniform(0.1, 5) + rng.uniform(-2, 2)).astype(np.float32))
    for i in (17, 100, 5, 298):
        data.pop(i, None)                                                             # owners the batch did not touch (parts of unions among them)
    kind[298] = SLOT_OWNER
    data[UPDATE_NAN_ONLY] = _frozen(np.array([np.nan, np.inf], np.float32))
    data[UPDATE_NAN_MIXED] = _frozen(np.array([50.0, np.nan, -60.25], np.float32))
    r0 = np.stack([-rng.uniform(0.1, 6, n), rng.uniform(0.1, 6, n)], 1).astype(np.float32)
    return dict(kind=_frozen(kind), p0=_frozen(p0), p1=_frozen(p1), data=data, r0=_frozen(r0))


def update_want(r_init, m, observe):
    """The table after the step, as tests/test_gpu_qat.py's test of seven slots states it: tests/qat_ref.update on every owner, then the
    unions in ascending order as min / max of their parts.  -> (ranges float32 [n, 2], flags [n])."""
    from k210_yolo_framework_amd.qat import SLOT_OWNER, SLOT_UNION
    from tests import qat_ref
    c = update_case()
    want = np.array(r_init, np.float32)
    for i in range(UPDATE_SLOTS):
        if c['kind'][i] == SLOT_OWNER:
            want[i] = qat_ref.update(r_init[i], qat_ref.extremes(c['data'][i]) if i in c['data'] else None, m, bool(observe))
    for i in range(UPDATE_SLOTS):
        if c['kind'][i] == SLOT_UNION:
            a, b = c['p0'][i], c['p1'][i]
            want[i] = min(want[a][0], want[b][0]), max(want[a][1], want[b][1])
    flags = np.array([int(i in c['data'] and not np.isfinite(c['data'][i]).all()) for i in range(UPDATE_SLOTS)])
    return want, flags


# ---------------------------------------------------------------------------------------------------- 4. fused calibration kernels
# (M, C): M * C / 4 float4 items, or M * C scalar items, = CAL_ITEMS + PAST.  C / 4 = 5 and C = 3 do not divide CAL_ITEMS, so the channel of
# an item and of the item one trip before it differ: a channel index that forgot the trip shows on every element of the second trip.
CALIB_SHAPES = {'vector': ((CAL_ITEMS + PAST) // 5, 20), 'scalar': ((CAL_ITEMS + PAST) // 3, 3)}
CALIB_ACT, CALIB_ALPHA = 3, 0.3                      # YK_ACT_LEAKY


def calib_vec(M, C, aligned=True):
    """The dispatch of yk_scale_act_range_f32 / yk_scale_act_hist_f32 (csrc/yk_calib.hip, scale_act_vec): the 16-byte kernel iff C % 4 == 0
    and z, y, scale and bias are 16-byte aligned (whole device allocations are)."""
    return C % 4 == 0 and aligned


def calib_items(M, C):
    return M * C // 4 if calib_vec(M, C) else M * C


@functools.lru_cache(maxsize=None)
def calib_case(path):
    """-> (z [M, C], scale [C], bias [C]) float32 as tests/test_gpu_quantize.py draws them; every channel its own scale and bias."""
    M, C = CALIB_SHAPES[path]
    rng = np.random.default_rng(M + C)
    z = rng.standard_normal((M, C)).astype(np.float32) * 3
    sc = rng.uniform(0.2, 2.0, C).astype(np.float32) * rng.choice([-1, 1], C).astype(np.float32)
    bi = rng.standard_normal(C).astype(np.float32)
    assert len(np.unique(sc)) == C and len(np.unique(bi)) == C
    return _frozen(z), _frozen(sc), _frozen(bi)


# ---------------------------------------------------------------------------------------------------- 5. matchers past MAP_GROUPS groups
MATCH_CLASSES = 20
MATCH_IMAGES = (MAP_GROUPS + 16 + MATCH_CLASSES - 1) // MATCH_CLASSES          # 13108: 16 groups take a second trip
EMPTY_D, EMPTY_G, EMPTY_H = _frozen(np.zeros((0, 6), np.float32)), _frozen(np.zeros((0, 6))), _frozen(np.zeros(0, bool))


def _rich_image(rng, class_num):
    """One image with, for EVERY class c: boxes A and B (and, for odd c, a difficult box C), and detections
      on A exactly (a true positive), on A again with a lower score (A is taken / matched: a false positive), on B shifted (a true positive
      at the lower thresholds), far from every box (a false positive, its score tied with another row), and for odd c on C (ignored).
    Rows and boxes of the classes are interleaved by a seeded permutation."""
    from tests import coco_cases as cc
    rows, gt, hard = [], [], []
    for c in range(class_num):
        t = 50.0 * c
        w = float(rng.choice([24.0, 30.0, 36.0]))
        A, B, Cb = [t, 0.0, t + 30.0, w], [t, 100.0, t + 30.0, 140.0], [t, 200.0, t + 30.0, 230.0]
        gt += [A + [1.0, c], B + [1.0, c]]
        hard += [False, False]
        s = rng.choice(cc.SCORES[2:], 2, replace=False)
        rows += [A + [0.875, c], [t + 1.0, 0.0, t + 30.0, w, min(s), c], [t, 105.0, t + 30.0, 145.0, max(s), c],
                 [t + 10.0, 300.0, t + 20.0, 320.0, min(s), c]]
        if c % 2:
            gt.append(Cb + [1.0, c]), hard.append(True)
            rows.append(Cb + [0.25, c])
    pr, pg = rng.permutation(len(rows)), rng.permutation(len(gt))
    return (np.asarray(rows, np.float32)[pr], np.asarray(gt, np.float64)[pg], np.asarray(hard, bool)[pg])


@functools.lru_cache(maxsize=None)
def match_case():
    """MATCH_IMAGES images x 20 classes = MAP_GROUPS + 16 groups.  Content in images 0 and 1 (first trip; their workgroups 0 .. 3 are the
    ones that come back for the second trip), in the last but one image (the last whole image of the first trip) and in the last image, whose
    classes 0 .. 3 are first-trip groups and 4 .. 19 second-trip groups.  Every other image has no rows and no boxes.
    -> dict(class_num, n_img, full, dets, gts, diff): dets / gts / diff list the `full` (non-empty) images only, in image order."""
    rng = np.random.default_rng(15)
    full = (0, 1, MATCH_IMAGES - 2, MATCH_IMAGES - 1)
    d, g, h = zip(*[_rich_image(rng, MATCH_CLASSES) for _ in full])
    return dict(class_num=MATCH_CLASSES, n_img=MATCH_IMAGES, full=full, dets=[_frozen(a) for a in d], gts=[_frozen(a) for a in g],
                diff=[_frozen(a) for a in h])


def spread(c):
    """The lists of all n_img images of a case that names only its `full` ones -> (dets, gts, diff)."""
    dets, gts, diff = [EMPTY_D] * c['n_img'], [EMPTY_G] * c['n_img'], [EMPTY_H] * c['n_img']
    for k, i in enumerate(c['full']):
        dets[i], gts[i], diff[i] = c['dets'][k], c['gts'][k], c['diff'][k]
    return dets, gts, diff


def second_trip_groups(c):
    """[(position in c['dets'], class)] of the groups past MAP_GROUPS that hold rows."""
    out = []
    for q in range(MAP_GROUPS, c['n_img'] * c['class_num']):
        i, k = divmod(q, c['class_num'])
        if i in c['full']:
            out.append((c['full'].index(i), k))
    return out


@functools.lru_cache(maxsize=None)
def match_reference(rule):
    """voc_eval.evaluate / coco_eval.evaluate of match_case's non-empty images (tests/test_grid_trip_cases.py shows on a small instance that
    the empty images change no output); computed once."""
    from k210_yolo_framework_amd import coco_eval, voc_eval
    c = match_case()
    if rule == 'voc':
        return voc_eval.evaluate(c['dets'], c['gts'], c['class_num'], difficult=c['diff'])
    return coco_eval.evaluate(c['dets'], c['gts'], c['class_num'], difficult=c['diff'])


# ---------------------------------------------------------------------------------------------------- 6. confusion and padded append
CONF_IMAGES = MAP_MAX_GRID + 4                        # workgroup k takes image k and image MAP_MAX_GRID + k, k = 0 .. 3
CONF_THRESH = 0.25


@functools.lru_cache(maxsize=None)
def confusion_case():
    """Eight images of the pool below at 0 .. 3 and MAP_MAX_GRID .. MAP_MAX_GRID + 3, every other image empty.
    -> dict as match_case's, + conf."""
    m = _confusion_pool()
    pick = confusion_pick()
    full = (0, 1, 2, 3, MAP_MAX_GRID, MAP_MAX_GRID + 1, MAP_MAX_GRID + 2, MAP_MAX_GRID + 3)
    return dict(class_num=20, n_img=CONF_IMAGES, full=full, dets=[m[0][i] for i in pick], gts=[m[1][i] for i in pick], diff=[m[2][i] for i in pick],
                conf=CONF_THRESH)


@functools.lru_cache(maxsize=None)
def _confusion_pool():
    """32 images drawn as tests/oppoint_cases.py draws 'mixed20' (tests/coco_cases.random_case, every fourth row moved to the next class)."""
    from tests import coco_cases as cc
    d, g, h = cc.random_case(np.random.default_rng(2031), 32, 20)
    d = [np.array(x, np.float32).reshape(-1, 6) for x in d]
    for x in d:
        x[::4, 5] = (x[::4, 5] + 1) % 20
    return [_frozen(x) for x in d], [_frozen(x) for x in g], [_frozen(x) for x in h]


def confusion_sizes(d, g, conf=CONF_THRESH, class_num=20):
    """(rows taking part, boxes) of one image, as confusion_kernel stages them in LDS."""
    d = np.asarray(d, np.float64).reshape(-1, 6)
    cls = d[:, 5].astype(int)
    return int(((d[:, 4] >= conf) & (cls >= 0) & (cls < class_num)).sum()), len(g)


@functools.lru_cache(maxsize=None)
def confusion_pick():
    """Eight images of the pool as four (first, second) pairs: both of a pair stage rows and boxes, in different numbers; the first and the
    last pair's second image is the larger in both.  Chosen by size alone."""
    m = _confusion_pool()
    size = [confusion_sizes(d, g) for d, g in zip(m[0], m[1])]
    ok = sorted((i for i in range(len(size)) if size[i][0] >= 3 and size[i][1] >= 3), key=lambda i: size[i])
    small = ok[:4]
    large = [i for i in ok[4:] if all(size[i][0] > size[j][0] and size[i][1] > size[j][1] for j in small)][-4:]
    assert len(large) == 4, size
    first = [small[0], large[1], large[2], small[3]]
    second = [large[0], small[1], small[2], large[3]]
    return tuple(first + second)


@functools.lru_cache(maxsize=None)
def confusion_reference():
    from k210_yolo_framework_amd import oppoint
    c = confusion_case()
    return oppoint.confusion(c['dets'], c['gts'], c['class_num'], c['conf'], 0.5, c['diff'])


APPEND_BATCH, APPEND_CAP, APPEND_BASE = MAP_MAX_GRID + 4, 3, 7
APPEND_BLOCK = 256                                   # csrc/yk_map.hip:93  `for (int j = threadIdx.x; j < b; j += MAP_BLOCK)`


@functools.lru_cache(maxsize=None)
def append_case():
    """-> dict(dets [batch, cap, 6] float32 (every value its own: 18 b + 6 k + e, exact in float32), counts int32 [batch] drawn from
    {-1, 0, 1, 3, 5}, rows, img): rows / img what yk_map_append_padded must write - a cumsum of the clamped counts."""
    rng = np.random.default_rng(16)
    B, cap = APPEND_BATCH, APPEND_CAP
    counts = rng.choice(np.array([-1, 0, 1, 3, 5], np.int32), B)
    counts[[3, 300, MAP_MAX_GRID + 1, B - 1]] = [3, 5, 1, 3]
    dets = np.arange(B * cap * 6, dtype=np.float32).reshape(B, cap, 6)
    clamped = np.clip(counts, 0, cap)
    keep = np.arange(cap)[None, :] < clamped[:, None]
    first = np.concatenate([[0], np.cumsum(clamped)])
    return dict(dets=_frozen(dets), counts=_frozen(counts), clamped=clamped, first=first, rows=_frozen(dets[keep]),
                img=_frozen((APPEND_BASE + np.repeat(np.arange(B), clamped)).astype(np.int32)))


# ---------------------------------------------------------------------------------------------------- 7. equal IoU across 64-box chunks
TIE_BOXES = 132
TIE_DUPLICATES = ((3, 70), (5, 69), (10, 11))        # different lanes and chunks; the same lane, different chunks; neighbouring lanes
TIE_DIFFICULT = (3, 69, 11)                          # one copy of every pair
TIE_SPLITS = ((20, 90), (30, 94), (40, 41))          # two HALVES of one cell: distinct boxes with the same IoU with the detection on the cell


@functools.lru_cache(maxsize=None)
def tie_case():
    """One image, one class, 132 boxes of 20 x 20 on a grid of 40-pixel cells (no two cells touch).
      duplicates  box b of a pair (a, b) has a's coordinates; one copy is difficult.  Rows 2p, 2p + 1: a detection exactly on the box (score
                  0.875) and the same again (0.5).
      splits      boxes a and b of a pair are the left and the right half of a's cell: IoU exactly 0.5 with a detection on the whole cell,
                  none with each other.  Rows 6 + 2p, 7 + 2p: the detection on the cell (0.75), then one exactly on the left half (0.25).  Who
                  took the left half decides the second row under both rules.
    Six more rows sit on plain boxes.  All coordinates are small integers: exact in float32.  -> dict(class_num, dets, gts, diff)."""
    k = np.arange(TIE_BOXES)
    top, left = (k // 12) * 40.0, (k % 12) * 40.0
    gt = np.stack([top, left, top + 20.0, left + 20.0, np.ones(TIE_BOXES), np.zeros(TIE_BOXES)], 1)
    hard = np.zeros(TIE_BOXES, bool)
    rows = []
    for a, b in TIE_DUPLICATES:
        gt[b, :4] = gt[a, :4]
        rows += [[*gt[a, :4], 0.875, 0.0], [*gt[a, :4], 0.5, 0.0]]
    hard[list(TIE_DIFFICULT)] = True
    for a, b in TIE_SPLITS:
        t, l = gt[a, 0], gt[a, 1]
        gt[a, :4], gt[b, :4] = [t, l, t + 20.0, l + 10.0], [t, l + 10.0, t + 20.0, l + 20.0]
        rows += [[t, l, t + 20.0, l + 20.0, 0.75, 0.0], [t, l, t + 20.0, l + 10.0, 0.25, 0.0]]
    for j in (0, 63, 64, 127, 128, 131):
        rows.append([gt[j, 0] + 1.0, gt[j, 1], gt[j, 2] + 1.0, gt[j, 3], 0.5, 0.0])
    return dict(class_num=1, dets=[_frozen(np.asarray(rows, np.float32))], gts=[_frozen(gt)], diff=[_frozen(hard)])


# rows 0 .. 11 of tie_case under voc_eval.evaluate (IoU 0.5): the LOWER index wins a tie, and a taken best box is a false positive
TIE_VOC_FLAGS = (0, 0, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2)
# ... and under coco_eval.evaluate at IoU 0.5, every area: a box that is not ignored goes before one that is, then the HIGHER index wins
TIE_COCO_FLAGS = (1, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1)

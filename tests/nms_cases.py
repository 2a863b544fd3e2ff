"""Exact heads, path labels and the case table for the Python-mode decode (csrc/yk_decode.hip: decode_py_kernel, nms_py_kernel<MAXC>, compact_py_kernel,
compact_packed_kernel), shared by tests/test_nms_cases.py (CPU: the table checked on its own) and tests/test_gpu_nms_paths.py (the kernels).
Nothing here touches a GPU.

EXACT HEADS.  tx = ty = 0 (sigmoid = 0.5), tw = th = 0 (exp = 1), power-of-two grids, dyadic anchors (0 allowed), network = image = 256 x 256 and
image_hw None: every box corner is a dyadic number that numpy and the device compute without rounding, so every IoU is the same correctly rounded
quotient on both sides and NMS can be compared by BOX INDEX.  Scores: the confidence logit is 30 (sigmoid == 1.0 in fp32) for a box that is a
candidate of at least one class and -30 otherwise; class logits come from LEVELS, or are OFF (-30: a score of 1e-13, below every threshold in
use) where the box is no candidate of that class - one confidence serves all classes of a box, so this is what lets the classes of one image
carry different cases.  Equal logits give bit-equal scores on each side (exact ties, decided by the box index); different levels differ by far
more than an ulp (the same order on both sides); level 0 is exactly 0.5 on both sides (the `>= obj_thresh` case).

LABELS.  nms_path() and radix_chunks() are Python copies of nms_py_kernel's dispatch and of the chunk loop of its radix select, used ONLY to
label the cases, so that tests/test_nms_cases.py can assert that every branch and boundary stays covered."""
import collections
import functools
import zlib

import numpy as np

from oracle import decode_ref as dr

F = np.float32
S = 256                                   # network and image, pixels
ON, OFF = 30.0, -30.0
LEVELS = (-2.0, -1.0, 0.0, 1.0, 2.0, 30.0)
HALF_BELOW = float(np.nextafter(F(0.5), F(0)))          # the largest fp32 below 0.5: an IoU of exactly 1/2 dies here and survives 0.5

Head = collections.namedtuple('Head', 'grids A')
H3 = Head(((8, 8), (16, 16), (32, 32)), 3)              # 4032 boxes: the 2048-candidate template
H1040 = Head(((16, 16), (2, 2)), 4)                     # 1040 boxes: the 1088-candidate template (the shipped 224x320 head has 1050), 4 anchors
H12 = Head(((2, 2),), 3)                                # 12 boxes


def ntot(head):
    return sum(h * w for h, w in head.grids) * head.A


@functools.lru_cache(maxsize=None)
def coords(head):
    """(layer, row, col, anchor) of every box in the reference's flattened (layer, h, w, anchor) order."""
    out = []
    for l, (h, w) in enumerate(head.grids):
        r, c, a = np.meshgrid(np.arange(h), np.arange(w), np.arange(head.A), indexing='ij')
        out.append(np.stack([np.full(r.size, l), r.ravel(), c.ravel(), a.ravel()], 1))
    out = np.concatenate(out).T.copy()
    out.setflags(write=False)
    return out


def build_preds(head, cls):
    """cls [B, ntot, C] class logits (OFF: no candidate of that class) -> preds[l] [B, h, w, A, 5 + C] fp32."""
    cls = np.asarray(cls, F)
    B, n, C = cls.shape
    assert n == ntot(head)
    conf = np.where((cls != F(OFF)).any(-1), F(ON), F(OFF)).astype(F)
    preds, o = [], 0
    for h, w in head.grids:
        m = h * w * head.A
        p = np.zeros((B, h, w, head.A, 5 + C), F)
        p[..., 4] = conf[:, o:o + m].reshape(B, h, w, head.A)
        p[..., 5:] = cls[:, o:o + m].reshape(B, h, w, head.A, C)
        preds.append(p)
        o += m
    return preds


def boxes_f64(head, anchors):
    """The boxes of an exact head in float64, straight from the geometry: [ntot, 4] = ymin, xmin, ymax, xmax in pixels."""
    l, r, c, a = coords(head)
    hw = np.asarray(head.grids, np.float64)[l]
    anc = np.asarray(anchors, np.float64)[l, a]
    cy, cx = (r + 0.5) / hw[:, 0], (c + 0.5) / hw[:, 1]
    return np.stack([cy - anc[:, 1] / 2, cx - anc[:, 0] / 2, cy + anc[:, 1] / 2, cx + anc[:, 0] / 2], 1) * S


# ------------------------------------------------------------------------------------------------ path labels (copies of the kernel's dispatch)
Path = collections.namedtuple('Path', 'template branch detail selp')


def nms_path(ntot_, n, max_out, all_tied):
    """The template choice (nms_maxc) and the branch chain at the end of nms_py_kernel in csrc/yk_decode.hip, branch for branch: keep the two
    together.  detail: P of a sorted sweep, the number of LDS chunks a tied class has."""
    maxc = 1088 if ntot_ <= 1088 else 2048
    sweep_ok = max_out <= 64 and ntot_ < (1 << 20)
    selp = 'selg' if max_out <= 256 else 'og'
    if n <= 512 and max_out <= 64:
        return Path(maxc, 'fast', None, None)
    if all_tied and sweep_ok:
        return Path(maxc, 'tied', (n + maxc - 1) // maxc, None)
    if n <= maxc and sweep_ok and (1024 if n <= 1024 else 2048) <= maxc:
        P = 64
        while P < n:
            P <<= 1
        return Path(maxc, 'sweep', P, None)
    if n <= maxc:
        return Path(maxc, 'greedy', None, None)
    if sweep_ok and maxc >= 2048:
        return Path(maxc, 'overflow-sweep', None, None)
    return Path(maxc, 'overflow-greedy', None, selp)


def key_of(score, index):
    """The 64-bit key of the overflow branch: (score bits, ~box index)."""
    return (int(np.asarray(score, F).view(np.uint32)) << 32) | (~int(index) & 0xffffffff)


Chunk = collections.namedtuple('Chunk', 'lo hi count exit passes skip')


def radix_chunks(scores, index, ntot_, obj_thresh, maxc):
    """The chunk loop of the overflow branch's MSD radix select, run to the end of the candidates (the kernel stops earlier once max_out boxes
    are kept).  scores / index: the candidates of one class.  Yields the key interval [lo, hi) of every chunk, its candidate count, the exit its
    search took ('all fits', 'half full', 'single keys'), the histogram passes it needed and whether the same-score skip fired."""
    nbl = 11 if maxc >= 2048 else 10
    keys = sorted((key_of(s, i) for s, i in zip(scores, index)), reverse=True)
    key_min = int(np.asarray(max(float(F(obj_thresh)), 0.0), F).view(np.uint32)) << 32
    hi = (1 << 64) - 1
    while True:
        lo_c, hi_c, lo = key_min, hi, key_min
        if hi_c <= lo_c:
            return
        taken, passes, skip = 0, 0, False
        while True:
            rng = hi_c - lo_c
            bits = (rng - 1).bit_length() if rng > 1 else 0
            sh = bits - nbl if bits > nbl else 0
            nb = ((rng - 1) >> sh) + 1
            hist = collections.Counter((k - lo_c) >> sh for k in keys if lo_c <= k < hi_c)
            passes += 1
            run, cross = taken, None
            for q in sorted(hist, reverse=True):                      # the bins from the top
                if run + hist[q] > maxc:
                    cross = q
                    break
                run += hist[q]
            if cross is None:
                lo, how = lo_c, 'all fits'
                break
            b_lo = lo_c + (cross << sh)
            b_hi = hi_c if cross + 1 >= nb else b_lo + (1 << sh)
            taken = run
            if taken >= maxc // 2 or sh == 0:
                lo, how = b_hi, 'half full' if taken >= maxc // 2 else 'single keys'
                break
            lo_c, hi_c = b_lo, b_hi
            if (lo_c >> 32) == ((hi_c - 1) >> 32):
                first = (lo_c & 0xffffffff00000000) | (0x100000000 - ntot_)
                if lo_c < first < hi_c:
                    lo_c, skip = first, True
        if lo >= hi:
            return
        yield Chunk(lo, hi, sum(1 for k in keys if lo <= k < hi), how, passes, skip)
        if lo == key_min:
            return
        hi = lo


# ------------------------------------------------------------------------------------------------ the case table
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _mixed(rng, cls, b, c, n, levels=LEVELS):
    """n boxes drawn without order, each at one of `levels`: hundreds of exact ties per level, the order inside a level is the box index."""
    g = rng.permutation(cls.shape[1])[:n]
    cls[b, g, c] = rng.choice(np.asarray(levels, F), n)


def _sq(*sizes):
    return [(s, s) for s in sizes]


# anchors (w, h), image-relative.  16 x 16 cells are 16 px: a box of 1/16 fills its cell (neighbours touch: IoU 0), the half-width box inside it has
# IoU exactly 1/2 with it, boxes of 1/8 overlap their row / column neighbours by exactly 1/3, and a zero width gives zero-area boxes
AN1040 = [[(1 / 16, 1 / 16), (1 / 32, 1 / 16), (1 / 8, 1 / 8), (0.0, 1 / 16)]] * 2
# the same three relations on every scale of the three-scale head (cells of 32, 16 and 8 px)
AN3 = [[(c, c), (c / 2, c), (2 * c, 2 * c)] for c in (1 / 8, 1 / 16, 1 / 32)]
# heavy overlap: the boxes of the coarse scales cover the picture, those of the fine scale a quarter of it (three identical anchors); a few
# dozen of the 4032 survive, spread over the whole index range, so that no chunk and no sweep ends early
AN_GIANT = [_sq(1, 1, 1), _sq(1, 1, 1), _sq(1 / 2, 1 / 2, 1 / 2)]
# the same on the 1040-box head: few survivors, so a sweep or a greedy run visits every candidate before it stops
AN_GIANT1040 = [[(1, 1), (1, 1 / 2), (1 / 2, 1), (1 / 2, 1 / 2)]] * 2
# giants on the two coarse scales; on the 32 x 32 grid a cell-filling box, its exact twin (IoU 1) and a giant
AN_TWIN = [_sq(1 / 2, 1 / 2, 1 / 2), _sq(1 / 2, 1 / 2, 1 / 2), _sq(1 / 32, 1 / 32, 1 / 2)]
# the twin class below: cells of the 32 x 32 grid whose cell-filling box gets level 2 / 1 / 0 (its twin one level lower)
TWIN_CELLS = (200, 240)

Case = collections.namedtuple('Case', 'name head anchors obj iou max_out')


def _cls_t1088():
    rng = _rng('t1088')
    cls = np.full((2, ntot(H1040), 6), OFF, F)
    for c, n in enumerate((0, 1, 64, 65, 512, 513)):                  # image 0: the fast path up to its limit, the first sorted sweep
        _mixed(rng, cls, 0, c, n)
    for c, n in enumerate((1024, 1025, 1040)):                        # image 1: the last sweep of this template, then the greedy fallback
        _mixed(rng, cls, 1, c, n)
    cls[1, :, 3] = ON                                                 # every box at 1.0: the presorted tied sweep, one chunk of 1040
    cls[1, rng.permutation(1040)[:600], 4] = 1.0                      # tied, 600
    cls[1, rng.permutation(1040)[:512], 5] = 0.0                      # tied at exactly 0.5 (the fast path; `>=` at obj_thresh 0.5)
    return cls


def _cls_t2048():
    rng = _rng('t2048')
    cls = np.full((2, ntot(H3), 6), OFF, F)
    for c, n in enumerate((513, 1025, 2048, 2049, 4032)):             # image 0: class 5 stays empty next to the full class 4
        _mixed(rng, cls, 0, c, n)
    _mixed(rng, cls, 1, 0, 512)
    cls[1, :, 1] = ON                                                 # tied, 4032: two chunks
    cls[1, :, 2] = 1.0                                                # more than 2048 ties on one level under a few higher scores: the same-score skip
    cls[1, rng.permutation(4032)[:1032], 2] = OFF
    cls[1, rng.permutation(4032)[:5], 2] = 2.0
    g = rng.permutation(4032)                                         # 1500 above 2532: the first chunk ends 'half full' without a split
    cls[1, g[:1500], 3], cls[1, g[1500:], 3] = 2.0, -1.0
    cls[1, rng.permutation(4032)[:2048], 4] = -2.0                    # tied, 2048: one full chunk
    cls[1, rng.permutation(4032)[:2049], 5] = 2.0                     # tied, 2049: a second chunk of one candidate
    return cls


def _cls_giants():
    rng = _rng('giants')
    cls = np.full((2, ntot(H3), 6), OFF, F)
    cls[0, :, 0] = ON                                                 # tied, 4032 giants
    for c, n in enumerate((4032, 513, 1025, 2048, 2049), 1):
        _mixed(rng, cls, 0, c, n)
    cls[1, :, 0] = 2.0
    _mixed(rng, cls, 1, 1, 3000, (1.0, 2.0))
    return cls


def _cls_g1040():
    rng = _rng('g1040')
    cls = np.full((1, ntot(H1040), 6), OFF, F)
    for c, n in enumerate((512, 513, 1024, 1025, 1040)):
        _mixed(rng, cls, 0, c, n)
    cls[0, :, 5] = 2.0                                                # tied, 1040
    return cls


def _cls_twins():
    """Class 0, by descending level: 2 - the giants of the coarse scales and the cell boxes of cells [0, 200): a first chunk of 1160 candidates
    that keeps fewer than 256; 1 - those cells' twins (dead by the first chunk), the giants of the fine scale and the cell boxes of cells
    [200, 240): the second chunk takes the count past 256; 0 - the twins of [200, 240), which only selections number 257 and later suppress,
    and the remaining cell boxes; -1 - the remaining twins.  Class 1: every box at one score."""
    l, r, c, a = coords(H3)
    cell = r * 32 + c
    k0, k1 = TWIN_CELLS
    lv = np.full(ntot(H3), 2.0, F)
    fine = l == 2
    lv[fine & (a == 2)] = 1.0
    lv[fine & (a == 0)] = np.where(cell < k0, 2.0, np.where(cell < k1, 1.0, 0.0))[fine & (a == 0)]
    lv[fine & (a == 1)] = np.where(cell < k0, 1.0, np.where(cell < k1, 0.0, -1.0))[fine & (a == 1)]
    cls = np.full((1, ntot(H3), 2), OFF, F)
    cls[0, :, 0] = lv
    cls[0, :, 1] = ON
    return cls


def _cls_many():
    """Batch 14 x 20 classes on one 2 x 2 head (batch x classes = 280 > 256); images 2, 3, 7 and 13 have no detection."""
    rng = _rng('many')
    cls = np.full((14, ntot(H12), 20), OFF, F)
    for b in range(14):
        if b not in (2, 3, 7, 13):
            on = rng.random((12, 20)) < 0.3
            cls[b][on] = rng.choice(np.asarray(LEVELS, F), int(on.sum()))
    return cls


_TABLE = [
    # name, head, anchors, class logits, [(obj_thresh, iou_thresh, max_out), ...]
    ('t1088', H1040, AN1040, _cls_t1088, [(0.05, 0.5, 30), (0.05, HALF_BELOW, 30), (0.05, 0.3, 64), (0.05, 0.0, 30), (0.5, 0.5, 30), (0.05, 0.5, 65),
                                          (0.6, HALF_BELOW, 300)]),
    ('t2048', H3, AN3, _cls_t2048, [(0.05, 0.5, 30), (0.05, HALF_BELOW, 64), (0.05, 0.3, 30), (0.05, 0.0, 64), (0.5, 0.3, 30), (0.05, 0.5, 65),
                                    (0.05, 0.3, 100)]),
    ('g1040', H1040, AN_GIANT1040, _cls_g1040, [(0.05, 0.5, 64), (0.05, 0.5, 65), (0.05, 0.3, 30)]),
    ('giants', H3, AN_GIANT, _cls_giants, [(0.05, 0.5, 30), (0.05, 0.5, 64), (0.05, 0.5, 65), (0.6, 0.3, 64)]),
    ('twins', H3, AN_TWIN, _cls_twins, [(0.05, 0.5, 65), (0.05, 0.5, 256), (0.05, 0.5, 257), (0.05, 0.5, 300), (0.05, 0.5, 64)]),
    ('many', H12, [_sq(1 / 2, 1 / 4, 1 / 8)], _cls_many, [(0.05, 0.3, 3)]),
]


@functools.lru_cache(maxsize=None)
def _cls(name):
    a = next(t[3] for t in _TABLE if t[0] == name)()
    a.setflags(write=False)
    return a


CASES = [Case(name, head, np.asarray(anc, np.float64), obj, iou, mo) for name, head, anc, _, params in _TABLE for obj, iou, mo in params]
THRESHOLDS = sorted({c.obj for c in CASES})


def case_id(c):
    return f'{c.name}-obj{c.obj:g}-iou{c.iou:.9g}-max{c.max_out}'


def by_id(cid):
    return next(c for c in CASES if case_id(c) == cid)


def class_logits(c):
    return _cls(c.name)


@functools.lru_cache(maxsize=None)
def preds(name):
    c = next(x for x in CASES if x.name == name)
    p = build_preds(c.head, _cls(name))
    for a in p:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def boxes_scores(name):
    """decode_ref.decode_boxes_scores of every image: (boxes [B, ntot, 4], scores [B, ntot, C]), fp32."""
    c = next(x for x in CASES if x.name == name)
    p = preds(name)
    bs = [dr.decode_boxes_scores([q[b] for q in p], c.anchors, (S, S), (S, S)) for b in range(p[0].shape[0])]
    out = np.stack([x[0] for x in bs]), np.stack([x[1] for x in bs])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    """decode_ref.decode_batch_fast of the case, computed once: [(dets [k, 6], box index [k])] per image, read-only."""
    c = by_id(cid)
    ref = dr.decode_batch_fast(preds(c.name), c.anchors, (S, S), (S, S), c.obj, c.iou, c.max_out)
    for d, i in ref:
        d.setflags(write=False)
        i.setflags(write=False)
    return ref


Slot = collections.namedtuple('Slot', 'case image cls n tied path cand selected')


@functools.lru_cache(maxsize=None)
def slots(cid):
    """Every (image, class) of a case with its candidate count, tie flag and path label, from the oracle's scores alone; `cand` are the
    candidates' box indices, `selected` the oracle's selection in order."""
    c = by_id(cid)
    _, scores = boxes_scores(c.name)
    out = []
    for b, (d, idx) in enumerate(reference(cid)):
        for k in range(scores.shape[2]):
            s = scores[b, :, k]
            cand = np.flatnonzero(s >= F(c.obj))
            tied = cand.size > 0 and s[cand].min() == s[cand].max()
            out.append(Slot(cid, b, k, int(cand.size), bool(tied), nms_path(ntot(c.head), int(cand.size), c.max_out, bool(tied)), cand,
                            idx[d[:, 5] == k]))
    return out


def slot_chunks(s):
    """radix_chunks of an overflow slot, cut where the kernel stops (max_out kept), each with the count kept when the chunk is entered."""
    c = by_id(s.case)
    boxes, scores = boxes_scores(c.name)
    sc = scores[s.image, :, s.cls]
    sel_keys = [key_of(sc[g], g) for g in s.selected]
    out = []
    for ch in radix_chunks(sc[s.cand], s.cand, ntot(c.head), c.obj, s.path.template):
        before = sum(1 for k in sel_keys if k >= ch.hi)
        if before >= c.max_out:
            break
        out.append((ch, before))
    return out

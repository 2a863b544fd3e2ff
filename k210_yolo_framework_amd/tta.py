"""Test-time augmentation: the statement of the views and of the fusion that yk_letterbox_views_u8 (csrc/yk_pre.hip) and
yk_fuse_views (csrc/yk_tta.hip) are held to.

A picture goes through the network several times - as it is, left-right mirrored, shrunk - each view a network frame of its own; the rows the
decode leaves per frame are mapped back into the picture and fused: boxes the views agree on are averaged, weighted by their scores, and a
box only some of the views found loses confidence in proportion.  That is Weighted Boxes Fusion,
  R. Solovyev, W. Wang, T. Gabruseva: "Weighted boxes fusion: Ensembling boxes from different object detection models", Image and Vision
  Computing 107 (2021),
restated from the paper, with the view set YOLOv5's `--augment` made common (gains 1 / 0.83 / 0.67, the middle view mirrored: the alias v5).
PARITY UNPINNED: neither the authors' ensemble_boxes package nor YOLOv5 is on hand, and no number here is held to either (their per-model
weights, their 'max' and 'box_and_model_avg' variants, YOLOv5's rounding of the shrunk size to the stride are not reproduced).  What is pinned
is this module against a loop-per-box restatement and hand cases (tests/test_tta.py) and the kernels against this module, bit for bit
(tests/test_gpu_tta.py).  One rule only: no per-view weights, no variants.

Views.  A view of an h x w picture is (ch, cw, oy, ox, mirror): a zero canvas of ch x cw pixels with the picture pasted at row oy, column
ox, left-right mirrored if mirror is set; its network frame is yk_letterbox_u8 of that canvas.  For a gain g in (0, 1]: ch = ceil(h / g),
cw = ceil(w / g), oy = (ch - h) // 2, ox = (cw - w) // 2; g = 1 is the picture itself.  A gain above 1 is refused (enlarging is what TILES
is for).  The command line is a comma list, each item a gain with `f` appended for a mirrored view: `1,1f`; aliases flip = 1,1f and
v5 = 1,0.83f,0.67.

Mapping a row back.  A frame is decoded with image_hw = (ch, cw), so its rows (top, left, bottom, right, score, class) are in canvas
pixels.  Per frame the triple (dy, dx, mw) = (-oy, -ox, cw if mirror else -1) in float32: if mw >= 0, left' = mw - right and
right' = mw - left; then top, bottom += dy and left, right += dx.  Each step is one float32 operation.

fuse(), for one picture of N views.  Candidates are the rows of all views, view by view and in row order, mapped back.  A row whose class is
not exactly one of 0 .. class_num - 1, or whose score is not above 0 (a NaN included), is dropped.  Of a class's candidates the first
N * max_out in candidate order take part and the rest are ignored: the decode leaves at most max_out rows of a class per frame, so this binds
only on rows that are not decode-shaped (it is the room yk_fuse_views has for a class; include/yolo_hip.h).  Per class the candidates are walked by
score descending (ties: the lowest candidate index) against a list of clusters in creation order: the candidate's IoU with every cluster's
CURRENT fused box (softnms.iou_to_all's float32 expression, the decode's own); the best cluster is the one with the largest IoU (ties: the
lowest cluster index); if that IoU is > thresh (strict) the candidate joins it, otherwise it opens a new cluster.  A cluster carries, in
join order, sw += s; st += s*top, sl += s*left, sb += s*bottom, sr += s*right; ss += s; cnt += 1.  Its fused box is its member's box
verbatim while it has one member and (st/sw, sl/sw, sb/sw, sr/sw) afterwards; its score is (ss / F(cnt)) * F(min(cnt, N)) / F(N), left to
right - the paper's rescaling: a box one of three views found keeps a third of its confidence.  Output per class in ascending class order,
clusters by final score descending (ties: the lowest cluster index), at most max_out per class.
Every step is np.float32 with one rounding per operation.  numpy only; nothing here touches a GPU."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

from . import softnms

F = np.float32
MAX_VIEWS = 8
MAX_SIDE = 1 << 24                        # canvas sides must be exact in float32
DEFAULT_THRESH = 0.55
ALIASES = {'flip': '1,1f', 'v5': '1,0.83f,0.67'}

# yk_view_row_t
VIEW_DTYPE = np.dtype([('offset', '<u8'), ('h', '<i4'), ('w', '<i4'), ('ch', '<i4'), ('cw', '<i4'), ('oy', '<i4'), ('ox', '<i4'),
                       ('mirror', '<i4'), ('reserved', '<i4'), ('scale', '<f8'), ('tx', '<i4'), ('ty', '<i4')])
assert VIEW_DTYPE.itemsize == 56


def parse(text) -> Optional[Tuple[Tuple[float, bool], ...]]:
    """'1,0.83f,0.67' of the command line (or an alias) -> ((gain, mirror), ...); None, '', 'None', 'off' -> None."""
    if text is None or str(text) in ('', 'None', 'off'):
        return None
    items = ALIASES.get(str(text).strip().lower(), str(text)).split(',')
    spec = []
    for it in items:
        it = it.strip().lower()
        mirror = it.endswith('f')
        try:
            gain = float(it[:-1] if mirror else it)
        except ValueError:
            raise ValueError(f'tta {text!r}: item {it!r} is not a gain or a gain followed by f (for instance 1,0.83f,0.67; aliases: '
                             f'{", ".join(ALIASES)})') from None
        spec.append((gain, mirror))
    return tuple(spec)


def text_of(spec) -> str:
    """The command-line form of a spec."""
    return ','.join(f'{g:g}{"f" if m else ""}' for g, m in spec)


def check(tta, thresh: float = DEFAULT_THRESH, nms: str = 'hard', tiles=None) -> Optional[Tuple[Tuple[float, bool], ...]]:
    """The options of test-time augmentation, refused by name: -> None (off) or ((gain, mirror), ...).  `tta` is the command line's text or
    a sequence of (gain, mirror) pairs."""
    if tta is None:
        return None
    if isinstance(tta, str):
        spec = parse(tta)
        if spec is None:
            return None
    else:
        try:
            spec = tuple((float(g), m) for g, m in tta)
        except (TypeError, ValueError):
            raise ValueError(f'tta {tta!r}: expected (gain, mirror) pairs') from None
        if not all(isinstance(m, (bool, np.bool_)) for _, m in spec):
            raise ValueError(f'tta {tta!r}: mirror is True or False')
        spec = tuple((g, bool(m)) for g, m in spec)
    if not 1 <= len(spec) <= MAX_VIEWS:
        raise ValueError(f'tta {tta!r}: {len(spec)} views, expected 1 .. {MAX_VIEWS}')
    for g, _ in spec:
        if not (math.isfinite(g) and g > 0.0):
            raise ValueError(f'tta {tta!r}: gain {g!r} is not a positive number')
        if g > 1.0:
            raise ValueError(f'tta {tta!r}: gain {g:g} is above 1: a view only shrinks the picture; running parts of it enlarged is what tiles do')
    if len(set(spec)) != len(spec):
        raise ValueError(f'tta {tta!r}: a duplicate view would count one opinion twice')
    if not (isinstance(thresh, (int, float, np.floating, np.integer)) and np.isfinite(thresh) and thresh >= 0.0):
        raise ValueError(f'tta_thresh {thresh!r}: expected a finite number >= 0')
    if tiles is not None:
        raise ValueError('tta with tiles: the tile merge keeps one box of several (partial objects at tile borders must not be averaged) and the '
                         'fusion averages them; one picture takes one of the two')
    if nms != 'hard':
        raise ValueError(f"nms {nms!r} with tta: the fusion averages the undecayed scores of the views and would mix decayed ones; tta needs nms 'hard'")
    return spec


def add_arguments(p) -> None:
    """The command line of test-time augmentation (keras_detect.py, keras_eval.py)."""
    p.add_argument('--tta', type=str, default='None',
                   help='test-time augmentation: a comma list of gains in (0, 1], f appended for a mirrored view, e.g. 1,1f; aliases flip = 1,1f, '
                        'v5 = 1,0.83f,0.67 (default: off)')
    p.add_argument('--tta_thresh', type=float, default=DEFAULT_THRESH, help='boxes of different views are fused when their IoU is above this')


def parse_arguments(a) -> None:
    """Checks what add_arguments read (ValueError by name) and leaves a.tta as None or ((gain, mirror), ...)."""
    a.tta = check(str(a.tta), a.tta_thresh, getattr(a, 'nms', 'hard'), getattr(a, 'tiles', None))


def run_options(a) -> dict:
    """The keyword arguments detect.run takes, from parsed arguments."""
    return dict(tta=a.tta, tta_thresh=a.tta_thresh)


def rule_of(spec, thresh: float) -> dict:
    """What detections.json and eval.json say about the rule."""
    return dict(tta=text_of(spec), tta_views=[[float(g), bool(m)] for g, m in spec], tta_thresh=float(thresh))


def views(h: int, w: int, spec) -> np.ndarray:
    """int32 [V, 5] of (ch, cw, oy, ox, mirror), one row per (gain, mirror) of spec."""
    spec = check(spec)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'picture {h} x {w}: expected at least 1 x 1')
    rows = []
    for g, mirror in spec:
        ch, cw = (h, w) if g == 1.0 else (int(math.ceil(h / g)), int(math.ceil(w / g)))
        if ch >= MAX_SIDE or cw >= MAX_SIDE:
            raise ValueError(f'picture {h} x {w} at gain {g:g}: a canvas side of 2^24 or more has coordinates that float32 cannot hold exactly')
        rows.append((ch, cw, (ch - h) // 2, (cw - w) // 2, int(mirror)))
    return np.asarray(rows, np.int32).reshape(-1, 5)


def table_rows(v: np.ndarray, offset: int, h: int, w: int) -> np.ndarray:
    """The yk_view_row_t rows (VIEW_DTYPE; scale / tx / ty left 0) of the views `v` of an h x w picture stored [h][w][3] at byte `offset`."""
    v = np.asarray(v, np.int32).reshape(-1, 5)
    t = np.zeros(len(v), VIEW_DTYPE)
    t['offset'], t['h'], t['w'] = int(offset), int(h), int(w)
    for k, name in enumerate(('ch', 'cw', 'oy', 'ox', 'mirror')):
        t[name] = v[:, k]
    return t


def canvas(img: np.ndarray, view) -> np.ndarray:
    """The canvas a view denotes, built on the host: uint8 [ch, cw, 3]."""
    ch, cw, oy, ox, mirror = (int(x) for x in view)
    h, w = img.shape[:2]
    out = np.zeros((ch, cw, 3), np.uint8)
    out[oy:oy + h, ox:ox + w] = img[:, ::-1] if mirror else img
    return out


def xforms(v: np.ndarray) -> np.ndarray:
    """float32 [V, 3] of (dy, dx, mw) = (-oy, -ox, cw if mirror else -1).  (-0.0 for an offset of 0: x + -0.0 is x for every x.)"""
    v = np.asarray(v, np.int32).reshape(-1, 5)
    return np.stack([-v[:, 2].astype(F), -v[:, 3].astype(F), np.where(v[:, 4] != 0, v[:, 1], -1).astype(F)], 1).astype(F)


def map_back(rows: np.ndarray, xform) -> np.ndarray:
    """Rows of one frame in canvas pixels -> in the picture's pixels, float32 [k, 6]."""
    r = np.asarray(rows, F).reshape(-1, 6).copy()
    dy, dx, mw = (F(x) for x in np.asarray(xform, F).reshape(3))
    if mw >= 0:
        left, right = (mw - r[:, 3]).astype(F), (mw - r[:, 1]).astype(F)
        r[:, 1], r[:, 3] = left, right
    r[:, 0] = (r[:, 0] + dy).astype(F)
    r[:, 2] = (r[:, 2] + dy).astype(F)
    r[:, 1] = (r[:, 1] + dx).astype(F)
    r[:, 3] = (r[:, 3] + dx).astype(F)
    return r


def fuse(rows_per_view: Sequence[np.ndarray], xforms_, class_num: int, max_out: int, thresh: float):
    """The views of ONE picture -> (rows [k, 6] float32, candidate index of each cluster's first member [k] int64)."""
    xf = np.asarray(xforms_, F).reshape(-1, 3)
    if len(xf) != len(rows_per_view):
        raise ValueError(f'fuse: {len(rows_per_view)} views, {len(xf)} transforms')
    n_views = F(len(rows_per_view))
    cand = [map_back(r, x) for r, x in zip(rows_per_view, xf)]
    cand = np.concatenate(cand, 0) if cand else np.zeros((0, 6), F)
    thr = F(thresh)
    out_rows, out_idx = [], []
    for c in range(int(class_num)):
        with np.errstate(invalid='ignore'):
            mine = np.flatnonzero((cand[:, 5] == F(c)) & (cand[:, 4] > 0))
        if not len(mine):
            continue
        mine = mine[:len(rows_per_view) * int(max_out)]                   # more than N * max_out of a class: the first in candidate order
        mine = mine[np.argsort(-cand[mine, 4], kind='stable')]           # score descending, ties to the lowest candidate index
        box = np.zeros((len(mine), 4), F)                                 # per cluster: the current fused box,
        acc = np.zeros((len(mine), 4), F)                                 # st, sl, sb, sr,
        sw, ss = np.zeros(len(mine), F), np.zeros(len(mine), F)
        cnt = np.zeros(len(mine), np.int64)
        first = np.zeros(len(mine), np.int64)
        n = 0
        for i in mine:
            b, s = cand[i, :4], cand[i, 4]
            k = n
            if n:
                o = softnms.iou_to_all(np.concatenate([b[None], box[:n]]), 0, F)[0][1:]
                best = int(np.argmax(o))                                  # the largest IoU, ties to the lowest cluster index
                if o[best] > thr:
                    k = best
            if k == n:
                first[n] = i
                n += 1
            sw[k] = sw[k] + s
            acc[k] = (acc[k] + (s * b).astype(F)).astype(F)
            ss[k] = ss[k] + s
            cnt[k] += 1
            box[k] = b if cnt[k] == 1 else (acc[k] / sw[k]).astype(F)
        final = np.asarray([((ss[k] / F(cnt[k])) * F(min(cnt[k], n_views))) / n_views for k in range(n)], F)
        for k in np.argsort(-final, kind='stable')[:int(max_out)]:
            out_rows.append([*box[k], final[k], F(c)])
            out_idx.append(int(first[k]))
    if not out_rows:
        return np.zeros((0, 6), F), np.zeros((0,), np.int64)
    return np.asarray(out_rows, F).reshape(-1, 6), np.asarray(out_idx, np.int64)

"""Sliced inference: the statement of the tile grid and of the cross-tile merge that yk_letterbox_tiles_u8 (csrc/yk_pre.hip)
and yk_merge_tiles (csrc/yk_tiles.hip) are held to.

A picture is cut into nx x ny overlapping tiles; every tile, and with full=True the whole picture as well, goes through the network as a
frame of its own; the rows the decode leaves per frame are moved back by the tile's origin and the duplicates that overlapping tiles
produce are removed by one greedy hard NMS per class over all of them.  That is the recipe of
  F. C. Akyon, S. O. Altinuc, A. Temizel: "Slicing Aided Hyper Inference and Fine-tuning for Small Object Detection", ICIP 2022 (SAHI),
restated from the paper.  PARITY UNPINNED: SAHI's own code is not on hand, and no number here is held to it (its slice placement, its
greedy-NMM merging of boxes and its post-processing defaults are not reproduced).  What is pinned is this module against an independent
float64 restatement (tests/test_tiles.py) and the kernels against this module, bit for bit (tests/test_gpu_tiles.py).

The merge, for one picture.  Candidates are all rows of all its tiles, tile by tile and in row order inside a tile; a row is (top, left,
bottom, right, score, class) as the decode leaves it.  Each candidate is translated by ONE float32 add per coordinate (top, bottom: + y0;
left, right: + x0).  A row whose class is not one of 0 .. class_num - 1 exactly, or whose score is not above -inf (a NaN), is dropped.
Per class, greedy: the live candidate with the largest score (ties: the lowest candidate index) is kept; every live candidate whose match
with it is > thresh (strict) is retired; at most max_out are kept.  Output: class-major ascending, score-descending inside a class.
    iou   softnms.iou_to_all's float32 expression - the decode's own hard-NMS rule
    ios   the same intersection divided by the smaller of the two areas; a pair whose smaller area is not positive matches nothing
Every step is np.float32 with one rounding per operation.  numpy only; nothing here touches a GPU."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

from . import softnms

F = np.float32
METRICS = ('iou', 'ios')                  # position = YK_MATCH_* (include/yolo_hip.h)
MAX_N = 8                                 # tiles per side
MAX_SIDE = 1 << 24                        # origins must be exact in float32

# yk_tile_row_t
TILE_DTYPE = np.dtype([('offset', '<u8'), ('h', '<i4'), ('w', '<i4'), ('stride', '<i8'), ('scale', '<f8'), ('tx', '<i4'), ('ty', '<i4')])
assert TILE_DTYPE.itemsize == 40


def metric_id(name: str) -> int:
    if name not in METRICS:
        raise ValueError(f'tile_match {name!r}: expected one of {", ".join(METRICS)}')
    return METRICS.index(name)


def check(tiles, overlap: float = 0.2, match: str = 'ios', thresh: float = 0.5, nms: str = 'hard') -> Optional[Tuple[int, int]]:
    """The options of sliced inference, refused by name: -> None (off) or (nx, ny)."""
    if tiles is None:
        return None
    try:
        nx, ny = (int(v) for v in tiles)
        whole = all(float(v) == int(v) for v in tiles)
    except (TypeError, ValueError):
        raise ValueError(f'tiles {tiles!r}: expected (nx, ny)') from None
    if not whole or not (1 <= nx <= MAX_N and 1 <= ny <= MAX_N):
        raise ValueError(f'tiles {tiles!r}: nx and ny are whole numbers in 1 .. {MAX_N}')
    if not (isinstance(overlap, (int, float, np.floating, np.integer)) and 0.0 <= float(overlap) <= 0.5):
        raise ValueError(f'tile_overlap {overlap!r}: expected a number in [0, 0.5]')
    metric_id(match)
    if not (np.isfinite(thresh) and thresh >= 0.0):
        raise ValueError(f'tile_thresh {thresh!r}: expected a finite number >= 0')
    if nms != 'hard':
        raise ValueError(f"nms {nms!r} with tiles: the cross-tile merge is a hard rule over undecayed duplicates and would undo a soft decode; "
                         f"tiles need nms 'hard'")
    return nx, ny


def parse_tiles(text) -> Optional[Tuple[int, int]]:
    """'NXxNY' of the command line -> (nx, ny); '', 'None', 'off' -> None."""
    if text is None or str(text) in ('', 'None', 'off'):
        return None
    parts = str(text).lower().split('x')
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f'tiles {text!r}: expected NXxNY, for instance 2x2')
    return int(parts[0]), int(parts[1])


def add_arguments(p) -> None:
    """The command line of sliced inference (keras_detect.py, keras_eval.py)."""
    p.add_argument('--tiles', type=str, default='None', help='sliced inference: run every picture as NXxNY overlapping tiles, e.g. 2x2 (default: off)')
    p.add_argument('--tile_overlap', type=float, default=0.2, help='overlap of neighbouring tiles as a fraction of a tile side, 0 .. 0.5')
    p.add_argument('--tile_full', type=str, choices=['True', 'False'], default='True', help='also run the whole picture as a frame')
    p.add_argument('--tile_match', type=str, default='ios', help='match of the cross-tile merge: ios (intersection over the smaller box) or iou')
    p.add_argument('--tile_thresh', type=float, default=0.5, help='a duplicate is a box whose match with a kept one is above this')


def parse_arguments(a) -> None:
    """Checks what add_arguments read (ValueError by name) and leaves a.tiles as None or (nx, ny), a.tile_full as a bool."""
    a.tiles = parse_tiles(a.tiles)
    a.tile_full = a.tile_full in (True, 'True')
    check(a.tiles, a.tile_overlap, a.tile_match, a.tile_thresh, getattr(a, 'nms', 'hard'))


def run_options(a) -> dict:
    """The keyword arguments detect.run / evaluate.run take, from parsed arguments."""
    return dict(tiles=a.tiles, tile_overlap=a.tile_overlap, tile_full=a.tile_full, tile_match=a.tile_match, tile_thresh=a.tile_thresh)


def _axis(size: int, n: int, overlap: float):
    t = min(size, int(math.ceil(float(size) / (n - (n - 1) * float(overlap)))))
    return t, [(i * (size - t)) // (n - 1) if n > 1 else 0 for i in range(n)]


def grid(h: int, w: int, nx: int, ny: int, overlap: float, full: bool = True) -> np.ndarray:
    """int32 [T, 4] of (y0, x0, th, tw): with `full` the whole picture first, then the ny x nx tiles row-major (j outer, i inner)."""
    check((nx, ny), overlap)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'picture {h} x {w}: expected at least 1 x 1')
    if h >= MAX_SIDE or w >= MAX_SIDE:
        raise ValueError(f'picture {h} x {w}: a side of 2^24 or more has origins that float32 cannot hold exactly')
    tw, xs = _axis(w, int(nx), overlap)
    th, ys = _axis(h, int(ny), overlap)
    rows = [(0, 0, h, w)] if full else []
    rows += [(y0, x0, th, tw) for y0 in ys for x0 in xs]
    return np.asarray(rows, np.int32).reshape(-1, 4)


def table_rows(g: np.ndarray, offset: int, w: int) -> np.ndarray:
    """The yk_tile_row_t rows (TILE_DTYPE; scale / tx / ty left 0) of the tiles `g` of a picture of width w stored [h][w][3] at byte `offset`."""
    g = np.asarray(g, np.int64).reshape(-1, 4)
    t = np.zeros(len(g), TILE_DTYPE)
    t['offset'] = int(offset) + (g[:, 0] * int(w) + g[:, 1]) * 3
    t['h'], t['w'] = g[:, 2], g[:, 3]
    t['stride'] = 3 * int(w)
    return t


def match_to_all(boxes: np.ndarray, m: int, metric: str) -> np.ndarray:
    """The match of box m with every box, float32 [n]."""
    o, y0, x0, y1, x1 = softnms.iou_to_all(boxes, m, F)
    if metric == 'iou':
        return o
    metric_id(metric)
    area = ((y1 - y0).astype(F) * (x1 - x0).astype(F)).astype(F)
    iy0, ix0 = np.maximum(y0[m], y0), np.maximum(x0[m], x0)
    iy1, ix1 = np.minimum(y1[m], y1), np.minimum(x1[m], x1)
    inter = (np.maximum((iy1 - iy0).astype(F), F(0)) * np.maximum((ix1 - ix0).astype(F), F(0))).astype(F)
    small = np.minimum(area[m], area)
    ok = small > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(ok, (inter / np.where(ok, small, F(1))).astype(F), F(0)).astype(F)


def merge(rows_per_tile: Sequence[np.ndarray], origins, class_num: int, max_out: int, thresh: float, metric: str = 'ios'):
    """The tiles of ONE picture -> (rows [k, 6] float32, candidate index [k] int64)."""
    metric_id(metric)
    origins = np.asarray(origins, F).reshape(-1, 2)
    if len(origins) != len(rows_per_tile):
        raise ValueError(f'merge: {len(rows_per_tile)} tiles, {len(origins)} origins')
    cand = []
    for r, (y0, x0) in zip(rows_per_tile, origins):
        r = np.asarray(r, F).reshape(-1, 6).copy()
        r[:, 0] = (r[:, 0] + y0).astype(F)
        r[:, 2] = (r[:, 2] + y0).astype(F)
        r[:, 1] = (r[:, 1] + x0).astype(F)
        r[:, 3] = (r[:, 3] + x0).astype(F)
        cand.append(r)
    cand = np.concatenate(cand, 0) if cand else np.zeros((0, 6), F)
    thr = F(thresh)
    out_rows, out_idx = [], []
    for c in range(int(class_num)):
        with np.errstate(invalid='ignore'):
            mine = np.flatnonzero((cand[:, 5] == F(c)) & (cand[:, 4] > -np.inf))
        if not len(mine):
            continue
        boxes, score = cand[mine, :4], cand[mine, 4]
        live = np.ones(len(mine), bool)
        kept = 0
        while kept < max_out and live.any():
            m = int(np.flatnonzero(live & (score == score[live].max()))[0])          # largest score, lowest candidate index
            out_rows.append(cand[mine[m]])
            out_idx.append(int(mine[m]))
            kept += 1
            live[m] = False
            live &= ~(match_to_all(boxes, m, metric) > thr)
    if not out_rows:
        return np.zeros((0, 6), F), np.zeros((0,), np.int64)
    return np.asarray(out_rows, F).reshape(-1, 6), np.asarray(out_idx, np.int64)

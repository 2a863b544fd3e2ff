"""Mosaic augmentation (`make train MOSAIC=True`; not in the reference): every training sample is composed of four
pictures of the training list, each at its own scale, cropped at a random seam - YOLOv4 / YOLOv5's default augmentation, on a 1x canvas.

Draws.  Per (seed, epoch, dataset row), never from a per-process stream, like augment.py: a sample's mosaic does not depend on the rank,
the world size, the thread pool or the batch it lands in.  One table per epoch, `np.random.default_rng([seed, epoch, 2]).random((n_rows,
11))`, indexed by row of the training list; from a row's uniforms u0..u10:
  the sample is a mosaic iff u0 < prob
  seam      cx = floor(W*(0.25 + 0.5*u1)), cy = floor(H*(0.25 + 0.5*u2))            integers; H, W = in_hw[0]
  partners  p_j = min(floor(u_{3+j} * n_items), n_items - 1), j = 0..2               rows of the training list; repeats and the row itself allowed
  gains     g_k = 0.5 + 0.5*u_{6+k}, k = 0..3                                        one per quadrant
  the sample's own picture goes to quadrant q0 = min(floor(4*u10), 3), the partners fill the other quadrants in order.
Quadrants: 0 top left [0,cx) x [0,cy), 1 top right [cx,W) x [0,cy), 2 bottom left, 3 bottom right.

Geometry, float64, in this order, for the picture (sh, sw) of quadrant k:
  scale = g_k * s                       s: the letterbox scale of (sh, sw) -> (H, W), min(W/sw, H/sh) (Helper.letterbox_params)
  pw = sw*scale, ph = sh*scale
  tx = cx - (int)ceil(pw) in the left quadrants, cx in the right ones;  ty = cy - (int)ceil(ph) in the top quadrants, cy in the bottom ones
The corner of the scaled picture nearest the seam sits at the seam and the frame cuts off the rest: YOLOv5's placement on a 1x canvas.
tx and ty may be negative.  yk_mosaic_params (include/yolo_hip.h) is the same arithmetic in C.

Pixels.  Output pixel (x, y) belongs to the quadrant its coordinates fall in; its value is the letterbox pixel of that quadrant's picture
with (scale, tx, ty) - yk_letterbox_u8's arithmetic unchanged, truncating cast, taps outside the picture read 0.  Quadrant k of the frame
is helper.letterbox_bilinear(img_k, (H, W), scale, (tx, ty)) restricted to the quadrant, bit for bit.  A sample that is not a mosaic is
four rows naming the same picture with its plain letterbox (scale, tx, ty): its frame is yk_letterbox_u8's wherever the seam is.
The kernel is yk_mosaic_ragged_u8 (one launch per ragged batch), `compose_u8` below its host copy.

Boxes.  Quadrants in order 0..3, inside a picture in source order (the order matters: box_to_label lets a later box overwrite an earlier
one of the same cell).  The corners of [cls, x, y, w, h] (fractions of the source) in frame pixels, X0 = (x - w/2)*sw*scale + tx and
likewise the others; clipped to the closed quadrant rectangle; kept iff clipped width >= 2 px and clipped height >= 2 px and clipped area
>= 0.1 x unclipped area; back to centre / size fractions of (W, H).  A non-mosaic sample's boxes are pipeline.letterbox_boxes' output, bit
for bit, nothing dropped.

With the training augmentation as well (`IAA=True`) the warp of augment.py acts on the mosaic frame and augment_boxes_batch on these
boxes: letterbox first, then augment, as without mosaic.  Validation is never mosaicked.

Out of scope: colour jitter, mixup, per-picture flips inside a mosaic."""
from __future__ import annotations

import math
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MIN_SIDE_PX = 2.0          # a clipped box narrower or lower than this is dropped
MIN_AREA_KEPT = 0.1        # ... and one that keeps less than this share of its area

# one quadrant of one sample: the dataset row of its picture, the picture's size and where it goes (yk_ragged_row_t's scale, tx, ty)
ROW_DTYPE = np.dtype([('item', '<i8'), ('h', '<i4'), ('w', '<i4'), ('scale', '<f8'), ('tx', '<i4'), ('ty', '<i4')])


class MosaicConfig(NamedTuple):
    """InputPipeline(mosaic=MosaicConfig(prob)): the share of the samples that are mosaics."""
    prob: float = 1.0


def param_table(seed: int, epoch: int, n_rows: int) -> np.ndarray:
    """The epoch's [n_rows, 11] uniforms, indexed by dataset row."""
    return np.random.default_rng([int(seed), int(epoch), 2]).random((int(n_rows), 11))


def decode(u: np.ndarray, n_items: int, hw, prob: float = 1.0):
    """Rows of uniforms [n, 11] -> (is mosaic [n], seam [n, 2] = (cx, cy) int32, partners [n, 3], gains [n, 4], own quadrant [n])."""
    u = np.asarray(u, np.float64).reshape(-1, 11)
    H, W = float(hw[0]), float(hw[1])
    seam = np.stack([np.floor(W * (0.25 + 0.5 * u[:, 1])), np.floor(H * (0.25 + 0.5 * u[:, 2]))], 1).astype(np.int32)
    partners = np.minimum(np.floor(u[:, 3:6] * float(n_items)), float(n_items - 1)).astype(np.int64)
    return u[:, 0] < float(prob), seam, partners, 0.5 + 0.5 * u[:, 6:10], np.minimum(np.floor(4.0 * u[:, 10]), 3.0).astype(int)


def members(rows, table: np.ndarray, hw, prob: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """The dataset rows of the pictures of each sample, [n, 4] in quadrant order (a non-mosaic sample names its own row four times), and
    which samples are mosaics [n]: what a producer must decode before it can `plan`."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    is_mosaic, _, partners, _, q0 = decode(table[rows], len(table), hw, prob)
    items = np.repeat(rows[:, None], 4, axis=1)
    for b in np.nonzero(is_mosaic)[0]:
        items[b, [k for k in range(4) if k != q0[b]]] = partners[b]
    return items, is_mosaic


def letterbox_params(img_hw, hw) -> Tuple[float, int, int]:
    """Helper.letterbox_params / yk_letterbox_u8: (scale, tx, ty) of the plain letterbox of img_hw into hw."""
    sh, sw, H, W = float(img_hw[0]), float(img_hw[1]), float(hw[0]), float(hw[1])
    s = min(W / sw, H / sh)
    return s, int((W - sw * s) / 2.0), int((H - sh * s) / 2.0)


def quadrant_params(img_hw, k: int, cx: int, cy: int, gain: float, hw) -> Tuple[float, int, int]:
    """(scale, tx, ty) of the picture img_hw in quadrant k of a mosaic with seam (cx, cy): the module docstring's geometry."""
    scale = float(gain) * letterbox_params(img_hw, hw)[0]
    pw, ph = float(img_hw[1]) * scale, float(img_hw[0]) * scale
    return scale, (int(cx) if k & 1 else int(cx) - int(math.ceil(pw))), (int(cy) if k & 2 else int(cy) - int(math.ceil(ph)))


def quadrant_rect(k: int, cx: int, cy: int, hw) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((x0, x1), (y0, y1)) of quadrant k, half open in pixels; the seam clamped to the frame as the kernel clamps it."""
    H, W = int(hw[0]), int(hw[1])
    cx, cy = min(max(int(cx), 0), W), min(max(int(cy), 0), H)
    return (cx, W) if k & 1 else (0, cx), (cy, H) if k & 2 else (0, cy)


def _plain_boxes(boxes: np.ndarray, img_hw, scale: float, tx: int, ty: int, hw) -> np.ndarray:
    """pipeline.letterbox_boxes with its operations in its order."""
    boxes = np.array(boxes, np.float64, copy=True).reshape(-1, 5)
    if boxes.size:
        src_wh, net_wh = np.tile(np.array(img_hw[::-1], float), 2), np.tile(np.array([hw[1], hw[0]], float), 2)
        moved = boxes[:, 1:5] * src_wh * np.tile(np.full(2, scale), 2)
        moved[:, :2] += np.array([tx, ty])
        boxes[:, 1:5] = moved / net_wh
    return boxes


def quadrant_boxes(boxes: np.ndarray, img_hw, scale: float, tx: int, ty: int, k: int, cx: int, cy: int, hw) -> Tuple[np.ndarray, int]:
    """One picture's boxes [n, 5] (fractions of the source) in quadrant k -> (the surviving boxes as fractions of the frame, how many were
    dropped)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 5)
    H, W = float(hw[0]), float(hw[1])
    sh, sw = float(img_hw[0]), float(img_hw[1])
    (qx0, qx1), (qy0, qy1) = quadrant_rect(k, cx, cy, hw)
    X0, X1 = (b[:, 1] - b[:, 3] / 2) * sw * scale + tx, (b[:, 1] + b[:, 3] / 2) * sw * scale + tx
    Y0, Y1 = (b[:, 2] - b[:, 4] / 2) * sh * scale + ty, (b[:, 2] + b[:, 4] / 2) * sh * scale + ty
    x0, x1, y0, y1 = np.clip(X0, qx0, qx1), np.clip(X1, qx0, qx1), np.clip(Y0, qy0, qy1), np.clip(Y1, qy0, qy1)
    cw, ch = x1 - x0, y1 - y0
    keep = (cw >= MIN_SIDE_PX) & (ch >= MIN_SIDE_PX) & (cw * ch >= MIN_AREA_KEPT * ((X1 - X0) * (Y1 - Y0)))
    out = np.stack([b[:, 0], (x0 + x1) / 2 / W, (y0 + y1) / 2 / H, cw / W, ch / H], 1)
    return out[keep], int(len(b) - keep.sum())


def plan(rows, table: np.ndarray, shapes_of: Callable[[int], Tuple[int, int]], hw, boxes_of: Optional[Callable[[int], np.ndarray]] = None,
         prob: float = 1.0, dropped: Optional[List[int]] = None):
    """The samples of dataset rows `rows` under the epoch's `table`: -> (quadrant rows [n, 4] ROW_DTYPE, centres [n, 2] int32 = (cx, cy),
    box lists: per sample float64 [k, 5] relative to the frame).  shapes_of(item) gives a picture's (h, w) and boxes_of(item) its boxes
    [m, 5]; without boxes_of the box lists are empty.  `dropped`, a list, receives the number of boxes each sample lost to its seam."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    items, is_mosaic = members(rows, table, hw, prob)
    _, centres, _, gains, _ = decode(table[rows], len(table), hw, prob)
    quads = np.zeros((len(rows), 4), ROW_DTYPE)
    box_lists = []
    for b in range(len(rows)):
        cx, cy = int(centres[b, 0]), int(centres[b, 1])
        per, lost = [], 0
        for k in range(4):
            item = int(items[b, k])
            sh, sw = (int(v) for v in shapes_of(item)[:2])
            scale, tx, ty = quadrant_params((sh, sw), k, cx, cy, gains[b, k], hw) if is_mosaic[b] else letterbox_params((sh, sw), hw)
            quads[b, k] = (item, sh, sw, scale, tx, ty)
            if boxes_of is None or (k and not is_mosaic[b]):
                continue
            if is_mosaic[b]:
                kept, n_lost = quadrant_boxes(boxes_of(item), (sh, sw), scale, tx, ty, k, cx, cy, hw)
                per.append(kept)
                lost += n_lost
            else:
                per.append(_plain_boxes(boxes_of(item), (sh, sw), scale, tx, ty, hw))
        box_lists.append(np.concatenate(per) if per else np.zeros((0, 5)))
        if dropped is not None:
            dropped.append(lost)
    return quads, centres, box_lists


def _letterbox_rect(img: np.ndarray, x0: int, x1: int, y0: int, y1: int, scale: float, tx: int, ty: int) -> np.ndarray:
    """helper.letterbox_bilinear's arithmetic for the output pixels [y0, y1) x [x0, x1) only."""
    ih, iw = img.shape[:2]
    inv = 1.0 / float(scale)
    c = inv * np.arange(x0, x1, dtype=np.float64) + (-(float(tx) * inv))
    r = inv * np.arange(y0, y1, dtype=np.float64) + (-(float(ty) * inv))
    c_lo, c_hi, r_lo, r_hi = np.floor(c), np.ceil(c), np.floor(r), np.ceil(r)
    dc, dr = (c - c_lo)[None, :, None], (r - r_lo)[:, None, None]
    src = img.astype(np.float64)

    def corner(rr, cc):
        rr, cc = rr.astype(int), cc.astype(int)
        live = ((rr >= 0) & (rr < ih))[:, None] & ((cc >= 0) & (cc < iw))[None, :]
        return np.where(live[..., None], src[rr.clip(0, ih - 1)[:, None], cc.clip(0, iw - 1)[None, :]], 0.0)
    top = (1 - dc) * corner(r_lo, c_lo) + dc * corner(r_lo, c_hi)
    bottom = (1 - dc) * corner(r_hi, c_lo) + dc * corner(r_hi, c_hi)
    return ((1 - dr) * top + dr * bottom).astype('uint8')


def compose_u8(images4: Sequence[Optional[np.ndarray]], rows4, centre, hw) -> np.ndarray:
    """Host copy of yk_mosaic_ragged_u8 for one sample without a warp: the four pictures [h, w, 3] uint8 (None: a row the kernel would
    refuse, its quadrant zeros), their rows (fields scale, tx, ty) and the seam (cx, cy) -> the frame uint8 [H, W, 3]."""
    out = np.zeros((int(hw[0]), int(hw[1]), 3), np.uint8)
    for k in range(4):
        (x0, x1), (y0, y1) = quadrant_rect(k, centre[0], centre[1], hw)
        if images4[k] is None or x1 <= x0 or y1 <= y0:
            continue
        out[y0:y1, x0:x1] = _letterbox_rect(np.asarray(images4[k])[..., :3], x0, x1, y0, y1, float(rows4[k]['scale']), int(rows4[k]['tx']),
                                            int(rows4[k]['ty']))
    return out


def ragged_rows(quads: np.ndarray, offset_of) -> np.ndarray:
    """Quadrant rows [n, 4] -> the kernel's table, draw.RAGGED_DTYPE [n * 4]: offset_of(item) is the byte offset of a picture in the packed
    buffer."""
    from .draw import RAGGED_DTYPE
    q = np.asarray(quads).reshape(-1)
    t = np.zeros(len(q), RAGGED_DTYPE)
    t['offset'] = [offset_of(int(i)) for i in q['item']]
    for f in ('h', 'w', 'scale', 'tx', 'ty'):
        t[f] = q[f]
    return t

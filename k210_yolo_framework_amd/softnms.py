"""Soft-NMS and DIoU-NMS per (image, class): the statement of the rule and the product's host copy of softnms_py_kernel (csrc/yk_decode.hip).

The rule restates
  N. Bodla, B. Singh, R. Chellappa, L. Davis: "Soft-NMS - Improving Object Detection With One Line of Code", ICCV 2017 (`linear`, `gaussian`);
  Z. Zheng, P. Wang, W. Liu, J. Li, R. Ye, D. Ren: "Distance-IoU Loss: Faster and Better Learning for Bounding Box Regression", AAAI 2020,
  section "DIoU-NMS" (`diou`).
PARITY UNPINNED: neither the authors' code nor torchvision, mmcv or any other implementation is on hand; no number here is held to theirs.
What is pinned is this module against hand-derived answers (tests/test_softnms_rule.py) and the kernel against this module
(tests/test_gpu_softnms.py).

One (image, class).  The candidates are the boxes with score >= obj_thresh; each one's CURRENT score starts as its score.  While a live
candidate exists and fewer than max_out rows are emitted:
    m = the live candidate with the largest current score (exact ties: the lowest box index);  emit (m, cur[m]);  retire m
    for every live i:  cur[i] = cur[i] * f(b_m, b_i)       one multiply
    retire every i with cur[i] < obj_thresh, and every i whose weight f was 0 (at a positive obj_thresh the second is the first)
Emitted rows carry the CURRENT, decayed score, in emission order.

o = tf_iou: the operations and order of oracle/decode_ref.py::tf_iou (corners normalised by min / max, zero or negative area gives 0).
    linear    f = 1 - o  if o > iou_thresh (strict), else 1
    gaussian  f = exp(-(o * o) / sigma)  for every o (no threshold, as in the paper);  sigma > 0
    diou      f = 0  if o - d2 / c2 > iou_thresh, else 1     (scores never decay)
    hard      f = 0  if o > iou_thresh, else 1               (the existing rule, here for the tests only)
DIoU's terms, from the normalised corners (y0, x0, y1, x1) of m and i, one rounding per operation, in this order:
    dy = (y0m + y1m) * 0.5 - (y0i + y1i) * 0.5        dx likewise        d2 = dy * dy + dx * dx
    ey = max(y1m, y1i) - min(y0m, y0i)                ex likewise        c2 = ey * ey + ex * ex
    penalty = d2 / c2 if c2 > 0 else 0

Every step is np.float32 with one rounding per operation (dtype=np.float64 runs the same steps in double: the tests' yardstick for the
Gaussian scores).  numpy only; nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

F = np.float32
METHODS = ('hard', 'linear', 'gaussian', 'diou')        # position = YK_NMS_* (include/yolo_hip.h)
DEFAULT_SIGMA = 0.5


def method_id(name: str) -> int:
    if name not in METHODS:
        raise ValueError(f'nms {name!r}: expected one of {", ".join(METHODS)}')
    return METHODS.index(name)


def check(name: str, sigma: float) -> None:
    """Refuse an unknown rule or a sigma the Gaussian cannot use, by name."""
    method_id(name)
    if name == 'gaussian' and not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f'nms_sigma {sigma!r}: expected a positive, finite number')


def iou_to_all(boxes: np.ndarray, m: int, dtype=F):
    """tf_iou of box m with every box, and the normalised corners -> (o [n], y0, x0, y1, x1)."""
    b = np.asarray(boxes, dtype)
    y0, x0 = np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3])
    y1, x1 = np.maximum(b[:, 0], b[:, 2]), np.maximum(b[:, 1], b[:, 3])
    area = ((y1 - y0).astype(dtype) * (x1 - x0).astype(dtype)).astype(dtype)
    iy0, ix0 = np.maximum(y0[m], y0), np.maximum(x0[m], x0)
    iy1, ix1 = np.minimum(y1[m], y1), np.minimum(x1[m], x1)
    zero = dtype(0)
    inter = (np.maximum((iy1 - iy0).astype(dtype), zero) * np.maximum((ix1 - ix0).astype(dtype), zero)).astype(dtype)
    union = ((area[m] + area).astype(dtype) - inter).astype(dtype)
    ok = (area[m] > 0) & (area > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        o = np.where(ok, (inter / np.where(ok, union, dtype(1))).astype(dtype), zero).astype(dtype)
    return o, y0, x0, y1, x1


def weights(boxes: np.ndarray, m: int, method: str, iou_thresh: float, sigma: float = DEFAULT_SIGMA, dtype=F) -> np.ndarray:
    """f(b_m, b_i) for every i."""
    o, y0, x0, y1, x1 = iou_to_all(boxes, m, dtype)
    one, thr = dtype(1), dtype(F(iou_thresh))
    if method == 'hard':
        return np.where(o > thr, dtype(0), one).astype(dtype)
    if method == 'linear':
        return np.where(o > thr, (one - o).astype(dtype), one).astype(dtype)
    if method == 'gaussian':
        return np.exp((-((o * o).astype(dtype)) / dtype(F(sigma))).astype(dtype), dtype=dtype)
    if method == 'diou':
        half = dtype(0.5)
        dy = (((y0[m] + y1[m]).astype(dtype) * half).astype(dtype) - ((y0 + y1).astype(dtype) * half).astype(dtype)).astype(dtype)
        dx = (((x0[m] + x1[m]).astype(dtype) * half).astype(dtype) - ((x0 + x1).astype(dtype) * half).astype(dtype)).astype(dtype)
        d2 = ((dy * dy).astype(dtype) + (dx * dx).astype(dtype)).astype(dtype)
        ey = (np.maximum(y1[m], y1) - np.minimum(y0[m], y0)).astype(dtype)
        ex = (np.maximum(x1[m], x1) - np.minimum(x0[m], x0)).astype(dtype)
        c2 = ((ey * ey).astype(dtype) + (ex * ex).astype(dtype)).astype(dtype)
        pos = c2 > 0
        pen = np.where(pos, (d2 / np.where(pos, c2, one)).astype(dtype), dtype(0)).astype(dtype)
        return np.where((o - pen).astype(dtype) > thr, dtype(0), one).astype(dtype)
    raise ValueError(f'nms {method!r}: expected one of {", ".join(METHODS)}')


def soft_nms(boxes: np.ndarray, scores: np.ndarray, obj_thresh: float, iou_thresh: float, sigma: float = DEFAULT_SIGMA, max_out: int = 30,
             method: str = 'linear', dtype=F, trace=None):
    """One (image, class).  boxes [n, 4] = ymin, xmin, ymax, xmax, scores [n] -> (box indices [k] int64, current scores [k]) in emission
    order.  trace: a list that receives, per round, the live current scores before the selection (for the tests' input conditions)."""
    check(method, sigma)
    boxes = np.asarray(boxes, F).astype(dtype)
    cur = np.asarray(scores, F).astype(dtype).copy()
    floor = dtype(F(obj_thresh))
    live = cur >= floor
    sel, out = [], []
    while len(sel) < max_out and live.any():
        if trace is not None:
            trace.append(cur[live].copy())
        m = int(np.flatnonzero(live & (cur == cur[live].max()))[0])           # largest current score, lowest index
        sel.append(m)
        out.append(cur[m])
        live[m] = False
        w = weights(boxes, m, method, iou_thresh, sigma, dtype)
        if method not in ('hard', 'diou'):
            cur[live] = (cur[live] * w[live]).astype(dtype)
        live &= ~((cur < floor) | (w == 0))
    return np.asarray(sel, np.int64), np.asarray(out, dtype)


def decode_image(boxes: np.ndarray, scores: np.ndarray, obj_thresh: float, iou_thresh: float, max_out: int = 30, method: str = 'linear',
                 sigma: float = DEFAULT_SIGMA, dtype=F):
    """One image: boxes [n, 4], scores [n, C] as the decode leaves them -> (rows [k, 6] = top, left, bottom, right, current score, class;
    box index [k]), classes concatenated class-major as yk_decode_py does."""
    rows, idxs = [], []
    for c in range(scores.shape[1]):
        sel, cs = soft_nms(boxes, scores[:, c], obj_thresh, iou_thresh, sigma, max_out, method, dtype)
        for g, s in zip(sel, cs):
            rows.append([*np.asarray(boxes[g], dtype), s, dtype(c)])
            idxs.append(g)
    if not rows:
        return np.zeros((0, 6), dtype), np.zeros((0,), np.int64)
    return np.asarray(rows, dtype), np.asarray(idxs, np.int64)

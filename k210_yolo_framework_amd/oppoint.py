"""Operating points of a detector: precision / recall / F1 over a sweep of confidence thresholds, the best-F1 threshold per class and over
all classes, and a confusion matrix at one threshold - the statement `map_gpu.MapEvaluator.sweep` / `.confusion` (csrc/yk_map.hip; DESIGN.md
3.24) are held to, as voc_eval.py is for `result()` and coco_eval.py for `coco_result()`.

The rule is this project's own, in the spirit of the P / R / F1 curves and the confusion matrix YOLOv5's `val.py` prints.  It is EXACT
COUNTING at every threshold, not their curves interpolated onto 1000 points and smoothed, and the confusion matrix's matching is stated
below, not copied: parity with their numbers is unpinned.

Row formats are voc_eval.evaluate's: (top, left, bottom, right, score, class); the class is read with `astype(int)`; a class outside
[0, class_num) belongs nowhere.  Pure numpy, float64, no torch.

sweep       Every detection row gets the flag voc_eval.evaluate's matching gives it (0 ignored, 1 true positive, 2 false positive: the
            meaning of MapEvaluator.result()['flags']).  A row is IN at threshold t if float64(score) >= t (so -0.0 is in at 0.0 and a
            score equal to the threshold is in).  Per class c and threshold k: tp, fp = the in-rows of the class with flag 1 / 2; n_gt the
            non-difficult boxes; precision = tp / (tp + fp), exactly 1.0 when tp + fp == 0; recall = tp / n_gt, NaN when n_gt == 0;
            f1 = ((2.0 * p) * r) / (p + r), exactly 0.0 when p + r == 0, NaN when n_gt == 0 - each one chain of float64 operations in that
            order.  best[c] = the lowest k with the largest f1[c, k] (-1 when n_gt == 0); mean_f1[k] = the f1[c, k] of the classes with
            n_gt > 0 added one after another in ascending class order, divided by their number (NaN if there are none); best_all = the
            lowest k with the largest mean_f1 (-1 if there are none).

            Because the matching walks the rows of a class in descending score, the flags of the rows at or above t do not depend on the rows
            below it: tp[:, k] and fp[:, k] are voc_eval.evaluate(...)['tp'] and ['fp'] of the list cut at score >= t_k
            (tests/test_oppoint.py holds this at every threshold).

confusion   Per image and class-agnostic.  Taking part: the rows with float64(score) >= conf_thresh and a class in range, and every
            ground-truth box with a class in range, difficult or not.  Candidate pairs (row, box) have voc_eval.box_iou >= iou_thresh.
            Greedy one-to-one matching: among the pairs whose row and box are both still free take the best one, repeatedly; best = the
            largest IoU, then the larger score (-0.0 == +0.0), then the lower row index, then the lower box index.  matrix[true][predicted],
            index class_num = background: a pair matched to a non-difficult box counts at [box class][row class], a pair matched to a
            difficult box counts nowhere, an unmatched row at [class_num][row class], an unmatched non-difficult box at
            [box class][class_num], an unmatched difficult box nowhere."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .voc_eval import box_iou

MAX_THRESHOLDS = 4096


def _rows2d(a) -> np.ndarray:
    a = np.asarray(a, np.float64)
    if a.size == 0:
        return np.zeros((0, 6))
    return a[None] if a.ndim == 1 else a


def _inputs(detections, ground_truth, difficult):
    if len(detections) != len(ground_truth):
        raise ValueError(f'{len(detections)} images of detections, {len(ground_truth)} of ground truth')
    dets = [_rows2d(d) for d in detections]
    gts = [_rows2d(g) for g in ground_truth]
    diff = [np.zeros(len(g), bool) if difficult is None else np.asarray(difficult[i], bool).reshape(-1) for i, g in enumerate(gts)]
    return dets, gts, diff


def check_thresholds(thresholds) -> np.ndarray:
    """-> float64 [n]; ValueError unless finite, strictly ascending and 1 <= n <= 4096."""
    t = np.asarray(thresholds, np.float64)
    if t.ndim != 1:
        raise ValueError(f'thresholds of shape {t.shape}: expected one dimension')
    if len(t) < 1:
        raise ValueError('thresholds: empty')
    if len(t) > MAX_THRESHOLDS:
        raise ValueError(f'thresholds: {len(t)} values, more than {MAX_THRESHOLDS}')
    if not np.all(np.isfinite(t)):
        raise ValueError('thresholds: not finite')
    if np.any(np.diff(t) <= 0):
        raise ValueError('thresholds: not strictly ascending')
    return t


def flags_of(detections: Sequence[np.ndarray], ground_truth: Sequence[np.ndarray], class_num: int, iou_thresh: float = 0.5,
             difficult: Optional[Sequence[np.ndarray]] = None, plus_one: bool = False):
    """voc_eval.evaluate's matching -> (flags [rows] uint8 in insertion order: 0 ignored, 1 tp, 2 fp; n_gt [class_num])."""
    dets, gts, diff = _inputs(detections, ground_truth, difficult)
    first = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(int)
    flags = np.zeros(int(first[-1]), np.uint8)
    n_gt = np.zeros(class_num, int)
    for c in range(class_num):
        rows = []
        for i, d in enumerate(dets):
            for k in np.nonzero(d[:, 5].astype(int) == c)[0]:
                rows.append((d[k, 4], i, int(k)))
        sel = [g[:, -1].astype(int) == c if len(g) else np.zeros(0, bool) for g in gts]
        n_gt[c] = sum(int((~diff[i][s]).sum()) for i, s in enumerate(sel))
        taken = [np.zeros(int(s.sum()), bool) for s in sel]
        for k in sorted(range(len(rows)), key=lambda k: -rows[k][0]):           # descending score; ties keep image / row order
            _, i, j = rows[k]
            boxes = gts[i][sel[i], :4]
            best, b = -1.0, -1
            if len(boxes):
                iou = box_iou(dets[i][j, :4], boxes, plus_one)
                b = int(np.argmax(iou))
                best = float(iou[b])
            f = 2
            if best >= iou_thresh:
                if diff[i][sel[i]][b]:
                    f = 0
                elif not taken[i][b]:
                    f = 1
                    taken[i][b] = True
            flags[first[i] + j] = f
    return flags, n_gt


def sweep(detections: Sequence[np.ndarray], ground_truth: Sequence[np.ndarray], class_num: int, thresholds, iou_thresh: float = 0.5,
          difficult: Optional[Sequence[np.ndarray]] = None, plus_one: bool = False) -> Dict[str, object]:
    """-> {'thresholds' [n], 'tp', 'fp' [class_num, n] int, 'n_gt' [class_num] int, 'precision', 'recall', 'f1' [class_num, n] float64,
    'best' [class_num] int, 'mean_f1' [n] float64, 'best_all' int, 'flags' [rows] uint8}: the module docstring's rule."""
    thr = check_thresholds(thresholds)
    n = len(thr)
    flags, n_gt = flags_of(detections, ground_truth, class_num, iou_thresh, difficult, plus_one)
    dets = [_rows2d(d) for d in detections]
    rows = np.concatenate(dets) if dets else np.zeros((0, 6))
    cls = rows[:, 5].astype(int)
    score = rows[:, 4]
    # a row of score s is in at the first j thresholds, j = the number of thresholds <= s: count rows per (class, j - 1), then add from the top
    j = np.searchsorted(thr, score, side='right')
    tp, fp = np.zeros((class_num, n), int), np.zeros((class_num, n), int)
    for out, flag in ((tp, 1), (fp, 2)):
        for c in range(class_num):
            at = j[(cls == c) & (flags == flag) & (j > 0)] - 1
            out[c] = np.cumsum(np.bincount(at, minlength=n)[::-1])[::-1]
    # elementwise float64: every entry is the one chain of operations the docstring states
    with np.errstate(divide='ignore', invalid='ignore'):
        t, den = tp.astype(np.float64), (tp + fp).astype(np.float64)
        precision = np.where(tp + fp == 0, 1.0, t / den)
        no_gt = (n_gt == 0)[:, None]
        recall = np.where(no_gt, np.nan, t / n_gt.astype(np.float64)[:, None])
        pr = precision + recall
        f1 = np.where(no_gt, np.nan, np.where(pr == 0, 0.0, ((2.0 * precision) * recall) / pr))
    best = np.array([int(np.argmax(f1[c])) if n_gt[c] else -1 for c in range(class_num)], int)      # the first of equal values
    have = [c for c in range(class_num) if n_gt[c] > 0]
    mean_f1 = np.full(n, np.nan)
    if have:
        s = np.zeros(n)
        for c in have:                                                           # ascending class order, one after another
            s = s + f1[c]
        mean_f1 = s / np.float64(len(have))
    best_all = int(np.argmax(mean_f1)) if have else -1
    return {'thresholds': thr, 'tp': tp, 'fp': fp, 'n_gt': n_gt, 'precision': precision, 'recall': recall, 'f1': f1, 'best': best,
            'mean_f1': mean_f1, 'best_all': best_all, 'flags': flags}


def confusion(detections: Sequence[np.ndarray], ground_truth: Sequence[np.ndarray], class_num: int, conf_thresh: float,
              iou_thresh: float = 0.5, difficult: Optional[Sequence[np.ndarray]] = None, plus_one: bool = False) -> Dict[str, np.ndarray]:
    """-> {'matrix' [class_num + 1, class_num + 1] int, [true][predicted], index class_num = background; 'match' [rows] int: the row's box in
    the concatenated ground truth, -1 unmatched, -2 the row takes no part}: the module docstring's rule."""
    dets, gts, diff = _inputs(detections, ground_truth, difficult)
    K = int(class_num)
    matrix = np.zeros((K + 1, K + 1), int)
    match = []
    g_first = 0
    for i, (d, g) in enumerate(zip(dets, gts)):
        dc = d[:, 5].astype(int) if len(d) else np.zeros(0, int)
        gc = g[:, -1].astype(int) if len(g) else np.zeros(0, int)
        score = d[:, 4] if len(d) else np.zeros(0)
        d_in = (score >= conf_thresh) & (dc >= 0) & (dc < K)
        g_in = (gc >= 0) & (gc < K)
        m = np.where(d_in, -1, -2).astype(int)
        pairs = []
        for r in np.nonzero(d_in)[0]:
            if not g_in.any():
                break
            iou = box_iou(d[r, :4], g[:, :4], plus_one)
            for b in np.nonzero(g_in & (iou >= iou_thresh))[0]:
                pairs.append((-float(iou[b]), -(float(score[r]) + 0.0), int(r), int(b)))
        row_free, box_free = d_in.copy(), g_in.copy()
        for _, _, r, b in sorted(pairs):                                         # best first: IoU, score, lower row, lower box
            if row_free[r] and box_free[b]:
                row_free[r] = box_free[b] = False
                m[r] = g_first + b
                if not diff[i][b]:
                    matrix[gc[b], dc[r]] += 1
        for r in np.nonzero(row_free)[0]:
            matrix[K, dc[r]] += 1
        for b in np.nonzero(box_free)[0]:
            if not diff[i][b]:
                matrix[gc[b], K] += 1
        match.append(m)
        g_first += len(g)
    return {'matrix': matrix, 'match': np.concatenate(match).astype(int) if match else np.zeros(0, int)}

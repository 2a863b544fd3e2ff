"""COCO-style detection metric (AP averaged over IoU 0.50:0.95, AP50, AP75, AP by object size, AR) for the rows this package's decode
produces - the host statement `map_gpu.MapEvaluator.coco_result` (csrc/yk_map.hip) is held to, as `voc_eval.evaluate`
is for the VOC metric.

pycocotools is not a dependency of this project; the rule is restated here from its public source (cocoeval.py: evaluateImg, accumulate,
summarize).  PARITY WITH pycocotools' OWN NUMBERS IS UNPINNED: nothing here has been run against it.  Where this statement knowingly
differs from COCO's use of it:

  * `difficult` plays the role of COCO's `ignore`; there are no crowd boxes (a crowd box may absorb several detections, an ignored box
    here is used up by one);
  * the area of an object is its BOX area (COCO uses the mask area of the annotation), in the pixels the rows are in - COCO's limits
    32^2 and 96^2 are meant in source-image pixels;
  * AR is taken at `max_dets` only (no AR@1 / AR@10).

The rule, float64 throughout, with T thresholds, A area ranges [a0, a1], R = 101 recall points:

  * a ground-truth box is IGNORED under range a if it is `difficult` or its area (bottom - top) * (right - left) is < a0 or > a1;
  * per (image, class) the detections are taken in descending score (stable: ties in row order); only the first `max_dets` take part,
    the others get flag 0 everywhere and are counted nowhere;
  * per (t, a), each detection in that order looks at the boxes of its image and class that are not yet matched at (t, a) and have
    IoU >= min(t, 1 - 1e-10) (voc_eval.box_iou, plus_one=False): the non-ignored one with the largest IoU if there is any, otherwise the
    ignored one with the largest IoU; on equal IoU the HIGHEST index wins (pycocotools' loop replaces on `>=`).  The chosen box is matched
    (an ignored box is used up too).  Matched to a non-ignored box: true positive, flag 1; matched to an ignored box: flag 0; unmatched
    with its own area outside [a0, a1]: flag 0; unmatched otherwise: false positive, flag 2.
    (The VOC rule takes the argmax over ALL boxes and calls a detection whose best box is taken a false positive; this one falls back
    to the next free box.)
  * per (class k, t, a), rows of the class over all images in stable descending score (ties in (image, row) order):
    npig = the non-ignored boxes of the class under a; npig == 0: every entry -1 (absent).  Otherwise, tp / fp the running counts of
    flags 1 / 2:  rc = tp / npig;  pr = tp / ((fp + tp) + eps), eps = 2.220446049250313e-16 ADDED;  recall[t,k,a] = rc[-1] (0 without
    rows);  pr <- its reverse running maximum;  precision[t,r,k,a] = pr[searchsorted(rc, REC_THRS[r], 'left')], 0 past the end.
  * every summary figure is the mean of the entries > -1 of its slice, NaN if there are none.

Row format: (top, left, bottom, right, score, class), as voc_eval.  Pure numpy."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .voc_eval import box_iou

REC_THRS = np.linspace(0.0, 1.0, 101)
EPS = 2.220446049250313e-16
SUMMARY = ('ap', 'ap50', 'ap75', 'ap_small', 'ap_medium', 'ap_large', 'ar', 'ar_small', 'ar_medium', 'ar_large')


def default_iou_thresholds() -> np.ndarray:
    return np.linspace(0.5, 0.95, 10)


def default_area_ranges() -> np.ndarray:
    return np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)


def _mean_present(s: np.ndarray) -> float:
    s = np.asarray(s, np.float64)
    s = s[s > -1]
    return float(s.mean()) if s.size else float('nan')


def summarize(precision: np.ndarray, recall: np.ndarray, iou_thresholds: np.ndarray) -> Dict[str, object]:
    """The ten summary figures and ap_class [K] of precision [T,R,K,A] / recall [T,K,A]."""
    thr = np.asarray(iou_thresholds, np.float64).reshape(-1)
    T, _, K, A = precision.shape
    out: Dict[str, object] = {}
    at = lambda v: np.nonzero(thr == v)[0]
    rng = lambda a: slice(a, a + 1) if a < A else slice(0, 0)
    out['ap'] = _mean_present(precision[:, :, :, rng(0)])
    out['ap50'] = _mean_present(precision[at(0.5)][:, :, :, rng(0)])
    out['ap75'] = _mean_present(precision[at(0.75)][:, :, :, rng(0)])
    for a, name in ((1, 'small'), (2, 'medium'), (3, 'large')):
        out['ap_' + name] = _mean_present(precision[:, :, :, rng(a)])
    out['ar'] = _mean_present(recall[:, :, rng(0)])
    for a, name in ((1, 'small'), (2, 'medium'), (3, 'large')):
        out['ar_' + name] = _mean_present(recall[:, :, rng(a)])
    out['ap_class'] = np.array([_mean_present(precision[:, :, k, rng(0)]) for k in range(K)], np.float64)
    return out


def evaluate(detections: Sequence[np.ndarray], ground_truth: Sequence[np.ndarray], class_num: int, iou_thresholds=None, area_ranges=None,
             max_dets: int = 100, difficult: Optional[Sequence[np.ndarray]] = None) -> Dict[str, object]:
    """detections[i]: [k,6] rows of image i; ground_truth[i]: [g,6] (or [g,5+]: columns 0-3 box, LAST column class); difficult[i]: [g]
    bool.  -> the summary figures (`SUMMARY`), 'ap_class' [K], 'precision' [T,101,K,A], 'recall' [T,K,A], 'npig' [K,A], 'n_det' [K] and
    'flags' [A,T,rows] uint8 in insertion order (0 ignored / not taking part, 1 true positive, 2 false positive)."""
    if len(detections) != len(ground_truth):
        raise ValueError(f'{len(detections)} images of detections, {len(ground_truth)} of ground truth')
    thr = default_iou_thresholds() if iou_thresholds is None else np.asarray(iou_thresholds, np.float64).reshape(-1)
    areas = default_area_ranges() if area_ranges is None else np.asarray(area_ranges, np.float64).reshape(-1, 2)
    T, A, R, K = len(thr), len(areas), len(REC_THRS), int(class_num)
    max_dets = int(max_dets)
    n_img = len(detections)

    def rows2d(a, width):
        a = np.asarray(a, np.float64)
        if a.size == 0:
            return np.zeros((0, width))
        return a[None] if a.ndim == 1 else a
    gts = [rows2d(g, 6) for g in ground_truth]
    dets = [rows2d(d, 6) for d in detections]
    diff = [np.zeros(len(g), bool) if difficult is None else np.asarray(difficult[i], bool).reshape(-1) for i, g in enumerate(gts)]
    first = np.zeros(n_img + 1, int)
    first[1:] = np.cumsum([len(d) for d in dets])
    n_rows = int(first[-1])
    flags = np.zeros((A, T, n_rows), np.uint8)
    part = np.zeros(n_rows, bool)                                    # the rows that take part (a class in range, inside max_dets)
    npig = np.zeros((K, A), int)
    for i in range(n_img):
        d, g = dets[i], gts[i]
        dcls = d[:, 5].astype(int) if len(d) else np.zeros(0, int)
        gcls = g[:, -1].astype(int) if len(g) else np.zeros(0, int)
        garea = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) if len(g) else np.zeros(0)
        gig = np.stack([diff[i] | (garea < a0) | (garea > a1) for a0, a1 in areas]) if A else np.zeros((0, len(g)), bool)   # [A, g]
        for c in range(K):
            gsel = np.nonzero(gcls == c)[0]
            for a in range(A):
                npig[c, a] += int((~gig[a, gsel]).sum())
            rows = np.nonzero(dcls == c)[0]
            if not len(rows):
                continue
            rows = rows[np.argsort(-d[rows, 4], kind='stable')][:max(max_dets, 0)]
            part[first[i] + rows] = True
            boxes = g[gsel, :4]
            iou = np.stack([box_iou(d[r, :4], boxes) for r in rows]) if len(rows) else np.zeros((0, len(gsel)))            # [rows, boxes]
            darea = (d[rows, 2] - d[rows, 0]) * (d[rows, 3] - d[rows, 1])
            for a, (a0, a1) in enumerate(areas):
                ig = gig[a, gsel]
                for t in range(T):
                    need = min(thr[t], 1 - 1e-10)
                    matched = np.zeros(len(gsel), bool)
                    for n, r in enumerate(rows):
                        cand = ~matched & (iou[n] >= need)
                        pool = cand & ~ig
                        if not pool.any():
                            pool = cand & ig
                        if pool.any():
                            best = iou[n][pool].max()
                            m = int(np.nonzero(pool & (iou[n] == best))[0][-1])                                          # highest index on ties
                            matched[m] = True
                            f = 0 if ig[m] else 1
                        else:
                            f = 0 if (darea[n] < a0 or darea[n] > a1) else 2
                        flags[a, t, first[i] + r] = f
    # ---- accumulate -------------------------------------------------------------------------------------------------------------------
    precision = -np.ones((T, R, K, A))
    recall = -np.ones((T, K, A))
    n_det = np.zeros(K, int)
    all_cls = np.concatenate([d[:, 5].astype(int) for d in dets]) if n_rows else np.zeros(0, int)
    all_score = np.concatenate([d[:, 4] for d in dets]) if n_rows else np.zeros(0)
    for k in range(K):
        rows = np.nonzero((all_cls == k) & part)[0]                                                                      # (image, row) order
        rows = rows[np.argsort(-all_score[rows], kind='stable')]
        n_det[k] = len(rows)
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for t in range(T):
                f = flags[a, t, rows]
                tp = np.cumsum(f == 1).astype(np.float64)
                fp = np.cumsum(f == 2).astype(np.float64)
                rc = tp / float(npig[k, a])
                pr = tp / ((fp + tp) + EPS)
                recall[t, k, a] = rc[-1] if len(rows) else 0.0
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                idx = np.searchsorted(rc, REC_THRS, side='left')
                q = np.zeros(R)
                ok = idx < len(rc)
                q[ok] = pr[idx[ok]]
                precision[t, :, k, a] = q
    out = summarize(precision, recall, thr)
    out.update(precision=precision, recall=recall, npig=npig, n_det=n_det, flags=flags)
    return out

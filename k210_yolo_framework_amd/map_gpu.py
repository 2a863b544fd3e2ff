"""VOC mAP on the GPU (csrc/yk_map.hip): `voc_eval.evaluate`'s rule applied to detection rows where the decode leaves
them, in device memory.

    ev = MapEvaluator(class_num=20)
    for every batch:  ev.add(dets, counts, gts)          # dets [B, cap, 6] + counts [B] as engine.decode_py / Pipeline.submit return them,
                                                         # or packed rows [R, 6] + offsets [B + 1]; cuda tensors or numpy arrays
    r = ev.result()                                      # {'map', 'ap', 'n_gt', 'n_det', 'tp', 'fp'} as voc_eval.evaluate, + 'flags'
    c = ev.coco_result()                                 # the COCO-style figures of the same rows, as coco_eval.evaluate
    s = ev.sweep()                                       # precision / recall / F1 at 1000 confidence thresholds, as oppoint.sweep
    m = ev.confusion(0.6)                                # the confusion matrix of the rows at or above a threshold, as oppoint.confusion

The detection rows are accumulated in device buffers that grow by doubling; the only thing read back per batch is the batch's counts
(4 bytes per image), which size the append.  The ground truth (a few boxes per image, float64) is kept on the host until `result()`
uploads it once.  `flags` has one entry per detection row in insertion order: 0 ignored (matched to a difficult box, or a class outside
[0, class_num)), 1 true positive, 2 false positive.  Scores and boxes must be finite.

There is no CPU fallback: without the library or a HIP device every entry point raises engine.YkError; `voc_eval.evaluate` is the
reference the kernels are tested against, not a substitute."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import engine

MAX_ROWS = 2 ** 31 - 1


def _gt_rows(g) -> np.ndarray:
    """One image's ground truth as evaluate takes it ([g,6] or [g,5+]: columns 0-3 the box, the LAST column the class) -> [g,6] float64."""
    a = np.asarray(g, np.float64)
    if a.size == 0:
        return np.zeros((0, 6))
    if a.ndim == 1:
        a = a[None]
    out = np.zeros((len(a), 6))
    out[:, :4] = a[:, :4]
    out[:, 5] = a[:, -1]
    return out


class MapEvaluator:
    def __init__(self, class_num: int, iou_thresh: float = 0.5, use_07_metric: bool = False, plus_one: bool = False, device: int = 0):
        import torch
        engine.require_gpu()
        if int(class_num) <= 0:
            raise engine.YkError(f'MapEvaluator: class_num {class_num}')
        self.class_num, self.iou_thresh = int(class_num), float(iou_thresh)
        self.use_07_metric, self.plus_one = bool(use_07_metric), bool(plus_one)
        self.dev = torch.device(f'cuda:{int(device)}')
        self.reset()

    def reset(self) -> None:
        """Forget every row and every image; the device buffers are kept."""
        self.n_rows, self.n_img = 0, 0
        self._gts: List[np.ndarray] = []
        self._diff: List[np.ndarray] = []
        if not hasattr(self, '_rows'):
            self._rows = self._img = None
            self._cap = 0

    # -- buffers ------------------------------------------------------------------------------------
    def _reserve(self, need: int) -> None:
        import torch
        if need > MAX_ROWS:
            raise engine.YkError(f'MapEvaluator: {need} detection rows: more than 2^31-1')
        if need <= self._cap:
            return
        cap = max(1024, self._cap)
        while cap < need:
            cap *= 2
        cap = min(cap, MAX_ROWS)
        rows = torch.empty((cap, 6), dtype=torch.float32, device=self.dev)
        img = torch.empty((cap,), dtype=torch.int32, device=self.dev)
        if self.n_rows:                                                         # (on the stream of the add() that needs the room)
            rows[:self.n_rows].copy_(self._rows[:self.n_rows])
            img[:self.n_rows].copy_(self._img[:self.n_rows])
            self._rows.record_stream(torch.cuda.current_stream())
            self._img.record_stream(torch.cuda.current_stream())
        self._rows, self._img, self._cap = rows, img, cap

    # -- accumulation -------------------------------------------------------------------------------
    def add(self, dets, offsets_or_counts, gts: Sequence, difficult: Optional[Sequence] = None, stream=None) -> None:
        """dets [R,6] + offsets [B+1] (packed), or dets [B,cap,6] + counts [B] (padded); cuda tensors (used in place) or numpy arrays.
        gts: one [g,6] / [g,5+] array per image of the batch; difficult: one [g] bool array per image, or None.  A device input must
        be complete on `stream` (default: the current stream) - the append runs there."""
        import torch
        if torch.is_tensor(dets):
            d = dets
        else:
            a = np.asarray(dets, np.float32)
            d = torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a.reshape(-1, 6)))
        c = offsets_or_counts if torch.is_tensor(offsets_or_counts) else torch.from_numpy(np.ascontiguousarray(offsets_or_counts, np.int32))
        if d.dtype != torch.float32 or c.dtype != torch.int32 or d.shape[-1] != 6 or d.dim() not in (2, 3) or c.dim() != 1:
            raise engine.YkError(f'MapEvaluator.add: rows {tuple(d.shape)} {d.dtype}, offsets / counts {tuple(c.shape)} {c.dtype}: '
                                 'expected float32 [R,6] + int32 [B+1], or float32 [B,cap,6] + int32 [B]')
        padded = d.dim() == 3
        B = len(c) if padded else len(c) - 1
        if B != len(gts) or (padded and d.shape[0] < B) or B < 0:
            raise engine.YkError(f'MapEvaluator.add: {B} images of detections, {len(gts)} of ground truth')
        if difficult is not None and len(difficult) != B:
            raise engine.YkError(f'MapEvaluator.add: {B} images, {len(difficult)} difficult arrays')
        if self.n_img + B > MAX_ROWS:
            raise engine.YkError('MapEvaluator.add: more than 2^31-1 images')
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream() if stream is None else stream
            with torch.cuda.stream(st):
                last = getattr(self, '_last', None)
                if last is not None and last != st:
                    st.wait_stream(last)                                      # earlier appends, and the buffers they wrote
                host = c.cpu().numpy().astype(np.int64)                       # the one read-back: 4 bytes per image
                if padded:
                    cap = int(d.shape[1])
                    n_new = int(np.clip(host, 0, cap).sum())
                else:
                    if len(host) == 0 or np.any(np.diff(host) < 0) or host[0] < 0 or host[-1] > d.shape[0]:
                        raise engine.YkError('MapEvaluator.add: offsets must ascend inside the rows')
                    n_new = int(host[-1] - host[0])
                self._reserve(self.n_rows + n_new)
                if n_new and B:
                    d = d.to(self.dev).contiguous()
                    c = c.to(self.dev).contiguous()
                    if padded:
                        engine.call('yk_map_append_padded', d, c, B, cap, self.n_img, n_new, self._rows, self._img, self.n_rows, self._cap,
                                    engine._stream(st))
                    else:
                        engine.call('yk_map_append_packed', d, c, B, self.n_img, n_new, self._rows, self._img, self.n_rows, self._cap,
                                    engine._stream(st))
                    self._last = st
        for i in range(B):
            g = _gt_rows(gts[i])
            self._gts.append(g)
            h = np.zeros(len(g), np.uint8) if difficult is None else np.asarray(difficult[i], bool).reshape(-1).astype(np.uint8)
            if len(h) != len(g):
                raise engine.YkError(f'MapEvaluator.add: image {self.n_img + i}: {len(g)} boxes, {len(h)} difficult flags')
            self._diff.append(h)
        self.n_rows += n_new
        self.n_img += B

    def synchronize(self) -> None:
        """Wait for every append issued so far.  A stream given to `add` must stay alive until this or `result()` has returned; after it
        the evaluator no longer refers to that stream (call it before closing the Pipeline whose streams carried the appends)."""
        last = getattr(self, '_last', None)
        if last is not None:
            last.synchronize()
            self._last = None

    def rows(self):
        """Host copies of what was added: (rows [n,6] float32, image index [n] int32), in insertion order."""
        import torch
        if not self.n_rows:
            return np.zeros((0, 6), np.float32), np.zeros(0, np.int32)
        with torch.cuda.device(self.dev):
            self.synchronize()
            return self._rows[:self.n_rows].cpu().numpy(), self._img[:self.n_rows].cpu().numpy()

    def ground_truth(self):
        """(gt [G,6] float64, offsets [images + 1] int64, difficult [G] uint8) as `result()` uploads them."""
        gt = np.concatenate(self._gts) if self._gts else np.zeros((0, 6))
        diff = np.concatenate(self._diff) if self._diff else np.zeros(0, np.uint8)
        off = np.zeros(self.n_img + 1, np.int64)
        if self.n_img:
            off[1:] = np.cumsum([len(g) for g in self._gts])
        return gt, off, diff

    # -- the metric ---------------------------------------------------------------------------------
    def result(self, stream=None) -> Dict[str, object]:
        """-> {'map', 'ap' [class_num] float64 (nan where a class has no ground truth), 'n_gt', 'n_det', 'tp', 'fp' [class_num] int,
        'flags' [rows] uint8}.  Runs on `stream` (default: the current one) after everything added so far; synchronises to read the results."""
        import torch
        Cn, R, N = self.class_num, self.n_rows, self.n_img
        gt, off, diff = self.ground_truth()
        G = int(off[-1])
        if G > MAX_ROWS:
            raise engine.YkError(f'MapEvaluator: {G} ground-truth rows: more than 2^31-1')
        nbytes = C.c_size_t()
        engine.call('yk_map_workspace_bytes', R, G, N, Cn, C.byref(nbytes))
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream() if stream is None else stream
            with torch.cuda.stream(st):
                last = getattr(self, '_last', None)
                if last is not None and last != st:
                    st.wait_stream(last)
                d_gt = torch.from_numpy(np.ascontiguousarray(gt)).to(self.dev) if G else None
                d_diff = torch.from_numpy(np.ascontiguousarray(diff)).to(self.dev) if G else None
                d_off = torch.from_numpy(off.astype(np.int32)).to(self.dev)
                work = torch.empty((int(nbytes.value),), dtype=torch.uint8, device=self.dev)
                flags = torch.empty((max(R, 1),), dtype=torch.uint8, device=self.dev)
                ints = torch.empty((4, Cn), dtype=torch.int32, device=self.dev)
                ap = torch.empty((Cn + 1,), dtype=torch.float64, device=self.dev)           # [class_num] + the mean
                engine.call('yk_map_eval', self._rows if R else None, self._img if R else None, R, N, d_gt, d_off, d_diff, G, Cn, self.iou_thresh,
                            int(self.use_07_metric), int(self.plus_one), work, nbytes.value, flags, ints[0], ints[1], ints[2], ints[3], ap,
                            ap[Cn:], engine._stream(st))
                st.synchronize()
                self._last = None                                             # everything added so far is complete
                h_ints, h_ap, h_flags = ints.cpu().numpy().astype(int), ap.cpu().numpy(), flags[:R].cpu().numpy()
        return {'map': float(h_ap[Cn]), 'ap': h_ap[:Cn].copy(), 'n_gt': h_ints[0], 'n_det': h_ints[1], 'tp': h_ints[2], 'fp': h_ints[3],
                'flags': h_flags}

    def coco_result(self, iou_thresholds=None, area_ranges=None, max_dets: int = 100, stream=None) -> Dict[str, object]:
        """The COCO-style metric of the rows added so far, by the rule of coco_eval.evaluate -> its dict: 'ap', 'ap50',
        'ap75', 'ap_small', 'ap_medium', 'ap_large', 'ar', 'ar_small', 'ar_medium', 'ar_large' (float, nan where nothing is present),
        'ap_class' [class_num], 'precision' [T,101,class_num,A], 'recall' [T,class_num,A] (-1 where absent), 'npig' [class_num,A],
        'n_det' [class_num], 'flags' [A,T,rows] uint8.  Independent of `iou_thresh`, `use_07_metric` and `plus_one`, and of `result()`:
        nothing accumulated is changed.  Runs on `stream` (default: the current one); synchronises to read the results."""
        import torch
        from . import coco_eval
        thr = coco_eval.default_iou_thresholds() if iou_thresholds is None else np.ascontiguousarray(iou_thresholds, np.float64).reshape(-1)
        area = coco_eval.default_area_ranges() if area_ranges is None else np.ascontiguousarray(area_ranges, np.float64).reshape(-1, 2)
        rec = coco_eval.REC_THRS
        T, A, Rn = len(thr), len(area), len(rec)
        Cn, R, N = self.class_num, self.n_rows, self.n_img
        gt, off, diff = self.ground_truth()
        G = int(off[-1])
        if G > MAX_ROWS:
            raise engine.YkError(f'MapEvaluator: {G} ground-truth rows: more than 2^31-1')
        nbytes = C.c_size_t()
        engine.call('yk_map_coco_workspace_bytes', R, G, N, Cn, T, A, Rn, C.byref(nbytes))          # refuses T * A > 64 by name
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream() if stream is None else stream
            with torch.cuda.stream(st):
                last = getattr(self, '_last', None)
                if last is not None and last != st:
                    st.wait_stream(last)
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
                d_gt, d_diff = (up(gt), up(diff)) if G else (None, None)
                d_off = up(off.astype(np.int32))
                d_thr, d_area, d_rec = up(thr), up(area), up(rec)
                work = torch.empty((int(nbytes.value),), dtype=torch.uint8, device=self.dev)
                flags = torch.empty((A * T * max(R, 1),), dtype=torch.uint8, device=self.dev)
                ints = torch.empty((Cn * A + Cn,), dtype=torch.int32, device=self.dev)             # npig [class_num][A], n_det [class_num]
                prec = torch.empty((T * Rn * Cn * A,), dtype=torch.float64, device=self.dev)
                rcl = torch.empty((T * Cn * A,), dtype=torch.float64, device=self.dev)
                summ = torch.empty((len(coco_eval.SUMMARY) + Cn,), dtype=torch.float64, device=self.dev)
                engine.call('yk_map_coco_eval', self._rows if R else None, self._img if R else None, R, N, d_gt, d_off, d_diff, G, Cn, d_thr, T,
                            d_area, A, d_rec, Rn, int(max_dets), work, nbytes.value, flags, ints, ints[Cn * A:], prec, rcl, summ,
                            summ[len(coco_eval.SUMMARY):], engine._stream(st))
                st.synchronize()
                self._last = None
                h_ints, h_summ = ints.cpu().numpy().astype(int), summ.cpu().numpy()
                out: Dict[str, object] = {k: float(h_summ[j]) for j, k in enumerate(coco_eval.SUMMARY)}
                out['ap_class'] = h_summ[len(coco_eval.SUMMARY):].copy()
                out['precision'] = prec.cpu().numpy().reshape(T, Rn, Cn, A)
                out['recall'] = rcl.cpu().numpy().reshape(T, Cn, A)
                out['npig'], out['n_det'] = h_ints[:Cn * A].reshape(Cn, A), h_ints[Cn * A:]
                out['flags'] = flags[:A * T * R].cpu().numpy().reshape(A, T, R)
        return out

    # -- operating points (oppoint.py) ------------------------------------------------
    def sweep(self, thresholds=None, stream=None) -> Dict[str, object]:
        """Precision / recall / F1 of the rows added so far at every confidence threshold, by the rule of oppoint.sweep with the evaluator's
        iou_thresh / plus_one -> its dict: 'thresholds' [n], 'tp', 'fp' [class_num, n] int, 'n_gt' [class_num] int, 'precision', 'recall',
        'f1' [class_num, n] float64 (recall / f1 NaN where a class has no ground truth), 'best' [class_num] int (-1 there), 'mean_f1' [n],
        'best_all' int, 'flags' [rows] uint8.  thresholds: float64, finite, strictly ascending, 1 .. 4096 of them (default
        np.arange(1000) / 1000); anything else raises engine.YkError.  Runs yk_map_eval, then yk_map_sweep, on `stream` (default: the current
        one); synchronises to read the results.  Nothing accumulated is changed."""
        import torch
        from . import oppoint
        try:
            thr = oppoint.check_thresholds(np.arange(1000) / 1000 if thresholds is None else thresholds)
        except ValueError as e:
            raise engine.YkError(f'MapEvaluator.sweep: {e}') from None
        T = len(thr)
        Cn, R, N = self.class_num, self.n_rows, self.n_img
        gt, off, diff = self.ground_truth()
        G = int(off[-1])
        if G > MAX_ROWS:
            raise engine.YkError(f'MapEvaluator: {G} ground-truth rows: more than 2^31-1')
        nbytes, sbytes = C.c_size_t(), C.c_size_t()
        engine.call('yk_map_workspace_bytes', R, G, N, Cn, C.byref(nbytes))
        engine.call('yk_map_sweep_workspace_bytes', R, Cn, T, C.byref(sbytes))
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream() if stream is None else stream
            with torch.cuda.stream(st):
                last = getattr(self, '_last', None)
                if last is not None and last != st:
                    st.wait_stream(last)
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
                d_gt, d_diff = (up(gt), up(diff)) if G else (None, None)
                d_off, d_thr = up(off.astype(np.int32)), up(thr)
                work = torch.empty((int(nbytes.value),), dtype=torch.uint8, device=self.dev)
                swork = torch.empty((int(sbytes.value),), dtype=torch.uint8, device=self.dev)
                flags = torch.empty((max(R, 1),), dtype=torch.uint8, device=self.dev)
                ints = torch.empty((4, Cn), dtype=torch.int32, device=self.dev)
                ap = torch.empty((Cn + 1,), dtype=torch.float64, device=self.dev)
                counts = torch.empty((2, Cn, T), dtype=torch.int32, device=self.dev)               # tp, fp
                curves = torch.empty((3, Cn, T), dtype=torch.float64, device=self.dev)             # precision, recall, f1
                mean = torch.empty((T,), dtype=torch.float64, device=self.dev)
                best = torch.empty((Cn + 1,), dtype=torch.int32, device=self.dev)                  # [class_num] + best_all
                engine.call('yk_map_eval', self._rows if R else None, self._img if R else None, R, N, d_gt, d_off, d_diff, G, Cn, self.iou_thresh,
                            int(self.use_07_metric), int(self.plus_one), work, nbytes.value, flags, ints[0], ints[1], ints[2], ints[3], ap,
                            ap[Cn:], engine._stream(st))
                engine.call('yk_map_sweep', self._rows if R else None, flags if R else None, R, Cn, ints[0], d_thr, T, swork, sbytes.value,
                            counts[0], counts[1], curves[0], curves[1], curves[2], best, mean, best[Cn:], engine._stream(st))
                st.synchronize()
                self._last = None
                h_counts, h_curves, h_best = counts.cpu().numpy().astype(int), curves.cpu().numpy(), best.cpu().numpy().astype(int)
                return {'thresholds': thr, 'tp': h_counts[0], 'fp': h_counts[1], 'n_gt': ints[0].cpu().numpy().astype(int),
                        'precision': h_curves[0], 'recall': h_curves[1], 'f1': h_curves[2], 'best': h_best[:Cn].copy(),
                        'mean_f1': mean.cpu().numpy(), 'best_all': int(h_best[Cn]), 'flags': flags[:R].cpu().numpy()}

    def confusion(self, conf_thresh: float, iou_thresh: Optional[float] = None, stream=None) -> Dict[str, np.ndarray]:
        """The confusion matrix of the rows added so far with score >= conf_thresh, by the rule of oppoint.confusion (iou_thresh: the
        evaluator's by default; its plus_one) -> {'matrix' [class_num + 1, class_num + 1] int, [true][predicted], index class_num =
        background; 'match' [rows] int: the row's box in the concatenated ground truth, -1 unmatched, -2 the row takes no part}.  Runs on
        `stream` (default: the current one); synchronises to read the results.  Nothing accumulated is changed."""
        import torch
        conf, iou = float(conf_thresh), float(self.iou_thresh if iou_thresh is None else iou_thresh)
        if conf != conf or iou != iou:
            raise engine.YkError(f'MapEvaluator.confusion: conf_thresh {conf_thresh}, iou_thresh {iou_thresh}: not a number')
        Cn, R, N = self.class_num, self.n_rows, self.n_img
        gt, off, diff = self.ground_truth()
        G = int(off[-1])
        if G > MAX_ROWS:
            raise engine.YkError(f'MapEvaluator: {G} ground-truth rows: more than 2^31-1')
        nbytes = C.c_size_t()
        engine.call('yk_map_confusion_workspace_bytes', G, C.byref(nbytes))
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream() if stream is None else stream
            with torch.cuda.stream(st):
                last = getattr(self, '_last', None)
                if last is not None and last != st:
                    st.wait_stream(last)
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
                d_gt, d_diff = (up(gt), up(diff)) if G else (None, None)
                d_off = up(off.astype(np.int32))
                work = torch.empty((int(nbytes.value),), dtype=torch.uint8, device=self.dev)
                matrix = torch.empty(((Cn + 1) * (Cn + 1),), dtype=torch.int32, device=self.dev)
                match = torch.empty((max(R, 1),), dtype=torch.int32, device=self.dev)
                engine.call('yk_map_confusion', self._rows if R else None, self._img if R else None, R, N, d_gt, d_off, d_diff, G, Cn, conf, iou,
                            int(self.plus_one), work, nbytes.value, matrix, match, engine._stream(st))
                st.synchronize()
                self._last = None
                return {'matrix': matrix.cpu().numpy().astype(int).reshape(Cn + 1, Cn + 1), 'match': match[:R].cpu().numpy().astype(int)}


def confusion_lds_boxes() -> int:
    """The largest (rows taking part + ground-truth boxes) of one image that MapEvaluator.confusion matches out of LDS; above it the same
    loop reads global memory."""
    return int(engine.lib().yk_map_confusion_lds_boxes())

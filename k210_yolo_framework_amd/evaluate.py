"""`make eval` - VOC mAP of a checkpoint, or with --metric coco its COCO-style AP as well, network and metric both on the GPU
(DESIGN.md 3.11, 3.17).

    python keras_eval.py CKPT [network flags of keras_inference.py] (--ann LIST.npy [--all] [--limit N] | --synthetic N)
                              [--precision f16x2|f16|kpu] [--obj_thresh 0.05] [--nms_iou 0.5] [--iou_thresh 0.5] [--voc07 True]
                              [--nms hard|linear|gaussian|diou] [--nms_sigma 0.5]
                              [--metric voc|coco] [--out eval.json] [--dump_rows rows.npz]
                              [--tiles NXxNY --tile_overlap 0.2 --tile_full True --tile_match ios|iou --tile_thresh 0.5]
                              [--tta 1,1f|flip|v5 --tta_thresh 0.55]
                              [--curves True --conf_thresh 0.6 --curve_steps 1000 --curves_out curves.npz]

CKPT: a Keras `.h5` / `.npz` checkpoint (float modes, through engine.Pipeline with several batches in flight) or a `.kmodel` / `.kfpkg`
(`--precision kpu`, the K210 KPU's exact integer arithmetic through engine.KpuPlan).  The images are the validation head of the list
make_voc_list.py writes (the whole list with --all), or N generated images with known boxes as `make train SYNTHETIC=N` trains on,
drawn from a seed of their own.  Every batch's detections go from the decode straight into map_gpu.MapEvaluator, in device memory; the
metric is voc_eval.evaluate's.  Prints the per-class AP table and the mAP, writes them to `eval.json` next to the checkpoint (or --out).

--metric coco (`make eval METRIC=coco`) scores the same accumulated rows a second time by the COCO rule (coco_eval.evaluate's statement,
computed by MapEvaluator.coco_result on the GPU): AP averaged over IoU 0.50:0.95, AP50, AP75, AP for small / medium / large objects, AR and
its three, and AP per class; `eval.json` gains a `coco` object.  The VOC lines and keys stay as they are, --iou_thresh and --voc07 keep
their meaning for them (--voc07 True with --metric coco is refused).  The rule is restated from pycocotools' public source and parity with
pycocotools' own numbers is unpinned; `difficult` stands in for COCO's `ignore` (no crowd boxes); an object's area is its box area in the
pixels of the picture it was scored in (COCO: mask area, source-image pixels); AR is at 100 detections per class and image only.

--curves True (`make eval CURVES=True`) adds the operating points of the same accumulated rows (oppoint.py's statement, computed by
MapEvaluator.sweep and .confusion on the GPU): per class precision / recall / F1 at --conf_thresh and at the class's best-F1
threshold, the threshold that maximises the mean F1, and the confusion matrix at --conf_thresh; `eval.json` gains an `operating` object and
--curves_out writes the full arrays.  The thresholds swept are k / --curve_steps at or above --obj_thresh (the decode never emitted the rows
below it), plus --conf_thresh.  Exact counting, not other frameworks' interpolated curves: parity with their numbers is unpinned.
The reference ships no evaluator; tools/map_eval.py is the host-side developer script this replaces as the product's entry point."""
from __future__ import annotations

import argparse
import json
import sys
from collections import deque
from pathlib import Path

import numpy as np

from . import softnms
from . import tiles as tl
from . import tta as tt
from .helper import INFO, Helper, VOC_ANCHORS
from .yolonet import MODEL_DEFS

SYNTHETIC_SEED = 7919        # `make train` draws its generated images from --rand_seed (3 in the Makefile, 6 by default)
CAP_NOTE = 'at most 30 detections per class and image as keras_inference.py:125'


def ground_truth_rows(boxes, img_hw) -> np.ndarray:
    """[n,5] (class, cx, cy, w, h) relative to the image -> [n,6] float64 (top, left, bottom, right, 1, class) in its pixels."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 5)
    ih, iw = float(img_hw[0]), float(img_hw[1])
    cx, cy, w, h = boxes[:, 1] * iw, boxes[:, 2] * ih, boxes[:, 3] * iw, boxes[:, 4] * ih
    return np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2, np.ones(len(boxes)), boxes[:, 0]], 1)


def parse(argv=None):
    p = argparse.ArgumentParser(description='VOC mAP of a checkpoint, evaluated on the GPU')
    p.add_argument('pre_ckpt', type=str, help='.h5 / .npz weights, or a .kmodel / .kfpkg with --precision kpu')
    p.add_argument('--ann', type=str, default=None, help='list file as make_voc_list.py writes (default data/<train_set>_img_ann.npy)')
    p.add_argument('--synthetic', type=int, default=0, help='evaluate on N generated images with known boxes instead of --ann')
    p.add_argument('--synthetic_seed', type=int, default=SYNTHETIC_SEED, help='seed of the generated images (not the training seed)')
    p.add_argument('--train_set', type=str, default='voc')
    p.add_argument('--class_num', type=int, default=20)
    p.add_argument('--model_def', type=str, default='yolo_mobilev1')
    p.add_argument('--depth_multiplier', type=float, choices=[0.5, 0.75, 1.0], default=0.75)
    p.add_argument('--image_size', type=int, default=(224, 320), nargs='+')
    p.add_argument('--output_size', type=int, default=(7, 10, 14, 20), nargs='+')
    p.add_argument('--precision', type=str, choices=['f16', 'f16x2', 'kpu'], default='f16x2')
    p.add_argument('--obj_thresh', type=float, default=0.05)
    p.add_argument('--nms_iou', type=float, default=0.5, help='IoU of the per-class NMS (keras_inference.py --iou_thresh)')
    p.add_argument('--iou_thresh', type=float, default=0.5, help='IoU a detection needs with a ground-truth box')
    p.add_argument('--nms', type=str, default='hard', help="suppression rule of the decode: hard (the reference's), linear or gaussian (Soft-NMS), diou")
    p.add_argument('--nms_sigma', type=float, default=0.5, help='sigma of --nms gaussian')
    p.add_argument('--voc07', type=str, choices=['True', 'False'], default='False', help='11-point AP')
    p.add_argument('--metric', type=str, choices=['voc', 'coco'], default='voc', help='coco: also AP over IoU .50:.95, by object size, AR')
    p.add_argument('--all', action='store_true', help='evaluate the whole list, not its validation head')
    p.add_argument('--limit', type=int, default=0)
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--depth', type=int, default=3, help='batches in flight (float modes)')
    p.add_argument('--out', type=str, default=None, help='result file (default: eval.json next to the checkpoint)')
    p.add_argument('--dump_rows', type=str, default=None, help='also write the detections and the ground truth that were scored (.npz)')
    p.add_argument('--curves', type=str, choices=['True', 'False'], default='False', help='also precision / recall / F1 over confidence and a confusion matrix')
    p.add_argument('--conf_thresh', type=float, default=0.6, help="--curves: the confidence threshold reported (the K210 demo's 0.6)")
    p.add_argument('--curve_steps', type=int, default=1000, help='--curves: thresholds k / N are swept')
    p.add_argument('--curves_out', type=str, default=None, help='--curves: also write the full arrays (.npz)')
    tl.add_arguments(p)
    tt.add_arguments(p)
    a = p.parse_args(sys.argv[1:] if argv is None else argv)
    if (a.precision == 'kpu') != a.pre_ckpt.endswith(('.kmodel', '.kfpkg')):
        p.error('--precision kpu runs a .kmodel / .kfpkg checkpoint, and only it does (the float modes take .h5 / .npz)')
    if a.synthetic and a.ann:
        p.error('--synthetic N replaces --ann')
    try:
        softnms.check(a.nms, a.nms_sigma)
    except ValueError as e:
        p.error(str(e))
    try:
        tl.parse_arguments(a)
        tt.parse_arguments(a)
    except ValueError as e:
        p.error(str(e))
    if a.tta is not None and len(a.tta) > a.batch:
        p.error(f'--tta {tt.text_of(a.tta)}: a picture is {len(a.tta)} frames and --batch holds {a.batch}')
    if a.metric == 'coco' and a.voc07 == 'True':
        p.error('--voc07 True is the 11-point VOC AP; --metric coco has its own 101-point AP: choose one')
    if a.curves == 'True':
        try:
            curve_grid(a.obj_thresh, a.conf_thresh, a.curve_steps)
        except ValueError as e:
            p.error(str(e))
    elif a.curves_out:
        p.error('--curves_out FILE is written by --curves True')
    return a


def curve_grid(obj_thresh: float, conf_thresh: float, steps: int) -> np.ndarray:
    """The thresholds `--curves True` sweeps: k / steps for k in range(steps) that are >= obj_thresh (the decode emitted no row below
    it, so counts there would be wrong), and conf_thresh in its place if it is not among them.  ValueError names what is refused."""
    from . import oppoint
    obj, conf, steps = float(obj_thresh), float(conf_thresh), int(steps)
    if not (conf == conf and abs(conf) != float('inf')):
        raise ValueError(f'--conf_thresh {conf_thresh}: not a finite number')
    if conf < obj:
        raise ValueError(f'--conf_thresh {conf:g} is below --obj_thresh {obj:g}: the decode emitted no row below --obj_thresh, the counts would be wrong')
    if steps < 1 or steps > oppoint.MAX_THRESHOLDS - 1:
        raise ValueError(f'--curve_steps {steps}: outside 1 .. {oppoint.MAX_THRESHOLDS - 1}')
    grid = np.arange(steps) / steps
    grid = grid[grid >= obj]
    if not np.any(grid == conf):
        grid = np.sort(np.append(grid, conf))
    return grid


def _items(a, h: Helper):
    """[(uint8 image or path, boxes [n,5])] to evaluate."""
    from . import engine
    if a.synthetic:
        from .training import synthetic_list
        return synthetic_list(int(a.synthetic), tuple(int(v) for v in h.in_hw[0]), a.class_num, a.synthetic_seed)
    ann = Path(a.ann or f'data/{a.train_set}_img_ann.npy')
    if not ann.exists():
        raise engine.YkError(f'{ann} not found (make_voc_list.py output); pass --synthetic N for generated data')
    rows = np.load(str(ann), allow_pickle=True)
    n_val = int(len(rows) * h.validation_split)
    rows = rows if a.all else rows[:n_val]
    return [(r[0], r[1]) for r in (rows[:a.limit] if a.limit else rows)]


def _load(h: Helper, item):
    img, boxes = item
    if not isinstance(img, np.ndarray):
        img = h._read_img(str(img))
    return np.ascontiguousarray(img[..., :3], np.uint8), np.asarray(boxes, np.float64)


def run(a, h: Helper, model, items, ev, tta=None, tta_thresh=None) -> None:
    """Every image of `items` through the network and the decode; detections and ground truth into `ev`.  tta / tta_thresh: test-time
    augmentation as detect.run takes it (tta.py); left None they are read from a.tta / a.tta_thresh where `a` has them (off, 0.55)."""
    import torch
    from . import engine
    in_hw = tuple(int(v) for v in h.in_hw[0])
    try:
        grid_xy = tl.check(a.tiles, a.tile_overlap, a.tile_match, a.tile_thresh, a.nms)
    except ValueError as e:
        raise engine.YkError(f'evaluate: {e}') from None
    T = 1 if grid_xy is None else grid_xy[0] * grid_xy[1] + (1 if a.tile_full else 0)      # network frames per picture
    tta = getattr(a, 'tta', None) if tta is None else tta
    tta_thresh = getattr(a, 'tta_thresh', tt.DEFAULT_THRESH) if tta_thresh is None else tta_thresh
    try:
        tta_spec = tt.check(tta, tta_thresh, a.nms, a.tiles)
    except ValueError as e:
        raise engine.YkError(f'evaluate: {e}') from None
    if tta_spec is not None:
        T = len(tta_spec)
        if T > int(a.batch):
            raise engine.YkError(f'evaluate: tta {tt.text_of(tta_spec)}: a picture is {T} frames and a batch holds {int(a.batch)}')
    B = max(1, min(int(a.batch) // T, len(items)))
    max_out = 30

    def tile_frames(imgs, out, stream):
        """Sliced inference (tiles.py): the pictures packed into one device buffer, their tiles letterboxed into `out` by one launch
        -> (what must stay alive until the batch has run, each frame's (h, w), origins, first)."""
        from . import draw as dr
        packed, table, shapes = dr.pack_ragged(imgs)
        with torch.cuda.stream(stream):
            d_packed = packed.to(out.device, non_blocking=False)
        grids = [tl.grid(sh, sw, grid_xy[0], grid_xy[1], a.tile_overlap, a.tile_full) for sh, sw in shapes]
        rows = np.concatenate([tl.table_rows(g, int(table['offset'][i]), shapes[i][1]) for i, g in enumerate(grids)])
        g_all = np.concatenate(grids)
        engine.letterbox_tiles_u8(d_packed, rows, in_hw, stream=stream, out=out)
        return d_packed, g_all[:, 2:4].astype(np.float32), np.ascontiguousarray(g_all[:, 0:2], np.float32), np.arange(len(imgs) + 1, dtype=np.int32) * T

    def view_frames(imgs, out, stream):
        """Test-time augmentation (tta.py): the pictures packed into one device buffer, their views letterboxed into `out` by one launch
        -> (what must stay alive until the batch has run, each frame's (h, w), the frames' (dy, dx, mw))."""
        from . import draw as dr
        packed, table, shapes = dr.pack_ragged(imgs)
        with torch.cuda.stream(stream):
            d_packed = packed.to(out.device, non_blocking=False)
        vws = [tt.views(sh, sw, tta_spec) for sh, sw in shapes]
        rows = np.concatenate([tt.table_rows(v, int(table['offset'][i]), *shapes[i]) for i, v in enumerate(vws)])
        v_all = np.concatenate(vws)
        engine.letterbox_views_u8(d_packed, rows, in_hw, stream=stream, out=out)
        return d_packed, v_all[:, 0:2].astype(np.float32), tt.xforms(v_all)

    if a.precision == 'kpu':
        plan = model._plan(B * T)
        cfg = engine.make_decode_cfg(h.anchors, h.class_num, h.in_hw[0], h.out_hw)
        for k in range(0, len(items), B):
            loaded = [_load(h, it) for it in items[k:k + B]]
            if tta_spec is not None:
                frames = torch.empty((len(loaded) * T, *in_hw, 3), dtype=torch.uint8, device='cuda')
                _, shapes, xf = view_frames([im for im, _ in loaded], frames, torch.cuda.current_stream())
            elif grid_xy is None:
                frames = torch.cat([engine.letterbox_u8(torch.from_numpy(im[None]).cuda(), in_hw) for im, _ in loaded])
                shapes = np.asarray([im.shape[:2] for im, _ in loaded], np.float32)
            else:
                frames = torch.empty((len(loaded) * T, *in_hw, 3), dtype=torch.uint8, device='cuda')
                _, shapes, origins, first = tile_frames([im for im, _ in loaded], frames, torch.cuda.current_stream())
            plan.run_u8(frames)
            dets, counts = engine.decode_py(cfg, plan.outputs(), len(frames), shapes, a.obj_thresh, a.nms_iou, max_out=max_out, nms=a.nms, sigma=a.nms_sigma)
            if grid_xy is not None:
                dets, counts = engine.merge_tiles(dets, counts, origins, first, h.class_num, max_out, a.tile_thresh, a.tile_match)
            if tta_spec is not None:
                dets, counts = engine.fuse_views(dets, counts, xf, T, h.class_num, max_out, tta_thresh)
            ev.add(dets, counts, [ground_truth_rows(b, im.shape[:2]) for im, b in loaded])
        return
    pipe = engine.Pipeline(model.spec, model.get_weights(), h.anchors, max_batch=B * T, depth=max(1, int(a.depth)), precision=a.precision, max_out=max_out)
    merged = [None] * pipe.depth                            # tiles, tta: each slot's merged / fused rows per picture
    pending = deque()                                       # (dets, counts, stream, ground truth) of the batches in flight

    def drain():
        dets, counts, stream, gts = pending.popleft()
        ev.add(dets, counts, gts, stream=stream)           # on the slot's stream: the rows never leave device memory

    try:
        for k in range(0, len(items), B):
            if len(pending) == pipe.depth:                  # the slot about to be reused still holds an unread result
                drain()
            loaded = [_load(h, it) for it in items[k:k + B]]
            slot = pipe.next_slot()
            buf, st = pipe.input(slot), pipe.streams[slot]
            if tta_spec is not None:
                keep, shapes, xf = view_frames([im for im, _ in loaded], buf[:len(loaded) * T], st)
            elif grid_xy is None:
                with torch.cuda.stream(st):
                    for j, (im, _) in enumerate(loaded):
                        engine.letterbox_u8(torch.from_numpy(im[None]).to(buf.device, non_blocking=False), in_hw, stream=st, out=buf[j:j + 1])
                shapes = np.asarray([im.shape[:2] for im, _ in loaded], np.float32)
            else:
                keep, shapes, origins, first = tile_frames([im for im, _ in loaded], buf[:len(loaded) * T], st)
            dets, counts, stream = pipe.submit(None, image_hw=shapes, obj_thresh=a.obj_thresh, iou_thresh=a.nms_iou, max_out=max_out,
                                               batch=len(loaded) * T, nms=a.nms, sigma=a.nms_sigma)
            if grid_xy is not None or tta_spec is not None:
                if merged[slot] is None:
                    merged[slot] = (torch.zeros((B, h.class_num * max_out, 6), dtype=torch.float32, device=buf.device),
                                    torch.zeros((B,), dtype=torch.int32, device=buf.device))
                    torch.cuda.current_stream().synchronize()           # (filled on torch's stream, written on the slot's)
                if tta_spec is not None:
                    dets, counts = engine.fuse_views(dets, counts, xf, T, h.class_num, max_out, tta_thresh, stream=stream,
                                                     out=merged[slot][0][:len(loaded)], out_counts=merged[slot][1][:len(loaded)])
                else:
                    dets, counts = engine.merge_tiles(dets, counts, origins, first, h.class_num, max_out, a.tile_thresh, a.tile_match, stream=stream,
                                                      out=merged[slot][0][:len(loaded)], out_counts=merged[slot][1][:len(loaded)])
                stream.synchronize()                                    # `keep`, the packed originals, may go once the frames are cut
            pending.append((dets, counts, stream, [ground_truth_rows(b, im.shape[:2]) for im, b in loaded]))
        while pending:
            drain()
        pipe.wait()
        ev.synchronize()                                    # the appends ran on the slots' streams, which close() destroys
    finally:
        pipe.close()


COCO_LINES = (('ap', 'AP   IoU .50:.95  all   '), ('ap50', 'AP   IoU .50      all   '), ('ap75', 'AP   IoU .75      all   '),
              ('ap_small', 'AP   IoU .50:.95  small '), ('ap_medium', 'AP   IoU .50:.95  medium'), ('ap_large', 'AP   IoU .50:.95  large '),
              ('ar', 'AR   IoU .50:.95  all   '), ('ar_small', 'AR   IoU .50:.95  small '), ('ar_medium', 'AR   IoU .50:.95  medium'),
              ('ar_large', 'AR   IoU .50:.95  large '))


def coco_report(ev, class_num: int, n_gt) -> dict:
    """The COCO-style figures of what `ev` holds (MapEvaluator.coco_result, defaults): printed, and returned as eval.json's `coco` object."""
    from . import coco_eval
    c = ev.coco_result()
    num = lambda v: None if v != v else float(v)
    pct = lambda v: '   nan' if v != v else f'{100 * v:6.2f}'
    print(f'COCO-style (restated rule, parity with pycocotools unpinned; box area; at most 100 detections per class and image; {CAP_NOTE}):')
    for key, label in COCO_LINES:
        print(f'   {label} {pct(c[key])}')
    for k in range(class_num):
        if n_gt[k]:
            print(f'   class {k:2d}: AP .50:.95 {pct(c["ap_class"][k])}   det {c["n_det"][k]:6d}')
    rep = {key: num(c[key]) for key in coco_eval.SUMMARY}
    rep.update(ap_class=[num(v) for v in c['ap_class']], iou_thresholds=[float(v) for v in coco_eval.default_iou_thresholds()],
               area_ranges=coco_eval.default_area_ranges().tolist(), max_dets=100, npig=c['npig'].tolist(), n_det=c['n_det'].tolist(),
               note=CAP_NOTE)
    return rep


def operating_report(ev, a, n_gt) -> dict:
    """The operating points of what `ev` holds (MapEvaluator.sweep over curve_grid, MapEvaluator.confusion at a.conf_thresh): printed, and
    returned as eval.json's `operating` object; a.curves_out receives the full arrays."""
    K, conf = a.class_num, float(a.conf_thresh)
    grid = curve_grid(a.obj_thresh, conf, a.curve_steps)
    s = ev.sweep(grid)
    cm = ev.confusion(conf)
    at = int(np.nonzero(grid == conf)[0][0])
    num = lambda v: None if v != v else float(v)
    pct = lambda v: '   nan' if v != v else f'{100 * v:6.2f}'
    rule = 'hard NMS scores' if a.nms == 'hard' else f'the decayed scores of nms {a.nms} (softnms.py)'
    print(f'operating points (oppoint.py: exact counting, parity with other frameworks\' curves unpinned; IoU {a.iou_thresh}; {rule}; '
          f'{len(grid)} thresholds from {grid[0]:g}; {CAP_NOTE}):')
    print(f'   class     gt |  at {conf:<5g}  P      R     F1 |  best thr      P      R     F1')
    have = [c for c in range(K) if n_gt[c]]
    for c in have:
        b = int(s['best'][c])
        print(f'   class {c:2d} {int(n_gt[c]):5d} |         {pct(s["precision"][c, at])} {pct(s["recall"][c, at])} {pct(s["f1"][c, at])} |'
              f'  {grid[b]:8.4f} {pct(s["precision"][c, b])} {pct(s["recall"][c, b])} {pct(s["f1"][c, b])}')
    mean = lambda key, k: float(np.mean([s[key][c, k] for c in have])) if have else float('nan')
    ba = int(s['best_all'])
    best_thr, best_f1 = (float(grid[ba]), float(s['mean_f1'][ba])) if ba >= 0 else (float('nan'), float('nan'))
    print(f'   all classes  |  at {conf:<5g}{pct(mean("precision", at))} {pct(mean("recall", at))} {pct(s["mean_f1"][at])} |'
          f'  best mean F1 {pct(best_f1)} at threshold {best_thr:g}')
    m = cm['matrix']
    shown = [c for c in range(K) if m[c].any() or m[:, c].any()]
    print(f'   confusion at {conf:g} (rows: true class, columns: predicted class; bg = background: a row of bg is a false positive, a column '
          f'of bg a missed box; classes without a count left out):')
    print('        true \\ pred ' + ' '.join(f'{c:5d}' for c in shown) + '    bg')
    for c in shown + [K]:
        print(f'        {"bg" if c == K else c:>11} ' + ' '.join(f'{int(m[c, d]):5d}' for d in shown) + f' {int(m[c, K]):5d}')
    rep = {'conf_thresh': conf, 'iou_thresh': a.iou_thresh, 'steps': int(a.curve_steps), 'thresholds': len(grid), 'scores': rule,
           'n_gt': [int(v) for v in n_gt],
           'precision': [num(v) for v in s['precision'][:, at]], 'recall': [num(v) for v in s['recall'][:, at]],
           'f1': [num(v) for v in s['f1'][:, at]], 'mean_precision': num(mean('precision', at)), 'mean_recall': num(mean('recall', at)),
           'mean_f1': num(s['mean_f1'][at]),
           'class_best_threshold': [None if b < 0 else float(grid[b]) for b in s['best']],
           'class_best_precision': [None if b < 0 else num(s['precision'][c, b]) for c, b in enumerate(s['best'])],
           'class_best_recall': [None if b < 0 else num(s['recall'][c, b]) for c, b in enumerate(s['best'])],
           'class_best_f1': [None if b < 0 else num(s['f1'][c, b]) for c, b in enumerate(s['best'])],
           'best_threshold': num(best_thr), 'best_mean_f1': num(best_f1),
           'confusion': m.tolist(), 'confusion_axes': f'confusion[true][predicted]; index {K} is background: confusion[{K}][c] counts false '
                                                      f'positives of class c, confusion[c][{K}] its missed boxes',
           'note': CAP_NOTE}
    if a.curves_out:
        np.savez(a.curves_out, thresholds=grid, tp=s['tp'], fp=s['fp'], precision=s['precision'], recall=s['recall'], f1=s['f1'],
                 mean_f1=s['mean_f1'], matrix=m)
    return rep


def main(argv=None):
    a = parse(argv)
    from . import engine
    from .map_gpu import MapEvaluator
    engine.require_gpu()
    anchor_file = Path(f'data/{a.train_set}_anchor.npy')
    h = Helper(None, a.class_num, str(anchor_file) if anchor_file.exists() else VOC_ANCHORS, np.reshape(np.array(a.image_size), (-1, 2)),
               np.reshape(np.array(a.output_size), (-1, 2)))
    model, _ = MODEL_DEFS[a.model_def]([a.image_size[0], a.image_size[1], 3], len(h.anchors[0]), a.class_num, alpha=a.depth_multiplier,
                                       precision=a.precision)
    model.load_weights(a.pre_ckpt)
    print(INFO, f' Load CKPT {a.pre_ckpt}')
    items = _items(a, h)
    if not items:
        raise engine.YkError('evaluate: no images to evaluate')
    voc07 = a.voc07 == 'True'
    ev = MapEvaluator(a.class_num, a.iou_thresh, voc07)
    run(a, h, model, items, ev)
    r = ev.result()
    print(f'{a.precision}: mAP {100 * r["map"]:.2f} over {len(items)} images ({"VOC07 11-point" if voc07 else "area"} AP, IoU {a.iou_thresh}; '
          f'obj_thresh {a.obj_thresh}, {CAP_NOTE})')
    if a.nms != 'hard':
        print(f'   nms {a.nms}, sigma {a.nms_sigma:g}: rows carry the decayed scores (softnms.py)')
    for c in range(a.class_num):
        if r['n_gt'][c]:
            print(f'   class {c:2d}: AP {100 * r["ap"][c]:6.2f}   gt {r["n_gt"][c]:5d}  det {r["n_det"][c]:6d}  tp {r["tp"][c]:5d}')
    num = lambda v: None if v != v else float(v)
    report = {'ckpt': str(a.pre_ckpt), 'precision': a.precision, 'images': len(items), 'rows': int(ev.n_rows), 'obj_thresh': a.obj_thresh,
              'nms_iou': a.nms_iou, 'iou_thresh': a.iou_thresh, 'voc07': voc07, 'note': CAP_NOTE, 'map': num(r['map']),
              'ap': [num(v) for v in r['ap']], 'n_gt': r['n_gt'].tolist(), 'n_det': r['n_det'].tolist(), 'tp': r['tp'].tolist(),
              'fp': r['fp'].tolist()}
    if a.nms != 'hard':
        report.update(nms=a.nms, nms_sigma=a.nms_sigma)
    if a.tiles is not None:
        report.update(tiles=list(a.tiles), tile_overlap=a.tile_overlap, tile_full=a.tile_full, tile_match=a.tile_match, tile_thresh=a.tile_thresh)
        print(f'   tiles {a.tiles[0]}x{a.tiles[1]}, overlap {a.tile_overlap:g}, whole picture {a.tile_full}: merged by {a.tile_match} > {a.tile_thresh:g} (tiles.py)')
    if a.tta is not None:
        report.update(tt.rule_of(a.tta, a.tta_thresh))
        print(f'   tta {tt.text_of(a.tta)}: {len(a.tta)} views a picture, fused by IoU > {a.tta_thresh:g}; rows carry the fused scores (tta.py)')
    if a.metric == 'coco':
        report['coco'] = coco_report(ev, a.class_num, r['n_gt'])
    if a.curves == 'True':
        report['operating'] = operating_report(ev, a, r['n_gt'])
    out = Path(a.out) if a.out else Path(a.pre_ckpt).resolve().parent / 'eval.json'
    out.write_text(json.dumps(report, indent=1))
    print(INFO, f' wrote {out}')
    if a.dump_rows:
        rows, img = ev.rows()
        gt, gt_off, diff = ev.ground_truth()
        np.savez(a.dump_rows, rows=rows, image=img, gt=gt, gt_offsets=gt_off, difficult=diff, flags=r['flags'])
    return report


cli = main

if __name__ == '__main__':
    main()

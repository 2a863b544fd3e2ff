"""Rate of the COCO-style metric alone: MapEvaluator.coco_result against coco_eval.evaluate (host) and against MapEvaluator.result() (the VOC
metric) on the same rows (profiles/coco_eval_rate.txt).
  python tools/coco_rate.py [images=4952] [classes=20] [runs=5] [host_images=256]
Seeded VOC07-test-sized input as tools/map_rate.py draws it: ~10 detections and ~2.5 ground-truth boxes per image.  The rows are added once
(device-resident); coco_result() and result() are each timed synchronised, median of `runs` after one warm-up, same process, GPU otherwise
idle.  coco_eval.evaluate is interpreted Python (10 thresholds x 4 ranges per detection): it is timed ONCE on the first `host_images` images,
after the device result on exactly those images has been compared with it, and its time for the whole set is NOT extrapolated here."""
import json
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch
from k210_yolo_framework_amd import coco_eval, engine
from k210_yolo_framework_amd.map_gpu import MapEvaluator

engine.require_gpu()
arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
n_img, class_num, runs, n_host = arg(1, 4952), arg(2, 20), arg(3, 5), arg(4, 256)
n_host = min(n_host, n_img)


def median_ms(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


rng = np.random.default_rng(2007)
dets, gts = [], []
for _ in range(n_img):
    g = int(rng.poisson(2.5))
    tl = rng.uniform(0, 350, (g, 2))
    gt = np.concatenate([tl, tl + rng.uniform(20, 150, (g, 2)), np.ones((g, 1)), rng.integers(0, class_num, (g, 1))], 1)
    n = int(rng.poisson(10))
    rows = np.zeros((n, 6), np.float32)
    for k in range(n):
        if g and rng.random() < 0.5:
            src = gt[int(rng.integers(0, g))]
            rows[k, :4], rows[k, 5] = src[:4] + rng.normal(0, 6.0, 4), src[5]
        else:
            t = rng.uniform(0, 350, 2)
            rows[k, :4], rows[k, 5] = np.concatenate([t, t + rng.uniform(20, 150, 2)]), rng.integers(0, class_num)
        rows[k, 4] = rng.uniform(0.05, 1.0)
    dets.append(rows)
    gts.append(gt)


def evaluator(d, g):
    off = np.zeros(len(d) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in d])
    ev = MapEvaluator(class_num)
    ev.add(torch.from_numpy(np.concatenate(d)).cuda(), torch.from_numpy(off).cuda(), g)
    return ev


# the head of the set: device against host, compared before any time is printed
small = evaluator(dets[:n_host], gts[:n_host])
got = small.coco_result()
t0 = time.perf_counter()
ref = coco_eval.evaluate(dets[:n_host], gts[:n_host], class_num)
host_ms = (time.perf_counter() - t0) * 1e3
assert all(np.array_equal(got[k], ref[k]) for k in ('flags', 'npig', 'n_det', 'precision', 'recall')), 'results differ'
assert all(abs(got[k] - ref[k]) <= 1e-12 or (got[k] != got[k] and ref[k] != ref[k]) for k in coco_eval.SUMMARY), 'summaries differ'
small_ms, small_all = median_ms(small.coco_result, runs)

ev = evaluator(dets, gts)
out = {}
coco_ms, coco_all = median_ms(lambda: out.__setitem__('coco', ev.coco_result()), runs)
voc_ms, voc_all = median_ms(lambda: out.__setitem__('voc', ev.result()), runs)
print(json.dumps(dict(images=n_img, classes=class_num, detections=int(ev.n_rows), ground_truth=int(sum(len(x) for x in gts)), runs=runs,
                      ap=out['coco']['ap'], ap50=out['coco']['ap50'], voc_map=out['voc']['map'],
                      coco_result_ms=round(coco_ms, 3), result_ms=round(voc_ms, 3), coco_over_voc=round(coco_ms / voc_ms, 2),
                      coco_result_runs_ms=[round(t, 3) for t in coco_all], result_runs_ms=[round(t, 3) for t in voc_all],
                      host_images=n_host, host_detections=int(small.n_rows), coco_eval_evaluate_ms_once=round(host_ms, 1),
                      coco_result_on_host_images_ms=round(small_ms, 3), host_ratio=round(host_ms / small_ms, 1),
                      coco_result_on_host_images_runs_ms=[round(t, 3) for t in small_all])))

"""Rate of the VOC metric alone: map_gpu.MapEvaluator against voc_eval.evaluate on the same arrays (profiles/map_eval_rate.txt).
  python tools/map_rate.py metric [images=4952] [classes=20] [runs=5]   seeded VOC07-test-sized input: ~10 detections and ~2.5 ground-truth
                                                                        boxes per image.  MapEvaluator = add() of device-resident packed rows
                                                                        + result(), synchronised; the baseline is voc_eval.evaluate on the
                                                                        host copies, same process, GPU otherwise idle.  Median of `runs`
                                                                        after one warm-up; the two results are compared before any time is
                                                                        printed.
  python tools/map_rate.py validate [runs=5]                            one training.validate pass, yolo_mobilev2-1.0, 16 generated images,
                                                                        with and without val_mAP (median of `runs` after one warm-up)"""
import json
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch
from k210_yolo_framework_amd import engine, voc_eval
from k210_yolo_framework_amd.map_gpu import MapEvaluator

if len(sys.argv) < 2 or sys.argv[1] not in ('metric', 'validate'):
    sys.exit(__doc__)
engine.require_gpu()


def median_ms(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


if sys.argv[1] == 'metric':
    n_img = int(sys.argv[2]) if len(sys.argv) > 2 else 4952
    class_num = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
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
    off = np.zeros(n_img + 1, np.int32)
    off[1:] = np.cumsum([len(d) for d in dets])
    d_rows, d_off = torch.from_numpy(np.concatenate(dets)).cuda(), torch.from_numpy(off).cuda()
    ev = MapEvaluator(class_num)
    out = {}

    def gpu():
        ev.reset()
        ev.add(d_rows, d_off, gts)
        out['gpu'] = ev.result()                       # synchronises

    def host():
        out['ref'] = voc_eval.evaluate(dets, gts, class_num)

    gpu_ms, gpu_all = median_ms(gpu, runs)
    ref_ms, ref_all = median_ms(host, runs)
    g, r = out['gpu'], out['ref']
    assert all(np.array_equal(g[k], r[k]) for k in ('n_gt', 'n_det', 'tp', 'fp')) and abs(g['map'] - r['map']) <= 1e-12, 'results differ'
    print(json.dumps(dict(images=n_img, classes=class_num, detections=int(off[-1]), ground_truth=int(sum(len(x) for x in gts)), runs=runs,
                          map=g['map'], map_evaluator_ms=round(gpu_ms, 3), voc_eval_evaluate_ms=round(ref_ms, 1),
                          ratio=round(ref_ms / gpu_ms, 1), map_evaluator_runs_ms=[round(t, 3) for t in gpu_all],
                          voc_eval_runs_ms=[round(t, 1) for t in ref_all])))
else:
    from k210_yolo_framework_amd import netspec, training
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.train import Trainer
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    spec = netspec.NETWORKS['yolo_mobilev2']([224, 320, 3], 3, 20, alpha=1.0)
    h = Helper(None, 20, VOC_ANCHORS, np.array([[224, 320]]), np.array(spec.out_hw()))
    h.test_list = training.synthetic_list(16, (224, 320), 20, 5)
    tr = Trainer(spec, spec.init_keras_default(3), h.anchors, 16)
    res = {}

    def plain():
        res['val_loss'] = training.validate(tr, h, spec, 16, 0)

    def with_map():
        res['with_map'] = training.validate(tr, h, spec, 16, 0, map_obj=0.05)

    a, a_all = median_ms(plain, runs)
    b, b_all = median_ms(with_map, runs)
    print(json.dumps(dict(network='yolo_mobilev2-1.0', images=16, runs=runs, validate_ms=round(a, 2), validate_with_val_map_ms=round(b, 2),
                          added_ms=round(b - a, 2), val_loss=res['val_loss'], val_loss_and_map=list(res['with_map']),
                          validate_runs_ms=[round(t, 2) for t in a_all], with_map_runs_ms=[round(t, 2) for t in b_all])))

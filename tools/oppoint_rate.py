"""Rate of the operating points alone: MapEvaluator.result(), .sweep() with 1000 thresholds and .confusion(0.6) against their host statements
(voc_eval.evaluate, oppoint.sweep, oppoint.confusion) on the same rows, and result() of this library against result() of another build of it
(profiles/oppoint_rate.txt).
  python tools/oppoint_rate.py [images=4952] [classes=20] [runs=5] [other_root=]
Seeded VOC07-test-sized input as tools/coco_rate.py draws it: ~10 detections and ~2.5 ground-truth boxes per image.  The rows are added once
(device-resident).  The three calls are timed synchronised, in turn, `runs` times after one warm-up round: the median of each.  The host
statements are interpreted Python: each is timed ONCE, after the device result has been compared with it.
other_root: a built checkout of another commit (the parent's).  result() is then also timed in fresh child processes, this checkout's
package and the other one's in turn, `runs` times each; a child prints the median of `runs` calls after one warm-up."""
import json
import os
import statistics
import subprocess
import sys
import time

only_result = '--only-result' in sys.argv
argv = [v for v in sys.argv[1:] if v != '--only-result']
arg = lambda k, d: int(argv[k]) if len(argv) > k else d
n_img, class_num, runs = arg(0, 4952), arg(1, 20), arg(2, 5)
other_root = os.path.abspath(argv[3]) if len(argv) > 3 else ''
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, other_root if only_result and other_root else root)           # a child imports the package of the checkout it times
import numpy as np
import torch
from k210_yolo_framework_amd import engine
from k210_yolo_framework_amd.map_gpu import MapEvaluator

engine.require_gpu()
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
off[1:] = np.cumsum([len(x) for x in dets])
ev = MapEvaluator(class_num)
ev.add(torch.from_numpy(np.concatenate(dets)).cuda(), torch.from_numpy(off).cuda(), gts)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


if only_result:
    ev.result()
    print(json.dumps(dict(result_ms=round(statistics.median(timed(ev.result)[1] for _ in range(runs)), 3))))
    sys.exit(0)

from k210_yolo_framework_amd import oppoint, voc_eval
CONF = 0.6
calls = {'result': ev.result, 'sweep': ev.sweep, 'confusion': lambda: ev.confusion(CONF)}
got = {k: fn() for k, fn in calls.items()}                                          # the warm-up round
ms = {k: [] for k in calls}
for _ in range(runs):
    for k, fn in calls.items():
        ms[k].append(timed(fn)[1])
host, host_ms = {}, {}
host['result'], host_ms['result'] = timed(lambda: voc_eval.evaluate(dets, gts, class_num))
host['sweep'], host_ms['sweep'] = timed(lambda: oppoint.sweep(dets, gts, class_num, np.arange(1000) / 1000))
host['confusion'], host_ms['confusion'] = timed(lambda: oppoint.confusion(dets, gts, class_num, CONF))
assert all(np.array_equal(got['result'][k], host['result'][k]) for k in ('tp', 'fp', 'n_gt', 'n_det')), 'result differs'
assert all(np.array_equal(got['sweep'][k], host['sweep'][k]) for k in ('tp', 'fp', 'best', 'flags')), 'sweep differs'
assert all(got['sweep'][k].tobytes() == host['sweep'][k].tobytes() for k in ('precision', 'recall', 'f1', 'mean_f1')), 'curves differ'
assert all(np.array_equal(got['confusion'][k], host['confusion'][k]) for k in ('matrix', 'match')), 'confusion differs'
out = dict(images=n_img, classes=class_num, detections=int(ev.n_rows), ground_truth=int(sum(len(x) for x in gts)), runs=runs, conf=CONF,
           map=got['result']['map'], best_threshold=float(got['sweep']['thresholds'][got['sweep']['best_all']]),
           best_mean_f1=float(got['sweep']['mean_f1'][got['sweep']['best_all']]), rows_at_conf=int((got['confusion']['match'] > -2).sum()),
           matched_at_conf=int((got['confusion']['match'] >= 0).sum()))
for k in calls:
    med = statistics.median(ms[k])
    out[k] = dict(ms=round(med, 3), runs_ms=[round(t, 3) for t in ms[k]], host_ms_once=round(host_ms[k], 1), host_ratio=round(host_ms[k] / med, 1))
if other_root:
    ab = {'this': [], 'other': []}
    for _ in range(runs):
        for who, where in (('other', other_root), ('this', root)):
            line = subprocess.run([sys.executable, os.path.abspath(__file__), str(n_img), str(class_num), str(runs), where, '--only-result'],
                                  check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
            ab[who].append(json.loads(line)['result_ms'])
    out['result_ab'] = dict(this_ms=ab['this'], other_ms=ab['other'], this_median=statistics.median(ab['this']),
                            other_median=statistics.median(ab['other']))
print(json.dumps(out))

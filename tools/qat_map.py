#!/usr/bin/env python
"""What quantisation-aware fine-tuning buys (profiles/qat_map.txt), on the protocol of profiles/r05_map_eval.json: train a
yolo_mobilev1-0.75 on generated images with known boxes, then score on the same unseen generated images (voc_eval.py, IoU 0.5)
  (a) the float checkpoint (f16x2),
  (b) its post-training kmodel (calibrated on 256 generated images, as `make kmodel SYNTHETIC=256`), precision 'kpu',
  (c) the kmodel of the same checkpoint after one QAT epoch, quantised with the learned ranges (`--ranges`), precision 'kpu'.

    python tools/qat_map.py [--steps 2500] [--train 2048] [--eval 1024] [--out profiles/qat_map.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from k210_yolo_framework_amd import engine, kmodel, netspec, quantize, training, voc_eval  # noqa: E402
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS  # noqa: E402
from k210_yolo_framework_amd.inference import detect  # noqa: E402
from k210_yolo_framework_amd.pipeline import InputPipeline  # noqa: E402
from k210_yolo_framework_amd.qat import QatConfig  # noqa: E402
from k210_yolo_framework_amd.train import Trainer  # noqa: E402
from k210_yolo_framework_amd.yolonet import MODEL_DEFS  # noqa: E402
from tools.map_eval import ground_truth_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=2500)
ap.add_argument('--train', type=int, default=2048)
ap.add_argument('--eval', type=int, default=1024)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--lr', type=float, default=1e-3)
ap.add_argument('--qat_lr', type=float, default=1e-4)
ap.add_argument('--observe', type=int, default=8)
ap.add_argument('--out', default='profiles/qat_map.txt')
a = ap.parse_args()

IN_HW, CAM_HW, C = (224, 320), (240, 320), 20
h = Helper(None, C, VOC_ANCHORS, np.array([IN_HW]), np.array([[7, 10], [14, 20]]))
h.batch_size = a.batch
train_items = training.synthetic_list(a.train, CAM_HW, C, seed=1)
eval_items = training.synthetic_list(a.eval, CAM_HW, C, seed=99)
spec = netspec.yolo_mobilev1((*IN_HW, 3), 3, C, alpha=0.75)
HYPER = dict(obj_thresh=0.7, iou_thresh=0.3, obj_weight=5.0, noobj_weight=0.5, wh_weight=0.5, decay=0.0)      # the Makefile's training defaults
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def run(tr, steps, observe=0):
    done, epoch, seen, last = 0, 0, 0, None
    while done < steps:
        pipe = InputPipeline(h, train_items, a.batch, 0, 1, seed=6, epoch=epoch, shuffle=True, device=0)
        try:
            for x, ys in pipe:
                if seen < observe:
                    tr.qat_observe(x)
                    seen += 1
                    continue
                last = tr.step(x, ys)['loss']
                done += 1
                if done >= steps:
                    break
        finally:
            pipe.close()
        epoch += 1
    return last


def score(model, tag):
    imgs = [it[0] for it in eval_items]
    gts = [ground_truth_rows(it[1], CAM_HW) for it in eval_items]
    out = {}
    for obj in (0.05, 0.7):
        d = []
        for k in range(0, len(imgs), 32):
            d += detect(h, model, imgs[k:k + 32], obj, 0.5)
        out[obj] = 100 * float(voc_eval.evaluate(d, gts, C, 0.5)['map'])
    say(f'  {tag:<44} mAP {out[0.05]:7.3f} (obj_thresh 0.05)   {out[0.7]:7.3f} (obj_thresh 0.7)')
    return out


def kpu_model(km):
    m, _ = MODEL_DEFS['yolo_mobilev1']([*IN_HW, 3], 3, C, alpha=0.75, precision='kpu')
    w, _ = kmodel.to_float_weights(km, spec)
    m.set_weights(w)
    m._s['kmodel'] = km
    return m


t0 = time.time()
tr = Trainer(spec, spec.init_keras_default(6), h.anchors, a.batch, lr=a.lr, **HYPER)
loss = run(tr, a.steps)
weights = tr.export_weights()
del tr
say(f'yolo_mobilev1-0.75, {a.train} generated training images, {a.steps} float steps of {a.batch} (lr {a.lr}): last loss {loss:.3f}, {time.time() - t0:.0f} s; '
    f'{a.eval} unseen generated images, voc_eval area AP at IoU 0.5')
fm, _ = MODEL_DEFS['yolo_mobilev1']([*IN_HW, 3], 3, C, alpha=0.75, precision='f16x2')
fm.set_weights(weights)
f = score(fm, '(a) float checkpoint, f16x2')
frames = quantize.synthetic_frames(256, IN_HW, 3)
km_ptq, rep_ptq = quantize.quantize(spec, weights, quantize.calibrate(spec, weights, frames, 32))
p = score(kpu_model(km_ptq), '(b) post-training kmodel, kpu')
t1 = time.time()
qsteps = a.train // a.batch
tq = Trainer(spec, weights, h.anchors, a.batch, lr=a.qat_lr, qat=QatConfig(0.99), **HYPER)
loss = run(tq, qsteps, a.observe)
wq, ranges = tq.export_weights(), tq.qat_ranges()
del tq
say(f'one QAT epoch from (a): {a.observe} observed batches + {qsteps} steps (lr {a.qat_lr}, momentum 0.99), last loss {loss:.3f}, {time.time() - t1:.0f} s')
km_qat, rep_qat = quantize.quantize(spec, wq, ranges)
q = score(kpu_model(km_qat), '(c) kmodel after one QAT epoch (--ranges), kpu')
for obj in (0.05, 0.7):
    say(f'  gap to float at obj_thresh {obj}: post-training {p[obj] - f[obj]:+.3f} points, after QAT {q[obj] - f[obj]:+.3f} points')
say('per-layer report of (b):')
say(quantize.format_report(rep_ptq))
say('per-layer report of (c):')
say(quantize.format_report(rep_qat))
Path(ROOT / a.out).write_text('\n'.join(lines) + '\n')

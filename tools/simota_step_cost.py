#!/usr/bin/env python3
"""What SimOTA costs per training step: Trainer.step of yolo_mobilev2-1.0 at 16 images, box_loss ciou, labels built on the GPU, with
assign 'best' (the label kernel runs before the step, as InputPipeline(labels='gpu') does) and with assign 'simota' (the step assigns).
Medians of REPEATS alternating repeats of STEPS steps after a warm-up, the spread (min .. max of the repeat means) beside each; appended to
profiles/simota_step_cost.txt under --label.  Run it in a checkout of the parent commit with --only best for the third figure."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REPEATS, STEPS, WARMUP, B, MAXB = 5, 40, 10, 16, 64


def main():
    import torch
    from k210_yolo_framework_amd import engine, netspec as ns
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.train import Trainer
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', default='this tree')
    ap.add_argument('--only', choices=['best', 'simota'])
    a = ap.parse_args()
    spec = ns.yolo_mobilev2((224, 320, 3), 3, 20, 1.0)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [list(v) for v in spec.out_hw()])
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(0, 1, (B, 224, 320, 3)).astype(np.float32)).cuda()
    counts = rng.integers(1, 6, B)
    N = int(counts.sum())
    boxes = np.zeros((B * MAXB, 5))
    boxes[:N] = np.stack([rng.integers(0, 20, N), rng.uniform(.2, .8, N), rng.uniform(.2, .8, N), rng.uniform(.1, .6, N), rng.uniform(.1, .6, N)], 1)
    d_boxes, d_first = torch.from_numpy(boxes).cuda(), torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    modes = [m for m in ('best', 'simota') if a.only in (None, m)]
    trs = {m: Trainer(spec, spec.init_weights(0), h.anchors, B, box_loss='ciou', **(dict(assign='simota', ota_max_boxes=MAXB) if m == 'simota' else {}))
           for m in modes}
    label_cfg = engine.make_label_cfg(h)

    def steps(m, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            if m == 'best':
                trs[m].step(x, engine.boxes_to_labels(d_boxes[:N], d_first, label_cfg)[0])
            else:
                trs[m].step(x, engine.BoxBatch(d_boxes, d_first))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    for m in modes:
        steps(m, WARMUP)
    means = {m: [] for m in modes}
    for _ in range(REPEATS):                                          # alternating: drift hits every configuration alike
        for m in modes:
            means[m].append(steps(m, STEPS))
    lines = [f'[{a.label}] Trainer.step, yolo_mobilev2-1.0, {B} images 224x320, ciou, {N} boxes, {REPEATS} x {STEPS} steps after {WARMUP}']
    for m in modes:
        lines.append(f'  assign {m:7s} median {statistics.median(means[m]):.3f} ms/step, spread {min(means[m]):.3f} .. {max(means[m]):.3f}')
    out = ROOT / 'profiles' / 'simota_step_cost.txt'
    with open(out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()

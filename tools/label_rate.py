#!/usr/bin/env python
"""Producer rate of the training input pipeline with the labels built on the host and on the GPU (DESIGN.md 3.26;
`InputPipeline.producer_images_per_sec()`), on the protocol of tools/hsv_rate.py: in-memory frames, the picture cache warm (CACHE=gpu: no
pixel crosses PCIe, so the labels are the largest thing the producer still writes and sends), per-rank batch 16, one rank; the modes
alternate, `--reps` times each, after one warm-up epoch of each, so the spread of a mode's repeats is the run-to-run spread.  Three label
shapes: yolo_mobilev1 224x320 (7x10, 14x20) at 20 classes, and the three-scale 416x416 shape (13, 26, 52) at 20 and 80 classes.

Also: the time of one `yk_boxes_to_labels_f32` call on the largest shape (HIP events around `--calls` back-to-back calls: launch cost
included, not a kernel trace), the label bytes that cross PCIe per batch in both modes (arithmetic on the shapes), and the mean number of
positives per box under assign='multi', assign_iou=0.213 with data/voc_anchor.npy on the generated training boxes (host arithmetic).

`--modes host --root DIR` measures the package of another checkout (the parent commit, which has no `labels=`) with the same script and
inputs; `--append` adds its lines to the same file.

    python tools/label_rate.py [--reps 5] [--n 256] [--shapes NAME,..] [--out profiles/label_rate.txt]
"""
import argparse
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--n', type=int, default=256, help='distinct in-memory frames')
ap.add_argument('--times', type=int, default=8, help='the list names every frame this often: an epoch of n * times samples')
ap.add_argument('--modes', default='host,gpu')
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--shapes', default='', help='comma list of shape names to measure (default: all three)')
ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'), help='checkout whose package is measured')
ap.add_argument('--label', default='this commit')
ap.add_argument('--out', default='profiles/label_rate.txt')
ap.add_argument('--append', action='store_true')
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
lines = []

# yolov3.cfg's anchors over 416, coarse layer first, as Helper wants them
V3_ANCHORS = np.array([[[116, 90], [156, 198], [373, 326]], [[30, 61], [62, 45], [59, 119]], [[10, 13], [16, 30], [33, 23]]], float) / 416
SHAPES = [('mobilev1_224x320_c20', (224, 320), [[7, 10], [14, 20]], None, 20),
          ('darknet53_416x416_c20', (416, 416), [[13, 13], [26, 26], [52, 52]], V3_ANCHORS, 20),
          ('darknet53_416x416_c80', (416, 416), [[13, 13], [26, 26], [52, 52]], V3_ANCHORS, 80)]


def say(s):
    print(s, flush=True)
    lines.append(s)


def _helper(in_hw, out_hw, anchors, class_num):
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    return Helper(None, class_num, VOC_ANCHORS if anchors is None else anchors, [list(in_hw)], out_hw)


def _items(in_hw, class_num, n, times):
    rng = np.random.default_rng(0)
    items = []
    for _ in range(n):
        k = int(rng.integers(1, 4))
        boxes = np.concatenate([rng.integers(0, class_num, (k, 1)).astype(float), rng.uniform(0.2, 0.8, (k, 2)), rng.uniform(0.05, 0.4, (k, 2))], 1)
        items.append((rng.integers(0, 256, (*in_hw, 3), dtype=np.uint8), boxes))
    return items * times


def _epoch(h, items, mode, epoch, cache):
    import torch
    from k210_yolo_framework_amd import pipeline
    pipe = pipeline.InputPipeline(h, items, 16, 0, 1, seed=1, epoch=epoch, shuffle=True, cache=cache, **({'labels': 'gpu'} if mode == 'gpu' else {}))
    for _ in pipe:
        pass
    torch.cuda.synchronize()
    rate = pipe.producer_images_per_sec()
    pipe.close()
    return rate


def rates():
    from k210_yolo_framework_amd.cache import PictureCache
    modes = a.modes.split(',')
    say(f'[{a.label}] producer_images_per_sec (samples/s), epochs of {a.n * a.times} samples, batch 16, one rank, picture cache warm, {a.reps} alternating '
        f'repeats after a warm-up epoch of each mode')
    for name, in_hw, out_hw, anchors, class_num in SHAPES:
        if a.shapes and name not in a.shapes.split(','):
            continue
        h = _helper(in_hw, out_hw, anchors, class_num)
        items = _items(in_hw, class_num, a.n, a.times)
        with PictureCache(a.n * in_hw[0] * in_hw[1] * 3 + (64 << 20), stage_bytes=64 << 20) as cache:
            runs = {m: [] for m in modes}
            for e, m in enumerate(modes):
                _epoch(h, items, m, e, cache)                                   # warm: the cache, the pinned rings, the allocator
            for r in range(a.reps):
                for m in modes:
                    runs[m].append(_epoch(h, items, m, 10 + r, cache))
        med = {}
        for m in modes:
            v = np.array(runs[m])
            med[m] = float(np.median(v))
            say(f'[{a.label}] {name:24s} labels={m:4s} median {med[m]:8.0f}   runs ' + ' '.join(f'{x:.0f}' for x in v) +
                f'   spread (max-min)/median {100 * (v.max() - v.min()) / med[m]:.1f} %')
        if 'host' in med and 'gpu' in med:
            say(f'[{a.label}] {name:24s} gpu / host = {med["gpu"] / med["host"]:.2f}')


def kernel_time():
    import torch
    from k210_yolo_framework_amd import engine
    name, in_hw, out_hw, anchors, class_num = SHAPES[-1]
    h = _helper(in_hw, out_hw, anchors, class_num)
    rng = np.random.default_rng(1)
    per = [np.concatenate([rng.integers(0, class_num, (3, 1)).astype(float), rng.uniform(0.2, 0.8, (3, 2)), rng.uniform(0.05, 0.4, (3, 2))], 1) for _ in range(16)]
    boxes = torch.from_numpy(np.concatenate(per)).cuda()
    first = torch.arange(0, 49, 3, dtype=torch.int32).cuda()
    for assign in ('best', 'multi'):
        cfg = engine.make_label_cfg(h, assign, 0.213)
        views, status = engine.boxes_to_labels(boxes, first, cfg)
        out = views[0].new_empty((sum(v.numel() for v in views),))
        for _ in range(20):
            engine.boxes_to_labels(boxes, first, cfg, out=out, status=status)
        t = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                engine.boxes_to_labels(boxes, first, cfg, out=out, status=status)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / a.calls * 1e3)
        say(f'[{a.label}] yk_boxes_to_labels_f32 {name} batch 16, 48 boxes, assign={assign}: {np.median(t):.1f} us per call (HIP events around {a.calls} '
            f'back-to-back calls, 5 repeats: ' + ' '.join(f'{x:.1f}' for x in t) + f'); it writes {out.numel() * 4 / 1e6:.1f} MB')


def arithmetic():
    from k210_yolo_framework_amd import training
    for name, in_hw, out_hw, anchors, class_num in SHAPES:
        dense = 16 * sum(gh * gw for gh, gw in out_hw) * 3 * (5 + class_num) * 4
        say(f'label bytes per batch of 16, {name}: host 16 x {sum(gh * gw for gh, gw in out_hw)} cells x 3 anchors x {5 + class_num} floats x 4 = {dense} B; '
            f'gpu N boxes x 40 B + 17 offsets x 4 B + 4 B of status back = {32 * 40 + 68 + 4} B at the 2 boxes per sample of the generated lists')
    h = _helper((224, 320), [[7, 10], [14, 20]], np.load(os.path.join(HERE, 'data', 'voc_anchor.npy')), 20)
    items = training.synthetic_list(256, (224, 320), 20, 3)
    items = items[int(len(items) * 0.05):]                                       # the training split of make train SYNTHETIC=256
    boxes = [b for _, b in items]
    n_boxes = sum(len(b) for b in boxes)
    pos = lambda grids: int(sum((g[..., 4] == 1).sum() for g in grids))
    say(f'positives per box, data/voc_anchor.npy, the {n_boxes} generated training boxes of SYNTHETIC=256 (seed 3): assign=best '
        f'{pos(h.batch_box_to_label(boxes)) / n_boxes:.3f}, assign=multi assign_iou=0.213 {pos(h.batch_box_to_label(boxes, "multi", 0.213)) / n_boxes:.3f} '
        f'(slots, after collisions)')


rates()
if a.modes == 'host,gpu':
    kernel_time()
    arithmetic()
out = a.out if os.path.isabs(a.out) else os.path.join(HERE, a.out)
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, 'a' if a.append else 'w') as f:
    f.write('\n'.join(lines) + '\n')

"""Producer rate of the training input pipeline with and without augmentation (`InputPipeline.producer_images_per_sec()`).

Two inputs, per-rank batch 16, one rank: in-memory 224x320 frames, and a list of JPEG files of mixed sizes (VOC-like).  For each
input the two modes alternate, `--reps` times each, after one warm-up epoch of each; one JSON line per epoch and a summary line.
The consumer takes batches as they come (the rate is the producer's alone).

    python tools/pipeline_rate.py [--reps 3] [--n 1024] [--files 512]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def _boxes(rng):
    n = int(rng.integers(1, 4))
    return np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.05, 0.4, (n, 2))], 1)


def _epoch(h, items, augment, epoch):
    import torch
    from k210_yolo_framework_amd import pipeline
    pipe = pipeline.InputPipeline(h, items, 16, 0, 1, seed=1, epoch=epoch, shuffle=True, augment=augment)
    t0 = time.perf_counter()
    n = 0
    for x, _ in pipe:
        n += x.shape[0]
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rate = pipe.producer_images_per_sec()
    pipe.close()
    return rate, n / wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--n', type=int, default=1024, help='in-memory frames')
    ap.add_argument('--files', type=int, default=512, help='JPEG files of mixed sizes')
    a = ap.parse_args()
    import torch
    from PIL import Image
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    engine.require_gpu()
    torch.cuda.set_device(0)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    rng = np.random.default_rng(0)
    mem = [(rng.integers(0, 256, (224, 320, 3), dtype=np.uint8), _boxes(rng)) for _ in range(a.n)]
    with tempfile.TemporaryDirectory() as d:
        files = []
        sizes = [(375, 500), (333, 500), (500, 375), (281, 500), (240, 320), (480, 640)]
        for k in range(a.files):
            hw = sizes[k % len(sizes)]
            p = os.path.join(d, f'{k}.jpg')
            Image.fromarray(rng.integers(0, 256, (*hw, 3), dtype=np.uint8)).save(p, quality=90)
            files.append((p, _boxes(rng)))
        summary = {}
        for name, items in (('memory_224x320', mem), ('files_mixed', files)):
            for aug in (False, True):
                _epoch(h, items, aug, 0)                                        # warm-up: code objects, pinned rings, allocator
            runs = {False: [], True: []}
            for r in range(a.reps):
                for aug in (False, True):
                    rate, wall = _epoch(h, items, aug, r + 1)
                    runs[aug].append(rate)
                    print(json.dumps({'input': name, 'augment': aug, 'rep': r, 'producer_images_per_sec': round(rate, 1),
                                      'consumed_images_per_sec': round(wall, 1)}), flush=True)
            summary[name] = {'off': [round(v) for v in runs[False]], 'on': [round(v) for v in runs[True]],
                             'ratio_of_medians': round(float(np.median(runs[True]) / np.median(runs[False])), 3)}
        print(json.dumps({'summary': summary}), flush=True)


if __name__ == '__main__':
    main()

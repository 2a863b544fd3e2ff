#!/usr/bin/env python
"""Producer rate of the training input pipeline with mosaic off, mosaic on, and mosaic + augmentation (DESIGN.md 3.15;
`InputPipeline.producer_images_per_sec()`), on the inputs of tools/pipeline_rate.py: in-memory 224x320 frames, and JPEG files of mixed
sizes (VOC-like).  Per-rank batch 16, one rank; the modes alternate, `--reps` times each, after one warm-up epoch of each, so the spread of
a mode's repeats is the run-to-run spread.  A mosaic decodes up to four pictures per sample: the rate counts SAMPLES.

`--modes off --root DIR` measures the package of another checkout (the parent commit, which has no mosaic) with the same script and inputs;
`--append` adds its lines to the same file.

    python tools/mosaic_rate.py [--reps 3] [--n 1024] [--files 512] [--out profiles/mosaic_rate.txt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--n', type=int, default=1024, help='in-memory frames')
ap.add_argument('--files', type=int, default=512, help='JPEG files of mixed sizes')
ap.add_argument('--modes', default='off,mosaic,mosaic+iaa')
ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'), help='checkout whose package is measured')
ap.add_argument('--label', default='this commit')
ap.add_argument('--step_rate', type=float, default=3500.0, help='images/s of the training step the producer has to outrun')
ap.add_argument('--out', default='profiles/mosaic_rate.txt')
ap.add_argument('--append', action='store_true')
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def _boxes(rng):
    n = int(rng.integers(1, 4))
    return np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.05, 0.4, (n, 2))], 1)


def _epoch(h, items, mode, epoch):
    import torch
    from k210_yolo_framework_amd import pipeline
    kw = {}
    if mode != 'off':
        from k210_yolo_framework_amd.mosaic import MosaicConfig
        kw['mosaic'] = MosaicConfig(1.0)
    pipe = pipeline.InputPipeline(h, items, 16, 0, 1, seed=1, epoch=epoch, shuffle=True, augment=mode.endswith('+iaa'), **kw)
    for _ in pipe:
        pass
    torch.cuda.synchronize()
    rate = pipe.producer_images_per_sec()
    pipe.close()
    return rate


def main():
    import torch
    from PIL import Image
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    engine.require_gpu()
    torch.cuda.set_device(0)
    modes = a.modes.split(',')
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    rng = np.random.default_rng(0)
    mem = [(rng.integers(0, 256, (224, 320, 3), dtype=np.uint8), _boxes(rng)) for _ in range(a.n)]
    say(f'[{a.label}] producer_images_per_sec (samples/s), batch 16, one rank, 8 decode threads, {a.reps} alternating repeats after a warm-up epoch of each '
        f'mode; {time.strftime("%Y-%m-%d")}')
    with tempfile.TemporaryDirectory() as d:
        files = []
        sizes = [(375, 500), (333, 500), (500, 375), (281, 500), (240, 320), (480, 640)]
        for k in range(a.files):
            p = os.path.join(d, f'{k}.jpg')
            Image.fromarray(rng.integers(0, 256, (*sizes[k % len(sizes)], 3), dtype=np.uint8)).save(p, quality=90)
            files.append((p, _boxes(rng)))
        for name, items in ((f'memory_224x320 x{a.n}', mem), (f'jpeg_files_mixed x{a.files}', files)):
            for m in modes:
                _epoch(h, items, m, 0)                                          # warm-up: code objects, pinned rings, allocator
            runs = {m: [] for m in modes}
            for r in range(a.reps):
                for m in modes:
                    runs[m].append(_epoch(h, items, m, r + 1))
            for m in modes:
                v = np.array(runs[m])
                say(f'[{a.label}] {name:<24} {m:<11} median {np.median(v):8.0f}   runs {" ".join(f"{x:.0f}" for x in v)}   '
                    f'spread (max-min)/median {100 * (v.max() - v.min()) / np.median(v):.1f} %   '
                    f'{"outruns" if np.median(v) > a.step_rate else "does NOT outrun"} the {a.step_rate:.0f} images/s step')
    with open(os.path.join(HERE, a.out), 'a' if a.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

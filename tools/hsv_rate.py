#!/usr/bin/env python
"""Producer rate of the training input pipeline with the HSV colour jitter off and on (DESIGN.md 3.16;
`InputPipeline.producer_images_per_sec()`), on the protocol of tools/mosaic_rate.py: in-memory 224x320 frames, per-rank batch 16, one
rank; the modes alternate, `--reps` times each, after one warm-up epoch of each, so the spread of a mode's repeats is the run-to-run spread.
An epoch there is 1024 samples, 40 ms of producer time; here the list names each frame `--times` times, so a repeat times 8192 samples.

`--modes off --root DIR` measures the package of another checkout (the parent commit, which has no jitter) with the same script and inputs;
`--append` adds its lines to the same file.

    python tools/hsv_rate.py [--reps 5] [--n 1024] [--out profiles/hsv_rate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--n', type=int, default=1024, help='distinct in-memory frames')
ap.add_argument('--times', type=int, default=8, help='the list names every frame this often: an epoch of n * times samples, a third of a second')
ap.add_argument('--modes', default='off,hsv')
ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'), help='checkout whose package is measured')
ap.add_argument('--label', default='this commit')
ap.add_argument('--step_rate', type=float, default=3500.0, help='images/s of the training step the producer has to outrun')
ap.add_argument('--out', default='profiles/hsv_rate.txt')
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
        from k210_yolo_framework_amd.colour import HsvConfig
        kw['hsv'] = HsvConfig()
    pipe = pipeline.InputPipeline(h, items, 16, 0, 1, seed=1, epoch=epoch, shuffle=True, **kw)
    for _ in pipe:
        pass
    torch.cuda.synchronize()
    rate = pipe.producer_images_per_sec()
    pipe.close()
    return rate


def main():
    import torch
    import k210_yolo_framework_amd
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    engine.require_gpu()
    torch.cuda.set_device(0)
    modes = a.modes.split(',')
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    rng = np.random.default_rng(0)
    mem = [(rng.integers(0, 256, (224, 320, 3), dtype=np.uint8), _boxes(rng)) for _ in range(a.n)]
    mem = mem * a.times
    say(f'[{a.label}] producer_images_per_sec (samples/s), epochs of {len(mem)} samples, batch 16, one rank, {a.reps} alternating repeats after a warm-up epoch of each mode; '
        f'package {os.path.relpath(os.path.dirname(k210_yolo_framework_amd.__file__), HERE)}; {time.strftime("%Y-%m-%d")}')
    for m in modes:
        _epoch(h, mem, m, 0)                                                # warm-up: code objects, pinned rings, allocator
    runs = {m: [] for m in modes}
    for r in range(a.reps):
        for m in modes:
            runs[m].append(_epoch(h, mem, m, r + 1))
    med = {}
    for m in modes:
        v = np.array(runs[m])
        med[m] = float(np.median(v))
        say(f'[{a.label}] memory_224x320 x{len(mem)}   {m:<4} median {np.median(v):8.0f}   runs {" ".join(f"{x:.0f}" for x in v)}   '
            f'spread (max-min)/median {100 * (v.max() - v.min()) / np.median(v):.1f} %   '
            f'{"outruns" if np.median(v) > a.step_rate else "does NOT outrun"} the {a.step_rate:.0f} images/s step')
    if 'off' in med and 'hsv' in med:
        say(f'[{a.label}] hsv / off = {med["hsv"] / med["off"]:.3f}')
    with open(os.path.join(HERE, a.out), 'a' if a.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

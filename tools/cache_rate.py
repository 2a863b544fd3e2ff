#!/usr/bin/env python
"""What the device-resident picture cache (cache.py; `make train CACHE=gpu DECODE=gpu`) does to the producer of the training
input pipeline, by tools/mosaic_rate.py's protocol: the same generated JPEG files of mixed sizes (VOC-like), 8 decode threads, per-rank
batch 16, one rank, `InputPipeline.producer_images_per_sec()` in SAMPLES per second, medians of `--reps` alternating repeats after a
warm-up epoch of every row.  Rows: {plain, mosaic, mosaic+iaa+hsv} x {off, cache first epoch, cache later epoch} x {pil, gpu}:

  off          InputPipeline without a cache (decode pil: the parent commit's path, launch for launch - the baseline of this file;
               decode gpu: the staging ring alone, CACHE=off DECODE=gpu)
  cache first  a new, empty cache: every picture is a miss, decoded and admitted
  cache later  the cache the warm-up epoch filled: every picture is a hit

Then the training step's own rate in the same session (tools/train_step.py in a child process) - what the producer has to outrun - and the
wall time per epoch of `make train`'s entry on the same files, without and with --cache gpu.

    python tools/cache_rate.py [--reps 3] [--files 512] [--epochs 3] [--out profiles/cache_rate.txt]
"""
import argparse
import contextlib
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--files', type=int, default=512, help='JPEG files of mixed sizes')
ap.add_argument('--epochs', type=int, default=3, help='epochs of the two training runs (0: skip them)')
ap.add_argument('--cache_gb', type=float, default=1.0)
ap.add_argument('--cache_stage_mb', type=float, default=128.0)
ap.add_argument('--out', default='profiles/cache_rate.txt')
a = ap.parse_args()
HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, HERE)
MODES = ('plain', 'mosaic', 'mosaic+iaa+hsv')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def _boxes(rng):
    n = int(rng.integers(1, 4))
    return np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.05, 0.4, (n, 2))], 1)


def _epoch(h, items, mode, epoch, cache=None, decode='pil'):
    import torch
    from k210_yolo_framework_amd import pipeline
    from k210_yolo_framework_amd.colour import HsvConfig
    from k210_yolo_framework_amd.mosaic import MosaicConfig
    kw = {}
    if mode != 'plain':
        kw['mosaic'] = MosaicConfig(1.0)
    if mode.endswith('+iaa+hsv'):
        kw.update(augment=True, hsv=HsvConfig())
    if cache is not None or decode == 'gpu':
        kw.update(cache=cache, decode=decode)
    pipe = pipeline.InputPipeline(h, items, 16, 0, 1, seed=1, epoch=epoch, shuffle=True, **kw)
    for _ in pipe:
        pass
    torch.cuda.synchronize()
    rate = pipe.producer_images_per_sec()
    pipe.close()
    return rate


def _train(folder, extra):
    """`make train`'s entry on the list of `folder` (its data/voc_img_ann.npy): -> seconds of every epoch, from the epoch lines."""
    from k210_yolo_framework_amd import training
    out = io.StringIO()
    cwd = os.getcwd()
    os.chdir(folder)
    try:
        with contextlib.redirect_stdout(out):
            training.cli(['--model_def', 'yolo_mobilev2', '--depth_multiplier', '1.0', '--batch_size', '16', '--max_nrof_epochs', str(a.epochs),
                          '--vaildation_split', '0.05', '--mosaic', 'True', '--hsv', 'True', '--box_loss', 'ciou', '--log_dir',
                          os.path.join(folder, 'log')] + extra)
    finally:
        os.chdir(cwd)
    return [l for l in out.getvalue().splitlines() if re.match(r'epoch \d+: \d+ steps', l)]


def main():
    import torch
    from PIL import Image
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.cache import PictureCache
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    engine.require_gpu()
    torch.cuda.set_device(0)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    rng = np.random.default_rng(0)
    new_cache = lambda: PictureCache(int(a.cache_gb * (1 << 30)), int(a.cache_stage_mb * (1 << 20)))
    say(f'producer_images_per_sec (samples/s), batch 16, one rank, 8 decode threads, {a.reps} alternating repeats after a warm-up epoch of each row; '
        f'cache {a.cache_gb} GB, staging regions of {a.cache_stage_mb} MB; {time.strftime("%Y-%m-%d")}')
    with tempfile.TemporaryDirectory() as d:
        files = []
        sizes = [(375, 500), (333, 500), (500, 375), (281, 500), (240, 320), (480, 640)]
        for k in range(a.files):
            p = os.path.join(d, f'{k}.jpg')
            Image.fromarray(rng.integers(0, 256, (*sizes[k % len(sizes)], 3), dtype=np.uint8)).save(p, quality=90)
            files.append((p, _boxes(rng)))
        name = f'jpeg_files_mixed x{a.files}'
        rows = [(m, c, dec) for m in MODES for dec in ('pil', 'gpu') for c in ('off', 'cache first', 'cache later')]
        warm = {}
        for m, c, dec in rows:                                              # warm-up: code objects, pinned rings, allocator - and the warm caches
            if c == 'off':
                _epoch(h, files, m, 0, decode=dec)
            elif c == 'cache later':
                warm[(m, dec)] = new_cache()
                _epoch(h, files, m, 0, cache=warm[(m, dec)], decode=dec)
        runs = {r: [] for r in rows}
        for r in range(a.reps):
            for m, c, dec in rows:
                if c == 'off':
                    runs[(m, c, dec)].append(_epoch(h, files, m, r + 1, decode=dec))
                elif c == 'cache first':
                    with new_cache() as cache:
                        runs[(m, c, dec)].append(_epoch(h, files, m, r + 1, cache=cache, decode=dec))
                else:
                    runs[(m, c, dec)].append(_epoch(h, files, m, r + 1, cache=warm[(m, dec)], decode=dec))
        for (m, dec), cache in warm.items():
            s = cache.stats()
            say(f'warm cache {m:<15} {dec}: {s.hits} hits, {s.misses} misses, {s.admitted} pictures, {s.bytes_used / 2 ** 20:.0f} MiB of {s.capacity / 2 ** 20:.0f}')
            cache.close()
        step = subprocess.run([sys.executable, os.path.join(HERE, 'tools', 'train_step.py'), '30'], capture_output=True, text=True, cwd=HERE)
        step_rate = None
        for l in step.stdout.splitlines():
            if l.startswith('{'):
                step_rate = 16e3 / json.loads(l)['step_ms']
        say('training step (tools/train_step.py, yolo_mobilev2-1.0, 16 images, this session): ' +
            (f'{step_rate:.0f} images/s' if step_rate else f'unmeasured (exit {step.returncode})'))
        for key in rows:
            v = np.array(runs[key])
            verdict = '' if step_rate is None else ('   outruns the step' if np.median(v) > step_rate else '   does NOT outrun the step')
            say(f'{name:<24} {key[0]:<15} {key[1]:<12} decode {key[2]:<4} median {np.median(v):8.0f}   runs {" ".join(f"{x:.0f}" for x in v)}   '
                f'spread (max-min)/median {100 * (v.max() - v.min()) / np.median(v):.1f} %{verdict}')
        if a.epochs > 0:                                                    # the whole loop on the same files: mosaic + hsv + ciou, the recipe of the README
            os.makedirs(os.path.join(d, 'data'))
            ann = np.empty(len(files), dtype=object)
            for k, f in enumerate(files):
                ann[k] = np.array([f[0], f[1]], dtype=object)
            np.save(os.path.join(d, 'data', 'voc_img_ann.npy'), np.stack(list(ann)), allow_pickle=True)
            np.save(os.path.join(d, 'data', 'voc_anchor.npy'), np.asarray(VOC_ANCHORS))
            for label, extra in (('CACHE=off DECODE=pil', []), ('CACHE=gpu DECODE=pil', ['--cache', 'gpu', '--cache_gb', str(a.cache_gb), '--cache_stage_mb', str(a.cache_stage_mb)]),
                                 ('CACHE=gpu DECODE=gpu', ['--cache', 'gpu', '--decode', 'gpu', '--cache_gb', str(a.cache_gb), '--cache_stage_mb', str(a.cache_stage_mb)])):
                for l in _train(d, extra):
                    say(f'make train MOSAIC=True HSV=True BOXLOSS=ciou {label}: {l}')
    with open(os.path.join(HERE, a.out), 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""What mosaic buys on generated images (profiles/mosaic_map.txt), on the protocol of tools/box_loss_map.py: yolo_mobilev1-0.75
trained from one seed on generated images with known boxes (training.synthetic_list) through the product's own command line (`make train
SYNTHETIC= VALMAP=True MOSAIC=`), once without mosaic, once with it and once with it switched off for the last epochs, the same seed, epochs and
loss weights for all; every checkpoint is then scored by evaluate.py (`make eval SYNTHETIC=`) on unseen generated images, which are never
mosaicked.  ONE run each: the spread between runs is not measured.  Generated rectangles on noise are not VOC: the numbers say nothing about
the default.

    python tools/mosaic_map.py [--train 2048] [--eval 1024] [--epochs 20] [--batch 32] [--off 4] [--out profiles/mosaic_map.txt]
"""
import argparse
import contextlib
import io
import re
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from k210_yolo_framework_amd import evaluate, training  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--train', type=int, default=2048)
ap.add_argument('--eval', type=int, default=1024)
ap.add_argument('--epochs', type=int, default=20)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--lr', type=float, default=1e-3)
ap.add_argument('--off', type=int, default=4, help='--mosaic_off_epochs of the third run')
ap.add_argument('--out', default='profiles/mosaic_map.txt')
a = ap.parse_args()

NET = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.75']
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f'yolo_mobilev1-0.75, {a.train} generated images (5 % of them the validation split), {a.epochs} epochs of batch {a.batch}, lr {a.lr}, seed 3, '
    f'obj / noobj / wh weights 5 / 0.5 / 0.5, iou_thresh 0.3, box loss mse; scored on {a.eval} unseen generated images '
    f'(evaluate.py, f16x2, area AP at IoU 0.5, obj_thresh 0.05); one run each, {time.strftime("%Y-%m-%d")}')
RUNS = [('plain', []), ('mosaic', ['--mosaic', 'True']), (f'mosaic_off{a.off}', ['--mosaic', 'True', '--mosaic_off_epochs', str(a.off)])]
with tempfile.TemporaryDirectory() as tmp:
    for name, extra in RUNS:
        log, t0 = io.StringIO(), time.time()
        with contextlib.redirect_stdout(log):
            training.cli(NET + ['--synthetic', str(a.train), '--batch_size', str(a.batch), '--max_nrof_epochs', str(a.epochs), '--rand_seed', '3',
                                '--init_learning_rate', str(a.lr), '--obj_weight', '5', '--noobj_weight', '0.5', '--wh_weight', '0.5',
                                '--iou_thresh', '0.3', '--vaildation_split', '0.05', '--val_map', 'True', '--log_dir', f'{tmp}/{name}'] + extra)
        secs = time.time() - t0
        epochs = re.findall(r'^epoch \d+: \d+ steps.*$', log.getvalue(), re.M)
        ckpt = next(Path(tmp, name).glob('*/yolo_model.h5'))
        with contextlib.redirect_stdout(io.StringIO()):
            rep = evaluate.main([str(ckpt)] + NET + ['--synthetic', str(a.eval), '--out', f'{tmp}/{name}.json'])
        vmap = [float(m) for m in re.findall(r'val_mAP ([0-9.]+)', '\n'.join(epochs))]
        say(f'{name:<12} mAP {100 * rep["map"]:7.3f}   ({secs:.0f} s of training and validation)')
        say('             val_mAP per epoch: ' + ' '.join(f'{v:.3f}' for v in vmap))
        say('             last epoch line: ' + (epochs[-1] if epochs else '-'))
Path(ROOT / a.out).write_text('\n'.join(lines) + '\n')

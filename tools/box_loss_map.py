#!/usr/bin/env python
"""What the IoU-family box losses buy on generated images (profiles/box_loss_map.txt), on the protocol of
profiles/r05_map_eval.json: yolo_mobilev1-0.75 trained from one seed on generated images with known boxes (training.synthetic_list), once
per box loss - mse, giou, diou, ciou - through the product's own command line (`make train SYNTHETIC= VALMAP=True BOXLOSS=`), the same seed,
epochs and loss weights for all four; every checkpoint is then scored by evaluate.py (`make eval SYNTHETIC=`) on unseen generated images.
Writes the mAP of each run and its per-epoch val_mAP.  Generated rectangles on noise are not VOC: the numbers say nothing about the default.

    python tools/box_loss_map.py [--train 2048] [--eval 1024] [--epochs 40] [--batch 32] [--box_weight 1.0] [--out profiles/box_loss_map.txt]
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
ap.add_argument('--epochs', type=int, default=40)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--lr', type=float, default=1e-3)
ap.add_argument('--box_weight', type=float, default=1.0)
ap.add_argument('--out', default='profiles/box_loss_map.txt')
a = ap.parse_args()

NET = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.75']
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f'yolo_mobilev1-0.75, {a.train} generated images (5 % of them the validation split), {a.epochs} epochs of batch {a.batch}, lr {a.lr}, seed 3, '
    f'obj / noobj / wh weights 5 / 0.5 / 0.5, iou_thresh 0.3, box_weight {a.box_weight}; scored on {a.eval} unseen generated images '
    f'(evaluate.py, f16x2, area AP at IoU 0.5, obj_thresh 0.05)')
with tempfile.TemporaryDirectory() as tmp:
    for box in ('mse', 'giou', 'diou', 'ciou'):
        log, t0 = io.StringIO(), time.time()
        with contextlib.redirect_stdout(log):
            training.cli(NET + ['--synthetic', str(a.train), '--batch_size', str(a.batch), '--max_nrof_epochs', str(a.epochs), '--rand_seed', '3',
                                '--init_learning_rate', str(a.lr), '--obj_weight', '5', '--noobj_weight', '0.5', '--wh_weight', '0.5',
                                '--iou_thresh', '0.3', '--vaildation_split', '0.05', '--val_map', 'True', '--box_loss', box,
                                '--box_weight', str(a.box_weight), '--log_dir', f'{tmp}/{box}'])
        secs = time.time() - t0
        epochs = re.findall(r'^epoch \d+: .*$', log.getvalue(), re.M)
        ckpt = next(Path(tmp, box).glob('*/yolo_model.h5'))
        with contextlib.redirect_stdout(io.StringIO()):
            rep = evaluate.main([str(ckpt)] + NET + ['--synthetic', str(a.eval), '--out', f'{tmp}/{box}.json'])
        vmap = [float(m) for m in re.findall(r'val_mAP ([0-9.]+)', '\n'.join(epochs))]
        say(f'{box:<5} mAP {100 * rep["map"]:7.3f}   ({secs:.0f} s of training and validation)')
        say('      val_mAP per epoch: ' + ' '.join(f'{v:.3f}' for v in vmap))
        say('      last epoch line: ' + (epochs[-1] if epochs else '-'))
Path(ROOT / a.out).write_text('\n'.join(lines) + '\n')

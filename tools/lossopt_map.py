#!/usr/bin/env python
"""What focal loss, label smoothing and the IoU objectness target buy on generated images (profiles/lossopt_map.txt), on the
protocol of tools/box_loss_map.py: yolo_mobilev1-0.75 trained from one seed on generated images with known boxes (training.synthetic_list)
through the product's own command line (`make train SYNTHETIC= VALMAP=True FOCAL= LABELSMOOTH= OBJTARGET=`), once plain, once per option alone
and once with all three, the same seed, epochs and loss weights for all; every checkpoint is then scored by evaluate.py (`make eval SYNTHETIC=`,
and `METRIC=coco`: AP at .75 and AP .50:.95, where a score that says how good the box is should show) on unseen generated images.  Writes the
figures of each run and its per-epoch val_mAP.  ONE run each resolves no spread: the plain run's own val_mAP swings by more than most
differences between rows.  Generated rectangles on noise are not VOC: the numbers say nothing about the defaults, which stay off.

    python tools/lossopt_map.py [--train 2048] [--eval 1024] [--epochs 40] [--batch 32] [--gamma 2.0] [--alpha 0.25] [--smooth 0.1]
                                [--out profiles/lossopt_map.txt]
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
ap.add_argument('--gamma', type=float, default=2.0)
ap.add_argument('--alpha', type=float, default=0.25)
ap.add_argument('--smooth', type=float, default=0.1)
ap.add_argument('--out', default='profiles/lossopt_map.txt')
a = ap.parse_args()

NET = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.75']
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f'yolo_mobilev1-0.75, {a.train} generated images (5 % of them the validation split), {a.epochs} epochs of batch {a.batch}, lr {a.lr}, seed 3, '
    f'obj / noobj / wh weights 5 / 0.5 / 0.5, iou_thresh 0.3, box loss mse; focal gamma {a.gamma}, alpha {a.alpha}, label smoothing {a.smooth}; '
    f'scored on {a.eval} unseen generated images (evaluate.py, f16x2, area AP at IoU 0.5 and --metric coco, obj_thresh 0.05).  '
    f'One run each: no spread is resolved.')
FOCAL = ['--focal_gamma', str(a.gamma), '--focal_alpha', str(a.alpha)]
RUNS = [('plain', []), ('focal_obj', ['--focal', 'obj'] + FOCAL), ('focal_cls', ['--focal', 'cls'] + FOCAL), ('focal_all', ['--focal', 'all'] + FOCAL),
        ('smooth', ['--label_smooth', str(a.smooth)]), ('obj_iou', ['--obj_target', 'iou']),
        ('all_three', ['--focal', 'all'] + FOCAL + ['--label_smooth', str(a.smooth), '--obj_target', 'iou'])]
with tempfile.TemporaryDirectory() as tmp:
    for box, flags in RUNS:
        log, t0 = io.StringIO(), time.time()
        with contextlib.redirect_stdout(log):
            training.cli(NET + ['--synthetic', str(a.train), '--batch_size', str(a.batch), '--max_nrof_epochs', str(a.epochs), '--rand_seed', '3',
                                '--init_learning_rate', str(a.lr), '--obj_weight', '5', '--noobj_weight', '0.5', '--wh_weight', '0.5',
                                '--iou_thresh', '0.3', '--vaildation_split', '0.05', '--val_map', 'True', '--log_dir', f'{tmp}/{box}'] + flags)
        secs = time.time() - t0
        epochs = re.findall(r'^epoch \d+: .*$', log.getvalue(), re.M)
        ckpt = next(Path(tmp, box).glob('*/yolo_model.h5'))
        with contextlib.redirect_stdout(io.StringIO()):
            rep = evaluate.main([str(ckpt)] + NET + ['--synthetic', str(a.eval), '--metric', 'coco', '--out', f'{tmp}/{box}.json'])
        vmap = [float(m) for m in re.findall(r'val_mAP ([0-9.]+)', '\n'.join(epochs))]
        say(f'{box:<10} mAP {100 * rep["map"]:7.3f}   coco: ' + ' '.join(f'{k} {100 * v:.3f}' for k, v in rep['coco'].items() if isinstance(v, float)) +
            f'   ({secs:.0f} s of training and validation)')
        say('      val_mAP per epoch: ' + ' '.join(f'{v:.3f}' for v in vmap))
        say('      last epoch line: ' + (epochs[-1] if epochs else '-'))
Path(ROOT / a.out).write_text('\n'.join(lines) + '\n')

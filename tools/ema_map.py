#!/usr/bin/env python
"""What the weight average and the learning-rate schedule do on generated images (profiles/ema_map.txt), on the protocol of
tools/box_loss_map.py: yolo_mobilev1-0.75 trained from one seed on generated images with known boxes (training.synthetic_list) through the
product's own command line (`make train SYNTHETIC= VALMAP=True`), once plain, once with EMA=True, once with EMA=True LRSCHED=cosine WARMUP=;
every run's checkpoint - the averaged one where there is one, and the live one beside it - is then scored by evaluate.py (`make eval
SYNTHETIC=`) on unseen generated images.  One run each.  Generated rectangles on noise are not VOC: the numbers say nothing about the default.

    python tools/ema_map.py [--train 2048] [--eval 1024] [--epochs 20] [--batch 32] [--ema_decay 0.99] [--ema_tau 200] [--warmup 120]
                            [--out profiles/ema_map.txt]
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
ap.add_argument('--ema_decay', type=float, default=0.99)
ap.add_argument('--ema_tau', type=float, default=200.0)
ap.add_argument('--warmup', type=int, default=120)
ap.add_argument('--out', default='profiles/ema_map.txt')
a = ap.parse_args()

NET = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.75']
EMA = ['--ema', 'True', '--ema_decay', str(a.ema_decay), '--ema_tau', str(a.ema_tau)]
ROWS = [('plain', []), ('ema', EMA), ('ema+cosine+warmup', EMA + ['--lr_schedule', 'cosine', '--warmup_steps', str(a.warmup)])]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def score(ckpt, tmp, tag):
    with contextlib.redirect_stdout(io.StringIO()):
        return 100 * evaluate.main([str(ckpt)] + NET + ['--synthetic', str(a.eval), '--out', f'{tmp}/{tag}.json'])['map']


say(f'yolo_mobilev1-0.75, {a.train} generated images (5 % of them the validation split), {a.epochs} epochs of batch {a.batch}, lr {a.lr}, seed 3, '
    f'obj / noobj / wh weights 5 / 0.5 / 0.5, iou_thresh 0.3; ema_decay {a.ema_decay}, ema_tau {a.ema_tau}, warmup {a.warmup} steps, lr_final 0.01; '
    f'scored on {a.eval} unseen generated images (evaluate.py, f16x2, area AP at IoU 0.5, obj_thresh 0.05).  val_mAP is of the averaged weights '
    f'where EMA is on.')
with tempfile.TemporaryDirectory() as tmp:
    for k, (name, extra) in enumerate(ROWS):
        log, t0 = io.StringIO(), time.time()
        with contextlib.redirect_stdout(log):
            training.cli(NET + ['--synthetic', str(a.train), '--batch_size', str(a.batch), '--max_nrof_epochs', str(a.epochs), '--rand_seed', '3',
                                '--init_learning_rate', str(a.lr), '--obj_weight', '5', '--noobj_weight', '0.5', '--wh_weight', '0.5',
                                '--iou_thresh', '0.3', '--vaildation_split', '0.05', '--val_map', 'True', '--log_dir', f'{tmp}/{k}'] + extra)
        secs = time.time() - t0
        epochs = re.findall(r'^epoch \d+: .*$', log.getvalue(), re.M)
        live = score(next(Path(tmp, str(k)).glob('*/yolo_model.h5')), tmp, f'{k}_live')
        avg = score(next(Path(tmp, str(k)).glob('*/yolo_ema_model.h5')), tmp, f'{k}_ema') if extra else None
        vmap = [float(m) for m in re.findall(r'val_mAP ([0-9.]+)', '\n'.join(epochs))]
        say(f'{name:<18} mAP live {live:7.3f}' + (f'   averaged {avg:7.3f}' if avg is not None else '') + f'   ({secs:.0f} s of training and validation)')
        say('      val_mAP per epoch: ' + ' '.join(f'{v:.3f}' for v in vmap))
        say('      last epoch line: ' + (epochs[-1] if epochs else '-'))
Path(ROOT / a.out).write_text('\n'.join(lines) + '\n')

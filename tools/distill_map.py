#!/usr/bin/env python
"""What knowledge distillation buys on generated images (profiles/distill_map.txt), on the protocol of tools/box_loss_map.py:
a yolo_mobilev2-1.0 teacher is trained from one seed on generated images with known boxes (training.synthetic_list) through the product's own
command line (`make train SYNTHETIC=`), then a yolo_mobilev1-0.5 student is trained the same way twice, without and with the teacher
(`TEACHERCKPT= TEACHER=yolo_mobilev2 TEACHERDEPTH=1.0 DISTILLWEIGHT=`); every checkpoint is scored by evaluate.py (`make eval SYNTHETIC=`) on unseen
generated images.  One run each: rectangles on noise are not VOC, the spread between runs is unknown, and the default stays off whatever it shows.

    python tools/distill_map.py [--train 2048] [--eval 1024] [--epochs 20] [--batch 32] [--distill_weight 1.0] [--out profiles/distill_map.txt]
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
ap.add_argument('--distill_weight', type=float, default=1.0)
ap.add_argument('--out', default='profiles/distill_map.txt')
a = ap.parse_args()

TEACHER = ['--model_def', 'yolo_mobilev2', '--depth_multiplier', '1.0']
STUDENT = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5']
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def run(tmp, name, net, extra=()):
    """One training run and its score -> the checkpoint."""
    log, t0 = io.StringIO(), time.time()
    with contextlib.redirect_stdout(log):
        training.cli(net + ['--synthetic', str(a.train), '--batch_size', str(a.batch), '--max_nrof_epochs', str(a.epochs), '--rand_seed', '3',
                            '--init_learning_rate', str(a.lr), '--obj_weight', '5', '--noobj_weight', '0.5', '--wh_weight', '0.5',
                            '--iou_thresh', '0.3', '--vaildation_split', '0.05', '--log_dir', f'{tmp}/{name}', *extra])
    secs = time.time() - t0
    epochs = re.findall(r'^epoch \d+: .*$', log.getvalue(), re.M)
    ckpt = next(Path(tmp, name).glob('*/yolo_model.h5'))
    with contextlib.redirect_stdout(io.StringIO()):
        rep = evaluate.main([str(ckpt)] + net + ['--synthetic', str(a.eval), '--out', f'{tmp}/{name}.json'])
    say(f'{name:<22} mAP {100 * rep["map"]:7.3f}   ({secs:.0f} s of training and validation)')
    say('      first epoch line: ' + (epochs[0] if epochs else '-'))
    say('      last epoch line:  ' + (epochs[-1] if epochs else '-'))
    return ckpt


say(f'{a.train} generated images (5 % of them the validation split), {a.epochs} epochs of batch {a.batch}, lr {a.lr}, seed 3, obj / noobj / wh weights '
    f'5 / 0.5 / 0.5, iou_thresh 0.3, distill_weight {a.distill_weight}; scored on {a.eval} unseen generated images (evaluate.py, f16x2, area AP at '
    f'IoU 0.5, obj_thresh 0.05); one run each')
with tempfile.TemporaryDirectory() as tmp:
    teacher = run(tmp, 'teacher mobilev2-1.0', TEACHER)
    run(tmp, 'student mobilev1-0.5', STUDENT)
    run(tmp, 'student + teacher', STUDENT, ['--teacher_ckpt', str(teacher), '--teacher_def', 'yolo_mobilev2', '--teacher_depth', '1.0',
                                            '--distill_weight', str(a.distill_weight)])
Path(ROOT / a.out).write_text('\n'.join(lines) + '\n')

#!/usr/bin/env python
"""Cost of knowledge distillation on the configs[3] training step (profiles/distill_step_cost.txt): yolo_mobilev2-1.0 at 16
images, the benchmark's network, weights, batch and optimizer settings (bench._train_setup).

    python tools/distill_step_cost.py off [--root TREE] [--steps 200]
        ms per replayed step with distillation off, as one JSON line.  --root: a built checkout of another commit (the parent) whose package and
        bench.py are timed instead of this tree's.
    python tools/distill_step_cost.py on [--steps 200]
        ms per replayed step with a yolo_mobilev1-1.0 teacher (seeded weights, f16x2), and the teacher's forward alone, as one JSON line.
    python tools/distill_step_cost.py report --parent TREE [--steps 200] [--out profiles/distill_step_cost.txt]
        five alternating repeats of `off` on this tree and on the parent's, each in a fresh process: the two medians must agree within the
        spread between the repeats, which is reported; then `on`, reported beside the teacher's forward time, without a bar.

Warm-up steps first (eager step, capture, replays), the device synchronised around the timed window, medians of the repeats."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('mode', choices=['off', 'on', 'report'])
ap.add_argument('--root', default=HERE)
ap.add_argument('--parent')
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--out', default='profiles/distill_step_cost.txt')
a = ap.parse_args()


def timed(fn, steps):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def child(mode, root):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), mode, '--root', root, '--steps', str(a.steps)], capture_output=True, text=True,
                         check=True, cwd=root).stdout
    return json.loads(out.strip().splitlines()[-1])


if a.mode in ('off', 'on'):
    sys.path.insert(0, a.root)
    os.chdir(a.root)
    import torch  # noqa: F401
    import bench
    tr, x, y = bench._train_setup(16, 0, 1, 0)
    res = dict(mode=a.mode, root=a.root, steps=a.steps)
    if a.mode == 'on':
        from k210_yolo_framework_amd import netspec
        from k210_yolo_framework_amd.distill import DistillConfig
        from k210_yolo_framework_amd.train import Trainer
        spec, weights, anchors = tr.spec, tr.export_weights(), tr.anchors
        del tr
        t_spec = netspec.yolo_mobilev1([*spec.in_hw, 3], spec.anchor_num, spec.class_num, alpha=1.0)
        tr = Trainer(spec, weights, anchors, 16, lr=5e-4, decay=0.0, distill=DistillConfig(t_spec, t_spec.init_weights(seed=2), 1.0))
        res['teacher'] = 'yolo_mobilev1-1.0'
        res['teacher_forward_ms'] = round(timed(lambda: tr.teacher_forward(x), a.steps), 3)
    res['step_ms'] = round(timed(lambda: tr.step(x, y), a.steps), 3)
    print(json.dumps(res))
else:
    if not a.parent:
        sys.exit('report needs --parent TREE, a built checkout of the parent commit')
    here, parent = [], []
    for _ in range(5):                                                   # alternating: drift of the machine lands on both
        here.append(child('off', HERE)['step_ms'])
        parent.append(child('off', os.path.abspath(a.parent))['step_ms'])
    on = child('on', HERE)
    mh, mp = statistics.median(here), statistics.median(parent)
    spread = max(max(here) - min(here), max(parent) - min(parent))
    lines = [f'yolo_mobilev2-1.0 training step, 16 images, replayed graph, {a.steps} steps per repeat, five alternating repeats in fresh processes',
             f'distillation off, this commit : median {mh:.3f} ms   repeats {" ".join(f"{v:.3f}" for v in here)}',
             f'distillation off, parent      : median {mp:.3f} ms   repeats {" ".join(f"{v:.3f}" for v in parent)}',
             f'difference of the medians {abs(mh - mp):.3f} ms, spread between repeats {spread:.3f} ms: ' +
             ('agree' if abs(mh - mp) <= spread else 'DO NOT AGREE'),
             f'distillation on, {on["teacher"]} teacher (f16x2, throughput schedule): {on["step_ms"]:.3f} ms per step; the teacher\'s forward alone '
             f'{on["teacher_forward_ms"]:.3f} ms (no bar)']
    print('\n'.join(lines))
    with open(os.path.join(HERE, a.out), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    sys.exit(0 if abs(mh - mp) <= spread else 1)

#!/usr/bin/env python
"""Cost of focal loss, label smoothing and the IoU objectness target on the configs[3] training step (DESIGN.md 3.25;
profiles/lossopt_step_cost.txt): Trainer.step of yolo_mobilev2-1.0 at 16 images, as tools/train_step.py times it, with the options off and
with focal='all', label_smooth=0.1, obj_target='iou' - and, with parent=<a built checkout of the parent commit>, that checkout's step beside
them.  Every figure is one fresh process; the configurations alternate within a round, `rounds` rounds (at least 3), the median and the range
of each are reported, and whether "off" lies inside the parent's own range.

    python tools/lossopt_step_cost.py [rounds=5] [steps=200] [parent=/path/to/parent/checkout] [out=profiles/lossopt_step_cost.txt]
    python tools/lossopt_step_cost.py worker <checkout> <off|on> <steps>        (what the driver starts)
"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(root, config, steps):
    sys.path.insert(0, root)
    os.chdir(root)
    import torch
    import bench
    from k210_yolo_framework_amd.train import Trainer
    tr, x, y = bench._train_setup(16, 0, 1, 0)                           # the benchmark's network, weights, batch and optimizer settings
    if config != 'off':                                                  # ... in a Trainer built WITH the options (bench.py's has none)
        spec, weights, anchors = tr.spec, tr.export_weights(), tr.anchors
        del tr
        tr = Trainer(spec, weights, anchors, 16, lr=5e-4, decay=0.0, focal='all', label_smooth=0.1, obj_target='iou')
    for _ in range(5):
        tr.step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(x, y)
    torch.cuda.synchronize()
    print(json.dumps(dict(config=config, step_ms=(time.perf_counter() - t0) / steps * 1e3, n_params=tr.n_params)))


if len(sys.argv) > 1 and sys.argv[1] == 'worker':
    worker(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    sys.exit(0)
opt = dict(a.split('=', 1) for a in sys.argv[1:])
rounds, steps = max(int(opt.get('rounds', 5)), 3), int(opt.get('steps', 200))
arms = ([('parent off', opt['parent'], 'off')] if 'parent' in opt else []) + [(c, HERE, c) for c in ('off', 'on')]
ms = {name: [] for name, _, _ in arms}
n_params = None
for r in range(rounds):
    for name, root, config in arms:
        # this file's worker drives either checkout: it only uses what both have, unless an option is asked for
        out = subprocess.run([sys.executable, os.path.abspath(__file__), 'worker', root, config, str(steps)], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.exit(f'{name}: worker failed ({out.returncode})\n{out.stderr[-2000:]}')
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        ms[name].append(rec['step_ms'])
        n_params = rec['n_params']
        print(f'round {r + 1} {name:<10} {rec["step_ms"]:.3f} ms', flush=True)
lines = [f'Trainer.step, yolo_mobilev2-1.0, 224x320, 16 images, {n_params} floats in the flat buffers; {steps} steps per figure after 5 warm-up steps, one fresh '
         f'process per figure, the configurations alternating within each of {rounds} rounds.  ms per step: median [min .. max] of the rounds.']
base = statistics.median(ms[arms[0][0]])
for name, _, _ in arms:
    v = ms[name]
    lines.append(f'{name:<10} {statistics.median(v):7.3f}  [{min(v):.3f} .. {max(v):.3f}]   median - {arms[0][0]} median = {statistics.median(v) - base:+.3f} ms')
if 'parent' in opt:
    lo, hi, off = min(ms['parent off']), max(ms['parent off']), statistics.median(ms['off'])
    lines.append(f'off median {off:.3f} ms lies {"inside" if lo <= off <= hi else "OUTSIDE"} the range of the parent [{lo:.3f} .. {hi:.3f}]')
else:
    lines.append('no parent checkout was given: whether "off" costs what the parent costs is unmeasured')
lines.append("on = focal='all' (gamma 2), label_smooth=0.1, obj_target='iou'; its difference from off is the options' whole cost in the step")
print('\n'.join(lines))
with open(os.path.join(HERE, opt.get('out', 'profiles/lossopt_step_cost.txt')), 'w') as f:
    f.write('\n'.join(lines) + '\n')

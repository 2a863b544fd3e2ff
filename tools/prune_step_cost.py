"""Cost of magnitude pruning on the configs[3] training step (profiles/prune_step_cost.txt).
  python tools/prune_step_cost.py step [steps=200] [frequency=100]   tr.step() as tools/train_step.py times it, pruning on at the given
                                                                     frequency (0: off); the window holds steps/frequency mask updates
  python tools/prune_step_cost.py call <network> [calls=5]           `calls` x Trainer.update_masks + apply_masks and nothing else: run it
                                                                     under `rocprofv3 --kernel-trace --stats` for the time of one call"""
import os, sys, time, json
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch
import bench
from k210_yolo_framework_amd import netspec
from k210_yolo_framework_amd.helper import VOC_ANCHORS
from k210_yolo_framework_amd.prune import PruneSchedule
from k210_yolo_framework_amd.train import Trainer

if len(sys.argv) < 2 or sys.argv[1] not in ('step', 'call') or (sys.argv[1] == 'call' and len(sys.argv) < 3):
    sys.exit(__doc__)
if sys.argv[1] == 'step':
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    freq = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    tr, x, y = bench._train_setup(16, 0, 1, 0)                           # the benchmark's network, weights, batch and optimizer settings
    if freq:                                                             # ... in a Trainer built WITH the schedule (bench.py's has none)
        spec, weights, anchors = tr.spec, tr.export_weights(), tr.anchors
        del tr
        tr = Trainer(spec, weights, anchors, 16, lr=5e-4, decay=0.0, prune=PruneSchedule(0.5, 0.9, 1000000, freq))
    for _ in range(3):
        tr.step(x, y)
    torch.cuda.synchronize()
    first = tr.iterations
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(x, y)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / steps * 1e3
    updates = len([s for s in range(first, first + steps) if freq and tr.prune.is_update(s)])
    print(json.dumps(dict(step_ms=round(step_ms, 3), steps=steps, prune_frequency=freq, mask_updates_in_window=updates)))
else:
    name, calls = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5
    spec = netspec.NETWORKS[name]([64, 96, 3], 3, 20, alpha=1.0)
    anchors = VOC_ANCHORS if len(spec.outputs) == 2 else __import__('numpy').concatenate([VOC_ANCHORS, VOC_ANCHORS[:1] * 0.5])
    tr = Trainer(spec, spec.init_weights(1), anchors, 1, prune=PruneSchedule(0.5, 0.9, 1000, 100))
    for i in range(calls):
        tr.update_masks(500)
        tr.apply_masks()
    torch.cuda.synchronize()
    rep = tr.prune_report()
    print(json.dumps(dict(network=name, kernels=len(rep), weights=sum(r['n'] for r in rep.values()), kept=sum(r['kept'] for r in rep.values()), calls=calls)))

"""Cost of quantisation-aware training on the training step: yolo_mobilev1-0.75 at 224x320,
16 images (a network the KPU path takes; bench.py's configs[3] network has `add`), timed as tools/train_step.py times a step.
  python tools/qat_step_cost.py step [steps=200] [qat=0|1]   tr.step() in a window of `steps` after 3 warm-up steps; qat=0 builds the
                                                             Trainer without the argument, so the same command runs on a parent commit
  python tools/qat_step_cost.py call [steps=5]               `steps` eager QAT steps and nothing else: run it under
                                                             `rocprofv3 --kernel-trace --stats` for the time of the four new kernels"""
import os, sys, time, json
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch
from k210_yolo_framework_amd import netspec
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
from k210_yolo_framework_amd.train import Trainer

if len(sys.argv) < 2 or sys.argv[1] not in ('step', 'call'):
    sys.exit(__doc__)
mode = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else (200 if mode == 'step' else 5)
qat = mode == 'call' or (len(sys.argv) > 3 and sys.argv[3] == '1')
B = 16
spec = netspec.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [list(v) for v in spec.out_hw()])
rng = np.random.default_rng(0)
ys = [[] for _ in spec.outputs]
for b in range(B):
    n = int(rng.integers(1, 6))
    boxes = np.stack([rng.integers(0, 20, n), rng.uniform(.2, .8, n), rng.uniform(.2, .8, n), rng.uniform(.1, .6, n), rng.uniform(.1, .6, n)], 1)
    for i, lab in enumerate(h.box_to_label(boxes)):
        ys[i].append(lab)
y = [torch.from_numpy(np.stack(v).astype(np.float32)).cuda() for v in ys]
x = torch.from_numpy(rng.uniform(0, 1, (B, 224, 320, 3)).astype(np.float32)).cuda()
kw = {}
if qat:
    from k210_yolo_framework_amd.qat import QatConfig
    kw = dict(qat=QatConfig(0.99))
tr = Trainer(spec, spec.init_weights(seed=1), h.anchors, B, lr=5e-4, decay=0.0, use_graph=mode == 'step', **kw)
if qat:
    tr.qat_observe(x)
for _ in range(3 if mode == 'step' else 1):
    tr.step(x, y)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    out = tr.step(x, y)
torch.cuda.synchronize()
step_ms = (time.perf_counter() - t0) / steps * 1e3
print(json.dumps(dict(mode=mode, qat=qat, step_ms=round(step_ms, 3), steps=steps, loss=round(out['loss'], 4))))

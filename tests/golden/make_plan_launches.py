"""Generate tests/golden/x2_plan_launches.json and tests/golden/f16_plan_launches.json: the launch lists of the two plan builders, the
f16x2 one (csrc/yk_xplan_build.h) and the f16 one (csrc/yk_plan_build.h), needs a GPU:

    python tests/golden/make_plan_launches.py [output directory, default: beside this script]

For every (precision, network, schedule, max_batch) of CASES the names, flops and bytes that `engine.Plan(...).launches()` reports.  The
names carry the tile geometry, ring depth and split-K of each launch, so the files record the planning rules;
tests/test_gpu_plan_record.py asserts that the builders still give exactly this.  A tuning change that moves a tile regenerates the
file and shows the move in its diff.  Flops and bytes are host doubles, written with repr.

The f16 builder never looks at the schedule: its rows are recorded for one schedule only ('throughput').  It does look at max_batch
(M = max_batch * Ho * Wo feeds the tile choice, the K split and the slab size), and Darknet-53 ('yolo', 416x416, the max_batch of 4 that
tests/test_gpu_e2e.py runs it at) is the network that reaches the folded residual Adds, the upsample + concat views and most of the
split-K launches.  The f16 rows carry a `precision` field; the x2 rows keep the format they were first written in.
"""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

NETWORKS = (('yolo_mobilev1', (224, 320, 3), 0.75), ('yolo_mobilev2', (224, 320, 3), 1.0), ('tiny_yolo', (416, 416, 3), 1.0))
SCHEDULES = ('latency', 'throughput')
MAX_BATCHES = (1, 32)
CASES = [('f16x2', n, s, a, sc, b) for n, s, a in NETWORKS for sc in SCHEDULES for b in MAX_BATCHES]
CASES += [('f16', n, s, a, 'throughput', b) for n, s, a in NETWORKS for b in MAX_BATCHES]
CASES += [('f16', 'yolo', (416, 416, 3), 1.0, 'throughput', 4)]
SWITCHES = ('YK_FUSE_DWPW', 'YK_PERSIST', 'YK_HEADS', 'YK_FUSE_HEAD', 'YK_SPLITK', 'YK_CLUSTER_WT', 'YK_REDUCE_PW')


def launches(precision, name, shape, alpha, schedule, max_batch):
    """[[launch name, repr(flops), repr(bytes)], ...] of the plan, built with every switch at its default."""
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd import netspec as ns
    assert not any(k in os.environ for k in SWITCHES), 'unset the YK_* switches: the record holds the default plans'
    spec = ns.NETWORKS[name](shape, 3, 20, alpha=alpha)
    with engine.Plan(spec, spec.init_weights(seed=1), max_batch=max_batch, precision=precision, schedule=schedule) as plan:
        return [[n, repr(fl), repr(by)] for n, fl, by in plan.launches()]


def main(out=None):
    out = Path(out) if out else Path(__file__).parent
    for precision, file in (('f16x2', 'x2_plan_launches.json'), ('f16', 'f16_plan_launches.json')):
        record = []
        for p, n, s, a, sc, b in CASES:
            if p != precision:
                continue
            row = {'network': n, 'shape': list(s), 'alpha': a, 'schedule': sc, 'max_batch': b, 'launches': launches(p, n, s, a, sc, b)}
            if p != 'f16x2':
                row = {'precision': p, **row}
            record.append(row)
        (out / file).write_text(json.dumps(record, indent=1) + '\n')


if __name__ == '__main__':
    main(*sys.argv[1:2])

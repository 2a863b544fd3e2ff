"""Generate tests/golden/x2_plan_launches.json: the launch list of the f16x2 plan builder (csrc/yk_xplan_build.h), needs a GPU:

    python tests/golden/make_x2_plan_launches.py [output file, default: beside this script]

For every (network, schedule, max_batch) of CASES the names, flops and bytes that `engine.Plan(...).launches()` reports.  The names carry
the tile geometry, ring depth and split-K of each launch, so the file records the planning rules; tests/test_gpu_plan_record.py asserts
that the builder still gives exactly this.  A tuning change that moves a tile regenerates the file and shows the move in its diff.
Flops and bytes are host doubles, written with repr.
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
CASES = [(n, s, a, sc, b) for n, s, a in NETWORKS for sc in SCHEDULES for b in MAX_BATCHES]
SWITCHES = ('YK_FUSE_DWPW', 'YK_PERSIST', 'YK_HEADS', 'YK_FUSE_HEAD', 'YK_SPLITK', 'YK_CLUSTER_WT')


def launches(name, shape, alpha, schedule, max_batch):
    """[[launch name, repr(flops), repr(bytes)], ...] of the plan, built with every switch at its default."""
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd import netspec as ns
    assert not any(k in os.environ for k in SWITCHES), 'unset the YK_* switches: the record holds the default plans'
    spec = ns.NETWORKS[name](shape, 3, 20, alpha=alpha)
    with engine.Plan(spec, spec.init_weights(seed=1), max_batch=max_batch, precision='f16x2', schedule=schedule) as plan:
        return [[n, repr(fl), repr(by)] for n, fl, by in plan.launches()]


def main(out=None):
    record = [{'network': n, 'shape': list(s), 'alpha': a, 'schedule': sc, 'max_batch': b, 'launches': launches(n, s, a, sc, b)}
              for n, s, a, sc, b in CASES]
    Path(out or Path(__file__).with_name('x2_plan_launches.json')).write_text(json.dumps(record, indent=1) + '\n')


if __name__ == '__main__':
    main(*sys.argv[1:2])

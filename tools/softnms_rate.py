"""Time of the decode tail (decode -> per-class NMS -> compaction, three launches) per suppression rule, against `hard` in the same session.

    python tools/softnms_rate.py [--out profiles/softnms_rate.txt]

Heads: the shipped yolo_mobilev1-0.75 head at 224x320 (1 050 boxes, the 1088-candidate template), 32 images, at obj_thresh 0.7 and 0.05, and the
three-scale Darknet-53 head at 416x416 (10 647 boxes, the 2048-candidate template; its saturated logits overflow the LDS), 32 images, at 0.05.
Seeded random weights.  Per (head, threshold): five repeats, each timing every rule in turn (20 calls between two events, 3 warm-up calls), the
median of the five per rule.  One box, one session: only lines of one block compare."""
import argparse
import statistics
import sys

sys.path.insert(0, '.')
import numpy as np      # noqa: E402
import torch            # noqa: E402

from k210_yolo_framework_amd import engine, netspec as ns, softnms      # noqa: E402
from k210_yolo_framework_amd.helper import VOC_ANCHORS                  # noqa: E402

B, CALLS, REPEATS = 32, 20, 5


def tail_us(cfg, outs, obj, rule):
    for _ in range(3):
        engine.decode_py(cfg, outs, B, None, obj, 0.5, nms=rule)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CALLS):
        d, c = engine.decode_py(cfg, outs, B, None, obj, 0.5, nms=rule)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3, float(c.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    heads = [('yolo_mobilev1-0.75 224x320', ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75), VOC_ANCHORS, (0.7, 0.05)),
             ('darknet-53 416x416', ns.NETWORKS['yolo']([416, 416, 3], 3, 20), np.concatenate([VOC_ANCHORS, VOC_ANCHORS[:1] * 0.5]), (0.05,))]
    for name, spec, anchors, thresholds in heads:
        plan = engine.Plan(spec, spec.init_weights(seed=1), max_batch=B)
        frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, *spec.in_hw, 3), dtype=np.uint8)).cuda()
        plan.run_u8(frames)
        torch.cuda.synchronize()
        outs = plan.outputs()
        cfg = engine.make_decode_cfg(anchors, 20, spec.in_hw, spec.out_hw())
        for obj in thresholds:
            t = {r: [] for r in softnms.METHODS}
            rows = {}
            for _ in range(REPEATS):
                for r in softnms.METHODS:                   # alternating: every rule once per repeat
                    us, rows[r] = tail_us(cfg, outs, obj, r)
                    t[r].append(us)
            lines.append(f'{name}, {B} images, obj_thresh {obj}:')
            hard = statistics.median(t['hard'])
            for r in softnms.METHODS:
                m = statistics.median(t[r])
                lines.append(f'   {r:9s} median {m:9.1f} us  (min {min(t[r]):9.1f}  max {max(t[r]):9.1f})  x{m / hard:5.2f} of hard   rows per image {rows[r]:6.1f}')
        plan.close()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('# tools/softnms_rate.py: decode tail (decode + NMS + compaction) per rule, median of five alternating repeats of 20 calls\n' + text + '\n')


if __name__ == '__main__':
    main()

"""Times MotEvaluator.result() (pack, upload, yk_mot_eval, read back) against the numpy rule motmetrics.evaluate on generated sequences,
and yk_lap_f64 (motmetrics_gpu.lap: upload, one launch, read back) against scipy.optimize.linear_sum_assignment and, at the sizes
where it ends in reasonable time, the numpy rule motmetrics.lap, on uniform random float64 costs at 64 x 64, 256 x 256 and 1024 x 1024, and
on a batch of 64 problems of 64 x 64.  Protocol: 3 warm-up rounds, then 9 rounds in which the contestants take turns; the median and the
min .. max of the 9 are written.  Wall-clock times around calls that wait for their result.  Figures are recorded, not judged: the
capability is new and there is no parent figure.

  python tools/trackeval_rate.py [--out profiles/trackeval_rate.txt]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    from scipy.optimize import linear_sum_assignment
    from k210_yolo_framework_amd import motmetrics as mm, motmetrics_gpu as mg
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='profiles/trackeval_rate.txt')
    p.add_argument('--rounds', type=int, default=9)
    a = p.parse_args()
    rng = np.random.default_rng(0)
    lines = ['yk_lap_f64 against scipy and the numpy rule: milliseconds per call, median (min .. max) of %d rounds after 3 warm-up rounds' % a.rounds]
    for label, shapes in (('64 x 64', [(64, 64)]), ('256 x 256', [(256, 256)]), ('1024 x 1024', [(1024, 1024)]), ('64 problems of 64 x 64', [(64, 64)] * 64)):
        costs = [rng.random(s) for s in shapes]
        runs = {'gpu': lambda: mg.lap(costs), 'scipy': lambda: [linear_sum_assignment(c) for c in costs]}
        if max(s[0] for s in shapes) * len(shapes) <= 256:
            runs['numpy rule'] = lambda: [mm.lap(c) for c in costs]
        want = [c[linear_sum_assignment(c)].sum() for c in costs]
        got = [c[np.arange(len(g)), g].sum() for c, g in zip(costs, mg.lap(costs))]
        assert np.allclose(got, want, rtol=1e-12, atol=0), label
        times = {k: [] for k in runs}
        for r in range(3 + a.rounds):
            for k, fn in runs.items():
                t = time.perf_counter()
                fn()
                if r >= 3:
                    times[k].append(1e3 * (time.perf_counter() - t))
        lines.append(f'{label:<24s} LDS-resident matrix: {mg.lds_resident(*shapes[0])}   ' + '   '.join(
            f'{k} {np.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})' for k, v in times.items()))
        print(lines[-1], flush=True)
    lines.append('MotEvaluator.result() against motmetrics.evaluate: milliseconds per call, same protocol')
    for n_seq, n_frames, n_obj in ((1, 60, 8), (8, 120, 10), (8, 120, 40)):
        seqs = mm.synthetic_sequences(n_seq, n_frames, n_obj, seed=0)
        ev = mg.MotEvaluator()
        for q in seqs:
            ev.add_sequence(*q)
        runs, times = {'gpu': ev.result, 'numpy rule': lambda: mm.evaluate(seqs)}, {'gpu': [], 'numpy rule': []}
        for r in range(3 + a.rounds):
            for k, fn in runs.items():
                t = time.perf_counter()
                fn()
                if r >= 3:
                    times[k].append(1e3 * (time.perf_counter() - t))
        lines.append(f'{n_seq} sequences x {n_frames} frames x {n_obj} objects   ' + '   '.join(
            f'{k} {np.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})' for k, v in times.items()))
        print(lines[-1], flush=True)
    Path(a.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

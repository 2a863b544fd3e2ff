"""The tracker's first HOTA / MOTA / IDF1 figures, at its default thresholds, on GENERATED detections: the ground truth of
motmetrics.synthetic_sequences (rectangles on straight paths - not MOT17, not pictures, no detector) turned into decode-shaped rows with
score noise, missed rows and clutter, tracked by engine.TrackState (yk_track_update) and scored by motmetrics_gpu.MotEvaluator
(yk_mot_eval).  The figures are recorded, not judged, and say nothing about real sequences; the tracker's defaults stay as they are.

  python tools/track_scores.py [--out profiles/track_scores.txt]"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def detections(gt, n_frames, rng, miss, clutter, cap):
    """-> dets [n_frames, cap, 6] (top, left, bottom, right, score, class 0), counts [n_frames]"""
    dets, counts = np.zeros((n_frames, cap, 6), np.float32), np.zeros(n_frames, np.int32)
    for f in range(1, n_frames + 1):
        rows = []
        for _, _, left, top, w, h in gt[gt[:, 0] == f]:
            if rng.random() >= miss:
                j = rng.normal(0, 0.03, 4) * [w, h, w, h]
                rows.append([top + j[1], left + j[0], top + h + j[3], left + w + j[2], float(np.clip(rng.normal(0.75, 0.15), 0.05, 0.99)), 0])
        for _ in range(int(rng.poisson(clutter))):
            w, h = rng.uniform(20, 60, 2)
            left, top = rng.uniform(0, 320 - w), rng.uniform(0, 224 - h)
            rows.append([top, left, top + h, left + w, float(rng.uniform(0.1, 0.6)), 0])
        rows = rows[:cap]
        counts[f - 1] = len(rows)
        dets[f - 1, :len(rows)] = np.asarray(rows, np.float32).reshape(-1, 6)
    return dets, counts


def main():
    import torch
    from k210_yolo_framework_amd import engine, motmetrics as mm, motmetrics_gpu as mg, track
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='profiles/track_scores.txt')
    a = p.parse_args()
    lines = ['engine.TrackState at track.DEFAULTS %r on generated detections (8 sequences of 120 frames, 10 objects; NOT MOT17), scored by '
             'motmetrics_gpu.MotEvaluator; recorded, not judged' % (track.DEFAULTS,)]
    for label, miss, clutter in (('clean: no misses, no clutter', 0.0, 0.0), ('10 % missed rows, 0.5 clutter boxes a frame', 0.1, 0.5),
                                 ('30 % missed rows, 2 clutter boxes a frame', 0.3, 2.0)):
        lines.append(label)
        for how, opts in (('greedy', {}), ('lap', dict(assign='lap')), ('lap + fuse', dict(assign='lap', fuse_score=True))):
            rng, ev, cap, n_frames = np.random.default_rng(0), mg.MotEvaluator(), 64, 120      # (the same detections for every row)
            for name, gt, _ in mm.synthetic_sequences(8, n_frames, 10, seed=7):
                dets, counts = detections(gt, n_frames, rng, miss, clutter, cap)
                state = engine.TrackState(1, 1, **opts)
                rows, ids, n = (t.cpu().numpy() for t in state.update(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(), [0, n_frames]))
                res = [[f + 1, ids[f, k], r[1], r[0], r[3] - r[1], r[2] - r[0]] for f in range(n_frames) for k, r in enumerate(rows[f, :n[f]])]
                ev.add_sequence(name, gt, np.asarray(res, np.float64).reshape(-1, 6))
            lines.append(f'  {how + ":":12s}' + mm.line('COMBINED', ev.result()['combined']))
            print('\n'.join(lines[-2 if how == 'greedy' else -1:]), flush=True)
    Path(a.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

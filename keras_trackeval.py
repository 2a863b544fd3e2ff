"""make trackeval: HOTA, CLEAR-MOT and identity scores of tracks files against ground truth (k210_yolo_framework_amd/motmetrics.py).

  python keras_trackeval.py --gt GT --res RES          GT and RES hold <sequence>.txt in the MOTChallenge text format (what
                                                       `make detect TRACK=True` writes to OUTDIR/tracks); GT may also be the MOTChallenge
                                                       layout <sequence>/gt/gt.txt.  Writes trackeval.json beside RES.
  python keras_trackeval.py --synthetic 4              scores motmetrics.synthetic_sequences: runs on a clean checkout

Scoring is class-agnostic.  --device gpu (default) runs motmetrics_gpu.MotEvaluator (yk_mot_eval: similarity, assignment and the three
scores in HIP; no device is an error); --device cpu runs the numpy rule, which the kernels are held to."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

from k210_yolo_framework_amd import motmetrics as mm


def find_sequences(gt_dir: Path, res_dir: Path):
    """-> (name, gt file, result file) each; a sequence present on one side only is an error naming it."""
    res = {p.stem: p for p in sorted(res_dir.glob('*.txt'))}
    gt = {p.stem: p for p in sorted(gt_dir.glob('*.txt'))}
    gt.update({p.parent.parent.name: p for p in sorted(gt_dir.glob('*/gt/gt.txt'))})
    for name in sorted(set(gt) ^ set(res)):
        raise ValueError(f'sequence {name!r} is in {gt_dir if name in gt else res_dir} only')
    if not gt:
        raise ValueError(f'no <sequence>.txt in {gt_dir} and {res_dir}')
    return [(name, gt[name], res[name]) for name in sorted(gt)]


def jsonable(m):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v.item() if isinstance(v, np.generic) else v) for k, v in m.items()}


def main(argv=None) -> dict:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--gt', type=str, default='', help='folder of ground-truth <sequence>.txt or <sequence>/gt/gt.txt')
    p.add_argument('--res', type=str, default='', help='folder of result <sequence>.txt')
    p.add_argument('--device', type=str, default='gpu', choices=['gpu', 'cpu'], help='gpu: the HIP evaluator; cpu: the numpy rule')
    p.add_argument('--synthetic', type=int, default=0, help='score this many generated sequences instead of files')
    p.add_argument('--seq_frames', type=int, default=60)
    p.add_argument('--seq_objects', type=int, default=8)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--out', type=str, default='', help='the JSON file (default: trackeval.json beside RES; with --synthetic none)')
    a = p.parse_args(argv)
    if a.synthetic > 0:
        seqs = mm.synthetic_sequences(a.synthetic, a.seq_frames, a.seq_objects, a.seed)
        out = Path(a.out) if a.out else None
    else:
        if not a.gt or not a.res:
            raise ValueError('--gt and --res (or --synthetic N) are needed')
        seqs = [(n, mm.load_mot_text(g, ground_truth=True), mm.load_mot_text(r)) for n, g, r in find_sequences(Path(a.gt), Path(a.res))]
        out = Path(a.out) if a.out else Path(a.res).resolve().parent / 'trackeval.json'
    if a.device == 'gpu':
        from k210_yolo_framework_amd import motmetrics_gpu
        ev = motmetrics_gpu.MotEvaluator()
        for seq in seqs:
            ev.add_sequence(*seq)
        result = ev.result()
    else:
        result = mm.evaluate(seqs)
    for name, m in result['sequences'].items():
        print(mm.line(name, m))
    print(mm.line('COMBINED', result['combined']))
    if out is not None:
        out.write_text(json.dumps(dict(sequences={n: jsonable(m) for n, m in result['sequences'].items()},
                                       combined=jsonable(result['combined'])), indent=1))
        print(f'wrote {out}')
    return result


if __name__ == '__main__':
    try:
        main()
    except ValueError as e:
        sys.exit(f'keras_trackeval: {e}')

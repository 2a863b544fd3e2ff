"""What `make kmodel BIASCORRECT=True` costs and buys on one MI355X -> profiles/biascorrect_error.txt.

    python tools/biascorrect_error.py [--images 256] [--batch 32] [--bins 2048] [--percentile 99.99] [--max-gain 64] [--out FILE]

The protocol of tools/equalize_error.py: the flagship yolo_mobilev1-0.75 at 224x320 with the float weights of the K210 demo's kmodel
(tests/golden/yolo.kmodel), `--images` generated calibration frames (training.synthetic_list, seed 3) and as many HELD-OUT ones (seed
evaluate.SYNTHETIC_SEED).  For minmax, percentile and mse, each with equalisation off and on, each with the correction off and on:
  (a) relative RMS error of the kmodel's dequantised logits (engine.KpuPlan) against the fp32 network on the ORIGINAL weights over the held-out
      frames - twelve figures; the comparison is on against off of the same run;
  (b) calibration images/s of minmax without and with the correction: the whole save_kmodel, host clock, after a warm-up run of each;
  (c) the statistics pass against a plain run on the same plan: KpuPlan.run_stats_u8 and KpuPlan.run_u8 on one batch, HIP events around 10
      back-to-back runs, the two alternated over five rounds after a warm-up round, median.
Nothing here is compared with a fixed number, and the default stays off whatever it prints."""
import argparse
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
METHODS = ('minmax', 'percentile', 'mse')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--bins', type=int, default=2048)
    ap.add_argument('--percentile', type=float, default=99.99)
    ap.add_argument('--max-gain', type=float, default=64.0)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'biascorrect_error.txt'))
    a = ap.parse_args(argv)
    import torch
    from k210_yolo_framework_amd import biascorrect, engine, evaluate, kmodel, quantize, yolonet
    from k210_yolo_framework_amd.training import synthetic_list
    engine.require_gpu()
    in_hw = (224, 320)
    W, _ = kmodel.to_float_weights(kmodel.parse((ROOT / 'tests' / 'golden' / 'yolo.kmodel').read_bytes()))
    model, _ = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.75)
    model.set_weights(W)
    spec = model.spec
    stack = lambda seed: np.stack([it[0] for it in synthetic_list(a.images, in_hw, 20, seed)])      # noqa: E731
    calib, held = stack(3), stack(evaluate.SYNTHETIC_SEED)
    names = quantize.tensor_names(spec)
    out_names = [names[o] for o in spec.outputs]
    F = [[] for _ in out_names]                                                # the fp32 network on the held-out frames
    ref = quantize.Calibrator(spec, W, max_batch=a.batch)
    for i in range(0, len(held), a.batch):
        keep = {}
        ref.feed(torch.from_numpy(held[i:i + a.batch]).cuda(), keep=keep)
        for k, n in enumerate(out_names):
            F[k].append(keep[n].cpu().numpy().astype(np.float64))
    F = [np.concatenate(f) for f in F]
    den = np.sqrt(sum((f ** 2).sum() for f in F))
    tmp = Path(tempfile.mkdtemp())

    def save(path, method, eq, bc):
        return model.save_kmodel(str(path), calib, batch=a.batch, method=method, percentile=a.percentile, bins=a.bins, equalize=eq,
                                 max_gain=a.max_gain, bias_correct=bc)

    rows, last = [], None
    for method in METHODS:
        for eq in (False, True):
            errs, info = [], None
            for bc in (False, True):
                path = tmp / f'{method}_{int(eq)}_{int(bc)}.kmodel'
                rep = save(path, method, eq, bc)
                km = kmodel.parse(path.read_bytes())
                last = km
                err2 = 0.0
                with engine.KpuPlan(km, max_batch=a.batch) as plan:
                    for i in range(0, len(held), a.batch):
                        fr = torch.from_numpy(held[i:i + a.batch]).cuda()
                        plan.run_u8(fr)
                        torch.cuda.synchronize()
                        for k, o in enumerate(plan.outputs()):
                            err2 += float(((o[:len(fr)].cpu().numpy().astype(np.float64) - F[k][i:i + len(fr)]) ** 2).sum())
                errs.append(np.sqrt(err2) / den)
                if bc:
                    b = rep['biascorrect']['layers']
                    info = (max(r['before'] for r in b.values()), max(r['delta_max'] for r in b.values()), sum(len(r['limited']) for r in b.values()))
            rows.append((method, eq, errs[0], errs[1]) + info)
    rates = {}
    for bc in (False, True, False, True):                                      # the first pair warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        save(tmp / 'rate.kmodel', 'minmax', False, bc)
        torch.cuda.synchronize()
        rates[bc] = len(calib) / (time.perf_counter() - t0)
    fr = torch.from_numpy(calib[:a.batch]).cuda()
    steps = biascorrect.steps_of(last)
    times = {'run_u8': [], 'run_stats_u8': []}
    with engine.KpuPlan(last, max_batch=a.batch) as plan:
        plan.reset_zsums()
        runs = {'run_u8': lambda: plan.run_u8(fr), 'run_stats_u8': lambda: plan.run_stats_u8(fr, steps)}
        for r in range(6):                                                     # round 0 warms up
            for k, f in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    f()
                e1.record()
                e1.synchronize()
                if r:
                    times[k].append(e0.elapsed_time(e1) / 10)
    t = {k: float(np.median(v)) for k, v in times.items()}
    lines = ['Per-channel bias correction of `make kmodel BIASCORRECT=True` on one MI355X (tools/biascorrect_error.py; DESIGN.md 3.9).',
             f'yolo_mobilev1-0.75, 224x320, the demo kmodel\'s float weights (BatchNorm already folded by nncase); {a.images} generated calibration '
             f'frames (seed 3), {a.images} held-out frames (seed {evaluate.SYNTHETIC_SEED}); batch {a.batch}, {a.bins} bins, percentile '
             f'{a.percentile}, max_gain {a.max_gain:g}.  Generated frames are not VOC: the effect on real images, and on mAP, is not measured.',
             '',
             f"{'method':<12}{'equalise':>9}{'(a) rel. RMS logit error, off':>32}{'on':>12}{'worst mean off by (codes)':>28}{'largest delta (codes)':>24}"
             f"{'limited':>9}"]
    for method, eq, e0, e1, before, dmax, nlim in rows:
        lines.append(f"{method:<12}{'on' if eq else 'off':>9}{e0:>32.6f}{e1:>12.6f}{before:>28.4f}{dmax:>24.4f}{nlim:>9}")
    lines += ['', f'(b) calibration images/s, minmax, the whole save_kmodel: {rates[False]:.1f} without, {rates[True]:.1f} with the correction '
                  f'({rates[False] / rates[True]:.2f}x the time; {len(spec.layers)} statistics passes over the {a.images} frames)',
              '', f"(c) one batch of {a.batch} on the same plan, median ms: KpuPlan.run_u8 {t['run_u8']:.4f}   KpuPlan.run_stats_u8 {t['run_stats_u8']:.4f} "
                  f"({t['run_stats_u8'] / t['run_u8']:.2f}x)"]
    text = '\n'.join(lines) + '\n'
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == '__main__':
    main()

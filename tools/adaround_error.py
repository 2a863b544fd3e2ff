"""What `make kmodel ADAROUND=True` costs and buys on one MI355X -> profiles/adaround_error.txt.

    python tools/adaround_error.py [--images 256] [--batch 32] [--bins 2048] [--percentile 99.99] [--max-gain 64] [--iters 1000] [--out FILE]

The protocol of tools/biascorrect_error.py: the flagship yolo_mobilev1-0.75 at 224x320 with the float weights of the K210 demo's kmodel
(tests/golden/yolo.kmodel), `--images` generated calibration frames (training.synthetic_list, seed 3) and as many HELD-OUT ones (seed
evaluate.SYNTHETIC_SEED).  For minmax, percentile and mse, each without and with EQUALIZE=True + BIASCORRECT=True, each with adaptive rounding
off and on (the defaults: lambda 0.01, lr 0.01):
  (a) relative RMS error of the kmodel's dequantised logits (engine.KpuPlan) against the fp32 network on the ORIGINAL weights over the held-out
      frames - twelve figures; the comparison is on against off of the same run;
  (b) calibration images/s of minmax + EQUALIZE=True without and with adaptive rounding: the whole save_kmodel, host clock, after a warm-up
      run of each;
  (c) the time of one iteration (P = D G + the step) of the layer with the most free weights, on the equalised weights: the HIP events
      gpu_optimise_layer records around its loop of `--iters` iterations, / iterations, median of five rounds after a warm-up round; and the
      host clock of the whole call.
The demo's float weights are the dequantised codes of an 8-bit file, so without equalisation nearly every weight lies on its own grid (r = 0)
and is frozen: the rows without equalisation show that case, and (b) and (c) are taken on the equalised weights, which are off the grid.
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
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'adaround_error.txt'))
    a = ap.parse_args(argv)
    import torch
    from k210_yolo_framework_amd import adaround, engine, evaluate, kmodel, netspec as ns, quantize, yolonet
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
    del ref
    tmp = Path(tempfile.mkdtemp())

    def save(path, method, both, ada, bc=None):
        return model.save_kmodel(str(path), calib, batch=a.batch, method=method, percentile=a.percentile, bins=a.bins, equalize=both,
                                 max_gain=a.max_gain, bias_correct=both if bc is None else bc, adaround=ada, ada_iters=a.iters)

    rows = []
    for method in METHODS:
        for both in (False, True):
            errs, info = [], None
            for ada in (False, True):
                path = tmp / f'{method}_{int(both)}_{int(ada)}.kmodel'
                rep = save(path, method, both, ada)
                km = kmodel.parse(path.read_bytes())
                err2 = 0.0
                with engine.KpuPlan(km, max_batch=a.batch) as plan:
                    for i in range(0, len(held), a.batch):
                        fr = torch.from_numpy(held[i:i + a.batch]).cuda()
                        plan.run_u8(fr)
                        torch.cuda.synchronize()
                        for k, o in enumerate(plan.outputs()):
                            err2 += float(((o[:len(fr)].cpu().numpy().astype(np.float64) - F[k][i:i + len(fr)]) ** 2).sum())
                errs.append(np.sqrt(err2) / den)
                if ada:
                    L = [r for r in rep['adaround']['layers'].values() if not r['skipped']]
                    info = (sum(r['flipped'] for r in L), sum(r['rows_changed'] for r in L), sum(r['rows'] for r in L),
                            float(np.mean([r['ratio'] for r in L])), len(rep['adaround']['layers']) - len(L),
                            sum(r['free'] for r in L), sum(r['rows'] * (r['free'] + r['frozen']) // max(1, r['rows']) for r in L))
            rows.append((method, both, errs[0], errs[1]) + info)
    rates = {}
    for ada in (False, True, False, True):                                     # the first pair warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        save(tmp / 'rate.kmodel', 'minmax', True, ada, bc=False)
        torch.cuda.synchronize()
        rates[ada] = len(calib) / (time.perf_counter() - t0)
    from k210_yolo_framework_amd import equalize
    We, _ = equalize.equalize(spec, W, quantize.calibrate_channels(spec, W, calib, a.batch), a.max_gain)
    big = max((op for op in spec.ops if op['type'] in (ns.OP_CONV, ns.OP_DWCONV)),
              key=lambda op: int((~adaround.setup(np.asarray(We[op['layer'] + '/kernel'], np.float64))['frozen']).sum()))
    G, _ = adaround.gpu_grams(spec, We, calib[:a.batch], a.batch, only={big['layer']})
    krows = adaround.rows_of(np.asarray(We[big['layer'] + '/kernel'], np.float64), big['type'] == ns.OP_DWCONV)
    per, whole, free = [], [], 0
    for r in range(6):                                                         # round 0 warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = adaround.gpu_optimise_layer(krows, G[big['layer']], a.iters, 0.01, 1e-2)
        torch.cuda.synchronize()
        if r:
            per.append(info['loop_ms'] / a.iters)
            whole.append(time.perf_counter() - t0)
        free = info['free']
    lines = ['Adaptive weight rounding of `make kmodel ADAROUND=True` on one MI355X (tools/adaround_error.py; DESIGN.md 3.9).',
             f'yolo_mobilev1-0.75, 224x320, the demo kmodel\'s float weights (BatchNorm already folded by nncase); {a.images} generated calibration '
             f'frames (seed 3), {a.images} held-out frames (seed {evaluate.SYNTHETIC_SEED}); batch {a.batch}, {a.bins} bins, percentile '
             f'{a.percentile}, max_gain {a.max_gain:g}; {a.iters} iterations, lambda 0.01, lr 0.01 (the defaults: starting points, not findings).  '
             f'Generated frames are not VOC: the effect on real images, and on `make eval PRECISION=kpu` mAP, is not run.',
             '',
             f"{'method':<12}{'equalise + bias':>16}{'(a) rel. RMS logit error, off':>32}{'on':>12}{'weights flipped':>17}{'rows changed':>16}"
             f"{'mean E ratio':>14}{'skipped':>9}{'free weights':>14}"]
    for method, both, e0, e1, flipped, changed, nrows, ratio, skipped, nfree, _ in rows:
        lines.append(f"{method:<12}{'on' if both else 'off':>16}{e0:>32.6f}{e1:>12.6f}{flipped:>17}{f'{changed}/{nrows}':>16}{ratio:>14.4f}{skipped:>9}{nfree:>14}")
    lines += ['', f'(b) calibration images/s, minmax + equalisation, the whole save_kmodel: {rates[False]:.1f} without, {rates[True]:.1f} with adaptive rounding '
                  f'({rates[False] / rates[True]:.2f}x the time; {len(spec.layers)} layers, {a.iters} iterations each)',
              '', f"(c) one iteration of {big['layer']} on the equalised weights ({krows.shape[0]} x {krows.shape[1]} weights, {free} free), median ms: {float(np.median(per)):.4f} "
                  f"(the whole layer - Gram matrix to the host, {a.iters} iterations, hardening in float64 on the host: {float(np.median(whole)):.3f} s)"]
    text = '\n'.join(lines) + '\n'
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == '__main__':
    main()

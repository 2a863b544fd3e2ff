"""What `make kmodel EQUALIZE=True` costs and buys on one MI355X -> profiles/equalize_error.txt.

    python tools/equalize_error.py [--images 256] [--batch 32] [--bins 2048] [--percentile 99.99] [--max-gain 64] [--no-map] [--out FILE]

The set-up of tools/calib_methods.py: the flagship yolo_mobilev1-0.75 at 224x320 with the float weights of the K210 demo's kmodel
(tests/golden/yolo.kmodel), `--images` generated calibration frames (training.synthetic_list, seed 3) and as many HELD-OUT ones (seed
evaluate.SYNTHETIC_SEED).  For minmax, percentile and mse, each with equalisation off and on:
  (a) relative RMS error of the kmodel's dequantised logits (engine.KpuPlan) against the fp32 network on the ORIGINAL weights (the
      Calibrator's own fp32 forward pass) over the held-out frames;
  (b) mAP of the kmodel through evaluate.main --precision kpu on the same held-out set, as that tool reports it (--no-map leaves it out);
  (c) calibration images/s of minmax with and without the per-channel pass: quantize.calibrate alone against quantize.calibrate_channels +
      equalize.equalize + quantize.calibrate, host clock around work that ends in a device synchronise, after a warm-up run;
  (d) the time of one yk_scale_act_chrange_f32 launch against one yk_scale_act_range_f32 launch - the same bytes read and written - on the
      largest tensor of the walk (conv1's output at `--batch` frames) and on its widest (the 7x10 tensor of conv_pw_13): HIP events around
      20 back-to-back launches, the two alternated over 7 rounds after a warm-up round, median.  Once into slots that already hold the
      tensor's range (a calibration after its first batches: the new kernel then skips its atomics), once with a yk_range_reset before
      every launch (its launch is in both kernels' figures).
Nothing here is compared with a fixed number, and the default stays off whatever it prints."""
import argparse
import ctypes as C
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
METHODS = ('minmax', 'percentile', 'mse')


def kernel_times(L, M, Cn, rounds=7, reps=20):
    """{kernel: median ms per launch} on an [M][Cn] LeakyReLU tensor."""
    import torch
    from k210_yolo_framework_amd import engine, netspec as ns
    p = engine._ptr
    rng = np.random.default_rng(0)
    z = torch.from_numpy(rng.standard_normal((M, Cn)).astype(np.float32)).cuda()
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, Cn).astype(np.float32)).cuda()
    bi = torch.from_numpy((0.1 * rng.standard_normal(Cn)).astype(np.float32)).cuda()
    y = torch.empty_like(z)
    d_range = torch.zeros(4 * (Cn + 1), dtype=torch.int32, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    engine._check(L.yk_range_reset(p(d_range), Cn + 1, s), 'yk_range_reset')
    runs = {'range': lambda: L.yk_scale_act_range_f32(p(z), C.c_longlong(M), Cn, p(sc), p(bi), ns.ACT_LEAKY, C.c_float(0.3), p(y), p(d_range), Cn, s),
            'chrange': lambda: L.yk_scale_act_chrange_f32(p(z), C.c_longlong(M), Cn, p(sc), p(bi), ns.ACT_LEAKY, C.c_float(0.3), p(y), p(d_range), 0, s)}
    reset = lambda: L.yk_range_reset(p(d_range), Cn + 1, s)                      # noqa: E731
    for k in ('range', 'chrange'):                                             # the same after a reset: every workgroup has something to fold in
        runs[k + '_fresh'] = (lambda f: lambda: reset() or f())(runs[k])
    times = {k: [] for k in runs}
    for r in range(rounds + 1):                                                # round 0 warms the kernels up
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                engine._check(f(), k)
            e1.record()
            e1.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) / reps)
    return {k: float(np.median(v)) for k, v in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--bins', type=int, default=2048)
    ap.add_argument('--percentile', type=float, default=99.99)
    ap.add_argument('--max-gain', type=float, default=64.0)
    ap.add_argument('--no-map', action='store_true')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'equalize_error.txt'))
    a = ap.parse_args(argv)
    import torch
    from k210_yolo_framework_amd import engine, equalize, evaluate, kmodel, quantize, yolonet
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
    rows, tmp, eq_rep = [], Path(tempfile.mkdtemp()), None
    for method in METHODS:
        for on in (False, True):
            path = tmp / f'{method}_{int(on)}.kmodel'
            rep = model.save_kmodel(str(path), calib, batch=a.batch, method=method, percentile=a.percentile, bins=a.bins, equalize=on,
                                    max_gain=a.max_gain)
            eq_rep = rep.get('equalize', eq_rep)
            km = kmodel.parse(path.read_bytes())
            err2 = 0.0
            with engine.KpuPlan(km, max_batch=a.batch) as plan:
                for i in range(0, len(held), a.batch):
                    fr = torch.from_numpy(held[i:i + a.batch]).cuda()
                    plan.run_u8(fr)
                    torch.cuda.synchronize()
                    for k, o in enumerate(plan.outputs()):
                        err2 += float(((o[:len(fr)].cpu().numpy().astype(np.float64) - F[k][i:i + len(fr)]) ** 2).sum())
            m = None
            if not a.no_map:
                m = evaluate.main([str(path), '--precision', 'kpu', '--synthetic', str(a.images), '--out', str(tmp / f'{method}_{int(on)}.json')])['map']
            rows.append((method, on, np.sqrt(err2) / den, m, min(r['bn_mul_min'] for r in rep['layers'].values())))

    def flow(on):
        w = W
        if on:
            w, _ = equalize.equalize(spec, W, quantize.calibrate_channels(spec, W, calib, a.batch), a.max_gain)
        quantize.calibrate(spec, w, calib, a.batch)                            # ends in the device-to-host read
    rates = {}
    for on in (False, True, False, True):                                      # the first pair warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flow(on)
        rates[on] = len(calib) / (time.perf_counter() - t0)
    h1, w1, c1 = spec.tensors[spec.ops[0]['out']]
    hw_, ww_, cw_ = max((spec.tensors[op['out']] for op in spec.ops if op.get('layer')), key=lambda t: t[2])
    shapes = [('largest', a.batch * h1 * w1, c1), ('widest', a.batch * hw_ * ww_, cw_)]
    kt = [(what, M, Cn, kernel_times(engine.lib(), M, Cn)) for what, M, Cn in shapes]
    lines = ['Cross-layer range equalisation of `make kmodel EQUALIZE=True` on one MI355X (tools/equalize_error.py; DESIGN.md 3.9).',
             f'yolo_mobilev1-0.75, 224x320, the demo kmodel\'s float weights (BatchNorm already folded by nncase); {a.images} generated calibration '
             f'frames (seed 3), {a.images} held-out frames (seed {evaluate.SYNTHETIC_SEED}); batch {a.batch}, {a.bins} bins, percentile '
             f'{a.percentile}, max_gain {a.max_gain:g}.  Generated frames are not VOC: the effect on real images is not measured.',
             '',
             f"{'method':<12}{'equalise':>9}{'(a) rel. RMS error of the logits':>34}{'(b) mAP, kpu':>16}{'smallest |bn_mul|':>19}"]
    for method, on, e, m, bm in rows:
        lines.append(f"{method:<12}{'on' if on else 'off':>9}{e:>34.6f}{'-' if m is None else f'{100 * m:.2f}':>16}{bm:>19}")
    if eq_rep:
        g = [r for r in eq_rep['layers'].values()]
        lines += ['', f"gains: {sum(r['a_changed'] for r in g)} output channels rescaled (step A, g in [{min(r['g_min'] for r in g):.4g}, "
                      f"{max(r['g_max'] for r in g):.4g}]), {sum(r['b_changed'] for r in g)} kernel channels stretched (step B, f up to "
                      f"{max(r['f_max'] for r in g):.4g}); {len(eq_rep['skipped'])} tensors skipped"]
    lines += ['', f'(c) calibration images/s, minmax: {rates[False]:.1f} without, {rates[True]:.1f} with the per-channel pass and the host-side rule '
                  f'({rates[True] / rates[False]:.2f}x)',
              '', '(d) one launch, LeakyReLU, median ms (both kernels read and write the same bytes):']
    for what, M, Cn, t in kt:
        lines.append(f"    {what:<8} {M} x {Cn} fp32   yk_scale_act_range_f32 {t['range']:.4f}   yk_scale_act_chrange_f32 {t['chrange']:.4f} "
                     f"({t['chrange'] / t['range']:.2f}x);   after a reset each: {t['range_fresh']:.4f} / {t['chrange_fresh']:.4f} "
                     f"({t['chrange_fresh'] / t['range_fresh']:.2f}x)")
    text = '\n'.join(lines) + '\n'
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == '__main__':
    main()

"""What the calibration methods of `make kmodel CALIBMETHOD=` cost and buy on one MI355X -> profiles/calib_methods.txt.

    python tools/calib_methods.py [--images 256] [--batch 32] [--bins 2048] [--percentile 99.99] [--alt-lib libyolo_hip_alt.so] [--out FILE]

The flagship yolo_mobilev1-0.75 at 224x320 with the float weights of the K210 demo's kmodel (tests/golden/yolo.kmodel), calibrated on
`--images` generated frames (training.synthetic_list, seed 3: what `make kmodel SYNTHETIC=` reads).  For minmax, percentile and mse:
  (a) relative RMS error of the kmodel's dequantised logits (engine.KpuPlan) against the fp32 network (the Calibrator's own fp32 forward
      pass, which normalises by 255 as the KPU does), over `--images` HELD-OUT generated frames (seed evaluate.SYNTHETIC_SEED);
  (b) mAP of the kmodel through evaluate.main --precision kpu (`make eval PRECISION=kpu`) on the same held-out set;
  (c) calibration images/s: quantize.calibrate over the calibration set (both passes and the host-side clipping where the method has
      them), host clock around work that ends in a device synchronise, after a warm-up run;
  (d) once: the time of one yk_scale_act_hist_f32 launch against one yk_scale_act_range_f32 launch on the largest tensor of the net at
      `--batch` frames (conv1's output), HIP events around 20 back-to-back launches, the two alternated over 7 rounds, median.  Taken on
      a LeakyReLU tensor (what this net has) and on a ReLU tensor (half the values in the bin of real zero).  --alt-lib times the
      histogram launch of a second build of the library beside it (the form without the per-wave sum of the zero bin).
The bar for (a) and (b) is minmax on the same weights and frames; nothing here is compared with a fixed number."""
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


def kernel_times(L, alt, M, Cn, bins, rounds=7, reps=20):
    """{act name: {kernel: median ms per launch}}"""
    import torch
    from k210_yolo_framework_amd import engine, netspec as ns, quantize
    p = engine._ptr
    rng = np.random.default_rng(0)
    z = torch.from_numpy(rng.standard_normal((M, Cn)).astype(np.float32)).cuda()
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, Cn).astype(np.float32)).cuda()
    bi = torch.from_numpy((0.1 * rng.standard_normal(Cn)).astype(np.float32)).cuda()
    y = torch.empty_like(z)
    d_range = torch.zeros(4, dtype=torch.int32, device='cuda')
    d_hist = torch.zeros(bins, dtype=torch.int64, device='cuda')
    d_flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for act_name, act, alpha in (('leaky', ns.ACT_LEAKY, 0.3), ('relu', ns.ACT_RELU, 0.0)):
        engine._check(L.yk_range_reset(p(d_range), 1, s), 'yk_range_reset')
        run_range = lambda: L.yk_scale_act_range_f32(p(z), C.c_longlong(M), Cn, p(sc), p(bi), act, C.c_float(alpha), p(y), p(d_range), 0, s)  # noqa: E731
        engine._check(run_range(), 'yk_scale_act_range_f32')
        lo, hi = float(y.min()), float(y.max())
        lo, hi = min(lo, 0.0), max(hi, 0.0)
        inv = quantize.hist_inv(np.float32(lo), np.float32(hi), bins)

        def hist_of(lib):
            return lambda: lib.yk_scale_act_hist_f32(p(z), C.c_longlong(M), Cn, p(sc), p(bi), act, C.c_float(alpha), p(y), C.c_float(lo),
                                                     C.c_float(inv), bins, p(d_hist), p(d_flag), 0, s)
        runs = {'range': run_range, 'hist': hist_of(L)}
        if alt is not None:
            runs['hist_alt'] = hist_of(alt)
        times = {k: [] for k in runs}
        for r in range(rounds + 1):                                            # round 0 warms every kernel up
            for k, f in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    engine._check(f(), k)
                e1.record()
                e1.synchronize()
                if r:
                    times[k].append(e0.elapsed_time(e1) / reps)
        out[act_name] = {k: float(np.median(v)) for k, v in times.items()}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--bins', type=int, default=2048)
    ap.add_argument('--percentile', type=float, default=99.99)
    ap.add_argument('--alt-lib', default=None)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'calib_methods.txt'))
    a = ap.parse_args(argv)
    import torch
    from k210_yolo_framework_amd import engine, evaluate, kmodel, quantize, yolonet
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
    quantize.calibrate(spec, W, calib[:a.batch], a.batch, 'mse', a.percentile, a.bins)               # warm-up: every kernel of both passes
    rows, tmp = [], Path(tempfile.mkdtemp())
    for method in METHODS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        quantize.calibrate(spec, W, calib, a.batch, method, a.percentile, a.bins)                    # ends in the device-to-host read
        rate = len(calib) / (time.perf_counter() - t0)
        path = tmp / f'{method}.kmodel'
        rep = model.save_kmodel(str(path), calib, batch=a.batch, method=method, percentile=a.percentile, bins=a.bins)
        km = kmodel.parse(path.read_bytes())
        err2 = 0.0
        with engine.KpuPlan(km, max_batch=a.batch) as plan:
            for i in range(0, len(held), a.batch):
                fr = torch.from_numpy(held[i:i + a.batch]).cuda()
                plan.run_u8(fr)
                torch.cuda.synchronize()
                for k, o in enumerate(plan.outputs()):
                    err2 += float(((o[:len(fr)].cpu().numpy().astype(np.float64) - F[k][i:i + len(fr)]) ** 2).sum())
        ev = evaluate.main([str(path), '--precision', 'kpu', '--synthetic', str(a.images), '--out', str(tmp / f'{method}.json')])
        rows.append((method, np.sqrt(err2) / den, ev['map'], rate, len(rep.get('clipped', []))))
    h1, w1, c1 = spec.tensors[spec.ops[0]['out']]
    alt = None
    if a.alt_lib:
        alt = C.CDLL(str(Path(a.alt_lib).resolve()))
        alt.yk_scale_act_hist_f32.restype = C.c_int
    kt = kernel_times(engine.lib(), alt, a.batch * h1 * w1, c1, a.bins)
    lines = ['Calibration methods of `make kmodel CALIBMETHOD=` on one MI355X (tools/calib_methods.py; DESIGN.md 3.9).',
             f'yolo_mobilev1-0.75, 224x320, the demo kmodel\'s float weights; {a.images} generated calibration frames (seed 3), {a.images} held-out '
             f'frames (seed {evaluate.SYNTHETIC_SEED}); batch {a.batch}, {a.bins} bins, percentile {a.percentile}.',
             '',
             f"{'method':<12}{'(a) rel. RMS error of the logits':>34}{'(b) mAP, kpu':>16}{'(c) calibration images/s':>28}{'clipped tensors':>18}"]
    for method, e, m, rate, nclip in rows:
        lines.append(f"{method:<12}{e:>34.6f}{'nan' if m is None else f'{100 * m:.2f}':>16}{rate:>28.1f}{nclip:>18}")
    lines += ['', f'(d) one launch on conv1\'s output at batch {a.batch} ({a.batch * h1 * w1} x {c1} fp32), median ms:']
    for act_name, t in kt.items():
        extra = f", without the per-wave zero-bin sum {t['hist_alt']:.4f} ({t['hist_alt'] / t['range']:.2f}x)" if 'hist_alt' in t else ''
        lines.append(f"    {act_name:<6} yk_scale_act_range_f32 {t['range']:.4f}   yk_scale_act_hist_f32 {t['hist']:.4f} ({t['hist'] / t['range']:.2f}x){extra}")
    text = '\n'.join(lines) + '\n'
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == '__main__':
    main()

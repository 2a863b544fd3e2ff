#!/usr/bin/env python
"""What `make kmodel ANALYZE=True` costs on one MI355X -> profiles/qerror_rate.txt, and what it shows on the demo's weights ->
profiles/qerror_demo.txt.

    python tools/qerror_rate.py [--images 256] [--batch 32] [--reps 5] [--out profiles/qerror_rate.txt] [--demo profiles/qerror_demo.txt]
    python tools/qerror_rate.py --modes off --root OTHER_CHECKOUT --label parent --append      # the parent commit, same script and frames

The flagship yolo_mobilev1-0.75 at 224x320 with the float weights of the K210 demo's kmodel (tests/golden/yolo.kmodel) on `--images` generated
frames (quantize.synthetic_frames, seed 3).
  (a) images/s of the whole model.save_kmodel (minmax) with analyze off and on: host clock around a call that ends in a file written (and, on, in
      the device-to-host read of the sums); the modes alternate, `--reps` times each, after one warm-up call of each; medians, and the spread
      of each mode's repeats.
  (b) one yk_qerr_u8_f32 call (both launches) beside one yk_scale_act_chsum_f32 call on the largest tensor of the net at `--batch` frames (conv1's
      output): HIP events around 20 back-to-back calls, the two alternated over 7 rounds after a warm-up round, medians.  The compare kernel
      reads 5 bytes per element and writes none; the other reads 4 and writes 4.
  --demo: the table under minmax and under EQUALIZE=True CALIBMETHOD=percentile, as the option prints it."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
ap = argparse.ArgumentParser()
ap.add_argument('--images', type=int, default=256)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--modes', default='off,on')
ap.add_argument('--root', default=str(HERE), help='checkout whose package is measured')
ap.add_argument('--label', default='this commit')
ap.add_argument('--out', default='profiles/qerror_rate.txt')
ap.add_argument('--demo', default=None, help='also write the demo tables to this file')
ap.add_argument('--append', action='store_true')
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def kernel_times(M, Cn, B, qh, qw, rounds=7, reps=20):
    import torch
    from k210_yolo_framework_amd import engine, netspec as ns
    rng = np.random.default_rng(0)
    z = torch.from_numpy(rng.standard_normal((M, Cn)).astype(np.float32)).cuda()
    q = torch.from_numpy(rng.integers(0, 256, (B, qh, qw, Cn)).astype(np.uint8)).cuda()
    sc, bi = torch.ones(Cn, device='cuda'), torch.zeros(Cn, device='cuda')
    y = torch.empty_like(z)
    need = C.c_size_t()
    engine.call('yk_chsum_workspace_bytes', M, Cn, C.byref(need))
    w_sum = torch.empty(need.value // 8, dtype=torch.float64, device='cuda')
    engine.call('yk_qerr_workspace_bytes', M, Cn, C.byref(need))
    w_err = torch.empty(need.value // 8, dtype=torch.int64, device='cuda')
    d_sum, d_flag = torch.zeros(Cn, dtype=torch.float64, device='cuda'), torch.zeros(Cn, dtype=torch.int32, device='cuda')
    d_err = torch.zeros(10 * Cn, dtype=torch.int64, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = {'yk_scale_act_chsum_f32': lambda: engine.call('yk_scale_act_chsum_f32', z, M, Cn, sc, bi, ns.ACT_LEAKY, 0.1, y, d_sum, d_flag, 0, w_sum, s),
            'yk_qerr_u8_f32': lambda: engine.call('yk_qerr_u8_f32', q, z, B, qh, qw, Cn, 1, 0.05, 30, d_err, 0, w_err, s)}
    times = {k: [] for k in runs}
    for r in range(rounds + 1):                                                # round 0 warms both up
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) / reps)
    return {k: float(np.median(v)) for k, v in times.items()}


def main():
    import torch
    import k210_yolo_framework_amd
    from k210_yolo_framework_amd import engine, kmodel, quantize, yolonet
    if a.demo:
        from k210_yolo_framework_amd import qerror
    engine.require_gpu()
    W, _ = kmodel.to_float_weights(kmodel.parse((HERE / 'tests' / 'golden' / 'yolo.kmodel').read_bytes()))
    model, _ = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.75)
    model.set_weights(W)
    frames = torch.from_numpy(quantize.synthetic_frames(a.images, (224, 320), seed=3)).cuda()
    tmp = Path(tempfile.mkdtemp())
    modes = a.modes.split(',')

    def save(mode, **kw):
        if mode == 'on':
            kw['analyze'] = True
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = model.save_kmodel(str(tmp / f'{mode}.kmodel'), frames, batch=a.batch, **kw)
        torch.cuda.synchronize()
        return a.images / (time.perf_counter() - t0), rep

    say(f'[{a.label}] model.save_kmodel images/s, yolo_mobilev1-0.75 224x320, the demo kmodel\'s float weights, {a.images} generated frames (seed 3), batch '
        f'{a.batch}, minmax; {a.reps} alternating repeats after a warm-up call of each mode; package '
        f'{os.path.relpath(os.path.dirname(k210_yolo_framework_amd.__file__), HERE)}; {time.strftime("%Y-%m-%d")}')
    for m in modes:
        save(m)
    runs = {m: [] for m in modes}
    for _ in range(a.reps):
        for m in modes:
            runs[m].append(save(m)[0])
    med = {}
    for m in modes:
        v = np.array(runs[m])
        med[m] = float(np.median(v))
        say(f'[{a.label}] (a) ANALYZE {m:<4} median {np.median(v):8.1f} images/s   runs {" ".join(f"{x:.1f}" for x in v)}   spread (max-min)/median '
            f'{100 * (v.max() - v.min()) / np.median(v):.1f} %')
    if 'off' in med and 'on' in med:
        say(f'[{a.label}] (a) on / off = {med["on"] / med["off"]:.3f}: the analysis takes {a.images / med["on"] - a.images / med["off"]:.3f} s of '
            f'{a.images / med["on"]:.3f} s')
    if 'on' in modes:
        h1, w1, c1 = model.spec.tensors[model.spec.ops[0]['out']]
        M = a.batch * h1 * w1
        kt = kernel_times(M, c1, a.batch, h1, w1)
        gb = {'yk_scale_act_chsum_f32': 8e-9 * M * c1, 'yk_qerr_u8_f32': 5e-9 * M * c1}
        for k, t in kt.items():
            say(f'[{a.label}] (b) {k:<24} {t:.4f} ms per call on conv1\'s output at batch {a.batch} ({M} x {c1}): {gb[k]:.4f} GB moved, '
                f'{gb[k] / (t * 1e-3):.0f} GB/s')
    out = HERE / a.out
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, 'a' if a.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if a.demo:
        text = [f'The table of `make kmodel ANALYZE=True` on the demo kmodel\'s float weights (tools/qerror_rate.py --demo), {a.images} generated calibration '
                f'frames (seed 3), measured on those frames; {time.strftime("%Y-%m-%d")}.']
        for title, kw in (('CALIBMETHOD=minmax', {}), ('EQUALIZE=True CALIBMETHOD=percentile', dict(equalize=True, method='percentile'))):
            rep = save('on', **kw)[1]
            text += ['', f'---- {title}', qerror.format_report(rep['qerror'])]
        (HERE / a.demo).write_text('\n'.join(text) + '\n')
        print('\n'.join(text))


if __name__ == '__main__':
    main()

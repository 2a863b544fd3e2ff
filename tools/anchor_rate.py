"""Rate of the many-start anchor k-means: datatools.run_kmeans_restarts(device='gpu') against device='cpu', the numpy loop.
  python tools/anchor_rate.py [out=profiles/anchor_kmeans_rate.txt] [gpu_runs=20] [cpu_runs=2] [n=40000] [restarts=256]
Generated boxes (w, h = clip(exp(N(-1.6, 0.7)), 0.004, 1), seed 0), k = 6 and 9, 10 iterations, starts = anchor_inits(k, restarts, True, seed=0).
  gpu call   run_kmeans_restarts(..., 'gpu'), wall clock: upload of boxes and starts, workspace allocation, the library call, a stream
             synchronise, download of centroids, assignments, scores and flags.  One warm-up, then `gpu_runs` runs.
  kernels    the library call alone between two device events on buffers that are already there, same runs.
  cpu loop   run_kmeans_restarts(..., 'cpu'), wall clock, `cpu_runs` runs (no warm-up: numpy has nothing to load).
The two results are compared (flags equal, centroids and scores within 1e-9) before a time is written.  Needs a device: no fallback."""
import ctypes as C
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch
from k210_yolo_framework_amd import datatools, engine

arg = lambda i, d: type(d)(sys.argv[i]) if len(sys.argv) > i else d
out_path, gpu_runs, cpu_runs, n, R = arg(1, os.path.join(root, 'profiles', 'anchor_kmeans_rate.txt')), arg(2, 20), arg(3, 2), arg(4, 40000), arg(5, 256)
ITERS = 10
engine.require_gpu()
x = np.clip(np.exp(np.random.default_rng(0).normal(-1.6, 0.7, (n, 2))), 0.004, 1.0)


def wall_ms(fn, runs, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def kernels_ms(inits, runs):
    """The library call alone: device events around it, buffers uploaded and allocated before."""
    (R_, k, _), nbytes = inits.shape, C.c_size_t()
    engine.call('yk_anchor_kmeans_workspace_bytes', n, k, R_, C.byref(nbytes))
    d_x, d_i = torch.from_numpy(x).cuda(), torch.from_numpy(inits).cuda()
    d_c, d_score = torch.empty_like(d_i), torch.empty((R_,), dtype=torch.float64, device='cuda')
    d_counts, d_empty = torch.empty((R_, k), dtype=torch.int32, device='cuda'), torch.empty((R_,), dtype=torch.int32, device='cuda')
    d_idx, work = torch.empty((R_, n), dtype=torch.uint8, device='cuda'), torch.empty((nbytes.value,), dtype=torch.uint8, device='cuda')
    ts = []
    for i in range(runs + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        engine.call('yk_anchor_kmeans_f64', d_x, n, d_i, k, R_, ITERS, d_c, d_counts, d_score, d_empty, d_idx, work, nbytes.value, engine._stream())
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return ts


row = lambda name, ts, f: f'      {name:<22}' + ' '.join(f'{t:9{f}}' for t in (ts if len(ts) <= 6 else ts[:6])) + ('  ...' if len(ts) > 6 else '')
lines = [f'Rate of the many-start anchor k-means (DESIGN.md 3.13).  One MI355X, one process, GPU otherwise idle.  python tools/anchor_rate.py',
         f'{n} generated boxes, {R} starts, {ITERS} iterations: {n * R * ITERS} assignments of one box, each against k centroids, per call.', '']
for k in (6, 9):
    inits = datatools.anchor_inits(k, R, True, seed=0)
    res = {}

    def gpu():
        res['gpu'] = datatools.run_kmeans_restarts(x, inits, ITERS, 'gpu')

    def cpu():
        res['cpu'] = datatools.run_kmeans_restarts(x, inits, ITERS, 'cpu')

    g = wall_ms(gpu, gpu_runs, 1)
    kt = kernels_ms(inits, gpu_runs)
    print(f'k = {k}: gpu done, median {statistics.median(g):.3f} ms; cpu loop running', flush=True)
    c = []
    for _ in range(cpu_runs):
        c += wall_ms(cpu, 1, 0)
        print(f'k = {k}: cpu run {c[-1]:.0f} ms', flush=True)       # (a sign of life: a run takes a minute)
    (gc, gs, ge), (cc, cs, ce) = res['gpu'], res['cpu']
    ok = ce == 0
    assert np.array_equal(ge, ce) and np.nanmax(np.abs(gc - cc), initial=0) <= 1e-9 and (np.abs(gs[ok] - cs[ok]) <= 1e-9).all(), 'results differ'
    best = datatools.select_anchors(gc, gs, ge)[0]
    assert best == datatools.select_anchors(cc, cs, ce)[0]
    gm, km, cm = statistics.median(g), statistics.median(kt), statistics.median(c)
    lines += [f'k = {k}: {int(ok.sum())}/{R} starts keep every cluster; mean IoU best {gs[best]:.6f} (start {best}), worst {np.nanmin(gs):.6f}, '
              f'start 0 {gs[0]:.6f}; both sides pick the same start, flags equal, centroids and scores within 1e-9',
              f'      {"":<22}' + ' '.join(f'{"run " + str(i + 1):>9}' for i in range(min(6, max(len(g), len(c))))),
              row('gpu call, ms', g, '.3f'), f'      {"":<22}median {gm:.3f}, min {min(g):.3f}, max {max(g):.3f} of {len(g)} runs after one warm-up',
              row('kernels alone, ms', kt, '.3f'), f'      {"":<22}median {km:.3f}, min {min(kt):.3f}, max {max(kt):.3f} of {len(kt)} runs '
              f'({2 * ITERS + 2} launches, a memset and a copy: {km / (2 * ITERS + 4) * 1e3:.1f} us each)',
              row('cpu loop, ms', c, '.0f'), f'      {"":<22}median {cm:.0f}, min {min(c):.0f}, max {max(c):.0f} of {len(c)} runs',
              f'      ratio of the medians, cpu loop / gpu call: {cm / gm:.0f}', '']
text = '\n'.join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(text.rstrip('\n') + '\n')

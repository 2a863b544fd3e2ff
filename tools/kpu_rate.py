"""Rate of the KPU-exact mode (engine.KpuPlan) on one device, with the CPU oracle's rate on this host for scale.

    python tools/kpu_rate.py [--batches 1 8 32 128] [--iters 20] [--oracle-images 2] [--json out.json]

Reports images/s of KpuPlan.run_u8 at every batch size, eager (one host call per launch) and graph-replayed (engine.capture, one host
call per run), the median duration of every launch at the largest batch (HIP events around each launch), and how many images/s
oracle/kpu_ref.py manages on the CPU.  Frames are seeded noise at the kmodel's input size; the rate does not depend on the pixels.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kmodel', default=str(ROOT / 'tests' / 'golden' / 'yolo.kmodel'))
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 32, 128])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--oracle-images', type=int, default=2)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    import torch
    from k210_yolo_framework_amd import engine, kmodel
    from oracle import kpu_ref
    km = kmodel.parse(Path(a.kmodel).read_bytes())
    Bmax = max(a.batches)
    plan = engine.KpuPlan(km, max_batch=Bmax)
    c, h, w = plan.input_chw
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (Bmax, h, w, c), dtype=np.uint8)).cuda()
    s = torch.cuda.Stream()
    sh = C.c_void_p(s.cuda_stream)
    res = {'batches': {}, 'launches': []}
    for B in a.batches:
        x = frames[:B].contiguous()
        torch.cuda.synchronize()
        for _ in range(3):
            plan.run_u8(x, stream=s)
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            plan.run_u8(x, stream=s)
        s.synchronize()
        eager = B * a.iters / (time.perf_counter() - t0)
        g = engine.capture(sh, lambda: plan.run_u8(x, stream=s))
        for _ in range(3):
            g.launch(sh)
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            g.launch(sh)
        s.synchronize()
        graph = B * a.iters / (time.perf_counter() - t0)
        g.close()
        res['batches'][B] = {'eager_img_s': eager, 'graph_img_s': graph}
        print(f'batch {B:4d}: eager {eager:10.1f} img/s   graph {graph:10.1f} img/s', flush=True)
    ms = plan.profile(frames, iters=max(3, a.iters // 2), stream=s)
    names = plan.launches()
    tot = float(ms.sum())
    print(f'per-launch medians at batch {Bmax} (sum {tot:.3f} ms = {Bmax / tot * 1e3:.1f} img/s of kernel time):')
    for n, m in sorted(zip(names, ms.tolist()), key=lambda t: -t[1]):
        res['launches'].append({'name': n, 'ms': m})
        print(f'  {m:8.4f} ms  {100 * m / tot:5.1f}%  {n}')
    if a.oracle_images > 0:
        f = rng.integers(0, 256, (c, h, w), dtype=np.uint8)
        t0 = time.perf_counter()
        for _ in range(a.oracle_images):
            kpu_ref.run(km, f)
        res['oracle_img_s'] = a.oracle_images / (time.perf_counter() - t0)
        print(f'oracle/kpu_ref.py on the CPU: {res["oracle_img_s"]:.2f} img/s')
    plan.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))
    return res


if __name__ == '__main__':
    main()

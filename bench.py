#!/usr/bin/env python
"""bench.py — images/sec end-to-end, yolo_mobilev1-0.75, 224x320 network tensor (320x240 frames), B=32/GPU.

One "step" = one pass of the hot path over one batch of synthetic u8 frames ALREADY RESIDENT IN HBM:
  per-image max normalise -> conv backbone + head (HIP) -> Python-mode decode + per-class NMS (keras_inference.py:94-135 semantics)
  -> detections in HBM.
`value` is quoted in the precision mode whose -m gpu test asserts BASELINE.json's tolerance (scores / coords within 1e-3 of the fp32
path, identical detection sets): `--precision f16x2`, the default.  The plain fp16-storage mode (5e-3 worst case, tests/test_gpu_e2e.py)
is measured in a `--full` run and reported under `secondary`.
`--streams` (default 4) independent batches are kept in flight (step i on stream i mod 4, own plan and decode scratch; the part has four
compute pipes: 3 -> 79 k, 4 -> 82 k, 5 -> 68 k, 6 -> 72 k, 8 -> 75 k images/s whoever creates the streams, profiles/r05_diag_batch_streams.txt);
the one-batch-in-flight rate is measured in a `--full` run and reported beside it.
N>1: one process per GPU (torch.distributed / RCCL used only for the barrier + max-over-ranks of the
timing); images are sharded across ranks, weights replicated, NO data-path collective ("weak" scaling).  `python bench.py --gpus N`
starts the N ranks itself (re-executes under torch.distributed.run on 127.0.0.1) when it is not already running under a launcher, and
refuses loudly when the box has fewer than N devices.  `--stub` replaces the GPU step by a fixed sleep and RCCL by gloo: the launcher,
rendezvous, barrier and max-over-ranks path of the bench can then be exercised on a CPU-only box (tests/test_bench_launcher.py).

Timing: W warm-up steps (at least 3), then ONE region of EXACTLY K steps (`--steps`), bracketed by barrier + synchronize on both sides;
`ms_per_step` = the region's time / K.

`--dump-outputs DIR` writes what the last timed step computed, as a caller of the step receives it, to DIR/<name>.npy (float32):
detections + counts (or, with --from-host, the host rows + offsets) and the network's output tensors behind them.  Frames and
weights are seeded, so two builds run with the same arguments can be compared output for output.

A plain run (no `--full`) sets up, warms up, times the K steps, dumps if asked and prints the headline line.  `--full` adds
everything else this file measures: the one-batch rate, per-launch profiles and the roofline, the from-host rate, the secondary
variants, the training step and the CPU baseline.

Prints ONE JSON line on rank 0 (contract in the task statement); with `--full` it also holds
  roofline        the dominant kernel, HIP-event timing on the launch stream, algorithmic bytes = SURVEY 8(d) in+out fp16
  cpu_baseline    the CPU path timed on this box's host cores on a bounded sample (oracle port + torch-CPU/oneDNN graph)
  value_from_host the same step fed from pinned host memory (H2D copy in front of the replayed graph, detections written straight into pinned
                  host memory): SURVEY 8(d)'s "end to end", named FIRST in the `metric` string.  It is a top-level field and not `value`
                  because the bench contract this file is written to says so, verbatim: "`value` is whole-job throughput with inputs already
                  resident in HBM when the timed region starts (if the boundary hands over host buffers, note the PCIe-inclusive rate in
                  DESIGN.md - it is never `value`)".  `config.from_host_host_busy_us_per_step` / `..._blocked_us_per_step` say whether the
                  submit thread is the bound (it is not: ~35 us busy per 330 us step, the rest blocked on the slot's input buffer).
  secondary       SURVEY 8(d) variants measured with the same harness: letterboxed camera frames, eager launches, the f16 precision mode, and
                  the training step of configs[3].
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')   # one hardware queue per stream in flight (k210_yolo_framework_amd/__init__.py), before any HIP call
os.environ.setdefault('OMP_PROC_BIND', 'close')   # cpu_baseline: OpenMP teams bound to cores (before libgomp initialises), or the thread probe reads noise
os.environ.setdefault('OMP_PLACES', 'cores')
# the CPUs this process may use, read BEFORE any OpenMP runtime starts (with OMP_PROC_BIND libgomp pins the main thread to its first place)
AFFINITY0 = sorted(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else list(range(os.cpu_count() or 1))
import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
MFMA_PEAK_TFLOPS = 2500.0    # dense fp16/bf16 MFMA
MIN_REGION_S = 0.25


def _cpu_chain(spec, weights, anchors, build, threads, channels_last, budget_s, start_at=None):
    """One CPU worker: batches of 32 synthetic frames through normalise -> fp32 conv stack (`build`: 'port' = oracle/yolo_net_ref.c, OpenMP |
    'graph' = oracle/torch_net_ref.Prepared, torch-CPU / oneDNN) -> decode_ref boxes / scores + per-class NMS in C, on `threads` threads, for
    about `budget_s` seconds.  -> dict(images, seconds, fwd_seconds)."""
    import torch
    import oracle
    from oracle import decode_ref, torch_net_ref
    plan = spec.compile_plan(weights)
    rng = np.random.default_rng(0)
    B = 32
    if build == 'port':
        oracle.set_threads(threads)
        fwd = lambda x: oracle.net_forward(plan, x, emulate_f16=False, out_ids=spec.outputs)   # noqa: E731
    else:
        torch.set_num_threads(threads)
        fwd = torch_net_ref.Prepared(spec, weights, torch.float32, channels_last=channels_last)
    dt = min(B, threads)

    def decode(outs):
        decode_ref.decode_batch_fast([o.reshape(B, o.shape[1], o.shape[2], spec.anchor_num, -1) for o in outs], anchors, spec.in_hw, spec.in_hw,
                                     0.7, 0.5, threads=dt)
    x0 = oracle.normalise_u8(rng.integers(0, 256, (B, *spec.in_hw, 3), dtype=np.uint8))
    decode(fwd(x0))                                                   # warm: thread pools, oneDNN primitives
    if start_at is not None:                                          # workers of one measurement start together
        time.sleep(max(0.0, start_at - time.time()))
    t_total = t_fwd = 0.0
    n = 0
    while t_total < budget_s and n < 4096:
        frames = rng.integers(0, 256, (B, *spec.in_hw, 3), dtype=np.uint8)
        t0 = time.perf_counter()
        outs = fwd(oracle.normalise_u8(frames))
        t1 = time.perf_counter()
        decode(outs)
        t2 = time.perf_counter()
        t_total += t2 - t0
        t_fwd += t1 - t0
        n += B
    return {'images': n, 'seconds': t_total, 'fwd_seconds': t_fwd}


def _cpu_worker_main(cfg):
    """`python bench.py --cpu-worker JSON`: one pinned worker of the whole-host CPU baseline (a fresh process: its OpenMP / torch pools are
    created AFTER the affinity is set, so they really live on its cores)."""
    if cfg.get('cpus') and hasattr(os, 'sched_setaffinity'):
        os.sched_setaffinity(0, set(cfg['cpus']))
    from k210_yolo_framework_amd import netspec
    from k210_yolo_framework_amd.helper import VOC_ANCHORS
    spec = netspec.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    r = _cpu_chain(spec, spec.init_weights(seed=1), VOC_ANCHORS, cfg['build'], cfg['threads'], cfg.get('channels_last', True), cfg['seconds'],
                   cfg.get('start_at'))
    print(json.dumps(r))


def _numa_cpu_blocks(threads, sysfs='/sys'):
    """The host's allowed CPUs as blocks of `threads` physical cores, never straddling a NUMA node: [[cpu ids], ...] (one per worker).
    One hardware thread per core is used (the first sibling), which is what the thread probe finds best for these builds."""
    allowed = list(AFFINITY0)
    first = []
    for c in allowed:                                                 # first hardware thread of every core
        try:
            sib = open(f'{sysfs}/devices/system/cpu/cpu{c}/topology/thread_siblings_list').read().strip()
            lead = int(sib.replace('-', ',').split(',')[0])
        except (OSError, ValueError):
            lead = c
        if lead == c or lead not in allowed:
            first.append(c)
    nodes = {}
    for c in first:
        node = 0
        try:
            for d in os.listdir(f'{sysfs}/devices/system/cpu/cpu{c}'):
                if d.startswith('node') and d[4:].isdigit():
                    node = int(d[4:])
        except OSError:
            pass
        nodes.setdefault(node, []).append(c)
    blocks = []
    for node in sorted(nodes):
        cs = nodes[node]
        for i in range(0, len(cs) - threads + 1, threads):
            blocks.append(cs[i:i + threads])
    return blocks or [first[:threads] or allowed[:threads]], len(nodes), len(first)


def cpu_baseline(spec, weights, anchors, budget_s=10.0):
    """The reference's CPU path (normalise -> conv stack fp32 -> decode + per-class NMS) on THIS box's host cores - all of them.  The reference
    itself (Keras on TensorFlow 1.14) is not installable here, so two ports of the same graph are timed: oracle/yolo_net_ref.c (C restatement,
    OpenMP) and oracle/torch_net_ref.Prepared (torch-CPU / oneDNN).  (1) the thread count one worker scales to is PROBED per build (both
    stop scaling at 16 - 32 threads: a 32-frame batch of 1.5 GFLOP images is a small problem); (2) the host is then filled with independent
    workers of that size, each a fresh process pinned to its own block of physical cores inside one NUMA node, all timed over the same
    window: `value` = the sum of their rates, `cores` = the cores they really used."""
    import subprocess
    import torch
    import oracle
    from oracle import torch_net_ref
    plan = spec.compile_plan(weights)
    rng = np.random.default_rng(0)
    B = 32
    logical = os.cpu_count() or 1
    try:
        import psutil
        physical = psutil.cpu_count(logical=False) or logical
    except Exception:
        physical = logical
    avail = len(AFFINITY0)
    cands = sorted({n for n in (4, 8, 16, 32, 64) if n <= avail} | {min(avail, 8)})
    x0 = oracle.normalise_u8(rng.integers(0, 256, (B, *spec.in_hw, 3), dtype=np.uint8))
    probes, best = {}, {}
    pr = {}
    for nt in cands:                                                  # (1a) the C port's OpenMP team
        oracle.set_threads(nt)
        tb = 1e9
        for _ in range(2):
            t0 = time.perf_counter()
            oracle.net_forward(plan, x0, emulate_f16=False, out_ids=spec.outputs)
            tb = min(tb, time.perf_counter() - t0)
        pr[nt] = tb
    probes['port'] = {k: round(B / v, 1) for k, v in pr.items()}
    best['port'] = (min(pr, key=pr.get), True, B / min(pr.values()))
    pr = {}
    for cl in (True, False):                                          # (1b) torch-CPU: layout and pool size
        model = torch_net_ref.Prepared(spec, weights, torch.float32, channels_last=cl)
        for nt in cands:
            torch.set_num_threads(nt)
            model(x0[:8])
            t0 = time.perf_counter()
            model(x0)
            pr[(nt, cl)] = time.perf_counter() - t0
    probes['graph'] = {f'{k[0]}{"cl" if k[1] else ""}': round(B / v, 1) for k, v in pr.items()}
    (nt, cl) = min(pr, key=pr.get)
    best['graph'] = (nt, cl, B / pr[(nt, cl)])
    build = max(best, key=lambda k: best[k][2])                       # the faster port fills the host
    # a worker size that scales: the smallest team within 10 % of the best per-core rate... in practice the probe's best team, capped at 32
    threads = min(best[build][0], 32)
    blocks, n_nodes, n_cores = _numa_cpu_blocks(threads)
    start_at = time.time() + 20.0 + 0.5 * len(blocks)                 # import torch + warm-up of every worker happen before this instant
    procs = []
    for cpus in blocks:
        cfg = {'build': build, 'threads': threads, 'cpus': cpus, 'channels_last': best[build][1], 'seconds': budget_s, 'start_at': start_at}
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND='close', OMP_PLACES='cores')
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve()), '--cpu-worker', json.dumps(cfg)], stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, env=env))
    rows, errs = [], []
    for pz in procs:
        try:
            so, se = pz.communicate(timeout=240)
            line = [l for l in so.splitlines() if l.startswith('{')]
            if pz.returncode == 0 and line:
                rows.append(json.loads(line[-1]))
            else:
                errs.append(se[-300:])
        except Exception as e:
            pz.kill()
            errs.append(f'{type(e).__name__}: {e}')
    if not rows:
        return {'value': None, 'unit': 'images/sec', 'cores': 0, 'kind': 'port', 'error': '; '.join(errs)[:600]}
    rates = [r['images'] / r['seconds'] for r in rows]
    fwd = [r['images'] / r['fwd_seconds'] for r in rows]
    names = {'port': 'oracle/yolo_net_ref.c (a port: the Keras graph restated in C, OpenMP)',
             'graph': f'oracle/torch_net_ref.Prepared (a port: the Keras graph restated on torch-CPU / oneDNN, {"channels_last" if best["graph"][1] else "NCHW"})'}
    return {'value': round(sum(rates), 1), 'unit': 'images/sec', 'cores': threads * len(rows), 'kind': 'port', 'build': names[build],
            'workers': len(rows), 'threads_per_worker': threads, 'numa_nodes': n_nodes, 'host_physical_cores_available': n_cores,
            'host_logical_cpus': logical, 'host_physical_cores': physical, 'worker_failures': len(errs),
            'per_worker_images_per_sec': {'min': round(min(rates), 1), 'max': round(max(rates), 1)},
            'conv_stack_only_images_per_sec': round(sum(fwd), 1),
            'one_worker_probe_images_per_sec': {'port': round(best['port'][2], 1), 'torch_cpu': round(best['graph'][2], 1)},
            'sample': f'{len(rows)} independent workers x {threads} threads, each a process pinned to its own block of physical cores inside one NUMA node, '
                      f'all timed over the same {budget_s:.0f} s window ({sum(r["images"] for r in rows)} frames in batches of 32 synthetic 224x320 frames): '
                      'normalise + fp32 conv stack + decode_ref.py boxes / scores + per-class NMS in C (oracle/decode_nms_ref.c)',
            'thread_probe_images_per_sec': probes}


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def maybe_launch(args):
    """`python bench.py --gpus N` outside a launcher: become the launcher.  Returns only in a rank process."""
    if args.gpus <= 1 and 'WORLD_SIZE' not in os.environ:
        return
    if 'WORLD_SIZE' in os.environ:                                    # already a rank (driver's torch.distributed.run or our own)
        world = int(os.environ['WORLD_SIZE'])
        if args.gpus != world:
            sys.exit(f'bench.py: --gpus {args.gpus} but the launcher started {world} ranks')
        return
    if not args.stub:
        import torch
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            sys.exit(f'bench.py: {args.gpus} ranks requested, {have} device(s) visible - one rank per GPU, refusing to oversubscribe')
    import subprocess
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), str(Path(__file__).resolve())] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def stub_main(args):
    """The distributed skeleton of the bench without a GPU: gloo, a sleeping step, the same barrier / max-over-ranks / JSON contract."""
    import torch
    import torch.distributed as dist
    from k210_yolo_framework_amd import shard
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo', rank=rank, world_size=world)
    B = args.batch
    mine = shard.shard_indices(B * world, rank, world)                # image i -> rank i mod world
    step_s = 0.002 * (1 + 0.5 * rank)                                 # ranks of unequal speed: the slowest one must define the time
    for _ in range(args.warmup):
        time.sleep(step_s / 10)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(step_s)
    el = time.perf_counter() - t0
    own = B * args.steps / el                                         # this rank's own rate, before the max over ranks (the real bench reports
    per_rank = [round(own, 1)]                                        # `from_host_per_rank` the same way: SURVEY 8(e), host feeding per rank)
    if world > 1:
        dist.barrier()
        t = torch.zeros(world, dtype=torch.float64)
        t[rank] = own
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        per_rank = [round(float(v), 1) for v in t.tolist()]
        el = shard.max_over_ranks(el, dist, device='cpu')
    if rank == 0:
        print(json.dumps({'metric': 'images/sec end-to-end, yolo_mobilev1-0.75 320x240 b32 (STUB step: launcher / rendezvous check only)',
                          'from_host_per_rank': {'images_per_sec': per_rank, 'min': min(per_rank), 'max': max(per_rank)},
                          'value': round(world * B * args.steps / el, 1), 'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps,
                          'warmup': args.warmup, 'ms_per_step': round(el / args.steps * 1e3, 4), 'higher_is_better': True, 'scaling': 'weak',
                          'vs_baseline': None, 'dtype': 'none', 'data': 'stub', 'stub': True,
                          'config': {'workload': 'stub', 'batch_per_gpu': B, 'global_batch': B * world, 'images_of_rank0': len(mine),
                                     'parallelism': f'image-sharded x{world}, no collective'}}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _train_setup(B, rank, world, local):
    import torch
    from k210_yolo_framework_amd import netspec
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.train import Trainer
    spec = netspec.yolo_mobilev2((224, 320, 3), 3, 20, alpha=1.0)
    weights = spec.init_weights(seed=1)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [list(x) for x in spec.out_hw()])
    rng = np.random.default_rng(rank)
    ys = [[] for _ in spec.outputs]
    for b in range(B):
        n = int(rng.integers(1, 6))
        boxes = np.stack([rng.integers(0, 20, n), rng.uniform(.2, .8, n), rng.uniform(.2, .8, n), rng.uniform(.1, .6, n),
                          rng.uniform(.1, .6, n)], 1)
        for i, lab in enumerate(h.box_to_label(boxes)):
            ys[i].append(lab)
    y_true = [torch.from_numpy(np.stack(y).astype(np.float32)).cuda() for y in ys]
    x = torch.from_numpy(rng.uniform(0, 1, (B, 224, 320, 3)).astype(np.float32)).cuda()
    tr = Trainer(spec, weights, h.anchors, B, lr=5e-4, decay=0.0, device=local, process_group=None, world_size=world)
    return tr, x, y_true


def pipeline_rate(B, local, n_items=512):
    """the training input pipeline alone (pipeline.InputPipeline on generated 240x320 u8 frames held in memory:
    thread-pool label scatter, H2D of u8 frames, GPU letterbox + normalise, 2 batches of prefetch), drained as fast as it delivers."""
    import torch
    from k210_yolo_framework_amd import pipeline, training
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    items = training.synthetic_list(n_items, (240, 320), 20, seed=1)
    rates = []
    for ep in range(2):                                                        # first epoch warms pinned allocations
        pipe = pipeline.InputPipeline(h, items, B, 0, 1, seed=0, epoch=ep, shuffle=True, device=local)
        t0 = time.perf_counter()
        n = 0
        for x, ys in pipe:
            n += x.shape[0]
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
        pipe.close()
    return round(rates[-1], 1)


def train_main(args):
    """BASELINE configs[3]: yolo_mobilev2 alpha=1.0 VOC training step, 16 images per GPU, YOLO loss, one flat RCCL
    all-reduce of the gradients.  Not the headline metric; same timing contract (barrier + sync, max over ranks)."""
    import torch
    from k210_yolo_framework_amd import engine, shard
    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    engine.require_gpu()
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device(f'cuda:{local}'))
    B = 16 if args.batch == 32 else args.batch
    tr, x, y_true = _train_setup(B, rank, world, local)
    steps, warm = min(args.steps, 50), min(max(args.warmup, 2), 5)
    for _ in range(warm):
        last = tr.step(x, y_true)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = tr.step(x, y_true)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        elapsed = shard.max_over_ranks(elapsed, dist, device='cuda')
    pipe = None
    try:
        pipe = pipeline_rate(B, local) if rank == 0 else None
    except Exception as e:  # never take the step number down
        pipe = f'{type(e).__name__}: {e}'
    if rank == 0:
        print(json.dumps({
            'metric': 'training images/sec, yolo_mobilev2-1.0 VOC step b16/GPU', 'value': round(world * B * steps / elapsed, 1),
            'input_pipeline_images_per_sec_per_rank': pipe,
            'unit': 'images/sec', 'n_gpus': world, 'steps': steps, 'warmup': warm, 'ms_per_step': round(elapsed / steps * 1e3, 3),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': 'configs[3]: yolo_mobilev2 alpha=1.0, 224x320x3, 20-class VOC head, forward(train-mode BN) + YOLO loss '
                                   '+ backward + l2 + Adam' + (' + flat RCCL all-reduce' if world > 1 else ''),
                       'batch_per_gpu': B, 'global_batch': B * world, 'params': int(tr.n_params), 'last_loss': round(last['loss'], 4),
                       'parallelism': f'data-parallel x{world}'}}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32, help='images per GPU per step (BASELINE: 32)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without the CPU baseline')
    ap.add_argument('--no-secondary', action='store_true', help='--full without the secondary measurements (variants, f16x2 mode, training step)')
    ap.add_argument('--streams', type=int, default=4, help='independent batches in flight: step i runs on stream i %% S with its own plan, '
                    'outputs and decode scratch (consecutive steps are independent batches)')
    ap.add_argument('--letterbox', action='store_true', help='SURVEY 8(d) variant (ii) as the timed step: 240x320 camera frames, letterboxed '
                    'on the GPU (yk_letterbox_u8) to the 224x320 network tensor')
    ap.add_argument('--from-host', action='store_true', help='frames start in pinned host memory and cross PCIe inside the timed step, '
                    'detections are copied back (reported for reference; never the headline value)')
    ap.add_argument('--precision', choices=['f16', 'f16x2'], default='f16x2',
                    help="'f16x2' (default): the mode that meets BASELINE.json's 1e-3 / exact-set tolerance; 'f16': fp16 storage, 5e-3 worst case")
    ap.add_argument('--eager', action='store_true', help='launch every kernel from the host (no hipGraph replay of the step)')
    ap.add_argument('--no-numa-bind', action='store_true', help='leave the process on whatever CPUs the launcher gave it')
    ap.add_argument('--stub', action='store_true', help='no GPU: sleeping step over gloo (launcher / rendezvous self-test)')
    ap.add_argument('--cpu-worker', default=None, help=argparse.SUPPRESS)          # internal: one pinned worker of cpu_baseline (JSON config)
    ap.add_argument('--cpu-baseline-only', action='store_true', help='print the cpu_baseline object alone (no GPU needed)')
    ap.add_argument('--mode', choices=['inference', 'train'], default='inference',
                    help="'train': BASELINE configs[3] (yolo_mobilev2 1.0 training step, 16 images/GPU, RCCL gradient all-reduce)")
    ap.add_argument('--full', action='store_true', help='besides the headline: one-batch rate, per-launch profiles and roofline, from-host '
                    'rate, secondary variants, training step, CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help="write the last timed step's results to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.cpu_worker:
        return _cpu_worker_main(json.loads(args.cpu_worker))
    if args.cpu_baseline_only:
        from k210_yolo_framework_amd import netspec as _ns
        from k210_yolo_framework_amd.helper import VOC_ANCHORS as _A
        _sp = _ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
        print(json.dumps(cpu_baseline(_sp, _sp.init_weights(seed=1), _A)))
        return
    maybe_launch(args)
    if args.stub:
        return stub_main(args)
    if args.mode == 'train':
        return train_main(args)

    import torch
    from k210_yolo_framework_amd import engine, netspec
    from k210_yolo_framework_amd.helper import VOC_ANCHORS

    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    engine.require_gpu()
    torch.cuda.set_device(local)
    # the N-GPU curve bends at host feeding - this rank's submit loop, producer threads and pinned frame ring go on the NUMA
    # node its GPU hangs off, before anything pinned is allocated (shard.bind_to_gpu_numa; a no-op on a single-node host)
    from k210_yolo_framework_amd import shard as _shard
    full_affinity = set(AFFINITY0) if hasattr(os, 'sched_setaffinity') else None   # (read at import, before libgomp pinned the main thread to its first place)
    numa = {'node': -1, 'cpus': None} if args.no_numa_bind else _shard.bind_to_gpu_numa(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device(f'cuda:{local}'))

    spec = netspec.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    weights = spec.init_weights(seed=1)
    B = args.batch
    cfg = engine.make_decode_cfg(VOC_ANCHORS, 20, spec.in_hw, spec.out_hw())
    g = torch.Generator(device='cuda').manual_seed(rank)
    frames = torch.randint(0, 256, (B, 224, 320, 3), dtype=torch.uint8, device='cuda', generator=g)
    cam = torch.randint(0, 256, (B, 240, 320, 3), dtype=torch.uint8, device='cuda', generator=g)

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    class Harness:
        """S batches in flight through the product API (engine.Pipeline): one step = (optional H2D) -> (optional letterbox) -> yk_run_u8 ->
        yk_decode_py -> (from host: detections written to pinned host memory at their live size).  graph=True: each slot's step is a
        captured hipGraph, one host call per batch."""

        def __init__(self, S, precision, letterbox=False, from_host=False, graph=True):
            self.S, self.letterbox, self.from_host = max(1, S), letterbox, from_host
            self.pipe = engine.Pipeline(spec, weights, VOC_ANCHORS, max_batch=B, depth=self.S, device=local, precision=precision,
                                        graph=graph, src_hw=(240, 320) if letterbox else None)
            self.plans = self.pipe.plans
            self.src = cam if letterbox else frames
            self.host_s = 0.0
            if from_host:
                h = self.src.cpu()
                for i in range(self.S):
                    self.pipe.host_input(i).copy_(h)              # the frames of every slot wait in pinned host memory

        def step(self):
            self.last_slot = self.pipe.next_slot()
            if self.from_host:
                # every slot's frames wait in pinned memory: the copy of the NEXT submit's batch is started before this one is launched
                # (Pipeline.stage_host: what a producer thread does when it has filled a slot) - each batch still crosses PCIe inside the timed region
                self.pipe.stage_host(self.pipe.next_slot() + 1)
                self.last = self.pipe.submit_host(None)
            else:
                self.last = self.pipe.submit(self.src, sync_input=False)   # resident frames: nothing to order them behind
            return self.last

        def dump(self, d):
            """The last step's results as its caller receives them (+ the network outputs they were decoded from) -> d/<name>.npy, float32."""
            d.mkdir(parents=True, exist_ok=True)
            torch.cuda.synchronize()
            if self.from_host:
                rows, off = self.last.result()
                arrs = {'detections': rows, 'detection_offsets': off}
            else:
                dets, counts = self.last[0].cpu().numpy().copy(), self.last[1].cpu().numpy()
                for b, n in enumerate(counts):
                    dets[b, n:] = 0.0                             # rows past an image's count are scratch, not results
                arrs = {'detections': dets, 'detection_counts': counts}
            for o in self.pipe.outs[self.last_slot]:
                arrs[f'network_output_{o.shape[1]}x{o.shape[2]}'] = o[:B].cpu().numpy()
            for k, v in arrs.items():
                np.save(d / f'{k}.npy', np.ascontiguousarray(v, dtype=np.float32))

        def measure(self, steps, warmup, min_s=MIN_REGION_S, max_regions=64):
            for _ in range(max(warmup, 3)):
                self.step()
            sync_all()
            times, host, local_times = [], [], []
            waits = []
            while True:
                sync_all()
                w0 = self.pipe.host_wait_us
                t0 = time.perf_counter()
                for _ in range(steps):
                    self.step()
                t1 = time.perf_counter()
                waits.append((self.pipe.host_wait_us - w0) / steps)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                local_times.append(el)
                if dist is not None:
                    from k210_yolo_framework_amd import shard
                    dist.barrier()
                    el = shard.max_over_ranks(el, dist, device='cuda')
                times.append(el)
                host.append((t1 - t0) / steps)
                if sum(times) >= min_s or len(times) >= max_regions:
                    break
            self.host_s = statistics.median(host)                 # host time to SUBMIT one step (the GPU runs behind it)
            self.host_wait_us = statistics.median(waits)          # ... of which BLOCKED on a slot's input buffer (from-host path)
            self.local_s = statistics.median(local_times)         # this rank's own time for the region (before the max over ranks)
            return statistics.median(times), len(times)

        def close(self):
            torch.cuda.synchronize()
            self.pipe.close()

    S = max(1, args.streams)
    use_graph = not args.eager
    head = Harness(S, args.precision, letterbox=args.letterbox, from_host=args.from_host, graph=use_graph)
    elapsed, regions = head.measure(args.steps, args.warmup, max_regions=1)
    ms_per_step = elapsed / args.steps * 1e3
    value = world * B * args.steps / elapsed
    host_us = head.host_s * 1e6
    graph_nodes = max((g.nodes for sl in head.pipe.slots for g in sl.graphs.values()), default=0)
    if args.dump_outputs and rank == 0:
        head.dump(Path(args.dump_outputs))
    inflight = f'{S} batches in flight' if S > 1 else 'one batch in flight'
    out = {
        'metric': f'images/sec end-to-end, yolo_mobilev1-0.75 320x240 b32 (`value_from_host`: SURVEY 8(d) end to end - u8 frames in pinned host '
                  f'memory -> H2D -> normalise -> backbone + heads -> decode -> NMS -> detections in host memory; `value`: the same step with the '
                  f'frames already resident in HBM, which is what the bench contract fixes `value` to be; {inflight})',
        'value': round(value, 1), 'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': round(ms_per_step, 4), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f16 storage / f32 accumulate' if args.precision == 'f16' else 'f16x2 (compensated fp16 MFMA operands: x = hi + lo, fp32 accumulate)',
        'data': 'synthetic u8 frames resident in HBM, seeded random-init weights',
        'timed_regions': regions,
        'full': args.full,
        'config': {'workload': 'configs[1]: yolo_mobilev1 alpha=0.75, network tensor 224x320x3 (320x240 frame, SURVEY F1), '
                               f'20-class VOC head, u8 normalise + backbone/head + python-mode decode + per-class NMS; {inflight} '
                               '(independent batches on separate HIP streams, one plan each)',
                   'batch_per_gpu': B, 'global_batch': B * world,
                   'launch_mode': 'graph' if use_graph else 'eager', 'graph_nodes_per_step': graph_nodes,
                   'streams': 'created by the library back to back (yk_stream_create): one hardware queue each; more than four lose (4 compute pipes)',
                   'schedule': getattr(head.pipe, 'schedule', None),
                   'host_us_per_step': round(host_us, 1), 'batches_in_flight': S, 'precision': args.precision,
                   'tolerance_carried': ('BASELINE north_star: identical detection sets, scores / coords within 1e-3 max '
                                         '(tests/test_gpu_e2e.py::test_north_star_*)' if args.precision == 'f16x2' else
                                         'fp16-storage budget: scores within 5e-3 max, >= 97 % of detections reproduced (tests/test_gpu_e2e.py)'),
                   'frames': ('240x320 letterboxed on GPU' if args.letterbox else '224x320 native') +
                             (', from pinned host memory, detections copied back' if args.from_host else ', resident in HBM'),
                   'parallelism': f'image-sharded x{world}, no collective'},
    }
    if not args.full:                                                # a plain run: the headline and nothing else
        head.close()
        if rank == 0:
            print(json.dumps(out))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    single = Harness(1, args.precision, letterbox=args.letterbox, from_host=args.from_host, graph=use_graph)
    el1, _ = single.measure(min(args.steps, 100), 5)
    single_ms = el1 / min(args.steps, 100) * 1e3
    # per-launch times of both plans while they are alive (rank 0)
    prof = None
    if rank == 0:
        p_head, p_lat = head.plans[0], single.plans[0]
        ms_head = p_head.profile(frames, iters=20)
        prof = (ms_head, p_head.launches(), p_lat.profile(frames, iters=20) if p_lat is not p_head else ms_head, p_lat.launches(),
                getattr(head.pipe, 'schedule', None), getattr(single.pipe, 'schedule', None))
    single.close()
    # SURVEY 8(d) "end to end" with the PCIe legs: the same step fed from pinned host memory (H2D copy in front of the captured step), detections
    # delivered to pinned host memory; every rank takes part (8(e): host feeding is where the N-GPU curve is expected to bend).  Measured on
    # the SAME pipeline (same plans, same streams) as `value`: a serving process has one pipeline, and a pipeline created later in this
    # process - on streams the runtime handed out later - feeds 10 % slower (66-70 k images/s in a fresh harness, 71-72 k in a second and
    # third one, 76 k on this one; profiles/r04_schedules.txt)
    value_from_host, fh_host_us, per_rank_fh, fh_wait_us = None, None, None, None
    if not args.from_host and not args.no_secondary:
        ok, err = 1, ''
        try:
            h_ = head.src.cpu()
            for i in range(head.S):
                head.pipe.host_input(i).copy_(h_)                    # the frames of every slot wait in pinned host memory
            head.from_host = True
        except Exception as e:
            ok, err = 0, f'{type(e).__name__}: {e}'
        if dist is not None:                                         # agree before entering the timed region's barrier
            t = torch.tensor([ok], device='cuda')
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            ok = int(t.item())
        if ok:
            el_fh, _ = head.measure(min(args.steps, 100), 10)
            value_from_host = world * B * min(args.steps, 100) / el_fh
            fh_host_us = head.host_s * 1e6
            fh_wait_us = head.host_wait_us
            mine = B * min(args.steps, 100) / head.local_s                       # this rank's own from-host rate
            if dist is not None:
                t = torch.zeros(world, dtype=torch.float64, device='cuda')
                t[rank] = mine
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                per_rank_fh = [round(float(v), 1) for v in t.cpu().tolist()]
            else:
                per_rank_fh = [round(mine, 1)]
        elif rank == 0:
            print(f'bench.py: from-host steps failed on some rank: {err}', file=sys.stderr)
        head.from_host = False
    head.close()

    if rank == 0:
        # ---- roofline of the dominant kernel, HIP events on the launch stream.  Algorithmic bytes are SURVEY 8(d)'s (every layer's
        # input + output once at fp16), whatever the mode stores: the f16x2 plan reports its bytes at 4 B per element, so its
        # launches are halved to that basis (the mode really moves twice as much: `traffic` / `traffic_GBps_frac_of_hbm_peak` are the counters' word on that)
        # The plan that produces `value` (S batches in flight: engine.Pipeline picks the launch-per-layer schedule for depth >= 2); the plan of
        # the one-batch measurement (depth 1: the two cluster launches, YK_SCHEDULE_LATENCY) is listed beside it in config.latency_schedule.
        ms, launches, lat_ms, lat_launches, sched_head, sched_lat = prof
        basis = 0.5 if args.precision == 'f16x2' else 1.0
        tags = ('r06_x2', 'r05_x2', 'r04_x2', 'r03_x2', 'r02') if args.precision == 'f16x2' else ('r03', 'r02', 'r01')

        def launch_roofline(k):
            """One launch against the bound that limits it: algorithmic bytes / flops over its HIP-event time; `traffic` = its HBM
            bytes from the committed counter passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate runs, tools/one_step.py +
            tools/profiles_post.py; counters cannot be collected from inside this process)."""
            name_, flops_img, bytes_img = launches[k]
            alg_bytes_ = bytes_img * B * basis
            alg_flops = flops_img * B
            t_k = float(ms[k]) * 1e-3
            if (alg_bytes_ / (HBM_PEAK_GBS * 1e9)) >= (alg_flops / (MFMA_PEAK_TFLOPS * 1e12)):
                ach = alg_bytes_ / t_k / 1e9
                r = {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': round(ach / HBM_PEAK_GBS, 4), 'traffic': None}
            else:
                ach = alg_flops / t_k / 1e12
                r = {'bound': 'mfma', 'achieved': round(ach, 1), 'peak': MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(ach / MFMA_PEAK_TFLOPS, 4),
                     'traffic': None}
            for tag in tags:
                try:
                    tp = json.load(open(ROOT / 'profiles' / f'{tag}_hbm_traffic.json'))
                    if f'{k}:{name_}' in tp:
                        r['traffic'] = tp[f'{k}:{name_}']
                        r['traffic_source'] = f'profiles/{tag}_hbm_traffic.json'
                        # what the launch really moves through the memory side, against the HBM peak (the counter bytes, not a model of them)
                        r['traffic_GBps_frac_of_hbm_peak'] = round(r['traffic'] / t_k / 1e9 / HBM_PEAK_GBS, 4)
                        break
                except Exception:
                    pass
            r.update({'kernel': name_, 'avg_us': round(float(ms[k]) * 1e3, 2), 'algorithmic_bytes_per_launch': int(alg_bytes_)})
            return r

        dom = int(np.argmax(ms))                                     # the dominant kernel = the launch the step spends the most time in
        roof = launch_roofline(dom)
        # the fused stem block was the longest launch through round 4 (0.34); round 5 took 16 % off it and the 3x3 head conv is now
        # longer - its line stays in the record beside the dominant one
        stem_k = [k for k, l in enumerate(launches) if 'stem' in l[0]]
        if stem_k and stem_k[0] != dom:
            roof['stem_block'] = launch_roofline(stem_k[0])
        # every launch against its own bound, and the time-weighted step fraction per kernel family: the largest launch alone hides
        # where the step really spends its time
        def families(launches_, ms_):
            fam_, t_sum = {}, 0.0
            for i, (nm, fl, by) in enumerate(launches_):
                t_roof = max(by * B * basis / (HBM_PEAK_GBS * 1e9), fl * B / (MFMA_PEAK_TFLOPS * 1e12)) * 1e6
                key = ('late backbone (cluster launch)' if nm.startswith('x:persist') else 'heads (cluster launch)' if nm.startswith('x:heads') else
                       'stem' if 'stem' in nm else 'u8_max' if 'u8_max' in nm else 'dw+pw block' if ('dw3x3' in nm and 'conv1x1' in nm) else
                       'depthwise' if 'dw3x3' in nm else 'conv3x3' if 'conv3x3' in nm else 'split-K finish' if 'splitk_reduce' in nm else 'conv1x1')
                f = fam_.setdefault(key, [0.0, 0.0, 0])
                f[0] += float(ms_[i]) * 1e3
                f[1] += t_roof
                f[2] += 1
                t_sum += t_roof
            return ({k: {'launches': v[2], 'us': round(v[0], 1), 'roofline_us': round(v[1], 1), 'frac': round(v[1] / v[0], 3)}
                     for k, v in sorted(fam_.items(), key=lambda kv: -kv[1][0])}, t_sum)
        fam, t_roof_sum = families(launches, ms)
        lat_fam, lat_roof_sum = families(lat_launches, lat_ms)
        roof.update({'sum_kernels_us': round(float(ms.sum()) * 1e3, 1),
                     'step_frac_time_weighted': round(t_roof_sum / (float(ms.sum()) * 1e3), 4),
                     'families': fam,
                     'per_kernel_us': {f'{i}:{launches[i][0]}': round(float(ms[i]) * 1e3, 2) for i in range(len(ms))}})
        alg_gb = spec.act_elems_per_image() * 2 * B / 1e9                     # in + out of every conv layer once, fp16
        alg_gflop = 2.0 * spec.macs_per_image() * B / 1e9
        roof_step_us = alg_gb / HBM_PEAK_GBS * 1e6                            # the whole step is HBM-bound under this model
        out.update({
            'value_from_host': None if value_from_host is None else round(value_from_host, 1),
            'from_host_frac_of_value': None if value_from_host is None else round(value_from_host / value, 3),
            'from_host_h2d_GBps': None if value_from_host is None else round(value_from_host / world * 224 * 320 * 3 / 1e9, 2),
            'from_host_per_rank': None if per_rank_fh is None else {'images_per_sec': per_rank_fh, 'min': min(per_rank_fh), 'max': max(per_rank_fh)},
            'host_placement': {'numa_node_of_gpu': numa.get('node'), 'cpus_bound': numa.get('cpus'), 'pci': numa.get('pci')},
            'roofline': roof,
        })
        out['config'].update({
                       'launches_per_step': len(launches) + 3,
                       'schedule': sched_head,
                       'latency_schedule': {'what': 'the plan of one_batch_in_flight_*: engine.Pipeline(depth=1) -> YK_SCHEDULE_LATENCY (late backbone and heads as '
                                                    'two launches of per-image workgroup clusters)',
                                            'schedule': sched_lat, 'launches_per_step': len(lat_launches) + 3,
                                            'sum_kernels_us': round(float(lat_ms.sum()) * 1e3, 1),
                                            'step_frac_time_weighted': round(lat_roof_sum / (float(lat_ms.sum()) * 1e3), 4), 'families': lat_fam,
                                            'per_kernel_us': {f'{i}:{lat_launches[i][0][:72]}': round(float(lat_ms[i]) * 1e3, 2) for i in range(len(lat_ms))}},
                       'from_host_host_us_per_step': None if fh_host_us is None else round(fh_host_us, 1),
                       'from_host_host_blocked_us_per_step': None if fh_wait_us is None else round(fh_wait_us, 1),
                       'from_host_host_busy_us_per_step': None if fh_wait_us is None else round(fh_host_us - fh_wait_us, 1),
                       'one_batch_in_flight_ms_per_step': round(single_ms, 4),
                       'one_batch_in_flight_images_per_sec': round(world * B / (single_ms * 1e-3), 1),
                       'algorithmic_GB_per_step': round(alg_gb, 4), 'algorithmic_GFLOP_per_step': round(alg_gflop, 2),
                       'step_roofline_us': round(roof_step_us, 1),
                       'step_frac_of_roofline': round(roof_step_us / (ms_per_step * 1e3), 4),
                       'one_batch_step_frac_of_roofline': round(roof_step_us / (single_ms * 1e3), 4)})

    def rate(S_, prec, lb, fh, steps=60, graph=None):
        hs = Harness(S_, prec, letterbox=lb, from_host=fh, graph=use_graph if graph is None else graph)
        el, _ = hs.measure(steps, 30, min_s=0.25, max_regions=16)
        hs.close()
        return round(B * steps / el, 1)

    if not args.no_secondary:
        sec = {}
        try:
            sec['from_host_note'] = ('value_from_host: pinned host u8 frames -> H2D copy in front of the captured step -> run -> decode -> detections '
                                     'written by the compaction kernel into pinned host memory at their live size (no D2H copy); whole job over all ranks')
            if world == 1:                                             # single-process extras: never inside a multi-rank barrier
                sec['eager_images_per_sec'] = rate(S, args.precision, False, False, graph=False)
                sec['eager_from_host_images_per_sec'] = rate(S, args.precision, False, True, graph=False)
                sec['letterbox_images_per_sec'] = rate(S, args.precision, True, False)
                sec['from_host_letterbox_images_per_sec'] = rate(S, args.precision, True, True)
                other = 'f16x2' if args.precision == 'f16' else 'f16'
                sec[f'{other}_images_per_sec'] = rate(S, other, False, False, steps=30)
                sec[f'{other}_one_batch_images_per_sec'] = rate(1, other, False, False, steps=30)
                sec[f'{other}_tolerance'] = ('identical detection sets, 1e-3 max' if other == 'f16x2' else
                                             'scores within 5e-3 max, >= 97 % of detections reproduced')
        except Exception as e:  # secondary numbers must never take the headline line down
            sec['error'] = f'{type(e).__name__}: {e}'
        if rank == 0 and world == 1:
            try:
                tr, x, y_true = _train_setup(16, 0, 1, local)
                for _ in range(3):
                    tr.step(x, y_true)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    tr.step(x, y_true)
                torch.cuda.synchronize()
                tms = (time.perf_counter() - t0) / 10 * 1e3
                sec['train'] = {'workload': 'configs[3]: yolo_mobilev2-1.0 224x320 training step, 16 images, fp32', 'ms_per_step': round(tms, 3),
                                'images_per_sec': round(16 / tms * 1e3, 1)}
                del tr
                sec['train']['input_pipeline_images_per_sec'] = pipeline_rate(16, local)
            except Exception as e:
                sec['train'] = {'error': f'{type(e).__name__}: {e}'}
        if rank == 0:
            out['secondary'] = sec
    if rank == 0:
        if not args.no_cpu_baseline and world == 1:
            # a FRESH process with the launcher's affinity (sched_setaffinity here would only widen this thread, not the OpenMP /
            # torch pools that already exist): it probes the worker size and fills the host with pinned workers
            import subprocess
            try:
                r = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--cpu-baseline-only'], capture_output=True, text=True, timeout=600,
                                   preexec_fn=(lambda: os.sched_setaffinity(0, full_affinity)) if full_affinity is not None else None)
                rows = [l for l in r.stdout.splitlines() if l.startswith('{')]
                out['cpu_baseline'] = json.loads(rows[-1]) if rows else {'value': None, 'kind': 'port', 'error': r.stderr[-400:]}
            except Exception as e:
                out['cpu_baseline'] = {'value': None, 'kind': 'port', 'error': f'{type(e).__name__}: {e}'}
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

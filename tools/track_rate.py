#!/usr/bin/env python3
"""What tracking costs -> profiles/track_rate.txt.

  (i)   one engine.TrackState.update call, device events around it, beside track.Tracker on the host for the same rows: 32 frames of one
        sequence at 10 and at 200 live tracks, and 8 sequences of 4 frames.  Device and host take turns in every round, after warm-up rounds
        of both.
  (ii)  detect.run pictures/s on generated frames of moving rectangles (JPEG files in a folder, seeded random weights), track off and on;
  (iii) the same off run by the package of a second tree - a checkout of the parent commit, built, given with --parent.  Off has to agree
        with it within the spread of the repeats: the acceptance condition on speed;
  (iv)  on against off, recorded and not judged;
  (v)   the call of (i) under --track_assign: greedy and lap by the parent commit's tree, greedy and lap by this tree, fresh processes in
        turns.  The two greedy rows have to agree within the spread of their own repeats, and so have the two lap rows; lap against greedy
        is recorded and not judged.  --only_assign measures (v) alone and replaces it in --out.
(ii) - (iv): every measurement is a fresh child process of this file (--child) that imports the package of ONE tree, runs a warm-up and then
--runs timed runs; the kinds (off, parent off, on) take turns, --rounds times, so each has rounds * runs repeats taken in one session.
Medians and the spread (min .. max) of the repeats.  Needs an MI355X; there is no CPU path.

    python tools/track_rate.py --parent ../parent_checkout [--out profiles/track_rate.txt] [--repeats 9] [--frames 96] [--rounds 4] [--runs 3]"""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
F = np.float32
CHILD_LIMIT = 240                        # seconds one child may take: torch's import, a warm-up and a few runs of under a second


def moving_rows(n_boxes: int, frames: int, seed: int):
    """frames x [n_boxes, 6]: boxes on a grid wide enough that they stay apart, each drifting its own way."""
    rng = np.random.default_rng(seed)
    top, left = 70.0 * (np.arange(n_boxes) // 20), 70.0 * (np.arange(n_boxes) % 20)
    vel = rng.uniform(-1.5, 1.5, (n_boxes, 2))
    score, cls = rng.uniform(0.65, 0.99, n_boxes), rng.integers(0, 20, n_boxes)
    return [np.stack([top + vel[:, 0] * t, left + vel[:, 1] * t, top + vel[:, 0] * t + 50, left + vel[:, 1] * t + 40, score, cls], 1).astype(F)
            for t in range(frames)]


def spread(v):
    v = np.asarray(v, np.float64)
    return f'median {np.median(v):.4g} (min {v.min():.4g} .. max {v.max():.4g}, {len(v)} repeats)'


def case_rows():
    return {'1 sequence x 32 frames, 10 tracks': [moving_rows(10, 32, 1)], '1 sequence x 32 frames, 200 tracks': [moving_rows(200, 32, 2)],
            '8 sequences x 4 frames, 50 tracks each': [moving_rows(50, 4, 10 + s) for s in range(8)]}


def assign_child(tree: str, assign: str, repeats: int):
    """One process, one tree's package: the cases of (i) under `assign`, three warm-up calls and `repeats` timed ones each -> a JSON line of
    ms per call."""
    sys.path.insert(0, tree)
    import torch
    from k210_yolo_framework_amd import engine
    assert Path(engine.__file__).resolve().is_relative_to(Path(tree).resolve()), engine.__file__
    times = {}
    for name, seqs in case_rows().items():
        frames = [f for s in seqs for f in s]
        dets, counts = np.zeros((len(frames), 600, 6), F), np.asarray([len(f) for f in frames], np.int32)
        for i, f in enumerate(frames):
            dets[i, :len(f)] = f
        state = engine.TrackState(len(seqs), 20, **({} if assign == 'greedy' else {'assign': assign}))
        first = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)).cuda()
        d, c = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
        out = state.update(d, c, first)
        times[name] = []
        for rep in range(3 + repeats):
            state.reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            state.update(d, c, first, out=out)
            b.record()
            b.synchronize()
            if rep >= 3:
                times[name].append(a.elapsed_time(b))
    print('TIMES ' + json.dumps(times))


def assign_rates(parent: str, rounds: int, repeats: int, lines):
    """(v): one yk_track_update call under greedy and under lap, each by the parent commit's tree and by this tree, fresh processes in
    turns.  -> do the two rows of either kind agree within the spread of their own repeats, in every case"""
    kinds = {f'{assign}{who}': (tree, assign) for assign in ('greedy', 'lap')
             for who, tree in ((', parent commit', str(Path(parent).resolve())), ('', str(ROOT)))}
    times = {k: {name: [] for name in case_rows()} for k in kinds}
    for _ in range(rounds):
        for kind, (tree, assign) in kinds.items():
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--assign-child', tree, assign, str(repeats)], capture_output=True,
                               text=True, timeout=CHILD_LIMIT, cwd=tree)
            if r.returncode != 0:                                       # nothing more is started after a child that failed
                raise SystemExit(f'track_rate: the {kind} child ended with {r.returncode}:\n{r.stderr[-2000:]}')
            for name, ms in json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('TIMES ')][-1][6:]).items():
                times[kind][name] += ms
    lines.append(f'(v) yk_track_update, ms per call by --track_assign: {rounds} rounds of fresh processes in turns ({", ".join(kinds)}), '
                 f'3 warm-up calls and {repeats} timed ones each')
    agree = True
    for name in case_rows():
        lines.append(f'    {name}')
        lines += [f'      {kind + ":":24s}{spread(times[kind][name])}' for kind in kinds]
        for assign in ('greedy', 'lap'):
            old, new = times[f'{assign}, parent commit'][name], times[assign][name]
            inside = min(old) <= np.median(new) <= max(old) and min(new) <= np.median(old) <= max(new)
            agree &= bool(inside)
            lines.append(f'      {assign} / parent = {np.median(new) / np.median(old):.3f}; each median lies {"INSIDE" if inside else "OUTSIDE"} the other\'s min .. max')
        lines.append(f'      lap / greedy = {np.median(times["lap"][name]) / np.median(times["greedy"][name]):.2f} (recorded, not judged)')
    lines.append('    not measured: the solver\'s worst case (a stage of one class in which every augmentation walks every row: rows x rows x '
                 'columns / 64 lane steps); these rows have twenty classes and boxes that stay apart')
    return agree


def kernel_cases(repeats: int, lines):
    import torch
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd import track as tk
    cases = case_rows()
    prepared = {}
    for name, seqs in cases.items():
        cap = 600
        frames = [f for s in seqs for f in s]
        dets, counts = np.zeros((len(frames), cap, 6), F), np.asarray([len(f) for f in frames], np.int32)
        for i, f in enumerate(frames):
            dets[i, :len(f)] = f
        state = engine.TrackState(len(seqs), 20)
        first = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)).cuda()
        d, c = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
        out = state.update(d, c, first)
        prepared[name] = (state, d, c, first, out, [], [])
    for rep in range(3 + repeats):                                      # three warm-up rounds of both sides, then device and host in turns
        for name, (state, d, c, first, out, ms, host_ms) in prepared.items():
            state.reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            state.update(d, c, first, out=out)
            b.record()
            b.synchronize()
            t0 = time.perf_counter()
            for s in cases[name]:
                t = tk.Tracker(20, max_tracks=256)
                for f in s:
                    t.update(f, cap=600)
            t1 = time.perf_counter()
            if rep >= 3:
                ms.append(a.elapsed_time(b))
                host_ms.append((t1 - t0) * 1e3)
    for name in cases:
        live = prepared[name][0].read()[0].tolist()
        lines.append(f'(i) {name}: live tracks at the end {live}')
        lines.append(f'      yk_track_update, ms per call: {spread(prepared[name][5])}')
        lines.append(f'      track.Tracker on the host (numpy), ms: {spread(prepared[name][6])}')


# seeded random weights saturate (several hundred rows a frame above 0.5): high thresholds, the largest track_max
ON = dict(track=True, track_thresh=0.85, track_low=0.5, track_buffer=2, track_max=1024)


def write_frames(src: Path, n_frames: int):
    from PIL import Image
    src.mkdir()
    for t in range(n_frames):
        p = np.full((240, 320, 3), 40, np.uint8)
        p[40:120, (10 + 2 * t) % 260:(10 + 2 * t) % 260 + 50] = (220, 60, 60)
        p[130:220, (250 - 2 * t) % 260:(250 - 2 * t) % 260 + 60] = (60, 200, 240)
        Image.fromarray(p).save(src / f'{t:05d}.jpg', quality=90)


def child(tree: str, src: str, out_dir: str, on: bool, runs: int):
    """One process, one tree's package: a warm-up run, then `runs` timed ones -> a JSON line of pictures/s."""
    sys.path.insert(0, tree)
    from k210_yolo_framework_amd import detect
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.yolonet import MODEL_DEFS
    assert Path(detect.__file__).resolve().is_relative_to(Path(tree).resolve()), detect.__file__
    h = Helper(None, 20, VOC_ANCHORS, np.array([[224, 320]]), np.array([[7, 10], [14, 20]]))
    model, _ = MODEL_DEFS['yolo_mobilev1']([224, 320, 3], 3, 20, alpha=0.75, precision='f16x2')
    paths = detect.expand_sources(src)
    rates = []
    for rep in range(1 + runs):
        t0 = time.perf_counter()
        detect.run(h, model, paths, out_dir=out_dir, draw=True, batch=32, depth=4, obj_thresh=0.5, verbose=False, **(ON if on else {}))
        if rep:
            rates.append(len(paths) / (time.perf_counter() - t0))
    print('RATES ' + json.dumps(rates))


def detect_rates(parent: str, n_frames: int, rounds: int, runs: int, lines):
    kinds = {'off': (str(ROOT), False), 'parent off': (str(Path(parent).resolve()), False), 'on': (str(ROOT), True)}
    rates = {k: [] for k in kinds}
    with tempfile.TemporaryDirectory() as tmp:
        write_frames(Path(tmp) / 'frames', n_frames)
        for _ in range(rounds):
            for kind, (tree, on) in kinds.items():
                r = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--child', tree, str(Path(tmp) / 'frames'), str(Path(tmp) / 'out'),
                                    str(int(on)), str(runs)], capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=tree)
                if r.returncode != 0:                                   # nothing more is started after a child that failed
                    raise SystemExit(f'track_rate: the {kind} child ended with {r.returncode}:\n{r.stderr[-2000:]}')
                rates[kind] += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RATES ')][-1][6:])
    med = {k: float(np.median(v)) for k, v in rates.items()}
    lines.append(f'(ii) detect.run, {n_frames} frames 240 x 320, yolo_mobilev1 0.75 with seeded random weights, draw and PIL encode, batch 32, depth 4;')
    lines.append(f'      {rounds} rounds of fresh processes in turns (off, parent off, on), {runs} timed runs each after a warm-up run')
    lines.append(f'      track off, pictures/s: {spread(rates["off"])}')
    lines.append(f'      track on,  pictures/s: {spread(rates["on"])}')
    lines.append(f'(iii) the parent commit, track off, pictures/s: {spread(rates["parent off"])}')
    lo, hi = min(rates['parent off']), max(rates['parent off'])
    inside = lo <= med['off'] <= hi and min(rates['off']) <= med['parent off'] <= max(rates['off'])
    lines.append(f'      off / parent = {med["off"] / med["parent off"]:.3f}; each median lies {"INSIDE" if inside else "OUTSIDE"} the other\'s min .. max: off '
                 f'{"agrees" if inside else "DOES NOT agree"} with the parent within the spread of the repeats')
    lines.append(f'(iv) on / off = {med["on"] / med["off"]:.2f} (recorded, not judged.  Not like for like: on, the tracker runs when a batch is drained, so '
                 f'the draw and the copies back no longer overlap the next batch; but on draws and copies only the tracked rows, and these '
                 f'weights give several hundred rows a frame of which few are tracked)')
    return inside


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        return child(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] == '1', int(sys.argv[6]))
    if len(sys.argv) > 1 and sys.argv[1] == '--assign-child':
        return assign_child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    sys.path.insert(0, str(ROOT))
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--parent', type=str, required=True, help='a built checkout of the parent commit: its track-off detect.run is measured beside this tree\'s')
    p.add_argument('--out', type=str, default=str(ROOT / 'profiles' / 'track_rate.txt'))
    p.add_argument('--repeats', type=int, default=9, help='timed rounds of (i)')
    p.add_argument('--frames', type=int, default=96)
    p.add_argument('--rounds', type=int, default=4)
    p.add_argument('--runs', type=int, default=3)
    p.add_argument('--only_assign', action='store_true', help='measure (v) alone and replace it in --out, whose other lines stay')
    a = p.parse_args()
    if not (Path(a.parent) / 'k210_yolo_framework_amd' / 'csrc' / 'libyolo_hip.so').exists():
        p.error(f'--parent {a.parent}: no built k210_yolo_framework_amd/csrc/libyolo_hip.so there')
    if a.only_assign:
        kept = Path(a.out).read_text().splitlines() if Path(a.out).exists() else []
        lines = kept[:next((i for i, ln in enumerate(kept) if ln.startswith('(v) ')), len(kept))]
        agrees = assign_rates(a.parent, a.rounds, a.repeats, lines)
        Path(a.out).write_text('\n'.join(lines) + '\n')
        print('\n'.join(lines))
        return 0 if agrees else 1
    lines = ['tools/track_rate.py: tracking (DESIGN.md 3.27); times from device events, rates from a host clock around runs that end synchronised']
    agrees = detect_rates(a.parent, a.frames, a.rounds, a.runs, lines)   # first: the children run before this process opens the GPU
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    kernel_cases(a.repeats, lines)
    lines.append('not measured: tracking quality (MOTA, IDF1) - no annotated sequences; PRECISION=kpu with TRACK=True (it shares the padded-row path)')
    agrees &= assign_rates(a.parent, a.rounds, a.repeats, lines)         # last: the section --only_assign replaces
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 0 if agrees else 1


if __name__ == '__main__':
    sys.exit(main())

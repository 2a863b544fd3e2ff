#!/usr/bin/env python3
"""What camera-motion compensation costs -> profiles/gmc_rate.txt.

  (i)   detect.run pictures/s with track=True on generated 1280 x 720 frames of a panning camera (JPEG files in a folder, seeded random
        weights), gmc off and on;
  (ii)  the same off run by the package of a second tree - a checkout of the parent commit, built, given with --parent.  Off has to agree
        with it within the spread of the repeats: the acceptance condition on speed;
  (iii) on against off, recorded and not judged;
  (iv)  one engine.gmc_motion call on 32 such frames, device events around it (the three launches together).
(i) - (iii): every measurement is a fresh child process of this file (--child) that imports the package of ONE tree, runs a warm-up and then
--runs timed runs; the kinds (off, parent off, on) take turns, --rounds times.  Medians and the spread (min .. max) of the repeats.  Needs an
MI355X; there is no CPU path.

    python tools/gmc_rate.py --parent ../parent_checkout [--out profiles/gmc_rate.txt] [--frames 64] [--rounds 6] [--runs 2]"""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CHILD_LIMIT = 240
TRACK = dict(track=True, track_thresh=0.85, track_low=0.5, track_buffer=2, track_max=1024)       # as tools/track_rate.py, for saturated weights


def spread(v):
    v = np.asarray(v, np.float64)
    return f'median {np.median(v):.4g} (min {v.min():.4g} .. max {v.max():.4g}, {len(v)} repeats)'


def frames_of(n: int):
    """n views of 720 x 1280 of one smooth seeded canvas, the window moving 12 px a frame to and fro."""
    from PIL import Image
    rng = np.random.default_rng(3)
    canvas = np.asarray(Image.fromarray(rng.integers(0, 256, (100, 180, 3), dtype=np.uint8)).resize((1440, 800), Image.BICUBIC))
    return [np.ascontiguousarray(canvas[40:760, (x := 12 * min(t % 12, 12 - t % 12)):x + 1280]) for t in range(n)]


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
        detect.run(h, model, paths, out_dir=out_dir, draw=True, batch=32, depth=4, obj_thresh=0.5, verbose=False, **TRACK, **({'gmc': True} if on else {}))
        if rep:
            rates.append(len(paths) / (time.perf_counter() - t0))
    print('RATES ' + json.dumps(rates))


def detect_rates(parent: str, src: Path, out_dir: Path, n_frames: int, rounds: int, runs: int, lines):
    kinds = {'off': (str(ROOT), False), 'parent off': (str(Path(parent).resolve()), False), 'on': (str(ROOT), True)}
    rates = {k: [] for k in kinds}
    for r_ in range(rounds):                                            # the kinds take turns, and the turn that goes first rotates
        for kind, (tree, on) in (list(kinds.items()) * 2)[r_ % 3:r_ % 3 + 3]:
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--child', tree, str(src), str(out_dir), str(int(on)), str(runs)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=tree)
            if r.returncode != 0:                                       # nothing more is started after a child that failed
                raise SystemExit(f'gmc_rate: the {kind} child ended with {r.returncode}:\n{r.stderr[-2000:]}')
            rates[kind] += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RATES ')][-1][6:])
    med = {k: float(np.median(v)) for k, v in rates.items()}
    lines.append(f'(i) detect.run track=True, {n_frames} frames 720 x 1280 of a panning camera, yolo_mobilev1 0.75 with seeded random weights, draw and PIL '
                 f'encode, batch 32, depth 4;')
    lines.append(f'      {rounds} rounds of fresh processes in turns (off, parent off, on; the first turn rotates), {runs} timed run(s) each after a warm-up run')
    lines.append(f'      gmc off, pictures/s: {spread(rates["off"])}')
    lines.append(f'      gmc on,  pictures/s: {spread(rates["on"])}')
    lines.append(f'(ii) the parent commit, track=True, pictures/s: {spread(rates["parent off"])}')
    inside = min(rates['parent off']) <= med['off'] <= max(rates['parent off']) and min(rates['off']) <= med['parent off'] <= max(rates['off'])
    lines.append(f'      off / parent = {med["off"] / med["parent off"]:.3f}; each median lies {"INSIDE" if inside else "OUTSIDE"} the other\'s min .. max: off '
                 f'{"agrees" if inside else "DOES NOT agree"} with the parent within the spread of the repeats')
    lines.append(f'(iii) on / off = {med["on"] / med["off"]:.3f} (recorded, not judged; on also reads every picture\'s header before the run)')
    return inside


def call_times(pics, repeats: int, lines):
    import torch
    from k210_yolo_framework_amd import draw as dr
    from k210_yolo_framework_amd import engine
    state = engine.GmcState(1, len(pics), (720 // 4) * (1280 // 4))
    packed, table, _ = dr.pack_ragged(pics)
    d_packed = packed.cuda()
    table_d = engine.ragged_table_to_device(table, None, d_packed.numel(), d_packed.device)
    first = torch.tensor([0, len(pics)], dtype=torch.int32, device='cuda')
    out = engine.gmc_motion(state, d_packed, table_d, first)
    ms = []
    for rep in range(3 + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        engine.gmc_motion(state, d_packed, table_d, first, out=out)
        b.record()
        b.synchronize()
        if rep >= 3:
            ms.append(a.elapsed_time(b))
    lines.append(f'(iv) one yk_gmc_motion_u8 call, {len(pics)} frames 720 x 1280 of one sequence (190 blocks a frame at the defaults), ms by device '
                 f'events: {spread(ms)}')
    lines.append(f'      the motions it found: {sorted(set(map(tuple, out.cpu().numpy().tolist())))}')


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        return child(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] == '1', int(sys.argv[6]))
    sys.path.insert(0, str(ROOT))
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--parent', type=str, required=True, help='a built checkout of the parent commit: its track=True detect.run is measured beside this tree\'s')
    p.add_argument('--out', type=str, default=str(ROOT / 'profiles' / 'gmc_rate.txt'))
    p.add_argument('--frames', type=int, default=64)
    p.add_argument('--rounds', type=int, default=6)
    p.add_argument('--runs', type=int, default=2)
    p.add_argument('--repeats', type=int, default=9, help='timed calls of (iv)')
    a = p.parse_args()
    if not (Path(a.parent) / 'k210_yolo_framework_amd' / 'csrc' / 'libyolo_hip.so').exists():
        p.error(f'--parent {a.parent}: no built k210_yolo_framework_amd/csrc/libyolo_hip.so there')
    from PIL import Image
    pics = frames_of(a.frames)
    lines = ['tools/gmc_rate.py: camera-motion compensation (DESIGN.md 3.30); rates from a host clock around runs that end synchronised, times from device events']
    with tempfile.TemporaryDirectory() as tmp:
        (Path(tmp) / 'frames').mkdir()
        for t, pic in enumerate(pics):
            Image.fromarray(pic).save(Path(tmp) / 'frames' / f'{t:05d}.jpg', quality=90)
        agrees = detect_rates(a.parent, Path(tmp) / 'frames', Path(tmp) / 'out', a.frames, a.rounds, a.runs, lines)   # first: before this process opens the GPU
    call_times(pics[:32], a.repeats, lines)
    lines.append('not measured: the effect on HOTA / IDF1 (only generated panning sequences could show it; none on real video), the three launches each on '
                 'its own, PRECISION=kpu and DECODE=gpu with TRACKGMC=True (they feed the same packed buffer)')
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 0 if agrees else 1


if __name__ == '__main__':
    sys.exit(main())

"""Rates of `make detect` (profiles/detect_rate.txt):  python tools/detect_rate.py [OUT.txt]
  (i)   256 in-memory pictures of mixed VOC-like sizes through detect.run(draw=False) against the PARENT's inference.detect (restated below:
        one letterbox launch and one blocking copy per picture, torch.cat) on the same pictures in lists of 32;
  (ii)  the ragged letterbox of one 32-picture batch against 32 yk_letterbox_u8 launches + torch.cat, inputs resident;
  (iii) the draw launch alone, at the default obj_thresh and at 0.05 (many boxes);
  (iv)  draw=True end to end, with and without the JPEG files, and PIL's encode time for one picture;
  (v)   draw=True end to end with encode='gpu' against encode='pil' (files written by both), and the encode launches of one 32-picture
        batch alone (yk_jpeg_encode_ragged_u8, quality 75, inputs resident);
  (vi)  decode='gpu' against decode='pil' end to end on the same 256 pictures as JPEG files (PIL, quality 90, 4:2:0), draw=False, and the
        decode launches of one 32-picture batch alone (yk_jpeg_decode_ragged_u8, inputs resident) with the rounds the fixed-point
        iteration took per picture at the default chunk size.  Written to profiles/jpeg_decode_rate.txt when run as
        `python tools/detect_rate.py profiles/detect_rate.txt profiles/jpeg_decode_rate.txt`.
Both sides warmed up, synchronised on both ends, three alternated repeats; medians with min / max."""
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from k210_yolo_framework_amd import detect, draw, engine, inference, jpeg  # noqa: E402
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS  # noqa: E402
from k210_yolo_framework_amd.yolonet import MODEL_DEFS  # noqa: E402

OUT = Path(sys.argv[1]) if len(sys.argv) > 1 else None
OUT_DECODE = Path(sys.argv[2]) if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT is not None:
        OUT.write_text('\n'.join(lines) + '\n')


def parent_detect(h, model, orig_imgs, obj, iou):
    """inference.detect of the parent commit for pictures of different sizes: one letterbox launch and one blocking copy per picture, torch.cat."""
    shapes = [img.shape[:2] for img in orig_imgs]
    n = len(orig_imgs)
    in_hw = tuple(int(v) for v in h.in_hw[0])
    frames = torch.cat([engine.letterbox_u8(torch.from_numpy(np.ascontiguousarray(im[None], np.uint8)).cuda(), in_hw) for im in orig_imgs])
    plan = model._plan(n)
    plan.run_u8(frames.contiguous())
    cfg = engine.make_decode_cfg(h.anchors, h.class_num, h.in_hw[0], h.out_hw)
    dets, counts = engine.decode_py(cfg, plan.outputs(), n, np.asarray(shapes, np.float32), obj, iou)
    torch.cuda.synchronize()
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    return [dets[i, :counts[i]] for i in range(n)]


def med(xs):
    return f'median {statistics.median(xs):.3f} (min {min(xs):.3f}, max {max(xs):.3f})'


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    engine.require_gpu()
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    model, _ = MODEL_DEFS['yolo_mobilev1']([224, 320, 3], 3, 20, alpha=0.75, precision='f16x2')
    rng = np.random.default_rng(0)
    sizes = [(375, 500), (500, 375), (333, 500), (500, 333), (281, 500), (500, 400), (480, 640), (366, 500)]
    pics = []
    for i in range(256):
        hh, ww = sizes[int(rng.integers(0, len(sizes)))]
        pics.append(rng.integers(0, 256, (hh // 8 + 1, ww // 8 + 1, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)[:hh, :ww].copy())
    say(f'256 pictures in memory, sizes drawn from {sizes}, {sum(p.size for p in pics) / 1e6:.1f} MB; yolo_mobilev1-0.75 f16x2, seeded random weights')
    OBJ, IOU = 0.7, 0.3

    # (i) detect.run(draw=False) against the parent's inference.detect in lists of 32
    new = lambda n_rep=1: detect.run(h, model, pics * n_rep, out_dir=None, draw=False, batch=32, depth=4, obj_thresh=OBJ, iou_thresh=IOU, verbose=False)
    old = lambda: [parent_detect(h, model, pics[k:k + 32], OBJ, IOU) for k in range(0, 256, 32)]
    new(); old()                                                    # warm-up of both
    tn, to, tn4 = [], [], []
    for _ in range(3):
        tn.append(timed(new)); to.append(timed(old)); tn4.append(timed(lambda: new(4)))
    say('(i) 256 pictures, draw=False, seconds per call (pipeline construction and graph capture inside every detect.run call):')
    say(f'    detect.run              {med(tn)}   -> {256 / statistics.median(tn):.0f} pictures/s')
    say(f'    parent inference.detect {med(to)}   -> {256 / statistics.median(to):.0f} pictures/s')
    say(f'    detect.run, 1024 pictures {med(tn4)}; marginal rate over the last 768: {768 / (statistics.median(tn4) - statistics.median(tn)):.0f} pictures/s')

    # (ii) one 32-picture batch: ragged launch against 32 launches + torch.cat, inputs resident
    batch = pics[:32]
    packed, table, _ = draw.pack_ragged(batch)
    d_packed = packed.cuda()
    d_table = engine.ragged_table_to_device(table, (224, 320), d_packed.numel(), d_packed.device)
    singles = [torch.from_numpy(p[None]).cuda() for p in batch]
    out = torch.empty((32, 224, 320, 3), dtype=torch.uint8, device='cuda')
    rag = lambda: [engine.letterbox_ragged_u8(d_packed, d_table, (224, 320), out=out) for _ in range(50)]
    per = lambda: [torch.cat([engine.letterbox_u8(s, (224, 320)) for s in singles]) for _ in range(50)]
    rag(); per()
    tr, tp = [], []
    for _ in range(3):
        tr.append(timed(rag) / 50 * 1e6); tp.append(timed(per) / 50 * 1e6)
    ref = torch.cat([engine.letterbox_u8(s, (224, 320)) for s in singles])
    say(f'(ii) letterbox of one 32-picture batch, inputs resident, microseconds per batch (50 in a row, host included); bytes equal: {bool(torch.equal(ref, out))}')
    say(f'    yk_letterbox_ragged_u8, one launch        {med(tr)}')
    say(f'    32 x yk_letterbox_u8 + torch.cat (parent) {med(tp)}')

    # (iii) the draw launch alone
    colormap = torch.from_numpy(np.asarray(h.colormap, np.uint8).reshape(-1, 3)).cuda()
    atlas = torch.from_numpy(draw.glyph_atlas()).cuda()
    max_px = max(p.shape[0] * p.shape[1] for p in batch)
    for obj in (OBJ, 0.05):
        rows = parent_detect(h, model, batch, obj, IOU)
        dets = np.zeros((32, 600, 6), np.float32)
        for i, r in enumerate(rows):
            dets[i, :len(r)] = r
        d_dets, d_counts = torch.from_numpy(dets).cuda(), torch.from_numpy(np.asarray([len(r) for r in rows], np.int32)).cuda()
        dr = lambda: [engine.draw_detections_u8(d_packed, d_table, d_dets, d_counts, colormap, atlas, max_pixels=max_px) for _ in range(50)]
        dr()
        td = [timed(dr) / 50 * 1e6 for _ in range(3)]
        say(f'(iii) yk_draw_dets_u8 alone, 32 pictures ({d_packed.numel() / 1e6:.1f} MB), obj_thresh {obj}: {sum(len(r) for r in rows)} rows '
            f'(max {max(len(r) for r in rows)} per picture): microseconds per launch {med(td)}')

    # (iv) draw=True end to end: with and without the JPEG files
    tmp = Path(tempfile.mkdtemp())
    try:
        jpg = lambda: detect.run(h, model, pics, out_dir=str(tmp), draw=True, batch=32, depth=4, obj_thresh=OBJ, iou_thresh=IOU, verbose=False, workers=16)
        arr = lambda: detect.run(h, model, pics, out_dir=None, draw=True, batch=32, depth=4, obj_thresh=OBJ, iou_thresh=IOU, verbose=False, return_arrays=True)
        jpg(); arr()
        tj, ta = [], []
        for _ in range(3):
            tj.append(timed(jpg)); ta.append(timed(arr))
        from PIL import Image
        t0 = time.perf_counter()
        for p in pics[:32]:
            Image.fromarray(p).save(tmp / 'one.jpg')
        enc = (time.perf_counter() - t0) / 32
        say('(iv) 256 pictures, draw=True, seconds per call:')
        say(f'    drawn, copied back, no files        {med(ta)}   -> {256 / statistics.median(ta):.0f} pictures/s')
        say(f'    + <stem>_res.jpg on 16 pool threads {med(tj)}   -> {256 / statistics.median(tj):.0f} pictures/s')
        say(f'    PIL JPEG encode of one picture on one thread: {enc * 1e3:.1f} ms (256 of them over 16 threads: {256 * enc / 16:.3f} s if they scaled perfectly)')
        # (v) who encodes: the GPU right after the draw, or PIL on 16 pool threads
        run_as = lambda enc_: lambda: detect.run(h, model, pics, out_dir=str(tmp / enc_), draw=True, batch=32, depth=4, obj_thresh=OBJ,
                                                 iou_thresh=IOU, verbose=False, workers=16, encode=enc_, quality=75)
        gpu, pil = run_as('gpu'), run_as('pil')
        gpu(); pil()
        tg, tl = [], []
        for _ in range(3):
            tg.append(timed(gpu)); tl.append(timed(pil))
        size = lambda enc_: sum(f.stat().st_size for f in (tmp / enc_).glob('*_res.jpg')) / 1e6
        say('(v) 256 pictures, draw=True, files written, seconds per call:')
        say(f"    encode='gpu' (quality 75)     {med(tg)}   -> {256 / statistics.median(tg):.0f} pictures/s, {size('gpu'):.1f} MB of files")
        say(f"    encode='pil' (16 pool threads) {med(tl)}   -> {256 / statistics.median(tl):.0f} pictures/s, {size('pil'):.1f} MB of files")
        qtab = torch.from_numpy(engine.jpeg_tables(75)).cuda()
        jsizes = engine.jpeg_workspace_bytes(table)
        work = torch.empty(jsizes[0], dtype=torch.uint8, device='cuda')
        scan = torch.empty(jsizes[1], dtype=torch.uint8, device='cuda')
        off = torch.empty(33, dtype=torch.int64, device='cuda')
        enc_gpu = lambda: [engine.jpeg_encode_ragged_u8(d_packed, d_table, qtab, sizes=jsizes, work=work, out=scan, out_off=off) for _ in range(50)]
        enc_gpu()
        te = [timed(enc_gpu) / 50 * 1e6 for _ in range(3)]
        say(f'    yk_jpeg_encode_ragged_u8 alone, 32 pictures ({d_packed.numel() / 1e6:.1f} MB -> {int(off[32].item()) / 1e6:.2f} MB of scans, workspace '
            f'{jsizes[0] / 1e6:.0f} MB): microseconds per call (9 launches, 50 calls in a row, host included) {med(te)}')
        # (vi) who decodes: the GPU in front of the letterbox, or PIL on 16 pool threads
        mark = len(lines)
        from PIL import Image
        (tmp / 'src').mkdir()
        paths = []
        for i, p in enumerate(pics):
            paths.append(str(tmp / 'src' / f'p{i:03d}.jpg'))
            Image.fromarray(p).save(paths[-1], quality=90)
        dec_as = lambda d_: lambda: detect.run(h, model, paths, out_dir=None, draw=False, batch=32, depth=4, obj_thresh=OBJ, iou_thresh=IOU,
                                               verbose=False, workers=16, decode=d_)
        dgpu, dpil = dec_as('gpu'), dec_as('pil')
        dgpu(); dpil()
        tg, tl = [], []
        for _ in range(3):
            tg.append(timed(dgpu)); tl.append(timed(dpil))
        mb = sum(Path(f).stat().st_size for f in paths) / 1e6
        say(f'(vi) 256 JPEG files ({mb:.1f} MB, PIL quality 90, 4:2:0), draw=False, seconds per call:')
        say(f"    decode='gpu'                   {med(tg)}   -> {256 / statistics.median(tg):.0f} pictures/s")
        say(f"    decode='pil' (16 pool threads) {med(tl)}   -> {256 / statistics.median(tl):.0f} pictures/s")
        parsed = [jpeg.parse_baseline(Path(f).read_bytes()) for f in paths[:32]]
        buf, jpics, scan_bytes, table_bytes = jpeg.plan_decode(parsed)
        d_buf = torch.from_numpy(buf).cuda()
        d_jpics = torch.from_numpy(jpics.view(np.uint8).reshape(32, -1).copy()).cuda()
        need = engine.jpeg_decode_workspace_bytes(jpics)
        jwork = torch.empty(need, dtype=torch.uint8, device='cuda')
        status = torch.empty(32, dtype=torch.int32, device='cuda')
        dec_gpu = lambda: [engine.jpeg_decode_ragged_u8(d_buf[:scan_bytes], d_jpics, d_buf[scan_bytes:], d_table, d_packed, work_bytes=need, work=jwork,
                                                        status=status) for _ in range(50)]
        dec_gpu()
        tdec = [timed(dec_gpu) / 50 * 1e6 for _ in range(3)]
        at = (4 * 33 + 15) & ~15
        rounds = jwork[at:at + 4 * 32].cpu().numpy().view(np.uint32)
        tiles = [-(-(-(-len(q.scan) // 128)) // 256) for q in parsed]
        say(f'    yk_jpeg_decode_ragged_u8 alone, 32 pictures ({scan_bytes / 1e6:.2f} MB of scans -> {d_packed.numel() / 1e6:.1f} MB, workspace {need / 1e6:.0f} MB, '
            f'statuses all 0: {not status.any().item()}): microseconds per call (6 launches, 50 calls in a row, host included) {med(tdec)}')
        say(f'    fixed-point rounds per picture at chunk_bytes {128} (summed over its tiles of 256 chunks; tiles per picture {min(tiles)} .. {max(tiles)}): '
            f'min {int(rounds.min())}, median {int(np.median(rounds))}, max {int(rounds.max())}')
        if OUT_DECODE is not None:
            OUT_DECODE.write_text('\n'.join(lines[:1] + lines[mark:]) + '\n')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


main()

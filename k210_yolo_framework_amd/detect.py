"""`make detect` - a folder of pictures through the pipeline: detections and annotated pictures out.

    python keras_detect.py CKPT SRC --out_dir D [--draw True|False] [--decode pil|gpu] [--encode pil|gpu] [--quality 75] [--batch 32] [--depth 4]
                           [--tiles NXxNY --tile_overlap 0.2 --tile_full True --tile_match ios|iou --tile_thresh 0.5]
                           [--tta 1,1f|flip|v5 --tta_thresh 0.55]
                           [network and threshold flags of keras_inference.py]

SRC: a folder (its .jpg / .jpeg / .png / .bmp files, in sorted order), a text file with one picture path per line, or one picture.
What the reference's keras_inference.py:137-174 does for one picture, for all of them at the pipeline's rate: the pictures are decoded on
a thread pool, each batch is packed into ONE pinned buffer (pictures of different sizes back to back), crosses PCIe in one copy, is
letterboxed by one launch (yk_letterbox_ragged_u8) into a Pipeline slot and submitted; with --draw True the boxes and labels are painted
into the still-resident originals on the slot's stream (yk_draw_dets_u8), and only finished pictures come back, to be written as
<out_dir>/<stem>_res.jpg on the pool (--encode pil, the default), or are JPEG-encoded on the device right after the draw (--encode gpu,
yk_jpeg_encode_ragged_u8: only the compressed scans come back and are written between jpeg.py's headers and EOI).  With --decode gpu the pool
only reads and parses the files: the entropy-coded scans cross PCIe instead of the pixels and yk_jpeg_decode_ragged_u8 decodes them on the
slot's stream in front of the letterbox; a picture the parser refuses (progressive, CMYK, a PNG ...) is decoded by PIL as before and
travels in the same buffer.  Always writes <out_dir>/detections.json ([{path, detections: [[top, left, bottom, right, score,
class], ...]}, ...]) and prints the reference's table per picture.  `--precision kpu` runs a .kmodel / .kfpkg through engine.KpuPlan."""
from __future__ import annotations

import argparse
import io
import json
import sys
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np

from . import draw as dr
from . import jpeg
from . import softnms
from . import tiles as tl
from . import tta as tt
from .helper import INFO, NOTE, Helper, VOC_ANCHORS
from .yolonet import MODEL_DEFS

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')
MAX_WORKERS = 16                    # decode / encode pool: a fixed ceiling, never the machine's CPU count


def parse(argv=None):
    p = argparse.ArgumentParser(description='detections and annotated pictures for a folder or a list of pictures')
    p.add_argument('pre_ckpt', type=str, help='.h5 / .npz weights ("" = seeded random weights), or a .kmodel / .kfpkg with --precision kpu')
    p.add_argument('src', type=str, help='a folder of pictures, a text file of picture paths, or one picture')
    p.add_argument('--out_dir', type=str, default='out')
    p.add_argument('--draw', type=str, choices=['True', 'False'], default='True', help='write <stem>_res.jpg with boxes and labels')
    p.add_argument('--decode', type=str, choices=['pil', 'gpu'], default='pil',
                   help='who decodes the pictures: PIL on the thread pool, or (baseline JPEG files) the GPU in front of the letterbox')
    p.add_argument('--encode', type=str, choices=['pil', 'gpu'], default='pil',
                   help='who writes the JPEG of an annotated picture: PIL on the thread pool, or the GPU right after the draw')
    p.add_argument('--quality', type=int, default=75, help='JPEG quality 1 .. 100 of --encode gpu')
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--depth', type=int, default=4, help='batches in flight (float modes)')
    p.add_argument('--workers', type=int, default=8, help=f'decode / encode threads (at most {MAX_WORKERS})')
    p.add_argument('--train_set', type=str, default='voc')
    p.add_argument('--class_num', type=int, default=20)
    p.add_argument('--model_def', type=str, default='yolo_mobilev2')
    p.add_argument('--depth_multiplier', type=float, choices=[0.5, 0.75, 1.0], default=1.0)
    p.add_argument('--image_size', type=int, default=(224, 320), nargs='+')
    p.add_argument('--output_size', type=int, default=(7, 10, 14, 20), nargs='+')
    p.add_argument('--obj_thresh', type=float, default=0.7)
    p.add_argument('--iou_thresh', type=float, default=0.3)
    p.add_argument('--precision', type=str, choices=['f16', 'f16x2', 'kpu'], default='f16x2')
    p.add_argument('--nms', type=str, default='hard', help="suppression rule of the decode: hard (the reference's), linear or gaussian (Soft-NMS), diou")
    p.add_argument('--nms_sigma', type=float, default=0.5, help='sigma of --nms gaussian')
    tl.add_arguments(p)
    tt.add_arguments(p)
    a = p.parse_args(sys.argv[1:] if argv is None else argv)
    if (a.precision == 'kpu') != a.pre_ckpt.endswith(('.kmodel', '.kfpkg')):
        p.error('--precision kpu runs a .kmodel / .kfpkg checkpoint, and only it does (the float modes take .h5 / .npz)')
    if a.batch < 1 or a.depth < 1 or a.workers < 1:
        p.error('--batch, --depth and --workers are at least 1')
    if not 1 <= a.quality <= 100:
        p.error('--quality is 1 .. 100')
    try:
        softnms.check(a.nms, a.nms_sigma)
    except ValueError as e:
        p.error(str(e))
    try:
        tl.parse_arguments(a)
        tt.parse_arguments(a)
    except ValueError as e:
        p.error(str(e))
    if a.tta is not None and len(a.tta) > a.batch:
        p.error(f'--tta {tt.text_of(a.tta)}: a picture is {len(a.tta)} frames and --batch holds {a.batch}')
    a.draw = a.draw == 'True'
    return a


def expand_sources(src) -> List[str]:
    """A folder -> its pictures (EXTENSIONS, any letter case) in sorted order; a picture -> itself; any other file -> the paths it lists, one
    per line (blank lines and lines starting with # skipped; a relative path that does not exist as written is taken relative to the list)."""
    p = Path(src)
    if p.is_dir():
        return [str(f) for f in sorted(p.iterdir()) if f.is_file() and f.suffix.lower() in EXTENSIONS]
    if not p.is_file():
        raise FileNotFoundError(f'{src}: neither a folder nor a file')
    if p.suffix.lower() in EXTENSIONS:
        return [str(p)]
    out = []
    for line in p.read_text().splitlines():
        line = line.strip()
        if not line or line.startswith('#'):
            continue
        q = Path(line)
        out.append(str(q if q.is_absolute() or q.exists() else p.parent / q))
    return out


def output_names(names: Sequence[str], out_dir) -> List[str]:
    """<out_dir>/<stem>_res.jpg per picture; a stem that occurred before (two folders in one list) gets _2, _3, ... appended."""
    seen, out = {}, []
    for n in names:
        stem = Path(n).stem
        seen[stem] = seen.get(stem, 0) + 1
        out.append(str(Path(out_dir) / (f'{stem}_res.jpg' if seen[stem] == 1 else f'{stem}_{seen[stem]}_res.jpg')))
    return out


def print_table(name: str, rows: np.ndarray) -> None:
    """keras_inference.py:146,154 for one picture, its path above."""
    print(name)
    if len(rows):
        print('[top\tleft\tbottom\tright\tscore\tclass]')
        for top, left, bottom, right, score, c in rows:
            print(f'[{top:.1f}\t{left:.1f}\t{bottom:.1f}\t{right:.1f}\t{score:.2f}\t{int(c):2d}]')
    else:
        print(NOTE, ' no boxes detected')


def _save_jpg(arr: np.ndarray, path: str) -> str:
    from PIL import Image
    Image.fromarray(arr).save(path)
    return path


class _Stage:
    """What one batch in flight owns besides its Pipeline slot."""

    def __init__(self):
        self.pinned = self.d_packed = self.h_dets = self.h_counts = None
        self.d_work = self.d_scan = self.h_scan = self.d_off = self.h_off = None       # encode='gpu'
        self.d_stage = self.d_jwork = self.d_jstatus = self.h_jstatus = None           # decode='gpu'
        self.d_mdets = self.d_mcounts = None                                            # tiles, tta: the merged / fused rows per picture


def run(h: Helper, model, sources, out_dir=None, draw: bool = True, batch: int = 32, depth: int = 4, precision: str = 'f16x2',
        obj_thresh: float = 0.7, iou_thresh: float = 0.3, workers: int = 8, names: Optional[Sequence[str]] = None,
        return_arrays: bool = False, verbose: bool = True, max_out: int = 30, encode: str = 'pil', quality: int = 75, decode: str = 'pil',
        nms: str = 'hard', nms_sigma: float = 0.5, tiles=None, tile_overlap: float = 0.2, tile_full: bool = True, tile_match: str = 'ios',
        tile_thresh: float = 0.5, tta=None, tta_thresh: float = 0.55):
    """sources: picture paths, or [h, w, 3] uint8 arrays already in memory (then `names` names them); with decode='gpu' paths or the bytes of
    picture files: baseline JPEGs are decoded on the device by the rule of include/yolo_hip.h (not PIL's bytes: DESIGN.md 3.12), every other
    file by PIL on the pool as with decode='pil'; a stream the device cannot finish raises YkError naming the file.  -> {'names', 'detections': one
    [k, 6] float32 array per picture, 'files': the pictures written, 'arrays': the annotated pictures as they leave the GPU, before any JPEG
    encoding (return_arrays=True with draw=True)}.  With out_dir also writes detections.json and, when drawing, the _res.jpg files:
    encode='pil' through PIL's save() on the pool; encode='gpu' encodes them on the slot's stream right after the draw at `quality`
     - then the uncompressed pictures come back only for return_arrays, and the files are headers + scan + EOI.
    tiles=(nx, ny): sliced inference (tiles.py) - every picture runs as nx * ny overlapping tiles (tile_overlap of a tile's
    side) plus, with tile_full, the whole picture, each a network frame of its own (yk_letterbox_tiles_u8 cuts them out of the resident
    originals), and yk_merge_tiles turns their rows into the picture's rows by a hard NMS at tile_thresh under tile_match ('ios' or 'iou');
    a batch then holds max(1, batch // frames per picture) pictures.  None (the default): everything as without the option.
    tta='1,0.83f,0.67' | 'flip' | 'v5' | ((gain, mirror), ...): test-time augmentation (tta.py) - every picture runs as one
    frame per view (yk_letterbox_views_u8 reads the shrunk and mirrored canvases out of the resident originals), each decoded at its canvas's
    size, and yk_fuse_views fuses their rows by Weighted Boxes Fusion at IoU > tta_thresh; a batch holds batch // views pictures (more views
    than `batch` are refused), and tta together with tiles or with a soft nms is refused.  None (the default): everything as without it."""
    import torch
    from . import engine
    engine.require_gpu()
    n_all = len(sources)
    if n_all == 0:
        raise engine.YkError('detect: no pictures')
    if encode not in ('pil', 'gpu'):
        raise engine.YkError(f'detect: encode {encode!r}: expected pil or gpu')
    if decode not in ('pil', 'gpu'):
        raise engine.YkError(f'detect: decode {decode!r}: expected pil or gpu')
    try:
        softnms.check(nms, nms_sigma)
    except ValueError as e:
        raise engine.YkError(f'detect: {e}') from None
    try:
        grid_xy = tl.check(tiles, tile_overlap, tile_match, tile_thresh, nms)
    except ValueError as e:
        raise engine.YkError(f'detect: {e}') from None
    T = 1 if grid_xy is None else grid_xy[0] * grid_xy[1] + (1 if tile_full else 0)      # network frames per picture
    try:
        tta_spec = tt.check(tta, tta_thresh, nms, tiles)
    except ValueError as e:
        raise engine.YkError(f'detect: {e}') from None
    if tta_spec is not None:
        T = len(tta_spec)
        if T > int(batch):
            raise engine.YkError(f'detect: tta {tt.text_of(tta_spec)}: a picture is {T} frames and a batch holds {int(batch)}')
    gpu_decode = decode == 'gpu'
    in_memory = isinstance(sources[0], (np.ndarray, bytes))
    if gpu_decode and any(isinstance(s, np.ndarray) for s in sources):
        raise engine.YkError("detect: decode='gpu' takes paths or the bytes of picture files, not arrays")
    names = list(names) if names is not None else ([f'img{i:05d}' for i in range(n_all)] if in_memory else [str(s) for s in sources])
    in_hw = tuple(int(v) for v in h.in_hw[0])
    B = max(1, min(int(batch) // T, n_all))                  # pictures per batch; the network sees B * T frames
    dev = torch.device('cuda', torch.cuda.current_device())
    if out_dir is not None:
        Path(out_dir).mkdir(parents=True, exist_ok=True)
    files = output_names(names, out_dir) if (draw and out_dir is not None) else [None] * n_all
    want_pixels = draw and (out_dir is not None or return_arrays)
    gpu_jpeg = encode == 'gpu' and draw and out_dir is not None
    copy_pixels = want_pixels and (return_arrays or not gpu_jpeg)       # the uncompressed pictures cross PCIe only when someone reads them
    cap = h.class_num * max_out
    colormap = torch.from_numpy(np.asarray(h.colormap, np.uint8).reshape(-1, 3)).to(dev)
    atlas = torch.from_numpy(dr.glyph_atlas()).to(dev)
    if gpu_jpeg:
        qtabs = engine.jpeg_tables(quality)
        d_qtab = torch.from_numpy(qtabs).to(dev)

    pipe = plan = None
    if precision == 'kpu':                                  # one batch at a time through the KPU's integer arithmetic, on the current stream
        plan = model._plan(B * T)
        cfg = engine.make_decode_cfg(h.anchors, h.class_num, h.in_hw[0], h.out_hw)
        frames = torch.empty((B * T, *in_hw, 3), dtype=torch.uint8, device=dev)
        depth = 1
    else:
        depth = max(1, int(depth))
        pipe = engine.Pipeline(model.spec, model.get_weights(), h.anchors, max_batch=B * T, depth=depth, precision=precision, max_out=max_out)
    stages = [_Stage() for _ in range(depth)]
    pool = ThreadPoolExecutor(max_workers=max(1, min(MAX_WORKERS, int(workers))))
    load = (lambda s: np.ascontiguousarray(s[..., :3], np.uint8)) if in_memory else \
        (lambda s: np.ascontiguousarray(h._read_img(str(s))[..., :3]).astype(np.uint8, copy=False))

    def load_file(s):
        """decode='gpu': -> a jpeg.Baseline, or (pixels, the parser's reason for refusing the file)."""
        data = s if isinstance(s, bytes) else Path(s).read_bytes()
        try:
            return jpeg.parse_baseline(data)
        except jpeg.Unsupported as e:
            return np.ascontiguousarray(h._read_img(io.BytesIO(data))[..., :3]).astype(np.uint8, copy=False), e.reason

    if gpu_decode:
        load = load_file
    starts = list(range(0, n_all, B))
    ahead = depth + 1                                       # batches whose pictures are being decoded while the GPU works
    loading = deque()
    pending = deque()                                       # batches on the GPU: (first picture, count, stage, table, device table, event, slot, stream)
    results = [None] * n_all
    arrays = [None] * n_all if (return_arrays and draw) else None
    saves = []
    written = []

    def copy(dst, src, nbytes, stream):
        """Pinned <-> device on a slot's stream through the library, as Pipeline copies: torch's pinned-memory allocator must never learn of
        the pipeline's own streams - it records an event on every stream a pinned block was copied on when the block is FREED, and by then
        Pipeline.close() has destroyed them."""
        engine.call('yk_memcpy_async', dst, src, int(nbytes), stream.cuda_stream)

    def start_load(k):
        loading.append([pool.submit(load, s) for s in sources[starts[k]:starts[k] + B]])

    def drain():
        first, n, st, table, keep, ev, slot, stream = pending.popleft()
        ev.synchronize()
        if pipe is not None:
            pipe.plans[slot].raise_if_failed()
        if gpu_decode and keep[1]:
            for j, code in zip(keep[1], st.h_jstatus[:len(keep[1])].numpy().tolist()):
                if code:
                    raise engine.YkError(f'detect: {names[first + j]}: the JPEG stream does not decode (status {code}: yk_jpeg_decode_ragged_u8)')
        counts = st.h_counts[:n].numpy()
        for i in range(n):
            results[first + i] = st.h_dets[i, :int(counts[i])].numpy().copy()
        if copy_pixels:
            flat = st.pinned.numpy()
            for i, view in enumerate(dr.unpack_ragged(flat, table)):
                arr = view.copy()                           # the slot's buffer is packed again while the pool encodes
                if arrays is not None:
                    arrays[first + i] = arr
                if files[first + i] is not None and not gpu_jpeg:
                    saves.append(pool.submit(_save_jpg, arr, files[first + i]))
        if gpu_jpeg:
            off = st.h_off[:n + 1].numpy()                  # came back with the batch; now the second copy knows its size
            total = int(off[n])
            if total:
                copy(st.h_scan, st.d_scan, total, stream)
                stream.synchronize()
            scan = st.h_scan.numpy()
            for i in range(n):
                with open(files[first + i], 'wb') as f:
                    f.write(jpeg.assemble(int(table['h'][i]), int(table['w'][i]), qtabs, scan[int(off[i]):int(off[i + 1])].tobytes()))
                written.append(files[first + i])
        if verbose:
            for i in range(n):
                print_table(names[first + i], results[first + i])

    try:
        for k in range(min(ahead, len(starts))):
            start_load(k)
        for k, first in enumerate(starts):
            imgs = [f.result() for f in loading.popleft()]
            if k + ahead < len(starts):
                start_load(k + ahead)
            if len(pending) == depth:                       # the slot about to be reused still holds an unread batch
                drain()
            n = len(imgs)
            slot = pipe.next_slot() if pipe is not None else 0
            st = stages[slot]
            if gpu_decode:
                # the pinned buffer carries, 16-byte aligned: the pixels of the refused pictures, the scans and tables of the others,
                # their yk_jpeg_pic_t rows and their rows of the destination's table
                a16 = lambda v: (v + 15) & ~15
                jp = [j for j, it in enumerate(imgs) if isinstance(it, jpeg.Baseline)]
                parsed = [imgs[j] for j in jp]
                raw = [(j, it[0]) for j, it in enumerate(imgs) if not isinstance(it, jpeg.Baseline)]
                if verbose:
                    for j, it in enumerate(imgs):
                        if not isinstance(it, jpeg.Baseline):
                            print(NOTE, f' {names[first + j]}: {it[1]}: decoded by PIL')
                shapes = [(it.h, it.w) if isinstance(it, jpeg.Baseline) else it[0].shape[:2] for it in imgs]
                table = dr.ragged_table(shapes)
                total = dr.packed_bytes(table)
                raw_bytes = sum(a16(im.size) for _, im in raw)
                jbytes = a16(sum((len(q.scan) + jpeg.SCAN_PAD + 3) // 4 * 4 for q in parsed)) + len(jp) * jpeg.PIC_TABLE_BYTES
                stage_bytes = raw_bytes + a16(jbytes) + a16(len(jp) * jpeg.PIC_DTYPE.itemsize) + len(jp) * dr.RAGGED_DTYPE.itemsize
                need = max(stage_bytes, total)
            else:
                need = sum(im.size for im in imgs)
            if st.pinned is None or st.pinned.numel() < need:
                size = need + need // 4                     # grown rarely: pinning is slow
                st.pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
                st.d_packed = torch.empty(size, dtype=torch.uint8, device=dev)
                st.h_dets = torch.empty((B, cap, 6), dtype=torch.float32).pin_memory()
                st.h_counts = torch.empty((B,), dtype=torch.int32).pin_memory()
            stream = pipe.streams[slot] if pipe is not None else torch.cuda.current_stream()
            keep = None
            if gpu_decode:
                if st.d_stage is None or st.d_stage.numel() < stage_bytes:
                    st.d_stage = torch.empty(stage_bytes + stage_bytes // 4, dtype=torch.uint8, device=dev)
                    st.d_jstatus = torch.empty(B, dtype=torch.int32, device=dev)
                    st.h_jstatus = torch.empty(B, dtype=torch.int32).pin_memory()
                flat = st.pinned.numpy()
                at, raw_at = 0, []
                for j, im in raw:
                    flat[at:at + im.size] = im.reshape(-1)
                    raw_at.append(at)
                    at += a16(im.size)
                d_packed = st.d_packed[:total]
                if jp:
                    _, pics, scan_bytes, table_bytes = jpeg.plan_decode(parsed, out=flat[at:at + jbytes])
                    pics_at = at + a16(jbytes)
                    rows_at = pics_at + a16(len(jp) * jpeg.PIC_DTYPE.itemsize)
                    flat[pics_at:rows_at][:pics.nbytes] = pics.view(np.uint8)
                    flat[rows_at:rows_at + len(jp) * dr.RAGGED_DTYPE.itemsize] = np.ascontiguousarray(table[jp]).view(np.uint8)
                    work_bytes = engine.jpeg_decode_workspace_bytes(pics)
                    if st.d_jwork is None or st.d_jwork.numel() < work_bytes:
                        torch.cuda.synchronize()                                            # grown rarely; nothing in flight reads the old one
                        st.d_jwork = torch.empty(work_bytes + work_bytes // 4, dtype=torch.uint8, device=dev)
                copy(st.d_stage, st.pinned, stage_bytes, stream)                            # the batch's one copy to the device
                for (j, im), o in zip(raw, raw_at):                                         # refused pictures: device to device, to their offsets
                    copy(d_packed[int(table['offset'][j]):], st.d_stage[o:], im.size, stream)
                if jp:
                    engine.jpeg_decode_ragged_u8(st.d_stage[at:at + scan_bytes], st.d_stage[pics_at:pics_at + pics.nbytes].view(len(jp), -1),
                                                 st.d_stage[at + scan_bytes:at + scan_bytes + table_bytes],
                                                 st.d_stage[rows_at:rows_at + len(jp) * dr.RAGGED_DTYPE.itemsize].view(len(jp), -1), d_packed,
                                                 stream=stream, work_bytes=work_bytes, work=st.d_jwork, status=st.d_jstatus[:len(jp)])
                    copy(st.h_jstatus, st.d_jstatus, len(jp) * 4, stream)
                table_d = engine.ragged_table_to_device(table, in_hw, total, dev)
                keep = (table_d, jp)
            else:
                _, table, shapes = dr.pack_ragged(imgs, out=st.pinned)
                total = dr.packed_bytes(table)
                d_packed = st.d_packed[:total]
                table_d = engine.ragged_table_to_device(table, in_hw, total, dev)          # (a blocking copy of 40 bytes per picture)
                copy(d_packed, st.pinned, total, stream)                                    # the batch's one copy to the device
                keep = (table_d, None)
            nf = n * T                                                                      # network frames of this batch
            dst = pipe.input(slot)[:nf] if pipe is not None else frames[:nf]
            if tta_spec is not None:
                vws = [tt.views(sh, sw, tta_spec) for sh, sw in shapes]
                rows = np.concatenate([tt.table_rows(v, int(table['offset'][i]), *shapes[i]) for i, v in enumerate(vws)])
                v_all = np.concatenate(vws)
                views_d = engine.view_table_to_device(rows, in_hw, total, dev)             # (blocking copies of a few bytes per view, as above)
                engine.letterbox_views_u8(d_packed, views_d, in_hw, stream=stream, out=dst)
                hw = v_all[:, 0:2].astype(np.float32)                                       # every frame is decoded at its canvas's size
                xform_d = torch.from_numpy(tt.xforms(v_all)).to(dev)
                if st.d_mdets is None:
                    st.d_mdets = torch.zeros((B, cap, 6), dtype=torch.float32, device=dev)
                    st.d_mcounts = torch.zeros((B,), dtype=torch.int32, device=dev)
                    torch.cuda.current_stream().synchronize()                               # (filled on torch's stream, written on the slot's)
                keep = (*keep, views_d, xform_d)
            elif grid_xy is None:
                engine.letterbox_ragged_u8(d_packed, table_d, in_hw, stream=stream, out=dst)
                hw = np.asarray(shapes, np.float32)
            else:
                grids = [tl.grid(sh, sw, grid_xy[0], grid_xy[1], tile_overlap, tile_full) for sh, sw in shapes]
                rows = np.concatenate([tl.table_rows(g, int(table['offset'][i]), shapes[i][1]) for i, g in enumerate(grids)])
                g_all = np.concatenate(grids)
                tiles_d = engine.tile_table_to_device(rows, in_hw, total, dev)             # (blocking copies of a few bytes per tile, as above)
                engine.letterbox_tiles_u8(d_packed, tiles_d, in_hw, stream=stream, out=dst)
                hw = g_all[:, 2:4].astype(np.float32)                                       # every frame is decoded at its tile's size
                origin_d = torch.from_numpy(np.ascontiguousarray(g_all[:, 0:2], np.float32)).to(dev)
                first_d = torch.from_numpy(np.arange(n + 1, dtype=np.int32) * T).to(dev)
                if st.d_mdets is None:
                    st.d_mdets = torch.zeros((B, cap, 6), dtype=torch.float32, device=dev)
                    st.d_mcounts = torch.zeros((B,), dtype=torch.int32, device=dev)
                    torch.cuda.current_stream().synchronize()                               # (filled on torch's stream, written on the slot's)
                keep = (*keep, tiles_d, origin_d, first_d)
            if pipe is not None:
                dets, counts, _ = pipe.submit(None, image_hw=hw, obj_thresh=obj_thresh, iou_thresh=iou_thresh, max_out=max_out, batch=nf, nms=nms, sigma=nms_sigma)
            else:
                plan.run_u8(frames[:nf])
                dets, counts = engine.decode_py(cfg, plan.outputs(), nf, hw, obj_thresh, iou_thresh, max_out=max_out, nms=nms, sigma=nms_sigma)
            if grid_xy is not None:
                dets, counts = engine.merge_tiles(dets, counts, origin_d, first_d, h.class_num, max_out, tile_thresh, tile_match, stream=stream,
                                                  out=st.d_mdets[:n], out_counts=st.d_mcounts[:n])
            if tta_spec is not None:
                dets, counts = engine.fuse_views(dets, counts, xform_d, T, h.class_num, max_out, tta_thresh, stream=stream, out=st.d_mdets[:n],
                                                 out_counts=st.d_mcounts[:n])
            if want_pixels:
                max_px = int(max(s[0] * s[1] for s in shapes))
                engine.draw_detections_u8(d_packed, table_d, dets, counts, colormap, atlas, stream=stream, max_pixels=max_px)
                if copy_pixels:
                    copy(st.pinned, d_packed, total, stream)                                # only finished pictures come back
                if gpu_jpeg:
                    sizes = engine.jpeg_workspace_bytes(table)
                    if st.d_work is None or st.d_work.numel() < sizes[0] or st.d_scan.numel() < sizes[1]:
                        torch.cuda.synchronize()                                            # grown rarely; nothing in flight reads the old ones
                        st.d_work = torch.empty(sizes[0] + sizes[0] // 4, dtype=torch.uint8, device=dev)
                        st.d_scan = torch.empty(sizes[1] + sizes[1] // 4, dtype=torch.uint8, device=dev)
                        st.h_scan = torch.empty(st.d_scan.numel(), dtype=torch.uint8).pin_memory()
                        st.d_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
                        st.h_off = torch.empty(B + 1, dtype=torch.int64).pin_memory()
                    engine.jpeg_encode_ragged_u8(d_packed, table_d, d_qtab, stream=stream, sizes=sizes, work=st.d_work, out=st.d_scan,
                                                 out_off=st.d_off[:n + 1])
                    copy(st.h_off, st.d_off, (n + 1) * 8, stream)
            copy(st.h_dets, dets, n * cap * 6 * 4, stream)
            copy(st.h_counts, counts, n * 4, stream)
            ev = torch.cuda.Event()
            ev.record(stream)
            pending.append((first, n, st, table, keep, ev, slot, stream))                   # (keep: the device table, alive until the batch has run)
        while pending:
            drain()
        written += [f.result() for f in saves]
    finally:
        pool.shutdown(wait=True)
        if pipe is not None:
            pipe.close()
    if out_dir is not None:
        rule = {} if nms == 'hard' else {'nms': nms, 'nms_sigma': float(nms_sigma)}      # (hard: the file is what it always was)
        if grid_xy is not None:
            rule.update(tiles=[int(grid_xy[0]), int(grid_xy[1])], tile_overlap=float(tile_overlap), tile_full=bool(tile_full), tile_match=tile_match,
                        tile_thresh=float(tile_thresh))
        if tta_spec is not None:
            rule.update(tt.rule_of(tta_spec, tta_thresh))
        doc = [{'path': names[i], **rule, 'detections': [[float(v) for v in row] for row in results[i]]} for i in range(n_all)]
        (Path(out_dir) / 'detections.json').write_text(json.dumps(doc, indent=1))
    out = {'names': names, 'detections': results, 'files': written}
    if arrays is not None:
        out['arrays'] = arrays
    return out


def main(argv=None):
    a = parse(argv)
    from . import engine
    engine.require_gpu()
    anchor_file = Path(f'data/{a.train_set}_anchor.npy')
    h = Helper(None, a.class_num, str(anchor_file) if anchor_file.exists() else VOC_ANCHORS, np.reshape(np.array(a.image_size), (-1, 2)),
               np.reshape(np.array(a.output_size), (-1, 2)))
    model, _ = MODEL_DEFS[a.model_def]([a.image_size[0], a.image_size[1], 3], len(h.anchors[0]), a.class_num, alpha=a.depth_multiplier,
                                       precision=a.precision)
    if a.pre_ckpt and a.pre_ckpt not in ('None', '""'):
        model.load_weights(a.pre_ckpt)
        print(INFO, f' Load CKPT {a.pre_ckpt}')
    else:
        print(NOTE, ' no checkpoint given: seeded random weights')
    paths = expand_sources(a.src)
    if not paths:
        raise engine.YkError(f'detect: no pictures ({", ".join(EXTENSIONS)}) in {a.src}')
    res = run(h, model, paths, out_dir=a.out_dir, draw=a.draw, batch=a.batch, depth=a.depth, precision=a.precision,
              obj_thresh=a.obj_thresh, iou_thresh=a.iou_thresh, workers=a.workers, encode=a.encode, quality=a.quality, decode=a.decode,
              nms=a.nms, nms_sigma=a.nms_sigma, **tl.run_options(a), **tt.run_options(a))
    if a.nms != 'hard':
        print(INFO, f' nms {a.nms}, sigma {a.nms_sigma:g}: scores are the decayed ones')
    if a.tiles is not None:
        print(INFO, f' tiles {a.tiles[0]}x{a.tiles[1]}, overlap {a.tile_overlap:g}, whole picture {a.tile_full}: merged by {a.tile_match} > {a.tile_thresh:g}')
    if a.tta is not None:
        print(INFO, f' tta {tt.text_of(a.tta)}: {len(a.tta)} views a picture, fused by IoU > {a.tta_thresh:g} (tta.py); scores are the fused ones')
    print(INFO, f' {len(paths)} pictures, {sum(len(d) for d in res["detections"])} detections -> {Path(a.out_dir) / "detections.json"}'
          + (f', {len(res["files"])} annotated pictures' if a.draw else ''))
    return res


cli = main

if __name__ == '__main__':
    main()

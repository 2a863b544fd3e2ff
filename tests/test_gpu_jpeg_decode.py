"""JPEG decoding on the device (yk_jpeg_decode_ragged_u8) against the restatement tests/jpeg_dec_ref.py, byte for byte:
every size, layout, quality and restart interval PIL writes, the project's own encoder's streams, every chunk size down to the 4 bytes at
which most symbols straddle chunks, corrupt input, graph replay, run-to-run identity, and `make detect --decode gpu` end to end.
tests/test_jpeg_decode_host.py pins the reference itself against PIL's decoder."""
import ctypes as C
import io
import json
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import draw, jpeg, netspec as ns
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
from tests import jpeg_dec_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SENTINEL = 0xA5
GAP = 5                                     # bytes between pictures: with 3-byte pixels every residue of the offset mod 4 occurs


def _rows(parsed, lead=1):
    table = draw.ragged_table([(p.h, p.w) for p in parsed], gap=GAP)
    table['offset'] += lead
    return table


def _decode(files, chunk_bytes=0, parsed=None, rows=None, dst_bytes=None, work_bytes=None, edit=None):
    """-> (status numpy [n], dst numpy: SENTINEL wherever nothing was written, with 64 bytes beyond dst_bytes, rows)."""
    import torch
    from k210_yolo_framework_amd import engine
    parsed = [jpeg.parse_baseline(f) for f in files] if parsed is None else parsed
    buf, pics, scan_bytes, table_bytes = jpeg.plan_decode(parsed)
    if edit is not None:
        edit(buf, pics)
    rows = _rows(parsed) if rows is None else rows
    dst_bytes = draw.packed_bytes(_rows(parsed)) + 3 if dst_bytes is None else dst_bytes
    d_buf = torch.from_numpy(buf).cuda()
    dst = torch.full((dst_bytes + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    need = engine.jpeg_decode_workspace_bytes(pics)
    work = torch.empty(need if work_bytes is None else work_bytes, dtype=torch.uint8, device='cuda')
    d_pics = torch.from_numpy(pics.view(np.uint8).reshape(len(pics), -1).copy()).cuda()
    status = engine.jpeg_decode_ragged_u8(d_buf[:scan_bytes], d_pics, d_buf[scan_bytes:scan_bytes + table_bytes], rows, dst[:dst_bytes],
                                          work_bytes=work.numel(), work=work, chunk_bytes=chunk_bytes)
    torch.cuda.synchronize()
    return status.cpu().numpy(), dst.cpu().numpy(), rows


def _check(files, status, dst, rows, skip=()):
    """Every picture equals the reference, every other byte is still SENTINEL."""
    seen = np.zeros(len(dst), bool)
    for i, f in enumerate(files):
        if i in skip:
            continue
        want = ref.decode(f)
        o = int(rows[i]['offset'])
        got = dst[o:o + want.size].reshape(want.shape)
        assert status[i] == 0, (i, status[i])
        assert np.array_equal(got, want), (i, want.shape, int(np.abs(got.astype(int) - want.astype(int)).max()))
        seen[o:o + want.size] = True
    assert (dst[~seen] == SENTINEL).all()


@pytest.mark.parametrize('n', [1, 33])
def test_sizes_equal_the_reference_byte_for_byte(n):
    files = ref.batch_files(n)
    parsed = [jpeg.parse_baseline(f) for f in files]
    assert n == 1 or {(p.h, p.w) for p in parsed} == set(ref.SIZES)
    status, dst, rows = _decode(files, parsed=parsed)
    assert n == 1 or len({int(o) % 4 for o in rows['offset']}) == 4
    _check(files, status, dst, rows)


@pytest.mark.parametrize('size', [(17, 33), (96, 128)])
def test_layouts_qualities_and_optimised_tables(size):
    pic = ref.noise(*size)
    files = [ref.pil_file(pic, quality=q, optimize=o, **ref.layout_kw(lay)) for lay in ref.LAYOUTS for q in (1, 75, 100) for o in (False, True)]
    status, dst, rows = _decode(files)
    _check(files, status, dst, rows)


def test_restart_intervals():
    files = []
    for sub in (2, 0):
        for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=7), dict(restart_marker_rows=1)):
            for pic in (ref.noise(17, 33), ref.noise(96, 128), ref.smooth(50, 70)):
                files.append(ref.pil_file(pic, subsampling=sub, quality=90, **kw))
    assert all(jpeg.parse_baseline(f).restart > 0 for f in files)
    for chunk in (0, 4):                                                      # (at 4 bytes a chunk often holds nothing but a marker)
        status, dst, rows = _decode(files, chunk_bytes=chunk)
        _check(files, status, dst, rows)


def test_every_chunk_size_gives_the_same_bytes():
    files = [ref.pil_file(ref.noise(96, 128), quality=100), (ROOT / 'tests' / 'golden' / 'jpeg_people.jpg').read_bytes()]
    assert len(jpeg.parse_baseline(files[0]).scan) > 8 * 256 * 4             # several tiles of 4-byte chunks
    first = None
    for chunk in (4, 16, 128, 1024):
        status, dst, rows = _decode(files, chunk_bytes=chunk)
        _check(files, status, dst, rows)
        first = dst if first is None else first
        assert np.array_equal(dst, first), chunk


def test_streams_of_the_projects_own_encoder():
    import torch
    from k210_yolo_framework_amd import engine
    pics = [ref.noise(33, 47), ref.smooth(96, 128), ref.noise(16, 16)]
    packed, table, _ = draw.pack_ragged(pics)
    qt = engine.jpeg_tables(75)
    out, off = engine.jpeg_encode_ragged_u8(packed.cuda(), table, torch.from_numpy(qt).cuda())
    torch.cuda.synchronize()
    off, out = off.cpu().numpy(), out.cpu().numpy()
    files = [jpeg.assemble(p.shape[0], p.shape[1], qt, out[off[i]:off[i + 1]].tobytes()) for i, p in enumerate(pics)]
    status, dst, rows = _decode(files)
    _check(files, status, dst, rows)


def test_bad_input_is_bounded():
    """Input validation: the clamps make these ordinary runs.  Bad rows report a status, write nothing outside their own bytes, and the good
    pictures of the same batch are exact."""
    from k210_yolo_framework_amd import engine
    good = [ref.pil_file(ref.noise(17, 33), quality=75), ref.pil_file(ref.smooth(96, 128), quality=90), ref.pil_file(ref.noise(16, 16), mode='L')]
    cut = jpeg.parse_baseline(ref.pil_file(ref.noise(96, 128), quality=75))
    cut.scan = cut.scan[:len(cut.scan) // 2]
    rnd = jpeg.parse_baseline(ref.pil_file(ref.noise(96, 128), quality=75))
    rnd.scan = np.random.default_rng(3).integers(0, 256, 4096, dtype=np.uint8).tobytes()
    parsed = [jpeg.parse_baseline(good[0]), cut, jpeg.parse_baseline(good[1]), rnd, jpeg.parse_baseline(good[2])]
    files = [good[0], None, good[1], None, good[2]]
    status, dst, rows = _decode(files, parsed=parsed)
    assert status[1] != 0 and status[3] != 0
    for i in (1, 3):                                                          # whatever they wrote lies inside their own bytes: forget it
        o = int(rows[i]['offset'])
        dst[o:o + 96 * 128 * 3] = SENTINEL
    _check(files, status, dst, rows, skip=(1, 3))
    # a row whose destination leaves dst_bytes: status, nothing written; the others exact
    parsed = [jpeg.parse_baseline(f) for f in good]
    rows = _rows(parsed)
    total = draw.packed_bytes(rows) + 3
    bad = rows.copy()
    bad[1]['offset'] = total - 96 * 128 * 3 + 1
    status, dst, _ = _decode(good, parsed=parsed, rows=bad, dst_bytes=total)
    assert status[1] != 0
    _check(good, status, dst, bad, skip=(1,))
    # a workspace one MCU too small: every status non-zero, nothing written
    _, pics, _, _ = jpeg.plan_decode(parsed)
    need = engine.jpeg_decode_workspace_bytes(pics)
    status, dst, _ = _decode(good, parsed=parsed, work_bytes=need - 192)
    assert (status != 0).all() and (dst == SENTINEL).all()
    # the host helper and the call refuse what they can see
    wrong = pics.copy()
    wrong[0]['hs'] = 3
    with pytest.raises(engine.YkError):
        engine.jpeg_decode_workspace_bytes(wrong)
    with pytest.raises(engine.YkError):
        _decode(good, parsed=parsed, chunk_bytes=6)
    with pytest.raises(engine.YkError):
        _decode(good, parsed=parsed, chunk_bytes=2048)


def test_recorded_in_a_graph_replayed_on_new_scans_and_repeatable():
    import torch
    from k210_yolo_framework_amd import engine
    shapes = [(96, 128), (17, 33), (50, 70)]
    a = [ref.pil_file(ref.noise(*s), quality=75) for s in shapes]
    b = [ref.pil_file(ref.smooth(*s), quality=75) for s in shapes]
    pa, pb = [jpeg.parse_baseline(f) for f in a], [jpeg.parse_baseline(f) for f in b]
    bufa, pics_a, sa, ta = jpeg.plan_decode(pa)
    bufb, pics_b, sb, tb = jpeg.plan_decode(pb)
    assert sb <= sa and ta == tb                                              # the smooth pictures fit the capacities of the noise
    rows = _rows(pa)
    total = draw.packed_bytes(rows) + 3
    d_scan = torch.zeros(sa, dtype=torch.uint8, device='cuda')
    d_tab = torch.zeros(ta, dtype=torch.uint8, device='cuda')
    d_pics = torch.zeros((3, 56), dtype=torch.uint8, device='cuda')
    d_rows = torch.from_numpy(rows.view(np.uint8).reshape(3, -1).copy()).cuda()
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device='cuda')
    need = engine.jpeg_decode_workspace_bytes(pics_a)
    work = torch.empty(need, dtype=torch.uint8, device='cuda')
    status = torch.full((3,), -1, dtype=torch.int32, device='cuda')
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def load(buf, pics, s, t):
        d_scan.zero_()
        d_scan[:s].copy_(torch.from_numpy(buf[:s]))
        d_tab.copy_(torch.from_numpy(buf[s:s + t]))
        d_pics.copy_(torch.from_numpy(pics.view(np.uint8).reshape(3, -1).copy()))
        torch.cuda.synchronize()

    issue = lambda: engine.jpeg_decode_ragged_u8(d_scan, d_pics, d_tab, d_rows, dst, stream=stream, work_bytes=need, work=work, status=status)
    load(bufa, pics_a, sa, ta)
    issue()                                                                   # eagerly once: a capture records, it does not load kernels
    stream.synchronize()
    once = dst.cpu().numpy()
    _check(a, status.cpu().numpy(), once, rows)
    dst.fill_(SENTINEL)
    torch.cuda.synchronize()
    issue()
    stream.synchronize()
    assert np.array_equal(dst.cpu().numpy(), once)                            # two runs, identical bytes
    dst.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = engine.capture(st, issue)
    try:
        stream.synchronize()
        assert (dst == SENTINEL).all().item()                                 # recorded, not executed
        for k, (files, args) in enumerate(((a, (bufa, pics_a, sa, ta)), (b, (bufb, pics_b, sb, tb)), (a, (bufa, pics_a, sa, ta)))):
            load(*args)
            status.fill_(-1)
            torch.cuda.synchronize()
            graph.launch(st)
            stream.synchronize()
            _check(files, status.cpu().numpy(), dst.cpu().numpy(), rows)
    finally:
        graph.close()


def test_detect_decode_gpu_end_to_end(tmp_path):
    """detect.run(decode='gpu') on a folder with a progressive and a PNG picture mixed in gives the detections of the same pixels fed as
    arrays (the reference decoder's for the baseline files, _read_img's for the two others); the CLI takes --decode gpu; with draw and
    encode='gpu' the files open at the right sizes."""
    from PIL import Image
    from k210_yolo_framework_amd import detect, keras_io
    from k210_yolo_framework_amd.yolonet import MODEL_DEFS
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    ck = tmp_path / 'yolo_model.h5'
    keras_io.save_keras_weights(spec, spec.init_weights(seed=1), ck)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    model, _ = MODEL_DEFS['yolo_mobilev1']([224, 320, 3], 3, 20, alpha=0.75, precision='f16x2')
    model.load_weights(str(ck))
    folder = tmp_path / 'pics'
    folder.mkdir()
    rng = np.random.default_rng(21)
    shapes = [(120, 160), (97, 131), (64, 200), (120, 160), (33, 47), (80, 90), (50, 70)]
    for i, (hh, ww) in enumerate(shapes):
        im = Image.fromarray(rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8))
        if i == 2:
            im.save(folder / f'p{i}.jpg', progressive=True)
        elif i == 4:
            im.save(folder / f'p{i}.png')
        elif i == 5:
            im.convert('L').save(folder / f'p{i}.jpg')
        else:
            im.save(folder / f'p{i}.jpg', quality=90, subsampling=(0, 1, 2)[i % 3])
    paths = detect.expand_sources(folder)
    assert len(paths) == len(shapes)
    by_hand = []
    for f in paths:
        data = Path(f).read_bytes()
        try:
            jpeg.parse_baseline(data)
            by_hand.append(np.array(ref.decode(data)))
        except jpeg.Unsupported:
            by_hand.append(np.ascontiguousarray(h._read_img(f)[..., :3]).astype(np.uint8))
    kw = dict(draw=False, batch=3, depth=2, obj_thresh=0.6, iou_thresh=0.5, verbose=False)
    g = detect.run(h, model, paths, decode='gpu', **kw)
    m = detect.run(h, model, by_hand, **kw)
    assert sum(len(d) for d in m['detections']) > 0
    for i in range(len(paths)):
        assert np.array_equal(g['detections'][i], m['detections'][i]), i
    gb = detect.run(h, model, [Path(f).read_bytes() for f in paths], decode='gpu', names=paths, **kw)         # bytes instead of paths
    for i in range(len(paths)):
        assert np.array_equal(gb['detections'][i], m['detections'][i]), i
    # a stream that ends early is an error naming the file, as a truncated file is with PIL
    data = (folder / 'p0.jpg').read_bytes()
    seg = jpeg.parse_baseline(data).scan
    at = data.index(seg)
    (tmp_path / 'short.jpg').write_bytes(data[:at + len(seg) // 2] + b'\xff\xd9')
    from k210_yolo_framework_amd import engine
    with pytest.raises(engine.YkError, match='short.jpg'):
        detect.run(h, model, [str(tmp_path / 'short.jpg')], decode='gpu', **kw)
    # the CLI
    res = detect.cli([str(ck), str(folder), '--out_dir', str(tmp_path / 'cli'), '--decode', 'gpu', '--draw', 'False', '--model_def', 'yolo_mobilev1',
                      '--depth_multiplier', '0.75', '--obj_thresh', '0.6', '--iou_thresh', '0.5', '--batch', '4', '--depth', '1'])
    doc = json.loads((tmp_path / 'cli' / 'detections.json').read_text())
    assert [d['path'] for d in doc] == paths
    anchor_file = Path('data/voc_anchor.npy')                                  # the CLI's own helper: the anchors of the working directory
    h_cli = Helper(None, 20, str(anchor_file) if anchor_file.exists() else VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    m_cli = detect.run(h_cli, model, by_hand, **{**kw, 'batch': 4, 'depth': 1})
    for i, d in enumerate(doc):
        assert np.array_equal(res['detections'][i], m_cli['detections'][i]), i
        assert np.allclose(np.asarray(d['detections'], np.float32).reshape(-1, 6), m_cli['detections'][i])
    # drawing and encoding behind a GPU decode
    d = detect.run(h, model, paths, out_dir=tmp_path / 'drawn', decode='gpu', encode='gpu', **{**kw, 'draw': True})
    assert len(d['files']) == len(paths)
    for f, (hh, ww) in zip(d['files'], shapes):
        pic = Image.open(f)
        pic.load()
        assert pic.size == (ww, hh)

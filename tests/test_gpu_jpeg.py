"""JPEG encoding on the device (yk_jpeg_encode_ragged_u8) against the numpy restatement tests/jpeg_ref.py, bit for bit:
ragged batches of 1 and 33 pictures at odd offsets with gaps, three qualities, nothing written beside the streams, bad rows, argument
errors, graph replay, run-to-run identity, and `make detect --encode gpu` end to end.  tests/test_jpeg_host.py pins the reference itself
and the conditions these pictures meet (stuffed bytes, ZRL, EOB-only blocks, padded and unpadded ends)."""
import ctypes as C
import io

import numpy as np
import pytest

from k210_yolo_framework_amd import draw, jpeg, netspec as ns
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
from tests import jpeg_ref

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GAP = 5                                     # bytes between pictures: with 3-byte pixels every residue of the offset mod 4 occurs


def _pack(pics, lead=1):
    """-> (packed host uint8 with `lead` bytes in front and GAP bytes between pictures, all 0x33; table)."""
    table = draw.ragged_table([p.shape[:2] for p in pics], gap=GAP)
    table['offset'] += lead
    flat = np.full(draw.packed_bytes(table) + 3, 0x33, np.uint8)
    for row, p in zip(table, pics):
        flat[int(row['offset']):int(row['offset']) + p.size] = p.reshape(-1)
    return flat, table


def _encode(flat, table, quality, sizes=None, device_table=None):
    """-> (out_off [n + 1] numpy, out numpy with everything beyond the streams still SENTINEL, the source as the device holds it after)."""
    import torch
    from k210_yolo_framework_amd import engine
    d_packed = torch.from_numpy(flat).cuda()
    qtab = torch.from_numpy(engine.jpeg_tables(quality)).cuda()
    sizes = engine.jpeg_workspace_bytes(table) if sizes is None else sizes
    out = torch.full((sizes[1] + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    if device_table is None:
        _, off = engine.jpeg_encode_ragged_u8(d_packed, table, qtab, out=out)
    else:
        _, off = engine.jpeg_encode_ragged_u8(d_packed, device_table, qtab, sizes=sizes, out=out)
    torch.cuda.synchronize()
    return off.cpu().numpy(), out.cpu().numpy(), d_packed.cpu().numpy()


def _want(indices, quality, n=33):
    scans = [jpeg_ref.encode_cached(i, quality, n)[0] for i in indices]
    return np.cumsum([0] + [len(s) for s in scans]), scans


@pytest.mark.parametrize('quality', jpeg_ref.QUALITIES)
@pytest.mark.parametrize('n', [1, 33])
def test_streams_equal_the_reference_bit_for_bit(n, quality):
    from k210_yolo_framework_amd import engine
    pics = jpeg_ref.batch_pictures(n)
    assert n == 1 or {p.shape[:2] for p in pics} == set(jpeg_ref.SIZES)
    assert np.array_equal(engine.jpeg_tables(quality), jpeg.quant_tables(quality))
    flat, table = _pack(pics)
    assert n == 1 or len({int(o) % 4 for o in table['offset']}) == 4
    off, out, src_after = _encode(flat, table, quality)
    want_off, scans = _want(range(n), quality, n)
    assert off.dtype == np.int64 and np.array_equal(off, want_off)
    for i, s in enumerate(scans):
        assert out[off[i]:off[i + 1]].tobytes() == s, (i, pics[i].shape)
    assert (out[off[n]:] == SENTINEL).all()                          # nothing at or beyond d_out_off[n]
    assert np.array_equal(src_after, flat)                           # the source is only read
    cap = engine.jpeg_workspace_bytes(table)[1]
    assert off[n] <= cap


def test_two_runs_give_identical_bytes():
    pics = jpeg_ref.batch_pictures(33)
    flat, table = _pack(pics)
    a, b = _encode(flat, table, 100), _encode(flat, table, 100)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_bad_rows_give_empty_streams_and_leave_their_neighbours_alone():
    """What the wrapper refuses on a host table the kernels must survive in a device table: a row that leaves the buffer and a row without
    pixels encode to nothing, read nothing, and the streams around them are the reference's."""
    import torch
    from k210_yolo_framework_amd import engine
    idx = [0, 1, 2, 3, 4]
    pics = [jpeg_ref.batch_pictures(33)[i] for i in idx]
    flat, table = _pack(pics)
    sizes = engine.jpeg_workspace_bytes(table)
    bad = table.copy()
    bad[1]['offset'] = len(flat) - 3 * int(bad[1]['h']) * int(bad[1]['w']) + 1         # ends one byte past src_bytes
    bad[3]['h'] = 0
    with pytest.raises(engine.YkError):
        engine.jpeg_encode_ragged_u8(torch.from_numpy(flat).cuda(), bad, torch.from_numpy(jpeg.quant_tables(75)).cuda())
    d_bad = torch.from_numpy(bad.view(np.uint8).reshape(len(bad), -1).copy()).cuda()
    off, out, _ = _encode(flat, table, 75, sizes=sizes, device_table=d_bad)
    _, scans = _want(idx, 75)
    lens = [len(scans[0]), 0, len(scans[2]), 0, len(scans[4])]
    assert np.array_equal(off, np.cumsum([0] + lens))
    for i in (0, 2, 4):
        assert out[off[i]:off[i + 1]].tobytes() == scans[i]
    assert (out[off[5]:] == SENTINEL).all()
    # a workspace or an output the device table does not fit: n empty streams, nothing written
    tiny = table.copy()
    tiny['h'][[0, 2, 3, 4]] = 0
    small = engine.jpeg_workspace_bytes(tiny)                                            # sized for the 1 x 1 picture alone
    assert small[1] == 2 * 1248 and small[0] < sizes[0]
    d_table = torch.from_numpy(table.view(np.uint8).reshape(len(table), -1).copy()).cuda()
    d_packed = torch.from_numpy(flat).cuda()
    qtab = torch.from_numpy(jpeg.quant_tables(75)).cuda()
    for work_bytes, cap in ((small[0], sizes[1]), (sizes[0], small[1])):
        work = torch.empty(work_bytes, dtype=torch.uint8, device='cuda')
        o = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
        d_off = torch.full((6,), -1, dtype=torch.int64, device='cuda')
        engine._check(engine.lib().yk_jpeg_encode_ragged_u8(C.c_void_p(d_packed.data_ptr()), C.c_size_t(d_packed.numel()),
                                                            C.c_void_p(d_table.data_ptr()), C.c_int(5), C.c_void_p(qtab.data_ptr()),
                                                            C.c_void_p(work.data_ptr()), C.c_size_t(work_bytes), C.c_void_p(o.data_ptr()),
                                                            C.c_size_t(cap), C.c_void_p(d_off.data_ptr()), None), 'yk_jpeg_encode_ragged_u8')
        torch.cuda.synchronize()
        assert not d_off.any().item() and (o == SENTINEL).all().item()


def test_argument_errors():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    pic = jpeg_ref.picture('noise', 17, 9)
    flat, table = _pack([pic])
    sizes = engine.jpeg_workspace_bytes(table)
    assert sizes == engine.jpeg_workspace_bytes(table[:1]) and sizes[1] == 2 * 2 * 1248            # 2 MCUs, 1248 bytes each, stuffed twice
    d_packed = torch.from_numpy(flat).cuda()
    d_table = torch.from_numpy(table.view(np.uint8).reshape(1, -1).copy()).cuda()
    qtab = torch.from_numpy(jpeg.quant_tables(75)).cuda()
    work = torch.empty(sizes[0] + 16, dtype=torch.uint8, device='cuda')
    out = torch.empty(sizes[1], dtype=torch.uint8, device='cuda')
    off = torch.empty(2, dtype=torch.int64, device='cuda')
    v = lambda t: C.c_void_p(t.data_ptr())
    ok = dict(buf=v(d_packed), nb=C.c_size_t(d_packed.numel()), tab=v(d_table), n=1, q=v(qtab), work=v(work), wb=C.c_size_t(sizes[0]), out=v(out),
              cap=C.c_size_t(sizes[1]), off=v(off))
    call = lambda **kw: (lambda a: L.yk_jpeg_encode_ragged_u8(a['buf'], a['nb'], a['tab'], C.c_int(a['n']), a['q'], a['work'], a['wb'], a['out'],
                                                              a['cap'], a['off'], None))({**ok, **kw})
    assert call() == 0
    for kw in (dict(buf=None), dict(tab=None), dict(q=None), dict(work=None), dict(out=None), dict(off=None), dict(n=0), dict(n=-2),
               dict(nb=C.c_size_t(0)), dict(wb=C.c_size_t(100)), dict(cap=C.c_size_t(100)), dict(work=C.c_void_p(work.data_ptr() + 4))):
        assert call(**kw) == -10, kw                                                               # YK_ERR_ARG
        assert b'yk_jpeg_encode_ragged_u8' in L.yk_last_error()
    torch.cuda.synchronize()
    q = np.zeros((2, 64), np.uint8)
    for quality in (0, 101, -5):
        assert L.yk_jpeg_tables(C.c_int(quality), q.ctypes.data_as(C.c_void_p)) == -10
    assert L.yk_jpeg_tables(C.c_int(75), None) == -10
    w_, c_ = C.c_size_t(0), C.c_size_t(0)
    t = np.ascontiguousarray(table)
    assert L.yk_jpeg_workspace_bytes(None, C.c_int(1), C.byref(w_), C.byref(c_)) == -10
    assert L.yk_jpeg_workspace_bytes(t.ctypes.data_as(C.c_void_p), C.c_int(0), C.byref(w_), C.byref(c_)) == -10
    assert L.yk_jpeg_workspace_bytes(t.ctypes.data_as(C.c_void_p), C.c_int(1), None, C.byref(c_)) == -10
    huge = table.copy()
    huge[0]['w'] = 65536
    assert L.yk_jpeg_workspace_bytes(huge.ctypes.data_as(C.c_void_p), C.c_int(1), C.byref(w_), C.byref(c_)) == -10
    # the wrapper checks capacities against the helper on the host table
    with pytest.raises(engine.YkError):
        engine.jpeg_encode_ragged_u8(d_packed, table, qtab, out=torch.empty(sizes[1] - 1, dtype=torch.uint8, device='cuda'))
    with pytest.raises(engine.YkError):
        engine.jpeg_encode_ragged_u8(d_packed, d_table, qtab)                                      # a device table without sizes


def test_recorded_in_a_graph_and_replayed_on_new_pixels():
    import torch
    from k210_yolo_framework_amd import engine
    idx = [0, 5, 6, 12]                                                # 96 x 128 noise, 15 x 33 noise, 7 x 640 flat, 17 x 9 ramp
    pics = [jpeg_ref.batch_pictures(33)[i] for i in idx]
    flat, table = _pack(pics)
    other = [jpeg_ref.picture('noise', *p.shape[:2], seed=77) for p in pics]
    flat2, _ = _pack(other)
    sizes = engine.jpeg_workspace_bytes(table)
    d_packed = torch.from_numpy(flat).cuda()
    d_table = engine.ragged_table_to_device(table, None, d_packed.numel(), d_packed.device)
    qtab = torch.from_numpy(jpeg.quant_tables(75)).cuda()
    work = torch.empty(sizes[0], dtype=torch.uint8, device='cuda')
    out = torch.full((sizes[1],), SENTINEL, dtype=torch.uint8, device='cuda')
    off = torch.zeros(len(idx) + 1, dtype=torch.int64, device='cuda')
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    v = lambda t: C.c_void_p(t.data_ptr())
    issue = lambda: engine._check(engine.lib().yk_jpeg_encode_ragged_u8(v(d_packed), C.c_size_t(d_packed.numel()), v(d_table), C.c_int(len(idx)),
                                                                        v(qtab), v(work), C.c_size_t(sizes[0]), v(out), C.c_size_t(sizes[1]),
                                                                        v(off), st), 'yk_jpeg_encode_ragged_u8')
    torch.cuda.synchronize()
    issue()                                                            # eagerly once: a capture records, it does not load kernels
    stream.synchronize()
    out.fill_(SENTINEL)
    off.zero_()
    torch.cuda.synchronize()
    graph = engine.capture(st, issue)
    try:
        stream.synchronize()
        assert (out == SENTINEL).all().item() and not off.any().item()      # recorded, not executed
        for k, (content, ref_pics) in enumerate(((flat, None), (flat2, other), (flat, None))):
            d_packed.copy_(torch.from_numpy(content))
            torch.cuda.synchronize()
            graph.launch(st)
            stream.synchronize()
            scans = [jpeg_ref.encode_cached(i, 75)[0] for i in idx] if ref_pics is None else [jpeg_ref.encode(p, 75)[0] for p in ref_pics]
            got_off, got = off.cpu().numpy(), out.cpu().numpy()
            assert np.array_equal(got_off, np.cumsum([0] + [len(s) for s in scans])), (k, got_off)
            for i, s in enumerate(scans):
                assert got[got_off[i]:got_off[i + 1]].tobytes() == s, (k, i)
    finally:
        graph.close()


def test_detect_encode_gpu_end_to_end(tmp_path):
    """detect.run(encode='gpu'): every file is headers + the reference's scan of the annotated array + EOI, the detections do not depend on
    who encodes, encode='pil' still writes PIL's bytes, and the CLI passes --encode / --quality through."""
    from PIL import Image
    from k210_yolo_framework_amd import detect, keras_io
    from k210_yolo_framework_amd.yolonet import MODEL_DEFS
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    ck = tmp_path / 'yolo_model.h5'
    keras_io.save_keras_weights(spec, spec.init_weights(seed=1), ck)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    model, _ = MODEL_DEFS['yolo_mobilev1']([224, 320, 3], 3, 20, alpha=0.75, precision='f16x2')
    model.load_weights(str(ck))
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8) for hh, ww in [(120, 160), (97, 131), (64, 200), (120, 160), (33, 47)]]
    kw = dict(draw=True, batch=3, depth=2, obj_thresh=0.6, iou_thresh=0.5, return_arrays=True, verbose=False)
    g = detect.run(h, model, imgs, out_dir=tmp_path / 'gpu', encode='gpu', quality=75, **kw)
    p = detect.run(h, model, imgs, out_dir=tmp_path / 'pil', encode='pil', **kw)
    assert sum(len(d) for d in g['detections']) > 0                                     # boxes were drawn
    assert len(g['files']) == len(p['files']) == len(imgs)
    qt = jpeg.quant_tables(75)
    for i, im in enumerate(imgs):
        assert np.array_equal(g['detections'][i], p['detections'][i]) and np.array_equal(g['arrays'][i], p['arrays'][i])
        arr = g['arrays'][i]
        data = open(g['files'][i], 'rb').read()
        assert data == jpeg.assemble(arr.shape[0], arr.shape[1], qt, jpeg_ref.encode(arr, 75)[0]), i
        pic = Image.open(io.BytesIO(data))
        pic.load()
        assert pic.size == (im.shape[1], im.shape[0])
        b = io.BytesIO()
        Image.fromarray(p['arrays'][i]).save(b, 'JPEG')
        assert open(p['files'][i], 'rb').read() == b.getvalue()
    assert any(not np.array_equal(a, im) for a, im in zip(g['arrays'], imgs))
    # without return_arrays the uncompressed pictures stay on the device; the files are the same
    g2 = detect.run(h, model, imgs, out_dir=tmp_path / 'gpu2', encode='gpu', quality=75, **{**kw, 'return_arrays': False})
    assert 'arrays' not in g2
    for a, b in zip(g['files'], g2['files']):
        assert open(a, 'rb').read() == open(b, 'rb').read()
    # the CLI
    folder = tmp_path / 'pics'
    folder.mkdir()
    for i, im in enumerate(imgs[:2]):
        Image.fromarray(im).save(folder / f'pic{i}.png')
    res = detect.cli([str(ck), str(folder), '--out_dir', str(tmp_path / 'cli'), '--encode', 'gpu', '--quality', '90', '--model_def', 'yolo_mobilev1',
                      '--depth_multiplier', '0.75', '--obj_thresh', '0.6', '--iou_thresh', '0.5', '--batch', '2', '--depth', '1'])
    assert len(res['files']) == 2
    for f in res['files']:
        pic = Image.open(f)
        pic.load()
        q90 = jpeg.quant_tables(90)
        for i in range(2):
            theirs = np.asarray(pic.quantization[i])
            assert np.array_equal(theirs, q90[i]) or np.array_equal(theirs, q90[i][jpeg.ZIGZAG])
    with pytest.raises(SystemExit):
        detect.parse([str(ck), str(folder), '--quality', '0'])

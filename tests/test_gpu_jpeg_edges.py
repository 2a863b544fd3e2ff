"""JPEG encoding on the device past the first 256-wide tile of every loop that carries state (yk_jpeg.hip), bit for bit
against tests/jpeg_ref.py: pictures of 256, 257, 513 and 272 MCUs (the carry of jpeg_offsets_kernel), a stream of more than 256 chunks
(the carry of jpeg_chunk_scan_kernel), 257 and 513 pictures with empty rows on the tile boundary (the base loops and the refusal loops
of jpeg_plan_kernel and jpeg_out_off_kernel), 0xFF bytes at a lane's, a chunk's and a picture's end (jpeg_stuff_kernel), and a workspace
twice as large as needed.  tests/test_jpeg_edge_cases.py proves that the cases are what they claim.  As in tests/test_gpu_jpeg.py every
test checks that nothing at or beyond d_out_off[n] is written and that the source is only read."""
import ctypes as C

import numpy as np
import pytest

from k210_yolo_framework_amd import jpeg
from tests import jpeg_edge_cases as ec
from tests.test_gpu_jpeg import SENTINEL, _encode, _pack

pytestmark = pytest.mark.gpu


def _device(table):
    import torch
    return torch.from_numpy(table.view(np.uint8).reshape(len(table), -1).copy()).cuda()


def _check(off, out, src_after, flat, scans):
    """d_out_off exact, every stream the reference's (an empty one where scans[i] is b''), nothing behind them, the source untouched."""
    n = len(scans)
    assert off.dtype == np.int64 and off.shape == (n + 1,)
    assert np.array_equal(off, np.cumsum([0] + [len(s) for s in scans]))
    want = np.frombuffer(b''.join(scans), np.uint8)
    if not np.array_equal(out[:off[n]], want):
        at = int(np.flatnonzero(out[:off[n]] != want)[0])
        i = int(np.searchsorted(off, at, side='right')) - 1
        raise AssertionError(f'picture {i}: the first wrong byte is byte {at - int(off[i])} of {len(scans[i])}')
    assert (out[off[n]:] == SENTINEL).all()
    assert np.array_equal(src_after, flat)


def _mcu_tile_batch():
    pics = [ec.picture(c) for c in ec.MCU_TILE]
    scans = [ec.encode_cached(c, ec.MCU_TILE_QUALITY)[0] for c in ec.MCU_TILE]
    return pics, scans


def test_pictures_of_more_than_256_mcus():
    pics, scans = _mcu_tile_batch()
    flat, table = _pack(pics)
    off, out, src_after = _encode(flat, table, ec.MCU_TILE_QUALITY)
    _check(off, out, src_after, flat, scans)


def test_a_workspace_and_an_output_twice_as_large_give_the_same_bytes():
    from k210_yolo_framework_amd import engine
    pics, scans = _mcu_tile_batch()
    flat, table = _pack(pics)
    work, cap = engine.jpeg_workspace_bytes(table)
    off, out, src_after = _encode(flat, table, ec.MCU_TILE_QUALITY, sizes=(2 * work, 2 * cap), device_table=_device(table))
    assert len(out) == 2 * cap + 64
    _check(off, out, src_after, flat, scans)


def test_a_stream_of_more_than_256_chunks():
    pics = [ec.picture(('noise', 1, 1)), ec.picture(ec.CHUNK_TILE)]
    scans = [ec.encode_cached(('noise', 1, 1), ec.CHUNK_TILE_QUALITY)[0], ec.encode_cached(ec.CHUNK_TILE, ec.CHUNK_TILE_QUALITY)[0]]
    flat, table = _pack(pics)
    off, out, src_after = _encode(flat, table, ec.CHUNK_TILE_QUALITY)
    _check(off, out, src_after, flat, scans)


@pytest.mark.parametrize('n', [257, 513])
def test_more_than_256_pictures_with_empty_rows_on_the_tile_boundary(n):
    from k210_yolo_framework_amd import engine
    cases = ec.many_cases(n)
    flat, table = _pack([ec.picture(c) for c in cases])
    bad = table.copy()
    for i in ec.MANY_BAD_ROWS:
        bad[i]['h'] = 0
    scans = [b'' if i in ec.MANY_BAD_ROWS else ec.encode_cached(c, ec.MANY_QUALITY)[0] for i, c in enumerate(cases)]
    off, out, src_after = _encode(flat, table, ec.MANY_QUALITY, sizes=engine.jpeg_workspace_bytes(table), device_table=_device(bad))
    assert off[255] == off[256] == off[257] and off[254] < off[255] and (n == 257 or off[257] < off[258])
    _check(off, out, src_after, flat, scans)


def test_257_pictures_a_workspace_or_an_output_for_one_mcu_refuse_every_row():
    """The refusal loops of jpeg_plan_kernel and jpeg_out_off_kernel past their first pass: all 258 offsets are 0, no byte is written."""
    import torch
    from k210_yolo_framework_amd import engine
    n = 257
    flat, table = _pack([ec.picture(c) for c in ec.many_cases(n)])
    sizes = engine.jpeg_workspace_bytes(table)
    one = table.copy()
    one['h'][1:] = 0
    small = engine.jpeg_workspace_bytes(one)                                  # the header of 257 rows and one MCU
    assert small[1] == 2 * 1248 and small[0] < sizes[0]
    d_table, d_packed = _device(table), torch.from_numpy(flat).cuda()
    qtab = torch.from_numpy(jpeg.quant_tables(ec.MANY_QUALITY)).cuda()
    for work_bytes, cap in ((small[0], sizes[1]), (sizes[0], small[1])):
        work = torch.empty(work_bytes, dtype=torch.uint8, device='cuda')
        o = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
        d_off = torch.full((n + 1,), -1, dtype=torch.int64, device='cuda')
        engine._check(engine.lib().yk_jpeg_encode_ragged_u8(C.c_void_p(d_packed.data_ptr()), C.c_size_t(d_packed.numel()),
                                                            C.c_void_p(d_table.data_ptr()), C.c_int(n), C.c_void_p(qtab.data_ptr()),
                                                            C.c_void_p(work.data_ptr()), C.c_size_t(work_bytes), C.c_void_p(o.data_ptr()),
                                                            C.c_size_t(cap), C.c_void_p(d_off.data_ptr()), None), 'yk_jpeg_encode_ragged_u8')
        torch.cuda.synchronize()
        assert d_off.numel() == 258 and not d_off.any().item() and (o == SENTINEL).all().item(), (work_bytes, cap)
        assert np.array_equal(d_packed.cpu().numpy(), flat)


def test_0xff_at_a_lanes_a_chunks_and_a_pictures_end():
    """One batch per quality; the picture whose last byte is 0xFF stands in front of another, whose first byte must follow its 0x00."""
    for q in sorted({q for _, q in ec.STUFF}):
        cases = [c for c, cq in ec.STUFF if cq == q] + [('noise', 1, 1)]
        flat, table = _pack([ec.picture(c) for c in cases])
        off, out, src_after = _encode(flat, table, q)
        _check(off, out, src_after, flat, [ec.encode_cached(c, q)[0] for c in cases])

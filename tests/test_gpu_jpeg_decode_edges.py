"""JPEG decoding on the device past the first 256-wide tile of every loop that carries state (yk_jpeg_dec.hip), byte for
byte against tests/jpeg_dec_ref.py: pictures of 272 and 544 MCUs whose restart intervals end before, on and after MCU 256 (the segmented
scan of jd_dc_kernel and its hand-over from tile to tile), 257 pictures with refused rows on the tile boundary (the carry loop and the
`over` loop of jd_plan_kernel), and the project's own encoder's streams of 257 and 513 MCUs and of more than 256 chunks.
tests/test_jpeg_edge_cases.py proves that the files are what they claim.  Every byte outside the pictures stays the sentinel."""
import numpy as np
import pytest

from k210_yolo_framework_amd import jpeg
from tests import jpeg_dec_ref as ref
from tests import jpeg_edge_cases as ec
from tests.test_gpu_jpeg import _encode, _pack
from tests.test_gpu_jpeg_decode import SENTINEL, _check, _decode

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('group', list(ec.RESTART_GROUPS))
def test_restart_intervals_around_mcu_256(group):
    files = [f for f, _ in ec.restart_files(group)]
    for chunk in (0, 4):
        status, dst, rows = _decode(files, chunk_bytes=chunk)
        _check(files, status, dst, rows)


def test_257_pictures_with_refused_rows_on_the_tile_boundary():
    files = ec.many_files(257)

    def no_scan(buf, pics):
        for i in ec.MANY_BAD_ROWS:
            pics[i]['scan_bytes'] = 0

    status, dst, rows = _decode(files, edit=no_scan)
    assert status.shape == (257,) and all(status[i] != 0 for i in ec.MANY_BAD_ROWS)
    _check(files, status, dst, rows, skip=ec.MANY_BAD_ROWS)                   # the other 255 exact, nothing written for the two


def test_257_pictures_a_workspace_one_block_short_refuses_every_row():
    from k210_yolo_framework_amd import engine
    files = ec.many_files(257)
    parsed = [jpeg.parse_baseline(f) for f in files]
    need = engine.jpeg_decode_workspace_bytes(jpeg.plan_decode(parsed)[1])
    status, dst, _ = _decode(files, parsed=parsed, work_bytes=need - 192)
    assert status.shape == (257,) and (status != 0).all() and (dst == SENTINEL).all()


def test_streams_of_the_projects_own_encoder_across_tiles():
    """The encoder's streams of the 257-MCU black / white picture, the 513-MCU picture and the picture of more than 256 chunks, decoded."""
    files = []
    for cases, q in (([ec.MCU_TILE[ec.MCU_TILE_BW], ec.MCU_TILE[ec.MCU_TILE_513]], ec.MCU_TILE_QUALITY), ([ec.CHUNK_TILE], ec.CHUNK_TILE_QUALITY)):
        pics = [ec.picture(c) for c in cases]
        flat, table = _pack(pics)
        off, out, _ = _encode(flat, table, q)
        qt = jpeg.quant_tables(q)
        for i, (c, p) in enumerate(zip(cases, pics)):
            scan = out[off[i]:off[i + 1]].tobytes()
            assert scan == ec.encode_cached(c, q)[0], c                       # (what tests/test_gpu_jpeg_edges.py pins; here: what is decoded)
            files.append(jpeg.assemble(p.shape[0], p.shape[1], qt, scan))
    status, dst, rows = _decode(files)
    _check(files, status, dst, rows)

"""The cases of tests/jpeg_edge_cases.py are the cases they claim to be, from the references alone: MCU, chunk and picture counts on both
sides of 256, restart intervals before, at and after MCU 256, 0xFF bytes at a lane's end, at a chunk's end and at a picture's end - so that
a later change of a helper cannot turn one of them into an ordinary picture unnoticed.  The reference streams of the large pictures open
in PIL.  DESIGN.md 3.12."""
import io

import numpy as np
import pytest
from PIL import Image, ImageFile, JpegImagePlugin

from k210_yolo_framework_amd import jpeg
from tests import jpeg_edge_cases as ec
from tests import jpeg_ref


def _mcus(case):
    h, w = case[1], case[2]
    return ((h + 15) // 16) * ((w + 15) // 16)


def test_mcu_tile_pictures_cross_the_tile_where_they_say():
    assert ec.TILE == 256 and [_mcus(c) for c in ec.MCU_TILE] == ec.MCU_TILE_MCUS == [1, 256, 257, 257, 513, 272]
    assert [c[1:3] for c in ec.MCU_TILE[1:]] == [(16, 4096), (16, 4112), (16, 4112), (16, 8208), (272, 256)]
    assert ec.MCU_TILE[ec.MCU_TILE_BW][0] == 'bw' and ec.MCU_TILE[ec.MCU_TILE_513][2] == 8208
    assert all(c[0] == 'noise' for i, c in enumerate(ec.MCU_TILE) if i != ec.MCU_TILE_BW) and ec.MCU_TILE_QUALITY == 75
    starts = np.cumsum([0] + ec.MCU_TILE_MCUS)
    assert all(int(s) % ec.TILE for s in starts[1:])                       # no picture begins on a tile boundary of the global MCU index
    for case, mcus in zip(ec.MCU_TILE, ec.MCU_TILE_MCUS):
        st = ec.encode_cached(case, ec.MCU_TILE_QUALITY)[1]
        assert st['blocks'] == 6 * mcus
    # the black / white picture: every MCU is one cell, so the luma DC jumps by the largest difference at every MCU boundary, 255 | 256 too
    y = jpeg_ref.planes(ec.picture(ec.MCU_TILE[ec.MCU_TILE_BW]))[0]
    dc = jpeg_ref.block_coefficients(y, jpeg.quant_tables(ec.MCU_TILE_QUALITY)[0])[0][..., 0]
    assert dc.shape == (2, 514)
    step = np.abs(np.diff(dc[0, ::2]))                                      # from an MCU (flat: its four blocks are equal) to the next
    assert len(step) == 256 and step.min() == step.max() > 200 and step[255] == step.max()


def test_chunk_tile_picture_is_the_smallest_square_with_more_than_256_chunks():
    st = ec.encode_cached(ec.CHUNK_TILE, ec.CHUNK_TILE_QUALITY)[1]
    assert st['unstuffed_bytes'] > 256 * 1248 and jpeg_ref.CHUNK_BYTES == 1248
    assert st['unstuffed_bytes'] == (st['bits'] + 7) // 8 and _mcus(ec.CHUNK_TILE) > ec.TILE
    h, w = ec.CHUNK_TILE[1:3]
    assert h == w and h % 16 == 0 and ec.CHUNK_TILE_BELOW[1:3] == (h - 16, w - 16) and ec.CHUNK_TILE_BELOW[0] == ec.CHUNK_TILE[0] == 'noise'
    below = jpeg_ref.encode(ec.picture(ec.CHUNK_TILE_BELOW), ec.CHUNK_TILE_QUALITY)[1]
    assert below['unstuffed_bytes'] <= 256 * 1248                           # noise streams grow with the area: no smaller square reaches it
    assert st['ff_at_lane_end'] > 0 and st['stuffed'] > 256                 # 0xFF bytes on both sides of chunk 256
    assert (st['ff_positions'] >= 256 * 1248).any()


def test_many_pictures_cycle_sizes_and_kinds_across_the_tile():
    for n in (257, 513):
        cases = ec.many_cases(n)
        assert len(cases) == n > ec.TILE and {c[1:] for c in cases} == set(ec.MANY_SIZES) and {c[0] for c in cases} == set(jpeg_ref.KINDS)
        assert len(set(cases)) == 20
    assert ec.MANY_SIZES == [(1, 1), (8, 8), (17, 9), (9, 17)] and ec.MANY_BAD_ROWS == (255, 256)
    cases = ec.many_cases(257)
    assert sum(_mcus(c) for c in cases) > 257                               # a workspace for one MCU does not hold them,
    assert sum(len(ec.encode_cached(c, ec.MANY_QUALITY)[0]) for c in cases) > 2 * 1248                # nor an output for one their streams
    assert all(len(ec.encode_cached(cases[i], ec.MANY_QUALITY)[0]) > 0 for i in (254, 255, 256))      # the rows around the boundary have streams


def test_stuffing_cases_have_their_0xff_where_they_say():
    lane = ec.encode_cached(*ec.STUFF_LANE_END)[1]
    assert lane['ff_at_lane_end'] > 0
    p = lane['ff_positions']
    assert (p % 1248 % 20 == 19).sum() == lane['ff_at_lane_end']
    chunk = ec.encode_cached(*ec.STUFF_CHUNK_END)[1]
    p = chunk['ff_positions']
    at_end = p[p % 1248 == 1247]
    assert chunk['ff_at_chunk_end'] == len(at_end) > 0 and (at_end < chunk['unstuffed_bytes'] - 1).any()        # more data follows in the picture
    for case in (ec.STUFF_LAST_BYTE, ec.STUFF_LAST_BYTE_Q75):
        scan, last = ec.encode_cached(*case)
        assert last['last_byte_ff'] and last['bits'] % 8 != 0 and scan.endswith(b'\xff\x00')
        assert last['ff_positions'][-1] == last['unstuffed_bytes'] - 1
    for case, q in ec.STUFF:
        scan, st = ec.encode_cached(case, q)
        assert case[0] == 'noise' and len(case) == 4                        # seeded noise
        assert len(scan) == st['unstuffed_bytes'] + st['stuffed'] and st['stuffed'] == len(st['ff_positions'])
        assert scan.replace(b'\xff\x00', b'\xff').count(b'\xff') == st['stuffed']


def test_stats_of_a_literal_stream():
    """stuffing_positions on bytes laid out by hand."""
    raw = bytearray(2 * 1248 + 20)
    for at in (19, 20, 1247, 1248 + 39, 2 * 1248 + 19):
        raw[at] = 0xFF
    st = jpeg_ref.stuffing_positions(bytes(raw))
    assert st['unstuffed_bytes'] == 2516 and st['ff_positions'].tolist() == [19, 20, 1247, 1287, 2515]
    assert st['ff_at_lane_end'] == 3 and st['ff_at_chunk_end'] == 1 and st['last_byte_ff'] is True       # (1247 % 20 = 7: lanes end at 19, 39, ...)
    assert jpeg_ref.stuffing_positions(b'\x00')['last_byte_ff'] is False and jpeg_ref.stuffing_positions(b'')['last_byte_ff'] is False


@pytest.mark.parametrize('group', list(ec.RESTART_GROUPS))
def test_restart_files_have_the_intervals_and_mcu_counts(group):
    h, w, layout, mcus, intervals = ec.RESTART_GROUPS[group]
    files = ec.restart_files(group)
    assert len(files) == 2 * len(intervals) and mcus > ec.TILE
    for data, want in files:
        p = jpeg.parse_baseline(data)
        assert (p.h, p.w) == (h, w) and p.restart == want and p.mcus[0] * p.mcus[1] == mcus
        assert p.ncomp == (1 if layout.get('mode') == 'L' else 3) and (p.hs, p.vs) == ((2, 2) if layout.get('subsampling') == 2 else (1, 1))
        markers = sum(p.scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8))
        assert markers == ((mcus + want - 1) // want - 1 if want else 0)
    wants = sorted({want for _, want in files})
    assert wants == {'rgb444_272': [1, 7, 16, 255, 256, 257], 'grey_272': [7, 256], 'rgb420_272': [7, 256], 'rgb444_544': [0, 100]}[group]
    assert len({data for data, _ in files}) == len(files)                   # noise and smooth, every interval: all different
    # an interval that straddles MCU 256, one that begins on it, one that ends on it (255: MCU 255 begins one)
    if group == 'rgb444_272':
        assert 256 % 7 != 0 and 256 % 256 == 0 and 255 % 255 == 0 and 256 % 257 != 0 and 257 < mcus


def test_many_files_cycle_layouts_and_sizes():
    files = ec.many_files(257)
    parsed = [jpeg.parse_baseline(f) for f in files]
    assert len(files) == 257 and len(set(files)) == 12
    assert {(p.h, p.w) for p in parsed} == {(1, 1), (9, 9), (17, 33)}
    assert {(p.ncomp, p.hs, p.vs) for p in parsed} == {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)}
    assert sum(p.mcus[0] * p.mcus[1] * p.blocks_per_mcu for p in parsed[:255]) > 0


def test_large_reference_streams_open_in_pil():
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    for case, q in [(c, ec.MCU_TILE_QUALITY) for c in ec.MCU_TILE] + [(ec.CHUNK_TILE, ec.CHUNK_TILE_QUALITY)]:
        h, w = case[1:3]
        scan, _ = ec.encode_cached(case, q)
        data = jpeg.assemble(h, w, jpeg.quant_tables(q), scan)
        im = Image.open(io.BytesIO(data))
        assert im.format == 'JPEG' and im.mode == 'RGB' and im.size == (w, h), case
        assert JpegImagePlugin.get_sampling(im) == 2
        im.load()
        if h * w > 1:
            with pytest.raises(OSError):
                Image.open(io.BytesIO(data[:-3])).load()                    # no missing bytes: cut short it no longer loads

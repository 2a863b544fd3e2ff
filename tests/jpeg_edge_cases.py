"""The pictures, files and seeds that take the JPEG kernels past the first 256-wide tile of every loop that carries state from one tile to
the next: MCUs, chunks and pictures of the encoder, MCUs with restart intervals and pictures of the decoder, and 0xFF
bytes at the places where the stuffing hands over between lanes, chunks and pictures.  Pictures, files and seeds only; the reference
results are computed once per session.  tests/test_jpeg_edge_cases.py proves from the references that every case is what it claims."""
from tests import jpeg_dec_ref, jpeg_ref

TILE = 256                                  # MCUs, chunks or pictures per pass of the scanning kernels

_enc, _file = {}, {}


def picture(case):
    """case = (kind, h, w) or (kind, h, w, seed) of jpeg_ref.picture"""
    return jpeg_ref.picture(*case)


def encode_cached(case, quality):
    """jpeg_ref.encode(picture(case), quality), computed once per session."""
    key = (tuple(case), quality)
    if key not in _enc:
        _enc[key] = jpeg_ref.encode(picture(case), quality)
    return _enc[key]


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
# MCU tiles: 256, 257 and 513 MCUs in one MCU row, 272 in 17 rows; the black / white cells put the largest DC differences on every MCU
# boundary, the tile's among them.  The 1 x 1 picture in front keeps picture and tile boundaries apart in the global MCU index.
MCU_TILE_QUALITY = 75
MCU_TILE = [('noise', 1, 1), ('noise', 16, 4096), ('noise', 16, 4112), ('bw', 16, 4112), ('noise', 16, 8208), ('noise', 272, 256)]
MCU_TILE_MCUS = [1, 256, 257, 257, 513, 272]
MCU_TILE_BW, MCU_TILE_513 = 3, 4

# chunk tiles: the smallest square of whole MCUs whose noise at quality 100 fills more than 256 chunks of 1248 unstuffed bytes
CHUNK_TILE_QUALITY = 100
CHUNK_TILE = ('noise', 416, 416)
CHUNK_TILE_BELOW = ('noise', 400, 400)

# more than 256 pictures
MANY_QUALITY = 75
MANY_SIZES = [(1, 1), (8, 8), (17, 9), (9, 17)]
MANY_BAD_ROWS = (255, 256)                  # the last row of the first tile and the first of the second


def many_cases(n):
    """n tiny pictures cycling MANY_SIZES and jpeg_ref.KINDS (4 and 5 are coprime: 20 different pictures)."""
    return [(jpeg_ref.KINDS[i % len(jpeg_ref.KINDS)],) + MANY_SIZES[i % len(MANY_SIZES)] for i in range(n)]


# stuffing positions: (case with its seed, quality), found once by encoding seeds 0, 1, 2, ... of the size with jpeg_ref and taking the
# first hit (8 x 8 at quality 75: the first in 0 .. 2999)
STUFF_LANE_END = (('noise', 17, 9, 2), 100)          # a 0xFF as a lane's last byte
STUFF_CHUNK_END = (('noise', 32, 32, 38), 100)       # a 0xFF as the first chunk's last byte, 758 bytes follow
STUFF_LAST_BYTE = (('noise', 8, 8, 12), 100)         # the picture's last byte is 0xFF after 1-padding: its 0x00 ends the stream
STUFF_LAST_BYTE_Q75 = (('noise', 8, 8, 2264), 75)
STUFF = [STUFF_LANE_END, STUFF_CHUNK_END, STUFF_LAST_BYTE, STUFF_LAST_BYTE_Q75]


# ---- decoder ------------------------------------------------------------------------------------------------------------------------
# PIL files with more than 256 MCUs and restart intervals that break before, at and after MCU 256: group -> (h, w, pil_file keywords,
# MCUs, [(restart keywords, the interval parse_baseline must report)])
RESTART_QUALITY = 90
RESTART_GROUPS = {
    'rgb444_272': (136, 128, dict(subsampling=0), 272,
                   [(dict(restart_marker_blocks=k), k) for k in (1, 7, 255, 256, 257)] + [(dict(restart_marker_rows=1), 16)]),
    'grey_272': (136, 128, dict(mode='L'), 272, [(dict(restart_marker_blocks=k), k) for k in (7, 256)]),
    'rgb420_272': (272, 256, dict(subsampling=2), 272, [(dict(restart_marker_blocks=k), k) for k in (7, 256)]),
    'rgb444_544': (136, 256, dict(subsampling=0), 544, [(dict(), 0), (dict(restart_marker_blocks=100), 100)]),
}
RESTART_CONTENT = {'noise': jpeg_dec_ref.noise, 'smooth': jpeg_dec_ref.smooth}


def restart_files(group):
    """-> [(file bytes, the restart interval it must have)] of a group, noise and smooth content for every interval."""
    h, w, layout, _, intervals = RESTART_GROUPS[group]
    out = []
    for kw, want in intervals:
        for name, make in RESTART_CONTENT.items():
            key = (group, want, name)
            if key not in _file:
                _file[key] = jpeg_dec_ref.pil_file(make(h, w), quality=RESTART_QUALITY, **layout, **kw)
            out.append((_file[key], want))
    return out


MANY_FILE_SIZES = [(1, 1), (9, 9), (17, 33)]


def many_files(n=257):
    """n tiny files cycling the four layouts and MANY_FILE_SIZES (12 different files)."""
    out = []
    for i in range(n):
        key = ('many', i % 4, i % 3)
        if key not in _file:
            _file[key] = jpeg_dec_ref.pil_file(jpeg_dec_ref.noise(*MANY_FILE_SIZES[i % 3]), quality=75, **jpeg_dec_ref.layout_kw(jpeg_dec_ref.LAYOUTS[i % 4]))
        out.append(_file[key])
    return out

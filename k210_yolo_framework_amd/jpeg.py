"""Host side of the GPU JPEG encoder (yk_jpeg_encode_ragged_u8): the standard tables of ITU-T T.81 Annex K as data, the
IJG quality rule, and the JFIF container around the entropy-coded scan the device produces.  Baseline sequential, 8 bit, YCbCr 4:2:0,
interleaved scan, Annex-K Huffman tables, no restart markers: structurally what PIL's default save() writes.
Host side of the GPU JPEG decoder (yk_jpeg_decode_ragged_u8): parse_baseline reads a file or refuses it by name (Unsupported), and
plan_decode packs the accepted files of a batch into the scan buffer, the yk_jpeg_pic_t table and the decode-ready tables the device
call takes."""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np

# T.81 Annex K.1, natural (row-major) order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)

# ZIGZAG[k] = natural index of the k-th coefficient in zigzag order (T.81 figure A.6)
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63], np.int64)

# T.81 Annex K.3: BITS (codes of length 1 .. 16) and HUFFVAL
DC_LUMA_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_LUMA_VALS = tuple(range(12))
DC_CHROMA_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC_CHROMA_VALS = tuple(range(12))
AC_LUMA_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)
AC_LUMA_VALS = (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa)
AC_CHROMA_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
AC_CHROMA_VALS = (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa)
assert sum(AC_LUMA_BITS) == len(AC_LUMA_VALS) == 162 and sum(AC_CHROMA_BITS) == len(AC_CHROMA_VALS) == 162

# the DHT segments in the order they are written: (class << 4 | id, BITS, HUFFVAL)
HUFFMAN_TABLES = ((0x00, DC_LUMA_BITS, DC_LUMA_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                  (0x01, DC_CHROMA_BITS, DC_CHROMA_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS))


def huffman_codes(bits, vals) -> Tuple[np.ndarray, np.ndarray]:
    """T.81 Annex C: -> (code [256], length [256]) indexed by symbol; length 0 = the table has no such symbol."""
    code = np.zeros(256, np.int64)
    length = np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, length


def dct_table() -> np.ndarray:
    """T[u][x] = rint(2^13 a(u) cos((2x+1) u pi / 16)), a(0) = sqrt(1/8), a(u>0) = 1/2: int32 [8, 8], evaluated in float64."""
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    a = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(8192.0 * a * np.cos((2.0 * x + 1.0) * u * np.pi / 16.0)).astype(np.int32)


def quant_tables(quality: int = 75) -> np.ndarray:
    """The Annex K.1 tables scaled by the IJG rule, in integers: uint8 [2, 64] (luminance, chrominance), natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f'jpeg quality {quality}: expected 1 .. 100')
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)]).astype(np.uint8)


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def headers(h: int, w: int, qtabs) -> bytes:
    """SOI, APP0 JFIF 1.01, two DQT, SOF0 (2x2 / 1x1 / 1x1), four DHT, SOS: everything in front of the scan data."""
    h, w = int(h), int(w)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f'jpeg: a {h} x {w} picture does not fit the frame header')
    qt = np.asarray(qtabs)
    if qt.shape != (2, 64) or qt.min() < 1 or qt.max() > 255:
        raise ValueError('jpeg: qtabs is [2, 64] of 1 .. 255 in natural order')
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    for i in range(2):
        out.append(_segment(0xDB, bytes([i]) + bytes(int(v) for v in qt[i][ZIGZAG])))
    out.append(_segment(0xC0, struct.pack('>BHHB', 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, bits, vals in HUFFMAN_TABLES:
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b''.join(out)


def assemble(h: int, w: int, qtabs, scan_bytes) -> bytes:
    """A complete JFIF file: headers, the entropy-coded scan (already byte-stuffed and padded), EOI."""
    return headers(h, w, qtabs) + bytes(scan_bytes) + b'\xff\xd9'


# ---- decoding: parse, refuse by name, plan (yk_jpeg_decode_ragged_u8) ------------------------------------------------
class Unsupported(Exception):
    """A file the GPU decoder does not take; .reason says why.  Never an error of a run: detect.run decodes such a picture with PIL."""

    def __init__(self, reason: str):
        super().__init__(reason)
        self.reason = reason


@dataclass
class Baseline:
    """What parse_baseline found: sizes, layout, the tables the scan selects and the entropy-coded segment itself."""
    h: int
    w: int
    ncomp: int                      # 1 (grey) or 3 (YCbCr)
    hs: int                         # luma sampling factors; chroma is 1 x 1
    vs: int
    restart: int                    # MCUs per restart interval, 0 = none
    tq: Tuple[int, ...]             # per component: quantisation table id, DC and AC Huffman table id
    td: Tuple[int, ...]
    ta: Tuple[int, ...]
    qtabs: Dict[int, np.ndarray]    # id -> uint8 [64], natural order
    dc: Dict[int, Tuple[bytes, bytes]]      # id -> (BITS [16], HUFFVAL)
    ac: Dict[int, Tuple[bytes, bytes]]
    scan: bytes                     # after the SOS header up to, not including, EOI: stuffing and RSTn left in place

    @property
    def blocks_per_mcu(self) -> int:
        return self.hs * self.vs + (2 if self.ncomp == 3 else 0)

    @property
    def mcus(self) -> Tuple[int, int]:
        return (self.h + 8 * self.vs - 1) // (8 * self.vs), (self.w + 8 * self.hs - 1) // (8 * self.hs)


_SOF_NAMES = {0xC1: 'extended sequential (SOF1)', 0xC2: 'progressive (SOF2)', 0xC3: 'lossless (SOF3)', 0xC5: 'differential sequential (SOF5)',
              0xC6: 'differential progressive (SOF6)', 0xC7: 'differential lossless (SOF7)', 0xC9: 'arithmetic coding (SOF9)',
              0xCA: 'arithmetic coding (SOF10)', 0xCB: 'arithmetic coding (SOF11)', 0xCD: 'arithmetic coding (SOF13)',
              0xCE: 'arithmetic coding (SOF14)', 0xCF: 'arithmetic coding (SOF15)'}


def parse_baseline(data) -> Baseline:
    """A baseline JFIF / JPEG file -> Baseline, or Unsupported(reason).  Accepted: SOF0, 8 bit, one component or three with luma sampling
    1x1 / 2x1 / 2x2 and chroma 1x1, one interleaved scan (Ss 0, Se 63, Ah = Al = 0), 8-bit quantisation tables, at most two DC and two AC
    Huffman tables, DRI with any interval; APPn / COM are skipped; three components are YCbCr (an Adobe APP14 must say transform 1)."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b'\xff\xd8':
        raise Unsupported('not a JPEG file (no SOI)')
    qtabs, dc, ac = {}, {}, {}
    frame = adobe = None
    restart = 0
    pos = 2
    while True:
        if pos + 4 > n:
            raise Unsupported('no SOS: the file ends inside its headers')
        if data[pos] != 0xFF:
            raise Unsupported(f'no marker at byte {pos}')
        m = data[pos + 1]
        if m == 0xFF:                                       # fill byte
            pos += 1
            continue
        if m == 0xD9:
            raise Unsupported('no SOS: EOI before any scan')
        if m == 0x01 or 0xD0 <= m <= 0xD7:                  # stand-alone markers
            pos += 2
            continue
        ln = struct.unpack_from('>H', data, pos + 2)[0]
        body = data[pos + 4:pos + 2 + ln]
        if ln < 2 or pos + 2 + ln > n:
            raise Unsupported('no SOS: a header segment is cut')
        pos += 2 + ln
        if m == 0xC0:
            if frame is not None:
                raise Unsupported('more than one frame header')
            if len(body) < 6:
                raise Unsupported('a short frame header')
            prec, fh, fw, nc = struct.unpack_from('>BHHB', body)
            if prec != 8:
                raise Unsupported(f'{prec}-bit samples')
            if nc == 4:
                raise Unsupported('four components (CMYK / YCCK)')
            if nc not in (1, 3):
                raise Unsupported(f'{nc} components')
            if fh == 0 or fw == 0:
                raise Unsupported('a dimension of 0' + (' (the height is left to DNL)' if fh == 0 else ''))
            if len(body) != 6 + 3 * nc:
                raise Unsupported('a frame header of the wrong length')
            frame = (fh, fw, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)])
        elif m in _SOF_NAMES:
            raise Unsupported(_SOF_NAMES[m])
        elif m == 0xC8:
            raise Unsupported('reserved frame type (JPG)')
        elif m == 0xCC:
            raise Unsupported('arithmetic coding (DAC)')
        elif m == 0xDC:
            raise Unsupported('DNL')
        elif m == 0xDB:
            i = 0
            while i < len(body):
                pq, tq = body[i] >> 4, body[i] & 15
                if pq != 0:
                    raise Unsupported('16-bit quantisation table')
                if tq > 3 or i + 65 > len(body):
                    raise Unsupported('a malformed DQT')
                t = np.zeros(64, np.uint8)
                t[ZIGZAG] = np.frombuffer(body, np.uint8, 64, i + 1)
                qtabs[tq] = t
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(body):
                if i + 17 > len(body):
                    raise Unsupported('a malformed DHT')
                tc, th = body[i] >> 4, body[i] & 15
                bits = body[i + 1:i + 17]
                cnt = sum(bits)
                if tc > 1 or th > 1:
                    raise Unsupported(f'Huffman table class {tc} id {th}: baseline has two DC and two AC tables')
                if cnt > 256 or i + 17 + cnt > len(body):
                    raise Unsupported('a malformed DHT')
                code = 0
                for ln_ in range(16):                       # Kraft: codes of every length fit, the all-ones code stays free
                    if code + bits[ln_] > (2 << ln_):
                        raise Unsupported('a Huffman table whose BITS over-subscribe the code space')
                    code = (code + bits[ln_]) << 1
                (dc if tc == 0 else ac)[th] = (bytes(bits), bytes(body[i + 17:i + 17 + cnt]))
                i += 17 + cnt
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported('a malformed DRI')
            restart = struct.unpack('>H', body)[0]
        elif m == 0xEE:
            if body[:5] == b'Adobe' and len(body) >= 12:
                adobe = body[11]                            # judged once the frame header says how many components
        elif m == 0xDA:
            sos = body
            break
        # APPn, COM and anything else with a length: skipped
    if frame is None:
        raise Unsupported('SOS before a frame header')
    fh, fw, comps = frame
    nc = len(comps)
    if adobe is not None and adobe != 1 and nc == 3:
        raise Unsupported(f'Adobe APP14 transform {adobe} (the components are not YCbCr)')
    if len(sos) != 4 + 2 * nc or sos[0] != nc:
        raise Unsupported('more than one scan (the first does not hold every component)')
    if sos[1 + 2 * nc] != 0 or sos[2 + 2 * nc] != 63 or sos[3 + 2 * nc] != 0:
        raise Unsupported('a scan that is not Ss 0, Se 63, Ah = Al = 0')
    hs, vs = comps[0][1], comps[0][2]
    if nc == 1:
        hs = vs = 1                                         # a single component is never interleaved: its factors do not matter
    elif (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1] != 1 or c[2] != 1 for c in comps[1:]):
        raise Unsupported('sampling factors ' + ', '.join(f'{c[1]}x{c[2]}' for c in comps))
    tq, td, ta = [], [], []
    for i, c in enumerate(comps):
        if sos[1 + 2 * i] != c[0]:
            raise Unsupported('scan components in another order than the frame')
        d, a = sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15
        if c[3] not in qtabs or d not in dc or a not in ac:
            raise Unsupported('a table the scan selects is not defined')
        tq.append(c[3]), td.append(d), ta.append(a)
    # the entropy-coded segment: up to EOI; RSTn and stuffing stay, any other marker ends the support
    start = pos
    at = start
    while True:
        at = data.find(b'\xff', at)
        if at < 0 or at + 1 >= n:
            raise Unsupported('no EOI: the file is cut inside its scan')
        m = data[at + 1]
        if m == 0x00 or 0xD0 <= m <= 0xD7:
            at += 2
        elif m == 0xFF:
            at += 1
        elif m == 0xD9:
            break
        elif m == 0xDC:
            raise Unsupported('DNL')
        elif m in (0xDA, 0xC4, 0xDB, 0xDD):
            raise Unsupported('more than one scan')
        else:
            raise Unsupported(f'marker 0x{m:02X} inside the scan')
    if at - start >= 1 << 28:
        raise Unsupported('a scan of 256 MiB or more')
    return Baseline(fh, fw, nc, hs, vs, restart, tuple(tq), tuple(td), tuple(ta), {k: qtabs[k] for k in set(tq)}, dict(dc), dict(ac),
                    data[start:at])


# yk_jpeg_pic_t
PIC_DTYPE = np.dtype([('scan_offset', '<u8'), ('scan_bytes', '<u4'), ('table_offset', '<u4'), ('h', '<i4'), ('w', '<i4'), ('ncomp', '<i4'),
                      ('hs', '<i4'), ('vs', '<i4'), ('restart', '<i4'), ('tq', 'u1', 4), ('td', 'u1', 4), ('ta', 'u1', 4), ('reserved', '<u4')])
assert PIC_DTYPE.itemsize == 56
HUFF_TABLE_BYTES = 896              # look u16 [256], maxcode i32 [16], delta i32 [16], vals u8 [256]
PIC_TABLE_BYTES = 256 + 4 * HUFF_TABLE_BYTES       # q u8 [4][64] natural order, then DC0 DC1 AC0 AC1
SCAN_PAD = 8                        # zero bytes after every segment


def decode_table(bits, vals) -> np.ndarray:
    """BITS / HUFFVAL -> the decode-ready form of include/yolo_hip.h, uint8 [896]: look[c] = length << 8 | symbol for the code of at most 8
    bits that the 8 bits c begin with (0: none); for the lengths l = 1 .. 16 maxcode[l - 1] = the largest code of that length (-1: none)
    and delta[l - 1] = index of its first value - its first code (T.81 F.2.2.3's VALPTR - MINCODE); vals = HUFFVAL."""
    look = np.zeros(256, '<u2')
    maxcode = np.full(16, -1, '<i4')
    delta = np.zeros(16, '<i4')
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = np.frombuffer(bytes(vals), np.uint8)
    code, k = 0, 0
    for ln in range(1, 17):
        cnt = bits[ln - 1]
        if cnt:
            delta[ln - 1] = k - code
            for _ in range(cnt):
                if ln <= 8:
                    look[code << (8 - ln):(code + 1) << (8 - ln)] = (ln << 8) | int(v[k])
                code += 1
                k += 1
            maxcode[ln - 1] = code - 1
        code <<= 1
    return np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), delta.view(np.uint8), v])


def plan_decode(pics: Sequence[Baseline], out=None):
    """The accepted files of a batch -> (buf, pic table [n] of PIC_DTYPE, scan_bytes, table_bytes): buf uint8 holds the packed scans (each
    segment 4-byte aligned and followed by at least SCAN_PAD zero bytes) in buf[:scan_bytes] and the per-picture tables in
    buf[scan_bytes:scan_bytes + table_bytes]; one copy takes both to the device.  out: a uint8 array to fill (grown by the caller)."""
    t = np.zeros(len(pics), PIC_DTYPE)
    off = 0
    for i, p in enumerate(pics):
        t[i]['scan_offset'], t[i]['scan_bytes'], t[i]['table_offset'] = off, len(p.scan), i * PIC_TABLE_BYTES
        t[i]['h'], t[i]['w'], t[i]['ncomp'], t[i]['hs'], t[i]['vs'], t[i]['restart'] = p.h, p.w, p.ncomp, p.hs, p.vs, p.restart
        t[i]['tq'][:p.ncomp], t[i]['td'][:p.ncomp], t[i]['ta'][:p.ncomp] = p.tq, p.td, p.ta
        off += (len(p.scan) + SCAN_PAD + 3) // 4 * 4
    scan_bytes, table_bytes = off, len(pics) * PIC_TABLE_BYTES
    if out is None:
        out = np.zeros(scan_bytes + table_bytes, np.uint8)
    if out.dtype != np.uint8 or out.ndim != 1 or out.size < scan_bytes + table_bytes:
        raise ValueError(f'plan_decode: out must be a 1-d uint8 array of at least {scan_bytes + table_bytes} bytes')
    out[:scan_bytes + table_bytes] = 0
    for i, p in enumerate(pics):
        o = int(t[i]['scan_offset'])
        out[o:o + len(p.scan)] = np.frombuffer(p.scan, np.uint8)
        o = scan_bytes + i * PIC_TABLE_BYTES
        for k, q in p.qtabs.items():
            out[o + 64 * k:o + 64 * k + 64] = q
        for base, tabs in ((256, p.dc), (256 + 2 * HUFF_TABLE_BYTES, p.ac)):
            for k, (bits, vals) in tabs.items():
                out[o + base + k * HUFF_TABLE_BYTES:o + base + (k + 1) * HUFF_TABLE_BYTES] = decode_table(bits, vals)
    return out, t, scan_bytes, table_bytes


def idct_table() -> np.ndarray:
    """The decoder's T[u][x] = rint(2^13 a(u) cos((2x+1) u pi / 16)) (float64): int32 [8, 8]; used transposed, columns then rows."""
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    a = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(8192.0 * a * np.cos((2.0 * x + 1.0) * u * np.pi / 16.0)).astype(np.int32)


# colour: rint(c * 2^16) of 1.40200, 0.34414, 0.71414, 1.77200
COLOUR = (91881, 22554, 46802, 116130)
assert COLOUR == tuple(int(np.rint(c * 65536.0)) for c in (1.402, 0.34414, 0.71414, 1.772))

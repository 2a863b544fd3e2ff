"""Host side of the GPU JPEG encoder (yk_jpeg_encode_ragged_u8): the standard tables of ITU-T T.81 Annex K as data, the
IJG quality rule, and the JFIF container around the entropy-coded scan the device produces.  Baseline sequential, 8 bit, YCbCr 4:2:0,
interleaved scan, Annex-K Huffman tables, no restart markers: structurally what PIL's default save() writes."""
from __future__ import annotations

import struct
from typing import Tuple

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

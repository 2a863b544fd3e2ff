"""Host side of drawing on the GPU (yk_draw_dets_u8): the glyph table, the label rule, and the packing of pictures of
different sizes into one buffer with its table (yk_ragged_row_t, include/yolo_hip.h).

The glyphs are this project's own: twelve 8 x 16 cells for "0123456789. ", the digits built from seven two-pixel strokes (the layout of
a seven-segment display), the point a 2 x 2 block on the base line, the space empty.  Columns 0 and 7 and rows 0-1 and 14-15 stay clear,
so neighbouring cells never touch and the label background frames the text."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

GLYPHS = '0123456789. '
GLYPH_H, GLYPH_W = 16, 8
LABEL_LEN = 7                                    # len('{:2d} {:.2f}'.format(c, s)) for c < 100, s < 9.995

# strokes as (y0, y1, x0, x1), half open, in cell pixels
_STROKES = {'a': (2, 4, 1, 7), 'g': (7, 9, 1, 7), 'd': (12, 14, 1, 7),                      # top, middle, bottom bar
            'f': (2, 9, 1, 3), 'b': (2, 9, 5, 7), 'e': (7, 14, 1, 3), 'c': (7, 14, 5, 7)}   # upper left / right, lower left / right
_DIGITS = ['abcdef', 'bc', 'abged', 'abgcd', 'fgbc', 'afgcd', 'afgedc', 'abc', 'abcdefg', 'abcdfg']
_POINT = (12, 14, 3, 5)


def glyph_atlas() -> np.ndarray:
    """uint8 [12][16][8] of 0 / 1, in the order of GLYPHS."""
    atlas = np.zeros((len(GLYPHS), GLYPH_H, GLYPH_W), np.uint8)
    for d, strokes in enumerate(_DIGITS):
        for s in strokes:
            y0, y1, x0, x1 = _STROKES[s]
            atlas[d, y0:y1, x0:x1] = 1
    y0, y1, x0, x1 = _POINT
    atlas[GLYPHS.index('.'), y0:y1, x0:x1] = 1
    return atlas


def label_glyphs(cls, score) -> List[int]:
    """The 7 glyph indices of '{:2d} {:.2f}'.format(int(cls), score) as the kernel computes them: the score is taken as fp32, its digits are
    rint(double(score) * 100) half to even - an exact product, hence Python's correctly rounded digits for every score in [0, 1].  A class
    >= 100 gives its low two digits, a score >= 10 the low three digits; a negative class counts as 0, a negative or non-finite score as 0."""
    c = float(np.float32(cls))
    c = int(min(c, 1.0e9)) if c >= 0.0 else 0
    s = float(np.float32(score))
    s100 = int(min(float(np.rint(s * 100.0)), 1.0e15)) if 0.0 <= s <= 3.0e38 else 0
    space, point = GLYPHS.index(' '), GLYPHS.index('.')
    return [space if c < 10 else (c // 10) % 10, c % 10, space, (s100 // 100) % 10, point, (s100 // 10) % 10, s100 % 10]


def thickness_of(h: int, w: int) -> int:
    """Rings of box outline for an h x w picture (inference.py / keras_inference.py:141)."""
    return max(1, (int(h) + int(w)) // 300)


def magnification_of(h: int) -> int:
    """Integer glyph magnification: the reference's font size floor(3e-2 * h + 0.5) (keras_inference.py:139) in units of the 16-pixel cell."""
    return max(1, int(math.floor(3e-2 * int(h) + 0.5)) // GLYPH_H)


# yk_ragged_row_t
RAGGED_DTYPE = np.dtype([('offset', '<u8'), ('h', '<i4'), ('w', '<i4'), ('scale', '<f8'), ('tx', '<i4'), ('ty', '<i4'),
                         ('thickness', '<i4'), ('mag', '<i4')])
assert RAGGED_DTYPE.itemsize == 40


def ragged_table(shapes: Sequence[Tuple[int, int]], offsets=None, gap: int = 0) -> np.ndarray:
    """The host table of pictures of `shapes` [(h, w)]: back to back (plus `gap` bytes after each) unless `offsets` says otherwise; outline
    thickness and glyph magnification by the rules above; scale / tx / ty are filled by engine.ragged_table_to_device for a network size."""
    t = np.zeros(len(shapes), RAGGED_DTYPE)
    off = 0
    for i, (h, w) in enumerate(shapes):
        h, w = int(h), int(w)
        t[i]['offset'] = off if offsets is None else int(offsets[i])
        t[i]['h'], t[i]['w'] = h, w
        t[i]['thickness'], t[i]['mag'] = thickness_of(h, w), magnification_of(h)
        off += 3 * h * w + int(gap)
    return t


def packed_bytes(table: np.ndarray) -> int:
    """Bytes of the packed buffer a table addresses."""
    if not len(table):
        return 0
    return int((table['offset'].astype(np.int64) + 3 * table['h'].astype(np.int64) * table['w'].astype(np.int64)).max())


def pack_ragged(images, gap: int = 0, out=None):
    """images: [h_i, w_i, 3] uint8 arrays -> (packed, table, shapes): one uint8 torch buffer holding them back to back (pinned when a GPU is
    visible, so that one asynchronous copy takes it to the device; `out`: a buffer to reuse, grown by the caller), the table, [(h, w)]."""
    import torch
    shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    for im in images:
        if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape[0] <= 0 or im.shape[1] <= 0:
            raise ValueError(f'pack_ragged: every picture is a non-empty [h, w, 3] uint8 array, not {im.dtype} {im.shape}')
    table = ragged_table(shapes, gap=gap)
    total = packed_bytes(table)
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        if gap:
            out.zero_()
    if out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < total:
        raise ValueError(f'pack_ragged: out must be a 1-d uint8 tensor of at least {total} bytes')
    flat = out.numpy()
    for row, im in zip(table, images):
        o, n = int(row['offset']), im.size
        flat[o:o + n] = np.ascontiguousarray(im).reshape(-1)
    return out[:max(total, 1)], table, shapes


def unpack_ragged(flat: np.ndarray, table: np.ndarray) -> List[np.ndarray]:
    """Views [h_i, w_i, 3] of the pictures in a packed host buffer."""
    return [flat[int(r['offset']):int(r['offset']) + 3 * int(r['h']) * int(r['w'])].reshape(int(r['h']), int(r['w']), 3) for r in table]

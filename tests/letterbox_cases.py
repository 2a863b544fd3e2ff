"""The case table, the pictures and the reference for the letterbox arithmetic of csrc/yk_pre.hip (letterbox_px, behind letterbox_u8_kernel,
letterbox_rows_u8_kernel<yk_ragged_row_t>, letterbox_augment_u8_kernel and mosaic_ragged_u8_kernel), shared by tests/test_letterbox_cases.py (CPU: the table
and the reference checked on their own) and tests/test_gpu_letterbox_edges.py (the kernels).  Nothing here touches a GPU.

CASES.  (source h x w -> destination h x w), each with the conditions it is in the table for.  tests/test_letterbox_cases.py asserts every
named condition from taps() below, so a table that drifts fails instead of testing less:
  small       the destination has fewer pixels than one 256-thread workgroup
  one_px      a single output pixel
  line_ty / line_tx   a one-pixel-high / one-pixel-wide source; the translation is on that one axis only
  upscale     scale > 1.6, the largest any other test reaches against something that is not the GPU
  edge_taps   taps at -1 AND at sw or sh in the same picture
  white_254   the constant-255 picture comes out with a 254: (1-d)*255 + d*255 falls an ulp short of 255 and the cast truncates
  dc_half     scale exactly 2: dc == 0 on every even column, 0.5 on every odd one
  dc_zero     scale exactly 0.5: dc == dr == 0 and floor == ceil everywhere
  near_up / near_down   the source is one less / one more than the destination in both dimensions
  sliver      an aspect ratio beyond 90:1
  odd_count   the destination's pixel count is not a multiple of 256

PICTURES.  Per case three contents: seeded noise, a constant 255, and a ramp whose first and last rows and columns are 255, so that a tap
one past the edge (which must read 0) shows.  A batch of three is the named content plus two further noise pictures of the same size.

REFERENCE.  reference() is helper.letterbox_bilinear, which tests/test_oracle_pre.py and tests/test_helper.py hold to real scikit-image outputs
(tests/golden/letterbox_golden.npz) and tests/test_letterbox_cases.py holds to the loop oracle oracle/preprocess_ref.py on this table.
warp_reference() is augment.warp_u8, the second resample of the augment and mosaic kernels as yk_pre.hip states it: c = M00*x + M01*y + M02 and
r likewise, floor / ceil taps, zero outside [0,dh) x [0,dw), min(255, floor((1-dr)*top + dr*bottom + 0.5)), float64 numpy."""
import collections
import functools
import zlib

import numpy as np

from k210_yolo_framework_amd import augment
from k210_yolo_framework_amd.helper import letterbox_bilinear
from oracle import preprocess_ref

Case = collections.namedtuple('Case', 'src dst why')

CASES = (
    Case((1, 1), (7, 5), ('small', 'upscale', 'edge_taps', 'odd_count')),
    Case((1, 1), (1, 1), ('small', 'one_px', 'odd_count')),
    Case((300, 400), (1, 1), ('small', 'one_px', 'odd_count')),
    Case((1, 37), (17, 31), ('line_ty', 'odd_count')),
    Case((37, 1), (17, 31), ('line_tx', 'odd_count')),
    Case((2, 2), (56, 80), ('upscale', 'edge_taps', 'white_254', 'odd_count')),
    Case((3, 5), (64, 48), ('upscale', 'edge_taps', 'white_254')),
    Case((9, 13), (255, 257), ('upscale', 'edge_taps', 'white_254', 'odd_count')),
    Case((29, 41), (58, 82), ('upscale', 'dc_half', 'odd_count')),
    Case((112, 160), (56, 80), ('dc_zero', 'odd_count')),
    Case((55, 79), (56, 80), ('near_up', 'odd_count')),
    Case((57, 81), (56, 80), ('near_down', 'odd_count')),
    Case((640, 7), (56, 80), ('sliver', 'odd_count')),
    Case((4000, 3), (17, 31), ('sliver', 'odd_count')),
    Case((223, 319), (224, 320), ('near_up',)),
    Case((225, 321), (224, 320), ('near_down',)),
)
IDS = tuple(f'{c.src[0]}x{c.src[1]}-{c.dst[0]}x{c.dst[1]}' for c in CASES)
CONTENTS = ('noise', 'white', 'ramp')
MAX_DST = (255, 257)                       # no destination is larger, but for the workload's own
WORKLOAD_DST = (224, 320)


def params(src_hw, dst_hw):
    """(scale, tx, ty) of the plain letterbox, from the oracle."""
    return preprocess_ref.letterbox_params(tuple(src_hw), tuple(dst_hw))


def taps(src_hw, dst_hw, scale=None, tx=None, ty=None):
    """The reference's intermediate values for every destination column and row: c, r, their floor and ceil taps (ints) and dc, dr.  The same
    float64 expressions as helper.letterbox_bilinear; test_taps_rebuild_the_reference ties the two together."""
    if scale is None:
        scale, tx, ty = params(src_hw, dst_hw)
    inv = 1.0 / float(scale)
    c = inv * np.arange(int(dst_hw[1]), dtype=np.float64) + (-(float(tx) * inv))
    r = inv * np.arange(int(dst_hw[0]), dtype=np.float64) + (-(float(ty) * inv))
    T = collections.namedtuple('Taps', 'c r c_lo c_hi r_lo r_hi dc dr')
    return T(c, r, np.floor(c).astype(int), np.ceil(c).astype(int), np.floor(r).astype(int), np.ceil(r).astype(int), c - np.floor(c),
             r - np.floor(r))


def _noise(h, w, variant):
    rng = np.random.default_rng(zlib.crc32(f'letterbox {h}x{w} #{variant}'.encode()))
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def picture(src_hw, content, variant=0):
    """One source picture uint8 [h, w, 3], read-only.  `variant` only tells noise pictures apart."""
    h, w = src_hw
    if content == 'noise':
        img = _noise(h, w, variant)
    elif content == 'white':
        img = np.full((h, w, 3), 255, np.uint8)
    elif content == 'ramp':
        y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
        img = ((7 * y + 3 * x + 50 * ch) % 251).astype(np.uint8)
        img[0], img[-1], img[:, 0], img[:, -1] = 255, 255, 255, 255
    else:
        raise KeyError(content)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def batch(src_hw, content):
    """Three different pictures of one size, uint8 [3, h, w, 3]: the named content (at a position that differs by content, so each content
    is also met behind the first image of a launch) and two more noise pictures."""
    pics = [picture(src_hw, 'noise', 1), picture(src_hw, 'noise', 2)]
    pics.insert(CONTENTS.index(content), picture(src_hw, content))
    out = np.stack(pics)
    out.setflags(write=False)
    return out


def reference(img, dst_hw, scale=None, tx=None, ty=None):
    """The letterboxed picture uint8 [dh, dw, 3]: helper.letterbox_bilinear's bytes.  Without (scale, tx, ty) the plain letterbox of the
    picture's size into dst_hw (oracle.preprocess_ref.letterbox_params); the explicit form is for the rows of a mosaic."""
    if scale is None:
        scale, tx, ty = params(img.shape[:2], dst_hw)
    return letterbox_bilinear(np.asarray(img), (int(dst_hw[0]), int(dst_hw[1])), float(scale), (int(tx), int(ty)))


@functools.lru_cache(maxsize=None)
def expected(src_hw, dst_hw, content, variant=0):
    """reference(picture(...), dst_hw), computed once and read-only."""
    out = reference(picture(src_hw, content, variant), dst_hw)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_batch(src_hw, dst_hw, content):
    out = np.stack([reference(im, dst_hw) for im in batch(src_hw, content)])
    out.setflags(write=False)
    return out


def warp_reference(frame, M):
    """The second resample of yk_letterbox_augment_u8 and yk_mosaic_ragged_u8: the u8 frame [dh, dw, 3] through one inverse map M [2, 3]."""
    return augment.warp_u8(np.asarray(frame), np.asarray(M, np.float64))

"""Camera-motion compensation for the tracker: the statement of the rule that yk_gmc_motion_u8 (csrc/yk_gmc.hip) is held to.

When the camera moves, every box of a frame jumps by the same amount and the tracker's constant-velocity filter cannot have learnt that
velocity; BoT-SORT (N. Aharon, R. Orfaig, B.-Z. Bobrovsky: "BoT-SORT: Robust Associations Multi-Pedestrian Tracking", 2022) calls the remedy
GMC.  THIS IS THE PROJECT'S OWN RULE: block matching on a shrunk grey picture, integers only, so that a kernel can be held to it exactly.
PARITY UNPINNED with BoT-SORT's OpenCV code (sparse optical flow + RANSAC affine).  Two deliberate deviations: the compensation is a
TRANSLATION only, and the previous frame's boxes are NOT masked out - objects that move on their own are outliers, which the median ignores
while they cover less than half of the kept blocks; the mask is later work.

Grey and shrink.  g = (77 R + 150 G + 29 B + 128) >> 8 per pixel; the small picture is H // f x W // f, each pixel the average of an
f x f cell of g as (sum + f * f // 2) // (f * f); partial cells on the right and at the bottom are dropped.  f = scale.
Blocks.  B x B blocks of the PREVIOUS small picture with their top-left corners at (R + i S, R + j S) for every i, j >= 0 at which the
block and its +-R window lie inside the small picture, in row-major (i, j) order.  For each displacement (dy, dx) in [-R, R]^2 the sum of
absolute differences against the CURRENT small picture at (R + i S + dy, R + j S + dx); the block's answer is the displacement of the least
SAD, ties to the smallest |dy| + |dx|, then the smallest dy, then the smallest dx.  A block whose own pixels span less than `texture`
between minimum and maximum is dropped (it is still matched: its row says kept 0).
Motion of a frame.  The lower median (element (n - 1) // 2 of the sorted n) of the kept blocks' dx and of their dy, each on its own, times
f: (mx, my) in source pixels, float32 values that are exact integers - where the picture's content went, so a box centre moves by
(+mx, +my).  Fewer than min_blocks kept blocks, a first frame, or a frame whose size differs from its predecessor's: (0, 0).
numpy only; nothing here touches a GPU."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

DEFAULTS = dict(scale=4, block=16, range=8, step=16, texture=16, min_blocks=8)
MAX_BLOCK, MAX_RANGE = 32, 16             # YK_GMC_MAX_BLOCK, YK_GMC_MAX_RANGE: what the kernel's window in LDS and its packed key hold
MAX_BLOCKS = 8192                         # YK_GMC_MAX_BLOCKS: blocks of one frame the median's LDS holds


def check(scale=4, block=16, range=8, step=16, texture=16, min_blocks=8) -> dict:
    """The options, refused by name -> them as a dict of ints."""
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not (whole(scale) and 1 <= scale <= 64):
        raise ValueError(f'gmc_scale {scale!r}: expected a whole number 1 .. 64')
    if not (whole(block) and 4 <= block <= MAX_BLOCK and block % 4 == 0):
        raise ValueError(f'gmc_block {block!r}: expected a multiple of 4 in 4 .. {MAX_BLOCK}')
    if not (whole(range) and 1 <= range <= MAX_RANGE):
        raise ValueError(f'gmc_range {range!r}: expected a whole number 1 .. {MAX_RANGE}')
    if not (whole(step) and 1 <= step <= 4096):
        raise ValueError(f'gmc_step {step!r}: expected a whole number 1 .. 4096')
    if not (whole(texture) and 0 <= texture <= 256):
        raise ValueError(f'gmc_texture {texture!r}: expected a whole number 0 .. 256')
    if not (whole(min_blocks) and 1 <= min_blocks <= MAX_BLOCKS):
        raise ValueError(f'gmc_min_blocks {min_blocks!r}: expected a whole number 1 .. {MAX_BLOCKS}')
    return dict(scale=int(scale), block=int(block), range=int(range), step=int(step), texture=int(texture), min_blocks=int(min_blocks))


def add_arguments(p) -> None:
    """The command line of the compensation (keras_detect.py)."""
    p.add_argument('--track_gmc', type=str, choices=['True', 'False'], default='False',
                   help='with --track True: estimate the camera translation between frames on the GPU and move the tracks by it (gmc.py)')
    p.add_argument('--gmc_scale', type=int, default=DEFAULTS['scale'], help='the pictures are matched shrunk by this factor')
    p.add_argument('--gmc_block', type=int, default=DEFAULTS['block'], help='side of a matched block in small pixels (a multiple of 4)')
    p.add_argument('--gmc_range', type=int, default=DEFAULTS['range'], help='displacements searched: +- this many small pixels')
    p.add_argument('--gmc_step', type=int, default=DEFAULTS['step'], help='pitch of the blocks in small pixels')
    p.add_argument('--gmc_texture', type=int, default=DEFAULTS['texture'], help='a block whose pixels span less than this is dropped')


def parse_arguments(a) -> None:
    """Checks what add_arguments read (ValueError by name) and leaves a.track_gmc as a bool."""
    a.track_gmc = a.track_gmc == 'True'
    if a.track_gmc:
        if not getattr(a, 'track', False):
            raise ValueError('track_gmc without track: the compensation moves the tracker\'s tracks; add --track True (make detect TRACK=True)')
        check(a.gmc_scale, a.gmc_block, a.gmc_range, a.gmc_step, a.gmc_texture)


def run_options(a) -> dict:
    """The keyword arguments detect.run takes, from parsed arguments."""
    return dict(gmc=a.track_gmc, gmc_scale=a.gmc_scale, gmc_block=a.gmc_block, gmc_range=a.gmc_range, gmc_step=a.gmc_step,
                gmc_texture=a.gmc_texture)


def shrink(img: np.ndarray, scale: int = 4) -> np.ndarray:
    """[H, W, 3] uint8 RGB -> [H // scale, W // scale] uint8."""
    a = np.asarray(img)[..., :3].astype(np.int64)
    g = (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8
    f = int(scale)
    sh, sw = g.shape[0] // f, g.shape[1] // f
    cells = g[:sh * f, :sw * f].reshape(sh, f, sw, f).sum((1, 3))
    return ((cells + f * f // 2) // (f * f)).astype(np.uint8)


def grid(sh: int, sw: int, block: int = 16, range: int = 8, step: int = 16) -> Tuple[int, int]:
    """Blocks down and across a small picture of sh x sw."""
    t = block + 2 * range
    return ((sh - t) // step + 1 if sh >= t else 0), ((sw - t) // step + 1 if sw >= t else 0)


def match_blocks(prev: np.ndarray, cur: np.ndarray, block: int = 16, range: int = 8, step: int = 16, texture: int = 16) -> np.ndarray:
    """Two small pictures of one size -> int32 [blocks, 4]: (dy, dx, sad, kept) per block, row-major."""
    prev, cur = np.asarray(prev).astype(np.int64), np.asarray(cur).astype(np.int64)
    assert prev.shape == cur.shape and prev.ndim == 2
    B, R, S = int(block), int(range), int(step)
    ni, nj = grid(*prev.shape, B, R, S)
    out = np.zeros((ni * nj, 4), np.int32)
    if ni * nj == 0:
        return out
    ys, xs = R + S * np.arange(ni), R + S * np.arange(nj)
    rows = (ys[:, None] + np.arange(B)[None, :]).reshape(-1)                    # [ni * B] picture rows of the blocks, block by block
    cols = (xs[:, None] + np.arange(B)[None, :]).reshape(-1)
    mine = prev[np.ix_(rows, cols)].reshape(ni, B, nj, B)
    best = np.full((ni, nj), np.iinfo(np.int64).max)
    for dy in np.arange(-R, R + 1):
        for dx in np.arange(-R, R + 1):
            sad = np.abs(mine - cur[np.ix_(rows + dy, cols + dx)].reshape(ni, B, nj, B)).sum((1, 3))
            key = (sad << 32) | ((abs(dy) + abs(dx)) << 16) | ((dy + R) << 8) | (dx + R)      # the tie rule as one ascending key
            best = np.minimum(best, key)
    out[:, 0] = (((best >> 8) & 255) - R).reshape(-1)
    out[:, 1] = ((best & 255) - R).reshape(-1)
    out[:, 2] = (best >> 32).reshape(-1)
    out[:, 3] = ((mine.max((1, 3)) - mine.min((1, 3))) >= int(texture)).reshape(-1)
    return out


def motion_of(blocks: np.ndarray, scale: int = 4, min_blocks: int = 8) -> np.ndarray:
    """match_blocks' rows -> (mx, my) float32."""
    kept = blocks[blocks[:, 3] != 0]
    if len(kept) < int(min_blocks):
        return np.zeros(2, np.float32)
    k = (len(kept) - 1) // 2
    return np.asarray([np.sort(kept[:, 1])[k] * int(scale), np.sort(kept[:, 0])[k] * int(scale)], np.float32)


class Estimator:
    """The host form of one sequence: update(picture [H, W, 3] uint8) -> (mx, my) float32 of that frame against the one before."""

    def __init__(self, **cfg):
        self.cfg = check(**cfg)
        self.reset()

    def reset(self) -> None:
        self.shape: Optional[Tuple[int, int]] = None
        self.small: Optional[np.ndarray] = None
        self.blocks = np.zeros((0, 4), np.int32)          # the blocks of the last update; none where the frame had no predecessor

    def update(self, img: np.ndarray) -> np.ndarray:
        c = self.cfg
        shape, small = tuple(np.asarray(img).shape[:2]), shrink(img, c['scale'])
        prev, self.small = (self.small if self.shape == shape else None), small
        self.shape = shape
        if prev is None:
            self.blocks = np.zeros((0, 4), np.int32)
            return np.zeros(2, np.float32)
        self.blocks = match_blocks(prev, small, c['block'], c['range'], c['step'], c['texture'])
        return motion_of(self.blocks, c['scale'], c['min_blocks'])

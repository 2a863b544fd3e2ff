"""Training augmentation: the imgaug OneOf of tools/utils.py:84-88 (`make train IAA=True`), applied to the letterboxed image.

Each training image gets one of three transforms, chosen uniformly: a horizontal flip with probability 0.5 (else unchanged), a
rotation of up to +-10 degrees, or a translation of up to +-10 % of the network tensor's width and height.  Validation is never
augmented (utils.py:447).

Random draws.  Parameters are drawn per (seed, epoch, dataset row), never from a per-process stream, so a row's augmentation does not
depend on the rank, the world size, the thread pool or the batch it lands in.  One table per epoch,
`np.random.default_rng([seed, epoch, 1]).random((n_rows, 5))`, indexed by row; from a row's uniforms u0..u4:
  branch = min(floor(3*u0), 2)                     (the OneOf choice)
  branch 0, flip:        flip when u1 < 0.5, otherwise the image is left as it is
  branch 1, rotation:    theta = -10 + 20*u2 degrees
  branch 2, translation: tx = (-0.1 + 0.2*u3)*W, ty = (-0.1 + 0.2*u4)*H   pixels of the network tensor (H, W = in_hw[0])

Geometry.  Continuous coordinates of the H x W network tensor: pixel (j, i) (column, row) has its centre at (j+0.5, i+0.5), and
c = (W/2, H/2).  The forward map is p' = A(p - c) + c + t, with A = [[cos, -sin], [sin, cos]] of theta, diag(-1, 1) for the flip,
or the identity, and t = (tx, ty).  With y pointing down, a positive theta turns the content CLOCKWISE on screen.  The host computes
the inverse map once per image in float64 with host cos/sin, as a 2x3 matrix M in pixel-index coordinates, src_idx = M . (x, y, 1):
  M[:, :2] = A^T (A is orthogonal),  M[:, 2] = A^T (0.5 - c - t) + c - 0.5
Identity and flip matrices come out with exact integer entries.  The kernel (yk_letterbox_augment_u8) and `warp_u8` below use the
same M; the device never evaluates a transcendental.

Pixels: two resamples, like the reference.  Letterbox first (yk_letterbox_u8's arithmetic, truncation to u8), then warp the u8
letterboxed image: c = M00*x + M01*y + M02 and r = M10*x + M11*y + M12 in that order, bilinear with floor/ceil taps as the
letterbox, taps outside [0,H) x [0,W) read 0, output min(255, floor(v + 0.5)).  Identity and flip give an exact pixel copy.

Boxes, from the letterboxed boxes ([cls, x, y, w, h], fractions of the network tensor): the four corners in pixels through the
forward map; their axis-aligned bounding box; boxes with no positive-area overlap with [0,W] x [0,H] are dropped; the rest are
clipped to the image; boxes whose clipped width or height is 0 are dropped; back to centre / size fractions.  Each class stays
with its own box.

Deviations from the reference:
  (a) utils.py:336 pairs the first n classes with whatever boxes survive, which mislabels a sample when any box but the last is
      dropped; here each class keeps its box.
  (b) imgaug 0.2.9's cv2 backend uses 1/32-pixel fixed-point weights, so pixels may differ from the reference by about +-1 per
      channel.
  (c) The random draws are per row (above), not from imgaug's global stream.
  (d) Boxes are the exact geometric counterpart of the pixel transform.  imgaug 0.2.9's keypoint convention (and the sign of its
      rotation) has not been checked against this: neither imgaug nor cv2 could be run to pin it.  Unpinned.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

FLIP, ROTATE, TRANSLATE = 0, 1, 2
MAX_DEGREES = 10.0
MAX_SHIFT = 0.1


def param_table(seed: int, epoch: int, n_rows: int) -> np.ndarray:
    """The epoch's [n_rows, 5] uniforms, indexed by dataset row (one numpy call per epoch, not one Generator per sample)."""
    return np.random.default_rng([int(seed), int(epoch), 1]).random((int(n_rows), 5))


def decode(u: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Rows of uniforms [n, 5] -> (branch, flip, theta degrees, tx, ty as fractions of W / H); theta / tx / ty are only meaningful
    in their own branch."""
    u = np.asarray(u, np.float64).reshape(-1, 5)
    branch = np.minimum(np.floor(3.0 * u[:, 0]), 2.0).astype(int)
    return (branch, u[:, 1] < 0.5, -MAX_DEGREES + 2 * MAX_DEGREES * u[:, 2], -MAX_SHIFT + 2 * MAX_SHIFT * u[:, 3],
            -MAX_SHIFT + 2 * MAX_SHIFT * u[:, 4])


def forward_maps(u: np.ndarray, hw) -> Tuple[np.ndarray, np.ndarray]:
    """Rows of uniforms [n, 5] -> (A [n, 2, 2], t [n, 2] in pixels) of the forward map p' = A(p - c) + c + t."""
    H, W = float(hw[0]), float(hw[1])
    branch, flip, theta, fx, fy = decode(u)
    n = len(branch)
    A = np.zeros((n, 2, 2))
    A[:, 0, 0] = A[:, 1, 1] = 1.0
    A[(branch == FLIP) & flip, 0, 0] = -1.0
    rot = branch == ROTATE
    rad = np.radians(theta[rot])
    cs, sn = np.cos(rad), np.sin(rad)
    A[rot, 0, 0], A[rot, 0, 1], A[rot, 1, 0], A[rot, 1, 1] = cs, -sn, sn, cs
    t = np.zeros((n, 2))
    tr = branch == TRANSLATE
    t[tr, 0], t[tr, 1] = fx[tr] * W, fy[tr] * H
    return A, t


def inverse_matrices(A: np.ndarray, t: np.ndarray, hw) -> np.ndarray:
    """The inverse maps [n, 2, 3] in pixel-index coordinates, src_idx = M . (x, y, 1): M[:, :2] = A^T, M[:, 2] = A^T (0.5 - c - t) + c - 0.5."""
    c = np.array([float(hw[1]) / 2, float(hw[0]) / 2])
    Ai = np.swapaxes(np.asarray(A, np.float64), 1, 2)
    v = (0.5 - c) - np.asarray(t, np.float64)                                   # [n, 2]
    M = np.empty((len(Ai), 2, 3))
    M[:, :, :2] = Ai
    M[:, :, 2] = (Ai[:, :, 0] * v[:, None, 0] + Ai[:, :, 1] * v[:, None, 1]) + c - 0.5
    return M


def matrices(u: np.ndarray, hw) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(A, t, M) for rows of uniforms."""
    A, t = forward_maps(u, hw)
    return A, t, inverse_matrices(A, t, hw)


def warp_u8(img: np.ndarray, M: np.ndarray) -> np.ndarray:
    """Host copy of the warp half of yk_letterbox_augment_u8: u8 [H, W, 3] (the letterboxed image) through one inverse map M [2, 3]
    -> u8 [H, W, 3].  Float64, the kernel's operations in the kernel's order."""
    H, W = img.shape[:2]
    m = np.asarray(M, np.float64).reshape(6)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    c = m[0] * x + m[1] * y + m[2]
    r = m[3] * x + m[4] * y + m[5]
    c_lo, c_hi, r_lo, r_hi = np.floor(c), np.ceil(c), np.floor(r), np.ceil(r)
    dc, dr = (c - c_lo)[..., None], (r - r_lo)[..., None]
    src = img.astype(np.float64)

    def tap(rr, cc):
        live = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
        ri, ci = np.where(live, rr, 0).astype(int), np.where(live, cc, 0).astype(int)
        return np.where(live[..., None], src[ri, ci], 0.0)
    top = (1.0 - dc) * tap(r_lo, c_lo) + dc * tap(r_lo, c_hi)
    bottom = (1.0 - dc) * tap(r_hi, c_lo) + dc * tap(r_hi, c_hi)
    return np.minimum(255.0, np.floor((1.0 - dr) * top + dr * bottom + 0.5)).astype(np.uint8)


def _map_boxes(boxes: np.ndarray, A: np.ndarray, t: np.ndarray, hw) -> Tuple[np.ndarray, np.ndarray]:
    """Boxes [n, 5] with one forward map per box (A [n, 2, 2], t [n, 2]) -> (mapped boxes [n, 5], keep mask [n])."""
    H, W = float(hw[0]), float(hw[1])
    cx, cy = W / 2, H / 2
    b = np.asarray(boxes, np.float64)
    x0, x1 = (b[:, 1] - b[:, 3] / 2) * W, (b[:, 1] + b[:, 3] / 2) * W
    y0, y1 = (b[:, 2] - b[:, 4] / 2) * H, (b[:, 2] + b[:, 4] / 2) * H
    px = np.stack([x0, x1, x0, x1], 1) - cx                                     # the four corners, relative to the centre
    py = np.stack([y0, y0, y1, y1], 1) - cy
    qx = (A[:, 0, 0, None] * px + A[:, 0, 1, None] * py) + cx + t[:, 0, None]
    qy = (A[:, 1, 0, None] * px + A[:, 1, 1, None] * py) + cy + t[:, 1, None]
    lx, hx, ly, hy = qx.min(1), qx.max(1), qy.min(1), qy.max(1)
    keep = (hx > 0) & (lx < W) & (hy > 0) & (ly < H)                             # positive-area overlap with [0,W] x [0,H]
    lx, hx, ly, hy = np.clip(lx, 0, W), np.clip(hx, 0, W), np.clip(ly, 0, H), np.clip(hy, 0, H)
    keep &= (hx - lx > 0) & (hy - ly > 0)
    out = np.empty_like(b)
    out[:, 0] = b[:, 0]
    out[:, 1], out[:, 2] = (lx + hx) / 2 / W, (ly + hy) / 2 / H
    out[:, 3], out[:, 4] = (hx - lx) / W, (hy - ly) / H
    return out, keep


def augment_boxes(boxes: np.ndarray, A: np.ndarray, t: np.ndarray, hw) -> np.ndarray:
    """One sample's letterboxed boxes [n, 5] through its forward map (A [2, 2], t [2]) -> the surviving boxes [k, 5], each class
    with its own box."""
    b = np.asarray(boxes, np.float64).reshape(-1, 5)
    n = len(b)
    out, keep = _map_boxes(b, np.broadcast_to(np.asarray(A, np.float64), (n, 2, 2)),
                           np.broadcast_to(np.asarray(t, np.float64), (n, 2)), hw)
    return out[keep]


def augment_boxes_batch(boxes_list: Sequence[np.ndarray], A: np.ndarray, t: np.ndarray, hw) -> List[np.ndarray]:
    """`augment_boxes` for every sample of a batch (A [n, 2, 2], t [n, 2]) in a handful of array operations; the same element-wise
    operations in the same order, so bit-identical to the per-sample function."""
    per = [np.asarray(b, np.float64).reshape(-1, 5) for b in boxes_list]
    counts = [len(b) for b in per]
    if sum(counts) == 0:
        return per
    out, keep = _map_boxes(np.concatenate(per), np.repeat(np.asarray(A, np.float64), counts, axis=0),
                           np.repeat(np.asarray(t, np.float64), counts, axis=0), hw)
    kept = np.bincount(np.repeat(np.arange(len(per)), counts)[keep], minlength=len(per))
    return np.split(out[keep], np.cumsum(kept)[:-1])

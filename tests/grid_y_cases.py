"""Tables, sources and expected frames for the five entry points that put the picture index in blockIdx.y and loop on the host past the 65535
rows of one launch (yk_letterbox_ragged_u8, yk_letterbox_tiles_u8, yk_letterbox_views_u8, yk_mosaic_ragged_u8 in csrc/yk_pre.hip and
yk_draw_dets_u8 in csrc/yk_draw.hip), shared by tests/test_grid_y_cases.py (CPU: the cases checked on their own) and tests/test_gpu_grid_y.py
(the kernels).  Nothing here touches a GPU or the library.

ROWS.  The content of row i is a function of (a, b) = (i % 7, i % 11) only, key(i) = 11 a + b.  65535 = 1 (mod 7) = 8 (mod 11): row i and row
i - 65535 differ in both indices, and so do rows i and i - 2 * 65535.  Per kernel there are 77 table rows and 77 reference frames; the table
and the expected output of a call of any n are one NumPy gather by key, so every row of a 131071-row call is compared, none sampled.

SOURCES.  A pool of 7 pictures of 1 x 1 .. 5 x 4 pixels, seeded bytes in 1 .. 255 (a tap outside a picture, which must read 0, shows), packed
with 5-byte gaps that hold 255.

WHAT (a, b) SELECT.
  ragged   picture (a + 2 b) % 7 -> 2 x 3.  (Seven pictures make seven frames; the stride 2 keeps rows one and two launches apart on different
           pictures: -1 - 16 = 4 and -2 - 32 = 1 (mod 7).)
  tiles    picture a, crop b of CROPS clipped to the picture, the parent's stride -> 2 x 3
  views    picture a, placement b of PLACEMENTS (canvas growth, offset, mirror) -> 5 x 7
  mosaic   quadrant b % 4 holds picture a, the other three hold pictures a + 1 + (b + k) % 6 (mod 7), k = 0, 1, 2; seam SEAMS[b]; gains GAINS rotated by
           b; with a warp also the inverse map maps()[b] -> 5 x 7
  draw     row i owns a 4 x 5 picture of its own (the kernel paints in place) whose content is pool picture a repeated; COUNTS[b] of the boxes
           BOXES[b]; cap 2, thickness 1, no label; rows of the cap beyond the count hold NaN

REFERENCES, none of them the code under test: letterbox_cases.reference (helper.letterbox_bilinear) of the picture, of a contiguous copy of the
crop, of tta.canvas of the view; the quadrant rule of tests/test_gpu_letterbox_edges.py with mosaic.quadrant_params, then
letterbox_cases.warp_reference; tests/test_gpu_draw.py's painter.

warp_loop() is the warp of yk_letterbox_augment_u8 / yk_mosaic_ragged_u8 as the kernel's header comment states it, one pixel at a time in
Python floats with integer tap tests: the reference for maps whose coordinates leave the int range, where augment.warp_u8's NumPy indexing is
not defined by anything."""
import functools
import math

import numpy as np

from k210_yolo_framework_amd import draw, mosaic, tiles, tta
from tests import letterbox_cases as lc

CHUNK = 65535                                       # rows of one launch
N_MAX = 2 * CHUNK + 1                               # a third launch of one row
NS = (CHUNK, CHUNK + 1, CHUNK + 3)
ROWS8 = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, N_MAX - 2, N_MAX - 1)
BAD_ROWS = (CHUNK - 1, CHUNK, CHUNK + 1)
BAD_QUADRANT = 0                                    # the mosaic quadrant whose row is spoilt in those rows
SMALL, ROOM = (2, 3), (5, 7)
KERNELS = ('ragged', 'tiles', 'views', 'mosaic', 'mosaic_inv', 'draw')
DST = dict(ragged=SMALL, tiles=SMALL, views=ROOM, mosaic=ROOM, mosaic_inv=ROOM, draw=(4, 5))
LARGEST = dict(ragged=N_MAX, tiles=NS[-1], views=NS[-1], mosaic=NS[-1], mosaic_inv=N_MAX, draw=NS[-1])

POOL_SHAPES = ((1, 1), (2, 3), (3, 2), (4, 4), (3, 4), (5, 3), (5, 4))
GAP = 5
# (y0, x0, h, w), clipped to the picture: y0 <- min(y0, H - 1), h <- min(h, H - y0), likewise x
CROPS = ((0, 0, 5, 4), (0, 0, 1, 1), (1, 1, 4, 3), (0, 1, 2, 2), (2, 0, 3, 4), (1, 0, 1, 4), (0, 2, 5, 1), (3, 3, 2, 1), (0, 0, 3, 2), (2, 1, 2, 3),
         (4, 0, 1, 2))
# (ch - h, cw - w, oy, ox, mirror)
PLACEMENTS = ((0, 0, 0, 0, 0), (0, 0, 0, 0, 1), (2, 3, 0, 0, 0), (2, 3, 2, 3, 1), (2, 3, 1, 1, 0), (4, 0, 2, 0, 1), (0, 5, 0, 5, 0), (1, 1, 1, 0, 1),
              (3, 2, 0, 2, 0), (3, 2, 3, 0, 1), (6, 6, 3, 3, 0))
# (cx, cy) in the 5 x 7 frame; the seams of the rows around 65535 (b = 7, 8, 9) leave all four quadrants pixels
SEAMS = ((3, 2), (0, 0), (7, 5), (1, 4), (6, 1), (4, 3), (2, 2), (5, 2), (3, 3), (4, 1), (7, 2))
GAINS = (1.0, 0.5, 0.75, 1.0)
# yk_draw_dets_u8: (top, left, bottom, right, score, class) in a 4 x 5 picture.  COUNTS[b] != COUNTS[(b + 3) % 11] for every b: the count one
# launch back (b - 8 = b + 3 mod 11) is never the row's own
BOXES = (((0.0, 0.0, 3.0, 4.0, 0.5, 0), (1.0, 1.0, 2.0, 3.0, 0.5, 1)),
         ((1.0, 1.0, 3.0, 3.0, 0.5, 1), (0.0, 0.0, 1.0, 1.0, 0.5, 2)),
         ((0.0, 2.0, 2.0, 4.0, 0.5, 2), (1.0, 0.0, 3.0, 2.0, 0.5, 3)),
         ((-2.0, -2.0, 1.0, 1.0, 0.5, 3), (2.0, 2.0, 3.0, 4.0, 0.5, 4)),
         ((0.0, 0.0, 1.0, 1.0, 0.5, 4), (2.0, 2.0, 3.0, 4.0, 0.5, 5)),
         ((2.0, 3.0, 9.0, 9.0, 0.5, 5), (0.0, 0.0, 2.0, 2.0, 0.5, 6)),
         ((0.0, 0.0, 3.0, 4.0, 0.5, 6), (0.0, 1.0, 2.0, 3.0, 0.5, 0)),
         ((0.4, 0.6, 2.5, 3.49, 0.5, 0), (0.0, 0.0, 3.0, 1.0, 0.5, 1)),
         ((1.0, 2.0, 3.0, 4.0, 0.5, 1), (0.0, 0.0, 3.0, 4.0, 0.5, 2)),
         ((0.0, 0.0, 2.0, 4.0, 0.5, 2), (1.0, 1.0, 3.0, 4.0, 0.5, 3)),
         ((0.0, 3.0, 3.0, 4.0, 0.5, 3), (0.0, 0.0, 3.0, 4.0, 0.5, 3)))
COUNTS = (0, 1, 2, 1, 2, 0, 2, 0, 1, 0, 1)
CAP = 2
COLOURS = np.asarray([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [128, 64, 32]], np.uint8)
NO_ATLAS = np.zeros((12, 0, 8), np.uint8)          # gh = 0: outlines alone
DRAW_HW = DST['draw']
DRAW_BYTES = 3 * DRAW_HW[0] * DRAW_HW[1]


def keys(n, first=0):
    """key(i) = 11 (i % 7) + i % 11 for i = first .. first + n - 1, int64 [n]."""
    i = np.arange(first, first + n, dtype=np.int64)
    return 11 * (i % 7) + i % 11


def ab(key):
    return int(key) // 11, int(key) % 11


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------- sources
@functools.lru_cache(maxsize=None)
def pool():
    """-> (the 7 pictures, their table of draw.RAGGED_DTYPE (scale / tx / ty 0), the packed buffer uint8 [bytes] with 255 in the gaps)."""
    rng = np.random.default_rng(20250101)
    pics = tuple(_frozen(rng.integers(1, 256, (h, w, 3), dtype=np.uint8)) for h, w in POOL_SHAPES)
    packed, table, _ = draw.pack_ragged(list(pics), gap=GAP)
    flat = packed.numpy().copy()
    used = np.zeros(flat.size, bool)
    for r in table:
        used[int(r['offset']):int(r['offset']) + 3 * int(r['h']) * int(r['w'])] = True
    flat[~used] = 255
    assert all(np.array_equal(got, im) for im, got in zip(pics, draw.unpack_ragged(flat, table)))
    return pics, _frozen(table), _frozen(flat)


def _fill(row, src_hw, dst):
    scale, tx, ty = lc.params(src_hw, dst)
    row['scale'], row['tx'], row['ty'] = scale, tx, ty


def crop_of(a, b):
    """Crop b of pool picture a -> (y0, x0, h, w)."""
    H, W = POOL_SHAPES[a]
    y0, x0, h, w = CROPS[b]
    y0, x0 = min(y0, H - 1), min(x0, W - 1)
    return y0, x0, min(h, H - y0), min(w, W - x0)


def view_of(a, b):
    """Placement b of pool picture a -> (ch, cw, oy, ox, mirror)."""
    h, w = POOL_SHAPES[a]
    gh, gw, oy, ox, mirror = PLACEMENTS[b]
    return h + gh, w + gw, oy, ox, mirror


def mosaic_of(a, b):
    """-> (pool picture per quadrant [4], (cx, cy), gains [4])."""
    own = b % 4
    others = [(a + 1 + (b + k) % 6) % 7 for k in range(3)]
    quad = others[:own] + [a] + others[own:]
    return quad, SEAMS[b], tuple(GAINS[(k + b) % 4] for k in range(4))


@functools.lru_cache(maxsize=None)
def maps():
    """The 11 inverse maps [11, 2, 3] of the 5 x 7 frame: the five of tests/test_gpu_letterbox_edges.py (identity, mirror, half-pixel shift,
    a drawn rotation, that rotation x 1.25) and six more by hand."""
    from tests.test_gpu_letterbox_edges import _inverse_maps
    H, W = ROOM
    hand = [[[1.0, 0.0, 0.0], [0.0, -1.0, H - 1.0]],            # upside down
            [[1.0, 0.0, -1.0], [0.0, 1.0, 0.0]],                # one whole pixel
            [[1.0, 0.0, 0.0], [0.0, 1.0, 1.5]],
            [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]],                 # transposed
            [[0.5, 0.0, 0.0], [0.0, 0.5, 0.0]],                 # enlarged
            [[1.0, 0.0, 2.25], [0.0, 1.0, -0.75]]]
    return _frozen(np.ascontiguousarray(np.concatenate([_inverse_maps(ROOM)[1], np.asarray(hand, np.float64)])))


@functools.lru_cache(maxsize=None)
def draw_pictures():
    """uint8 [7, 4, 5, 3]: pool picture a's pixels repeated to fill 4 x 5."""
    h, w = DRAW_HW
    return _frozen(np.stack([np.resize(p.reshape(-1, 3), (h * w, 3)).reshape(h, w, 3) for p in pool()[0]]))


# ---------------------------------------------------------------------------------------------------- the 77 rows of each table
@functools.lru_cache(maxsize=None)
def rows77(kernel):
    """The table rows by key, as the C entry point takes them: draw.RAGGED_DTYPE [77] (ragged, draw), tiles.TILE_DTYPE [77], tta.VIEW_DTYPE [77],
    draw.RAGGED_DTYPE [77, 4] (mosaic, mosaic_inv).  The draw rows' offsets are set per row by table()."""
    _, ptable, _ = pool()
    dst = DST[kernel]
    if kernel in ('mosaic', 'mosaic_inv'):
        out = np.zeros((77, 4), draw.RAGGED_DTYPE)
        for key in range(77):
            quad, (cx, cy), gains = mosaic_of(*ab(key))
            for k in range(4):
                r = out[key, k]
                r['offset'], r['h'], r['w'] = (ptable[quad[k]][f] for f in ('offset', 'h', 'w'))
                r['scale'], r['tx'], r['ty'] = mosaic.quadrant_params(POOL_SHAPES[quad[k]], k, cx, cy, gains[k], dst)
        return _frozen(out)
    out = np.zeros(77, {'ragged': draw.RAGGED_DTYPE, 'draw': draw.RAGGED_DTYPE, 'tiles': tiles.TILE_DTYPE, 'views': tta.VIEW_DTYPE}[kernel])
    for key in range(77):
        a, b = ab(key)
        if kernel == 'ragged':
            p = (a + 2 * b) % 7
            out[key]['offset'], out[key]['h'], out[key]['w'] = (ptable[p][f] for f in ('offset', 'h', 'w'))
            _fill(out[key], POOL_SHAPES[p], dst)
        elif kernel == 'tiles':
            g = crop_of(a, b)
            out[key] = tiles.table_rows(np.asarray([g]), int(ptable[a]['offset']), POOL_SHAPES[a][1])[0]
            _fill(out[key], g[2:], dst)
        elif kernel == 'views':
            v = view_of(a, b)
            out[key] = tta.table_rows(np.asarray([v], np.int32), int(ptable[a]['offset']), *POOL_SHAPES[a])[0]
            _fill(out[key], v[:2], dst)
        else:
            out[key]['h'], out[key]['w'] = DRAW_HW
            out[key]['thickness'], out[key]['mag'] = 1, 1
    return _frozen(out)


def table(kernel, n):
    """The table of a call of n rows, one gather: rows77(kernel)[keys(n)].  Row i of the draw table addresses picture i of a buffer of n + 2
    pictures of DRAW_BYTES (a guard picture in front and one behind)."""
    t = rows77(kernel)[keys(n)]
    if kernel == 'draw':
        t['offset'] = DRAW_BYTES * (1 + np.arange(n, dtype=np.uint64))
    return np.ascontiguousarray(t.reshape(-1))


@functools.lru_cache(maxsize=None)
def centres77():
    return _frozen(np.asarray([SEAMS[key % 11] for key in range(77)], np.int32))


@functools.lru_cache(maxsize=None)
def inv77():
    return _frozen(np.ascontiguousarray(maps()[np.arange(77) % 11].reshape(77, 6)))


@functools.lru_cache(maxsize=None)
def dets77():
    """-> (float32 [77, CAP, 6] with NaN beyond the count, int32 [77])."""
    dets = np.full((77, CAP, 6), np.nan, np.float32)
    counts = np.zeros(77, np.int32)
    for key in range(77):
        b = key % 11
        counts[key] = COUNTS[b]
        dets[key, :COUNTS[b]] = np.asarray(BOXES[b][:COUNTS[b]], np.float32).reshape(-1, 6)
    return _frozen(dets), _frozen(counts)


# ---------------------------------------------------------------------------------------------------- the references
def mosaic_frame(quad, seam, gains, missing=None):
    """The quadrant rule: quadrant k of the 5 x 7 frame is the letterbox reference of pool picture quad[k] with mosaic.quadrant_params'
    (scale, tx, ty), restricted to the quadrant; `missing`: a quadrant whose row is bad, left zero."""
    pics = pool()[0]
    H, W = ROOM
    cx, cy = seam
    frame = np.zeros((H, W, 3), np.uint8)
    for k in range(4):
        if k == missing:
            continue
        scale, tx, ty = mosaic.quadrant_params(POOL_SHAPES[quad[k]], k, cx, cy, gains[k], ROOM)
        ys, xs = (slice(cy, H) if k & 2 else slice(0, cy)), (slice(cx, W) if k & 1 else slice(0, cx))
        frame[ys, xs] = lc.reference(pics[quad[k]], ROOM, scale, tx, ty)[ys, xs]
    return frame


def painted(a, rows):
    """Draw picture a with `rows` painted by tests/test_gpu_draw.py's painter: outlines alone, thickness 1."""
    from tests.test_gpu_draw import paint
    return paint(draw_pictures()[a].copy(), [list(r) for r in rows], COLOURS, NO_ATLAS, 1, 1)


def slow_frame(kernel, i, bad=None):
    """The reference frame of row i, computed from i alone.  `bad`: the frame when the row is one the kernel must refuse (h = 0) - zeros; for
    the mosaic kernels `bad` is the quadrant whose row is refused, and only that quadrant is zero."""
    a, b = i % 7, i % 11
    pics = pool()[0]
    if kernel in ('mosaic', 'mosaic_inv'):
        frame = mosaic_frame(*mosaic_of(a, b), missing=bad)
        return lc.warp_reference(frame, maps()[b]) if kernel == 'mosaic_inv' else frame
    if bad is not None:
        return np.zeros((*DST[kernel], 3), np.uint8)
    if kernel == 'ragged':
        return lc.reference(pics[(a + 2 * b) % 7], SMALL)
    if kernel == 'tiles':
        y0, x0, h, w = crop_of(a, b)
        return lc.reference(np.ascontiguousarray(pics[a][y0:y0 + h, x0:x0 + w]), SMALL)
    if kernel == 'views':
        return lc.reference(tta.canvas(pics[a], view_of(a, b)), ROOM)
    if kernel == 'draw':
        return painted(a, BOXES[b][:COUNTS[b]])
    raise KeyError(kernel)


@functools.lru_cache(maxsize=None)
def frames77(kernel):
    """uint8 [77, H, W, 3], read-only: the reference frame of every key (key = key(i) of i = the least row with that key; any other gives the
    same, which tests/test_grid_y_cases.py checks on ROWS8)."""
    first = {int(k): i for i, k in reversed(list(enumerate(keys(77))))}
    assert len(first) == 77
    return _frozen(np.stack([slow_frame(kernel, first[key]) for key in range(77)]))


def expected(kernel, n):
    """uint8 [n, H, W, 3]: every frame of a call of n rows."""
    return frames77(kernel)[keys(n)]


def lagged77(kernel, pointer):
    """The 77 frames a call would give a row past 65535 if `pointer` alone had not been advanced by `base`: the row's own everything else, but the
    seam / inverse map / detections / count of the row 65535 before it (b + 3 mod 11, a - 1 mod 7).  None where the kernel would read a NaN
    row, which no reference defines."""
    out = []
    for key in range(77):
        a, b = ab(key)
        a1, b1 = (a - 1) % 7, (b + 3) % 11
        if kernel in ('mosaic', 'mosaic_inv'):
            quad, seam, gains = mosaic_of(a, b)
            # the rows keep their own (scale, tx, ty), made for their own seam; the other seam only moves the quadrants' borders
            H, W = ROOM
            cx, cy = SEAMS[b1] if pointer == 'centre' else seam
            frame = np.zeros((H, W, 3), np.uint8)
            for k in range(4):
                scale, tx, ty = mosaic.quadrant_params(POOL_SHAPES[quad[k]], k, seam[0], seam[1], gains[k], ROOM)
                ys, xs = (slice(cy, H) if k & 2 else slice(0, cy)), (slice(cx, W) if k & 1 else slice(0, cx))
                frame[ys, xs] = lc.reference(pool()[0][quad[k]], ROOM, scale, tx, ty)[ys, xs]
            if kernel == 'mosaic_inv':
                frame = lc.warp_reference(frame, maps()[b1 if pointer == 'inv' else b])
            out.append(frame)
        elif pointer == 'dets':
            out.append(None if COUNTS[b] > COUNTS[b1] else painted(a, BOXES[b1][:COUNTS[b]]))
        elif pointer == 'counts':
            out.append(None if COUNTS[b1] > COUNTS[b] else painted(a, BOXES[b][:COUNTS[b1]]))
        else:
            raise KeyError(pointer)
    return out


# ---------------------------------------------------------------------------------------------------- the warp, one pixel at a time
def warp_loop(frame, M):
    """The second resample of yk_letterbox_augment_u8 and yk_mosaic_ragged_u8 for one FINITE inverse map, as csrc/yk_pre.hip states it:
      c = M00*x + M01*y + M02, r = M10*x + M11*y + M12; taps floor / ceil, a tap outside [0, dh) x [0, dw) reads 0;
      top = (1-dc)*I[minr,minc] + dc*I[minr,maxc], bottom likewise on maxr; out = min(255, floor((1-dr)*top + dr*bottom + 0.5))
    in Python floats (IEEE double, one rounding per operation), the taps tested as Python integers, which have no range to leave."""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    m = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    if not all(math.isfinite(v) for v in m):
        raise ValueError('warp_loop: a map that is not finite has no stated result')
    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            c = m[0] * float(x) + m[1] * float(y) + m[2]
            r = m[3] * float(x) + m[4] * float(y) + m[5]
            if not (math.isfinite(c) and math.isfinite(r)):
                raise ValueError('warp_loop: the coordinates overflow')
            minc, maxc, minr, maxr = math.floor(c), math.ceil(c), math.floor(r), math.ceil(r)
            dc, dr = c - float(minc), r - float(minr)

            def tap(rr, cc, ch):
                return float(frame[rr, cc, ch]) if 0 <= rr < H and 0 <= cc < W else 0.0
            for ch in range(3):
                top = (1.0 - dc) * tap(minr, minc, ch) + dc * tap(minr, maxc, ch)
                bottom = (1.0 - dc) * tap(maxr, minc, ch) + dc * tap(maxr, maxc, ch)
                out[y, x, ch] = int(min(255.0, math.floor((1.0 - dr) * top + dr * bottom + 0.5)))
    return out


def hostile_maps():
    """Finite maps no other test feeds, for the 5 x 7 frame -> {name: M [2, 3]}."""
    H, W = ROOM
    return {
        'zero': [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],                                   # every pixel samples (0, 0)
        'far': [[1.0, 0.0, 1.0e12], [0.0, 1.0, 1.0e12]],                              # c, r beyond int: every tap outside
        'far_negative': [[1.0, 0.0, -1.0e12], [0.0, 1.0, 0.0]],
        'scale_1e-300': [[1.0e-300, 0.0, 0.0], [0.0, 1.0e-300, 0.0]],
        'scale_1e300': [[1.0e300, 0.0, 0.0], [0.0, 1.0e300, 0.0]],                    # only output pixel (0, 0) is inside
        'edge_low': [[1.0, 0.0, -1.0], [0.0, 1.0, -1.0]],                             # c = -1 at x = 0, r = -1 at y = 0: floor == ceil, the first illegal tap
        'edge_high': [[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]],                              # c = dw - 1 at x = dw - 2 and dw at x = dw - 1; r likewise
        'edge_both': [[2.0, 0.0, -1.0], [0.0, 2.0, -1.0]],                            # c = -1, 1, 3, 5, 7 = dw, ...; r = -1, 1, 3, 5 = dh, 7
        'edge_mirror': [[-1.0, 0.0, float(W)], [0.0, -1.0, float(H)]],                # c = dw at x = 0 down to 1; r = dh at y = 0
    }


def nonfinite_maps():
    """Maps with an entry that is not finite -> {name: M [2, 3]}.  The kernels promise no particular frame for them."""
    nan, inf = float('nan'), float('inf')
    return {'nan': [[1.0, 0.0, nan], [0.0, 1.0, 0.0]], 'nan_scale': [[1.0, 0.0, 0.0], [0.0, nan, 0.0]], '+inf': [[1.0, 0.0, inf], [0.0, 1.0, 0.0]],
            '-inf': [[1.0, 0.0, 0.0], [0.0, 1.0, -inf]], 'inf_scale': [[inf, 0.0, 0.0], [0.0, 1.0, 0.0]]}

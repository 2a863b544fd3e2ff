"""tests/letterbox_cases.py checked on its own, without a GPU: the inverse matrix the kernels use against numpy.linalg.inv, the four places
that compute (scale, tx, ty) against each other, the reference against the loop oracle, and every condition a case is in the table for.

MATRIX.  numpy.linalg.inv of [[s,0,tx],[0,s,ty],[0,0,1]] and the closed form 1/s, -(tx*(1/s)), -(ty*(1/s)) have the same bits in every entry
that is not zero.  Where tx or ty is 0 the closed form's -(0*(1/s)) is -0.0 and LAPACK's entry +0.0: the entries that are zero are compared
as numbers, and the source coordinates c = M00*x + M02, r = M11*y + M12 that the two matrices give are compared bit for bit, sign included
(inv*x is never -0.0, so the zero's sign cannot reach a pixel)."""
import numpy as np
import pytest

from k210_yolo_framework_amd import draw, mosaic
from oracle import preprocess_ref
from tests import letterbox_cases as lc

LOOP_ORACLE_MAX_PIXELS = 64 * 80          # the loop oracle runs about 10 us per pixel: larger destinations are left to the vectorised reference


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _closed_form(scale, tx, ty):
    inv = 1.0 / scale
    return np.array([[inv, 0.0, -(tx * inv)], [0.0, inv, -(ty * inv)], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize('case', lc.CASES, ids=lc.IDS)
def test_closed_form_inverse_is_numpy_linalg_inv(case):
    scale, tx, ty = lc.params(case.src, case.dst)
    closed = _closed_form(scale, tx, ty)
    x, y = np.arange(case.dst[1], dtype=np.float64), np.arange(case.dst[0], dtype=np.float64)
    # off-diagonal +0.0: the matrix as written; -0.0: what AffineTransform(scale=, translation=) builds from -sin(0) (only zeros may change sign)
    for z in (0.0, -0.0):
        M = np.linalg.inv(np.array([[scale, z, tx], [z, scale, ty], [0.0, 0.0, 1.0]]))
        assert np.array_equal(M, closed), (z, M, closed)
        nz = closed != 0.0
        assert np.array_equal(_bits(M)[nz], _bits(closed)[nz]), (z, M, closed)
        assert nz[0, 0] and nz[1, 1] and nz[0, 2] == (tx != 0) and nz[1, 2] == (ty != 0)
        # ... and the zeros' signs reach no coordinate: skimage's c = M00*x + M01*y + M02 against the kernel's inv*x + (-(tx*inv)), bit for bit
        for yy in (0.0, float(case.dst[0] - 1)):
            assert np.array_equal(_bits(M[0, 0] * x + M[0, 1] * yy + M[0, 2]), _bits(closed[0, 0] * x + closed[0, 2]))
        for xx in (0.0, float(case.dst[1] - 1)):
            assert np.array_equal(_bits(M[1, 0] * xx + M[1, 1] * y + M[1, 2]), _bits(closed[1, 1] * y + closed[1, 2]))
    t = lc.taps(case.src, case.dst)
    assert np.array_equal(_bits(t.c), _bits(closed[0, 0] * x + closed[0, 2])) and np.array_equal(_bits(t.r), _bits(closed[1, 1] * y + closed[1, 2]))


@pytest.fixture(scope='module')
def lib():
    from k210_yolo_framework_amd import engine
    if not engine.library_path().exists():
        import __graft_entry__ as g
        g.build()
    return engine.lib()


def test_four_places_compute_the_same_scale_and_translation(lib):
    """oracle, Helper, mosaic and the C function behind every ragged table (yk_letterbox_ragged_params, host code: no device needed; the path
    through engine.ragged_table_to_device, which uploads, is in tests/test_gpu_letterbox_edges.py).  scale as float64 bits."""
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    for dst in sorted({c.dst for c in lc.CASES}):
        srcs = [c.src for c in lc.CASES if c.dst == dst]
        table = draw.ragged_table(srcs)
        assert lib.yk_letterbox_ragged_params(table, len(table), dst[0], dst[1]) == 0
        h = Helper(None, 20, VOC_ANCHORS, [list(dst)], [[7, 10], [14, 20]])
        for src, row in zip(srcs, table):
            scale, tx, ty = preprocess_ref.letterbox_params(src, dst)
            assert isinstance(scale, float) and isinstance(tx, int) and isinstance(ty, int)
            want = (_bits(scale).item(), tx, ty)
            hs, ht = h.letterbox_params(src)
            assert hs[0] == hs[1] and (_bits(hs[0]).item(), int(ht[0]), int(ht[1])) == want, (src, dst, hs, ht)
            ms, mtx, mty = mosaic.letterbox_params(src, dst)
            assert (_bits(ms).item(), mtx, mty) == want, (src, dst)
            assert (_bits(row['scale']).item(), int(row['tx']), int(row['ty'])) == want, (src, dst, row)
            assert (int(row['h']), int(row['w'])) == src


def test_tile_and_view_params_are_the_ragged_ones(lib):
    """The one fill behind yk_letterbox_{ragged,tiles,views}_params, on the other two row types (host code: no device needed): a tile that is the
    whole picture, a view whose canvas is the picture, and a view whose canvas is larger - there the canvas, not (h, w), gives the result."""
    from k210_yolo_framework_amd import tiles, tta
    n = len(lc.CASES)
    for dst in sorted({c.dst for c in lc.CASES}):
        srcs = [c.src for c in lc.CASES if c.dst == dst]
        tile, view, wide = np.zeros(len(srcs), tiles.TILE_DTYPE), np.zeros(len(srcs), tta.VIEW_DTYPE), np.zeros(len(srcs), tta.VIEW_DTYPE)
        for t in (tile, view, wide):
            t['h'], t['w'] = [s[0] for s in srcs], [s[1] for s in srcs]
        tile['stride'] = 3 * tile['w'].astype(np.int64)
        view['ch'], view['cw'] = view['h'], view['w']
        wide['ch'], wide['cw'], wide['oy'], wide['ox'] = wide['h'] + 3, wide['w'] + 5, 1, 2
        assert lib.yk_letterbox_tiles_params(tile, len(tile), dst[0], dst[1]) == 0
        assert lib.yk_letterbox_views_params(view, len(view), dst[0], dst[1]) == 0
        assert lib.yk_letterbox_views_params(wide, len(wide), dst[0], dst[1]) == 0
        differ = 0
        for i, src in enumerate(srcs):
            scale, tx, ty = preprocess_ref.letterbox_params(src, dst)
            want = (_bits(scale).item(), tx, ty)
            for row in (tile[i], view[i]):
                assert (_bits(row['scale']).item(), int(row['tx']), int(row['ty'])) == want, (src, dst, row)
            scale, tx, ty = preprocess_ref.letterbox_params((src[0] + 3, src[1] + 5), dst)
            assert (_bits(wide['scale'][i]).item(), int(wide['tx'][i]), int(wide['ty'][i])) == (_bits(scale).item(), tx, ty), (src, dst, wide[i])
            differ += (_bits(scale).item(), tx, ty) != want
            n -= 1
        assert differ                                   # (the larger canvas is told from the picture for every destination)
    assert n == 0


def test_every_params_helper_refuses_what_it_cannot_fill(lib):
    """YK_ERR_ARG (-10) for a non-positive size in the fields the helper reads, n <= 0 and a NULL table; a view's (h, w) is not read."""
    from k210_yolo_framework_amd import tiles, tta
    for fn, dtype, fields in ((lib.yk_letterbox_ragged_params, draw.RAGGED_DTYPE, ('h', 'w')),
                              (lib.yk_letterbox_tiles_params, tiles.TILE_DTYPE, ('h', 'w')),
                              (lib.yk_letterbox_views_params, tta.VIEW_DTYPE, ('ch', 'cw'))):
        good = np.zeros(2, dtype)
        for name in fields:
            good[name] = 5
        assert fn(good.copy(), 2, 7, 5) == 0
        for name in fields:
            for v in (0, -1):
                bad = good.copy()
                bad[name][1] = v
                assert fn(bad, 2, 7, 5) == -10, (fn.__name__, name, v)
        for n in (0, -1):
            assert fn(good.copy(), n, 7, 5) == -10
        assert fn(None, 2, 7, 5) == -10
        assert fn(good.copy(), 2, 0, 5) == -10 and fn(good.copy(), 2, 7, -1) == -10
    view = np.zeros(1, tta.VIEW_DTYPE)
    view['ch'], view['cw'] = 8, 9
    assert lib.yk_letterbox_views_params(view, 1, 7, 5) == 0                 # h = w = 0: the check of rows is engine.check_view_rows's
    bad = np.zeros(1, tta.VIEW_DTYPE)
    assert lib.yk_letterbox_views_params(bad, 1, 7, 5) == -10 and lib.yk_last_error().decode() == 'yk_letterbox_views_params: row 0 has a canvas of 0 x 0'
    bad = np.zeros(1, tiles.TILE_DTYPE)
    assert lib.yk_letterbox_tiles_params(bad, 1, 7, 5) == -10 and lib.yk_last_error().decode() == 'yk_letterbox_tiles_params: row 0 is 0 x 0'


@pytest.mark.parametrize('case', lc.CASES, ids=lc.IDS)
def test_taps_rebuild_the_reference(case):
    """taps() is what the condition checks below read: the reference's bytes rebuilt from those values alone, every content."""
    t = lc.taps(case.src, case.dst)
    sh, sw = case.src
    for content in lc.CONTENTS:
        src = lc.picture(case.src, content).astype(np.float64)

        def tap(rr, cc):
            live = ((rr >= 0) & (rr < sh))[:, None] & ((cc >= 0) & (cc < sw))[None, :]
            return np.where(live[..., None], src[rr.clip(0, sh - 1)[:, None], cc.clip(0, sw - 1)[None, :]], 0.0)
        dc, dr = t.dc[None, :, None], t.dr[:, None, None]
        top = (1.0 - dc) * tap(t.r_lo, t.c_lo) + dc * tap(t.r_lo, t.c_hi)
        bottom = (1.0 - dc) * tap(t.r_hi, t.c_lo) + dc * tap(t.r_hi, t.c_hi)
        assert np.array_equal(((1.0 - dr) * top + dr * bottom).astype(np.uint8), lc.expected(case.src, case.dst, content))


def test_loop_oracle_and_vectorised_reference_agree_byte_for_byte():
    """oracle.preprocess_ref.letterbox (scalar loops, written independently) against reference(), every content, on every case whose destination
    has at most 64 x 80 pixels - the loop oracle's running time; the larger destinations share their arithmetic with these."""
    ran = 0
    for case in lc.CASES:
        if case.dst[0] * case.dst[1] > LOOP_ORACLE_MAX_PIXELS:
            continue
        for content in lc.CONTENTS:
            img = lc.picture(case.src, content)
            assert np.array_equal(preprocess_ref.letterbox(img, case.dst), lc.expected(case.src, case.dst, content)), (case, content)
        ran += 1
    assert ran >= 12
    assert {c.dst for c in lc.CASES if c.dst[0] * c.dst[1] > LOOP_ORACLE_MAX_PIXELS} == {lc.MAX_DST, lc.WORKLOAD_DST}


def test_the_table_holds_the_cases_it_is_for():
    have = {(c.src, c.dst) for c in lc.CASES}
    assert len(have) == len(lc.CASES) == len(lc.IDS)
    for src, dst in [((1, 1), (7, 5)), ((1, 1), (1, 1)), ((300, 400), (1, 1)), ((1, 37), (17, 31)), ((37, 1), (17, 31)), ((2, 2), (56, 80)),
                     ((3, 5), (64, 48)), ((9, 13), (255, 257)), ((29, 41), (58, 82)), ((112, 160), (56, 80)), ((55, 79), (56, 80)),
                     ((57, 81), (56, 80)), ((640, 7), (56, 80)), ((4000, 3), (17, 31)), ((223, 319), (224, 320)), ((225, 321), (224, 320))]:
        assert (src, dst) in have, (src, dst)
    for c in lc.CASES:                      # the whole GPU file stays at a few seconds
        assert c.dst == lc.WORKLOAD_DST or (c.dst[0] <= lc.MAX_DST[0] and c.dst[1] <= lc.MAX_DST[1]), c
    known = {'small', 'one_px', 'line_ty', 'line_tx', 'upscale', 'edge_taps', 'white_254', 'dc_half', 'dc_zero', 'near_up', 'near_down', 'sliver',
             'odd_count'}
    used = {w for c in lc.CASES for w in c.why}
    assert used == known, used ^ known      # a condition nobody carries any more is a lost case
    for why, at_least in (('white_254', 3), ('edge_taps', 4), ('upscale', 5), ('sliver', 2), ('near_up', 2), ('near_down', 2), ('small', 3)):
        assert sum(why in c.why for c in lc.CASES) >= at_least, why


@pytest.mark.parametrize('case', lc.CASES, ids=lc.IDS)
def test_each_case_meets_the_conditions_it_is_named_for(case):
    (sh, sw), (dh, dw) = case.src, case.dst
    scale, tx, ty = lc.params(case.src, case.dst)
    t = lc.taps(case.src, case.dst)
    assert case.why
    # conditions are also asserted ABSENT where not named, for the ones a neighbour could meet by accident: the labels stay true both ways
    assert ('odd_count' in case.why) == ((dh * dw) % 256 != 0)
    assert ('small' in case.why) == (dh * dw < 256)
    assert ('one_px' in case.why) == (dh * dw == 1)
    assert ('upscale' in case.why) == (scale > 1.6)
    for why in case.why:
        if why == 'line_ty':
            assert sh == 1 and sw > 1 and tx == 0 and ty > 0
        elif why == 'line_tx':
            assert sw == 1 and sh > 1 and ty == 0 and tx > 0
        elif why == 'edge_taps':
            lo = (t.c_lo == -1).any() or (t.r_lo == -1).any() or (t.c_hi == -1).any() or (t.r_hi == -1).any()
            hi = (t.c_hi == sw).any() or (t.r_hi == sh).any()
            assert lo and hi, (t.c_lo, t.c_hi, t.r_lo, t.r_hi)
            # ... and both blended with a live pixel somewhere (0 < d < 1), not only met with weight 0
            assert ((t.c_lo == -1) & (t.dc > 0)).any() or ((t.r_lo == -1) & (t.dr > 0)).any()
            assert ((t.c_hi == sw) & (t.c_lo == sw - 1) & (t.dc > 0)).any() or ((t.r_hi == sh) & (t.r_lo == sh - 1) & (t.dr > 0)).any()
        elif why == 'white_254':
            out = lc.expected(case.src, case.dst, 'white')
            inside = out[(t.r_lo >= 0) & (t.r_hi < sh)][:, (t.c_lo >= 0) & (t.c_hi < sw)]      # all four taps live: exactly 255 in real numbers
            assert inside.size and set(np.unique(inside).tolist()) == {254, 255}, np.unique(inside)
        elif why == 'dc_half':
            assert scale == 2.0 and tx == 0 and ty == 0
            assert (t.dc[0::2] == 0.0).all() and (t.dc[1::2] == 0.5).all() and (t.dr[0::2] == 0.0).all() and (t.dr[1::2] == 0.5).all()
            assert (t.c_lo[0::2] == t.c_hi[0::2]).all() and t.c_hi[-1] == sw and t.r_hi[-1] == sh
        elif why == 'dc_zero':
            assert scale == 0.5 and tx == 0 and ty == 0
            assert not t.dc.any() and not t.dr.any() and (t.c_lo == t.c_hi).all() and (t.r_lo == t.r_hi).all()
            assert np.array_equal(lc.expected(case.src, case.dst, 'noise'), lc.picture(case.src, 'noise')[::2, ::2])
        elif why == 'near_up':
            assert (sh + 1, sw + 1) == (dh, dw) and 1.0 < scale < 1.02
        elif why == 'near_down':
            assert (sh - 1, sw - 1) == (dh, dw) and 0.98 < scale < 1.0
        elif why == 'sliver':
            assert max(sh, sw) > 90 * min(sh, sw) and (tx > 0 or ty > 0)


def test_the_table_as_a_whole_covers_what_no_single_case_can():
    residues = {c.dst: (c.dst[0] * c.dst[1]) % 256 for c in lc.CASES}
    assert residues == {(7, 5): 35, (1, 1): 1, (17, 31): 15, (56, 80): 128, (64, 48): 0, (255, 257): 255, (58, 82): 148, (224, 320): 0}
    assert sum(r != 0 for r in residues.values()) >= 3
    p = [lc.params(c.src, c.dst) for c in lc.CASES]
    assert any(tx > 0 for _, tx, _ in p) and any(ty > 0 for _, _, ty in p)
    scales = [s for s, _, _ in p]
    assert max(scales) >= 28.0 and min(scales) < 0.005 and 1.0 in scales and 2.0 in scales and 0.5 in scales
    # three different pictures per batch, the named content at a position of its own
    for c in lc.CASES:
        for k, content in enumerate(lc.CONTENTS):
            b = lc.batch(c.src, content)
            assert b.shape == (3, *c.src, 3) and b.dtype == np.uint8 and np.array_equal(b[k], lc.picture(c.src, content))
            if c.src != (1, 1) or content != 'ramp':         # (a 1 x 1 ramp is its own border: the constant)
                assert len({im.tobytes() for im in b}) == 3
        ramp = lc.picture(c.src, 'ramp')
        assert (ramp[0] == 255).all() and (ramp[-1] == 255).all() and (ramp[:, 0] == 255).all() and (ramp[:, -1] == 255).all()
        assert (lc.picture(c.src, 'white') == 255).all()
    assert (lc.picture((57, 81), 'ramp')[1:-1, 1:-1] < 251).all()


def test_warp_reference_is_the_arithmetic_yk_pre_states():
    """warp_reference against scalar loops written from the comment in yk_pre.hip, on a frame small enough for loops."""
    import math
    frame = lc.expected((1, 1), (7, 5), 'white').copy()
    frame[:] = np.random.default_rng(3).integers(0, 256, frame.shape, dtype=np.uint8)
    H, W = frame.shape[:2]
    for M in ([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [[-1.0, 0.0, W - 1.0], [0.0, 1.0, 0.0]], [[1.0, 0.0, 0.5], [0.0, 1.0, 0.25]],
              [[1.1, -0.3, 0.7], [0.3, 1.1, -1.2]]):
        got = lc.warp_reference(frame, M)
        px = lambda rr, cc: frame[rr, cc].astype(np.float64) if 0 <= rr < H and 0 <= cc < W else np.zeros(3)
        for y in range(H):
            for x in range(W):
                c = M[0][0] * x + M[0][1] * y + M[0][2]
                r = M[1][0] * x + M[1][1] * y + M[1][2]
                c0, c1, r0, r1 = math.floor(c), math.ceil(c), math.floor(r), math.ceil(r)
                dc, dr = c - c0, r - r0
                top = (1.0 - dc) * px(r0, c0) + dc * px(r0, c1)
                bottom = (1.0 - dc) * px(r1, c0) + dc * px(r1, c1)
                want = np.minimum(255.0, np.floor((1.0 - dr) * top + dr * bottom + 0.5)).astype(np.uint8)
                assert np.array_equal(got[y, x], want), (M, y, x)
    assert np.array_equal(lc.warp_reference(frame, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), frame)
    assert np.array_equal(lc.warp_reference(frame, [[-1.0, 0.0, W - 1.0], [0.0, 1.0, 0.0]]), frame[:, ::-1])

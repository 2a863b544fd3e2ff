"""The cases of tests/grid_y_cases.py checked on their own (no GPU): a row past 65535 must differ from the row one launch before it on EVERY
row of every kernel's largest call, or a call that forgot `+ base` would be seen on a lucky few rows only; the gather must be the per-row
reference; and the tables must hold what the library's own host helpers fill in for the same rows."""
import numpy as np
import pytest

from k210_yolo_framework_amd import augment, draw, mosaic
from tests import grid_y_cases as gy
from tests import letterbox_cases as lc


@pytest.fixture(scope='module')
def lib():
    from k210_yolo_framework_amd import engine
    if not engine.library_path().exists():
        import __graft_entry__ as g
        g.build()
    return engine.lib()


def test_the_row_arithmetic_the_cases_rest_on():
    assert gy.CHUNK % 7 == 1 and gy.CHUNK % 11 == 8 and gy.N_MAX == 131071
    k = gy.keys(gy.N_MAX)
    assert k.min() == 0 and k.max() == 76 and len(np.unique(k[:77])) == 77
    a, b = k // 11, k % 11
    for back in (gy.CHUNK, 2 * gy.CHUNK):
        assert (a[back:] != a[:-back]).all() and (b[back:] != b[:-back]).all()
    assert np.array_equal(gy.keys(5, first=gy.CHUNK), k[gy.CHUNK:gy.CHUNK + 5])
    assert all(gy.COUNTS[b] != gy.COUNTS[(b + 3) % 11] for b in range(11)) and set(gy.COUNTS) == {0, 1, 2}
    assert gy.LARGEST['ragged'] == gy.LARGEST['mosaic_inv'] == gy.N_MAX and max(gy.NS) == 65538


def test_the_pool_is_packed_with_gaps_of_255_and_holds_no_zero():
    pics, table, flat = gy.pool()
    assert [p.shape[:2] for p in pics] == list(gy.POOL_SHAPES) and min(gy.POOL_SHAPES) == (1, 1) and max(gy.POOL_SHAPES) == (5, 4)
    assert len({p.tobytes() for p in pics}) == 7 and all(p.min() >= 1 for p in pics) and flat.min() >= 1
    ends = table['offset'][:-1] + 3 * table['h'][:-1].astype(np.uint64) * table['w'][:-1].astype(np.uint64)
    assert (table['offset'][1:] - ends == gy.GAP).all()
    for e in ends:
        assert (flat[int(e):int(e) + gy.GAP] == 255).all()
    assert any(int(o) % 2 for o in table['offset'])
    assert len({p.tobytes() for p in gy.draw_pictures()}) == 7


def test_the_selections_cover_what_they_name():
    assert gy.view_of(3, 0) == (4, 4, 0, 0, 0) and gy.view_of(3, 1) == (4, 4, 0, 0, 1)               # the identity and its mirror
    for a in range(7):
        H, W = gy.POOL_SHAPES[a]
        for b in range(11):
            y0, x0, h, w = gy.crop_of(a, b)
            assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W
            ch, cw, oy, ox, _ = gy.view_of(a, b)
            assert oy >= 0 and ox >= 0 and oy + H <= ch and ox + W <= cw
            quad, (cx, cy), gains = gy.mosaic_of(a, b)
            assert quad[b % 4] == a and len(set(quad)) == 4 and 0 <= cx <= gy.ROOM[1] and 0 <= cy <= gy.ROOM[0] and all(0 < g <= 1 for g in gains)
    assert len({gy.crop_of(6, b) for b in range(11)}) == 11                                           # in the largest picture every crop is its own
    for i in gy.BAD_ROWS:                                                                             # the seams around 65535 are inside the frame
        cx, cy = gy.SEAMS[i % 11]
        assert 0 < cx < gy.ROOM[1] and 0 < cy < gy.ROOM[0]
    M = gy.maps()
    assert M.shape == (11, 2, 3) and len({m.tobytes() for m in M}) == 11
    assert np.array_equal(M[0], [[1, 0, 0], [0, 1, 0]]) and np.array_equal(M[1], [[-1, 0, 6], [0, 1, 0]])
    dets, counts = gy.dets77()
    for key in range(77):
        assert np.isfinite(dets[key, :counts[key]]).all() and np.isnan(dets[key, counts[key]:]).all()


@pytest.mark.parametrize('kernel', gy.KERNELS)
def test_every_row_past_65535_differs_from_the_row_one_and_two_launches_before_it(kernel):
    """Decided once per pair of keys (77 x 77 frame comparisons), then looked up for every row: no row is excluded."""
    f = gy.frames77(kernel)
    assert f.shape == (77, *gy.DST[kernel], 3) and f.dtype == np.uint8 and not f.flags.writeable
    differ = (f[:, None] != f[None]).reshape(77, 77, -1).any(-1)
    k = gy.keys(gy.N_MAX)
    for back in (gy.CHUNK, 2 * gy.CHUNK):
        same = np.flatnonzero(~differ[k[back:], k[:-back]])
        assert not len(same), (kernel, back, len(same), [gy.ab(k[back + i]) for i in same[:5]])
    e = gy.expected(kernel, gy.LARGEST[kernel])                       # the same, on the bytes themselves
    assert (e[gy.CHUNK:] != e[:-gy.CHUNK]).reshape(len(e) - gy.CHUNK, -1).any(-1).all()
    assert f.reshape(77, -1).any(-1).all()                            # and no frame is the zero frame a refused row gives


@pytest.mark.parametrize('kernel', gy.KERNELS)
def test_the_gather_is_the_reference_of_the_row_computed_on_its_own(kernel):
    e = gy.expected(kernel, gy.N_MAX)
    for i in gy.ROWS8:
        want = gy.slow_frame(kernel, i)
        assert np.array_equal(e[i], want), (kernel, i)
    assert np.array_equal(gy.expected(kernel, gy.NS[0]), e[:gy.NS[0]])


def test_a_pointer_that_alone_lags_one_launch_shows_too():
    """centre, inv, dets and counts are advanced separately from the table: the frame of a row that got the right rows but the seam, map,
    detections or count of the row 65535 before it differs from the expected one - on every key for the seam and the map, and for the
    detections and the count wherever a reference can say what is painted."""
    for kernel, pointer in (('mosaic', 'centre'), ('mosaic_inv', 'centre'), ('mosaic_inv', 'inv')):
        lag, f = gy.lagged77(kernel, pointer), gy.frames77(kernel)
        same = [gy.ab(key) for key in range(77) if np.array_equal(lag[key], f[key])]
        assert not same, (kernel, pointer, same)
    f = gy.frames77('draw')
    for pointer in ('dets', 'counts'):
        lag = gy.lagged77('draw', pointer)
        known = [key for key in range(77) if lag[key] is not None]
        # (with the own count 0 nothing is read of the wrong detections: those keys cannot show them)
        live = [key for key in known if pointer == 'counts' or gy.COUNTS[key % 11] > 0]
        assert len(live) >= 21 and all(not np.array_equal(lag[key], f[key]) for key in live), pointer


def test_the_mosaic_quadrant_a_bad_row_blanks_held_pixels():
    for kernel in ('mosaic', 'mosaic_inv'):
        for i in gy.BAD_ROWS:
            good, cut = gy.slow_frame(kernel, i), gy.slow_frame(kernel, i, bad=gy.BAD_QUADRANT)
            assert not np.array_equal(good, cut), (kernel, i)
            if kernel == 'mosaic':
                (x0, x1), (y0, y1) = mosaic.quadrant_rect(gy.BAD_QUADRANT, *gy.SEAMS[i % 11], gy.ROOM)
                assert not cut[y0:y1, x0:x1].any()
                cut[y0:y1, x0:x1] = good[y0:y1, x0:x1]
                assert np.array_equal(cut, good)


def test_the_tables_hold_what_the_librarys_host_helpers_fill_in(lib):
    rows = np.asarray(gy.ROWS8)
    for kernel, helper in (('ragged', 'yk_letterbox_ragged_params'), ('tiles', 'yk_letterbox_tiles_params'), ('views', 'yk_letterbox_views_params')):
        t = gy.table(kernel, gy.N_MAX)[rows]
        blank = t.copy()
        blank['scale'], blank['tx'], blank['ty'] = 0.0, 0, 0
        assert getattr(lib, helper)(blank, len(blank), *gy.DST[kernel]) == 0
        assert blank.tobytes() == t.tobytes(), kernel
        assert (t['scale'] > 0).all()
    t = gy.table('mosaic', gy.N_MAX).reshape(-1, 4)[rows]
    assert np.array_equal(gy.table('mosaic_inv', gy.N_MAX).reshape(-1, 4)[rows], t)
    for i, rows4 in zip(rows, t):
        blank = rows4.copy()
        blank['scale'], blank['tx'], blank['ty'] = 0.0, 0, 0
        _, (cx, cy), gains = gy.mosaic_of(i % 7, i % 11)
        assert gy.centres77()[gy.keys(1, first=int(i))[0]].tolist() == [cx, cy]
        assert lib.yk_mosaic_params(blank, cx, cy, np.asarray(gains, np.float64), *gy.ROOM) == 0
        assert blank.tobytes() == rows4.tobytes(), i
    d = gy.table('draw', gy.NS[-1])
    assert d.dtype == draw.RAGGED_DTYPE and (d['h'] == 4).all() and (d['w'] == 5).all() and (d['thickness'] == 1).all()
    assert np.array_equal(d['offset'], gy.DRAW_BYTES * np.arange(1, gy.NS[-1] + 1, dtype=np.uint64))      # no two rows share a byte


def test_warp_loop_agrees_with_warp_u8_on_ordinary_maps_and_states_the_hostile_ones():
    from tests.test_gpu_letterbox_edges import _inverse_maps
    L = lc.reference(lc.picture((3, 5), 'noise'), gy.ROOM)
    frames = [L, gy.frames77('mosaic')[40], np.full((*gy.ROOM, 3), 255, np.uint8)]
    for name, M in zip(*_inverse_maps(gy.ROOM)):
        for f in frames:
            assert np.array_equal(gy.warp_loop(f, M), augment.warp_u8(f, M)), name
    for M in gy.maps():
        assert np.array_equal(gy.warp_loop(L, M), augment.warp_u8(L, M))
    assert L[0, 0].any() and L.all(-1).sum() >= 20
    H, W = gy.ROOM
    hm = {k: gy.warp_loop(L, M) for k, M in gy.hostile_maps().items()}
    assert (hm['zero'] == L[0, 0]).all() and (hm['scale_1e-300'] == L[0, 0]).all()
    assert not hm['far'].any() and not hm['far_negative'].any()
    assert np.array_equal(hm['scale_1e300'][0, 0], L[0, 0]) and not hm['scale_1e300'][0, 1:].any() and not hm['scale_1e300'][1:].any()
    want = np.zeros_like(L)
    want[1:, 1:] = L[:-1, :-1]
    assert np.array_equal(hm['edge_low'], want)                       # row 0 and column 0 sample -1: zero; the rest an exact copy
    want = np.zeros_like(L)
    want[:-1, :-1] = L[1:, 1:]
    assert np.array_equal(hm['edge_high'], want)                      # the last row and column sample dh and dw: zero
    want = np.zeros_like(L)
    want[1:3, 1:4] = L[1:4:2, 1:6:2]
    assert np.array_equal(hm['edge_both'], want)
    want = np.zeros_like(L)
    want[1:, 1:] = L[::-1, ::-1][:-1, :-1]
    assert np.array_equal(hm['edge_mirror'], want)
    for M in gy.nonfinite_maps().values():
        with pytest.raises(ValueError):
            gy.warp_loop(L, M)
    with pytest.raises(ValueError):
        gy.warp_loop(L, [[1.0e308, 1.0e308, 0.0], [0.0, 1.0, 0.0]])

"""tiles.py, the statement of sliced inference, on the CPU: the grid's cover and edges, the refusals by name, and the
merge against an independent float64 restatement on integer coordinates, where float32 and float64 agree exactly."""
import numpy as np
import pytest

from k210_yolo_framework_amd import tiles


def covered(h, w, g):
    m = np.zeros((h, w), bool)
    for y0, x0, th, tw in g:
        assert 0 <= y0 and 0 <= x0 and th >= 1 and tw >= 1 and y0 + th <= h and x0 + tw <= w, (h, w, (y0, x0, th, tw))
        m[y0:y0 + th, x0:x0 + tw] = True
    return bool(m.all())


@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (9, 9), (33, 47), (64, 48), (375, 500)])
@pytest.mark.parametrize('nxy', [(1, 1), (2, 2), (3, 1), (1, 3), (8, 8)])
@pytest.mark.parametrize('overlap', [0.0, 0.2, 0.5])
def test_grid_covers_and_ends_at_the_edge(hw, nxy, overlap):
    h, w = hw
    nx, ny = nxy
    g = tiles.grid(h, w, nx, ny, overlap, full=False)
    assert g.dtype == np.int32 and g.shape == (nx * ny, 4)
    assert covered(h, w, g)
    assert g[-1, 0] + g[-1, 2] == h and g[-1, 1] + g[-1, 3] == w          # the last tile ends exactly at the edge
    assert tuple(g[0, :2]) == (0, 0)
    assert len(set(map(tuple, g[:, 2:]))) == 1                            # one tile size
    assert np.array_equal(g.reshape(ny, nx, 4)[:, :, 1], np.broadcast_to(g[:nx, 1], (ny, nx)))       # row-major: j outer, i inner
    f = tiles.grid(h, w, nx, ny, overlap)
    assert f.shape == (nx * ny + 1, 4) and tuple(f[0]) == (0, 0, h, w) and np.array_equal(f[1:], g)


def test_grid_known_answers():
    assert tiles.grid(48, 64, 1, 1, 0.2, full=False).tolist() == [[0, 0, 48, 64]]
    assert tiles.grid(1, 1, 2, 2, 0.2).tolist() == [[0, 0, 1, 1]] * 5
    g = tiles.grid(9, 9, 8, 8, 0.2, full=False)                           # ceil(9 / 6.6) = 2 wide, origins 0 .. 7
    assert g[:8].tolist() == [[0, i, 2, 2] for i in range(8)] and g[8].tolist() == [1, 0, 2, 2]
    assert tiles.grid(10, 100, 2, 1, 0.0, full=False).tolist() == [[0, 0, 10, 50], [0, 50, 10, 50]]
    assert tiles.grid(10, 100, 2, 1, 0.5, full=False).tolist() == [[0, 0, 10, 67], [0, 33, 10, 67]]      # ceil(100 / 1.5)
    assert tiles.grid(10, 100, 3, 1, 0.5, full=False).tolist() == [[0, 0, 10, 50], [0, 25, 10, 50], [0, 50, 10, 50]]
    assert tiles.grid(10, 101, 3, 1, 0.0, full=False)[:, 1].tolist() == [0, 33, 67]                    # floor division: (i * 67) // 2


@pytest.mark.parametrize('args, word', [
    ((10, 10, 0, 1, 0.2), 'tiles'), ((10, 10, 9, 1, 0.2), 'tiles'), ((10, 10, 2, 0, 0.2), 'tiles'), ((10, 10, 2.5, 2, 0.2), 'tiles'),
    ((10, 10, 2, 2, -0.1), 'tile_overlap'), ((10, 10, 2, 2, 0.51), 'tile_overlap'), ((10, 10, 2, 2, float('nan')), 'tile_overlap'),
    ((0, 10, 2, 2, 0.2), 'picture'), ((1 << 24, 10, 2, 2, 0.2), 'picture'), ((10, 1 << 24, 2, 2, 0.2), 'picture')])
def test_grid_refusals_by_name(args, word):
    with pytest.raises(ValueError, match=word):
        tiles.grid(*args)


def test_option_refusals_by_name():
    assert tiles.check(None, nms='linear') is None                         # off: nothing is looked at
    assert tiles.check((2, 3)) == (2, 3)
    with pytest.raises(ValueError, match='tile_match'):
        tiles.check((2, 2), match='giou')
    with pytest.raises(ValueError, match='tile_thresh'):
        tiles.check((2, 2), thresh=float('nan'))
    with pytest.raises(ValueError, match="nms 'linear' with tiles"):
        tiles.check((2, 2), nms='linear')
    with pytest.raises(ValueError, match='tile_match'):
        tiles.merge([], np.zeros((0, 2)), 1, 1, 0.5, 'giou')
    assert tiles.parse_tiles('2x3') == (2, 3) and tiles.parse_tiles('None') is None
    with pytest.raises(ValueError, match='tiles'):
        tiles.parse_tiles('2by2')
    assert (2 ** 24 - 1) == int(np.float32(2 ** 24 - 1))                   # the largest origin grid() lets through is exact in float32


def test_table_rows_address_the_crop():
    rng = np.random.default_rng(0)
    pic = rng.integers(0, 256, (33, 47, 3), dtype=np.uint8)
    flat = np.concatenate([np.zeros(11, np.uint8), pic.reshape(-1)])
    g = tiles.grid(33, 47, 2, 2, 0.2)
    for (y0, x0, th, tw), r in zip(g, tiles.table_rows(g, 11, 47)):
        got = np.stack([flat[int(r['offset']) + j * int(r['stride']):][:3 * int(r['w'])] for j in range(int(r['h']))]).reshape(th, tw, 3)
        assert np.array_equal(got, pic[y0:y0 + th, x0:x0 + tw])


# ---- the merge, restated independently in float64 (sort, then sweep: the textbook form, not tiles.merge's iterated arg-max) ----------
def merge64(rows_per_tile, origins, class_num, max_out, thresh, metric):
    cand = []
    for r, (y0, x0) in zip(rows_per_tile, np.asarray(origins, np.float64)):
        for t, l, b, rr, s, c in np.asarray(r, np.float64).reshape(-1, 6):
            cand.append((t + y0, l + x0, b + y0, rr + x0, s, c))

    def match(p, q):
        ay0, ay1, ax0, ax1 = min(p[0], p[2]), max(p[0], p[2]), min(p[1], p[3]), max(p[1], p[3])
        by0, by1, bx0, bx1 = min(q[0], q[2]), max(q[0], q[2]), min(q[1], q[3]), max(q[1], q[3])
        a, b = (ay1 - ay0) * (ax1 - ax0), (by1 - by0) * (bx1 - bx0)
        inter = max(min(ay1, by1) - max(ay0, by0), 0.0) * max(min(ax1, bx1) - max(ax0, bx0), 0.0)
        if metric == 'iou':
            return inter / (a + b - inter) if a > 0 and b > 0 else 0.0
        return inter / min(a, b) if min(a, b) > 0 else 0.0

    out, idx = [], []
    for c in range(class_num):
        order = sorted((i for i, r in enumerate(cand) if r[5] == c), key=lambda i: (-cand[i][4], i))
        kept = []
        for i in order:
            if len(kept) == max_out:
                break
            if all(match(cand[k], cand[i]) <= thresh for k in kept):
                kept.append(i)
        out += [cand[i] for i in kept]
        idx += kept
    return np.asarray(out, np.float64).reshape(-1, 6), np.asarray(idx, np.int64)


def random_tiles(rng, n_tiles, k_max, class_num, side=64):
    """Integer corners, scores from a small set of exactly representable values (ties are common), integer origins."""
    rows = []
    for _ in range(n_tiles):
        k = int(rng.integers(0, k_max + 1))
        t, l = rng.integers(0, side, k), rng.integers(0, side, k)
        r = np.stack([t, l, t + rng.integers(1, side // 2, k), l + rng.integers(1, side // 2, k), rng.integers(1, 9, k) / 8.0,
                      rng.integers(0, class_num, k)], 1).astype(np.float32)
        rows.append(r.reshape(-1, 6))
    return rows, rng.integers(0, side, (n_tiles, 2)).astype(np.float32)


@pytest.mark.parametrize('metric', ['iou', 'ios'])
@pytest.mark.parametrize('seed', range(6))
def test_merge_matches_float64_restatement(metric, seed):
    rng = np.random.default_rng(seed)
    class_num, max_out = [1, 3, 20][seed % 3], [3, 30][seed % 2]
    rows, origins = random_tiles(rng, 5, 40, class_num)
    # thresholds that integer boxes do not hit exactly in one precision but not the other: inter / denominator of small integers against 2^-k sums
    thresh = [0.5, 0.25, 0.375][seed % 3]
    got, gi = tiles.merge(rows, origins, class_num, max_out, thresh, metric)
    ref, ri = merge64(rows, origins, class_num, max_out, thresh, metric)
    assert got.dtype == np.float32 and np.array_equal(gi, ri) and np.array_equal(got.astype(np.float64), ref)
    assert len(got) > 0 and np.all(np.diff(got[:, 5]) >= 0)               # class-major ascending


def test_merge_small_cases():
    A = [10, 10, 20, 20, 0.5, 0]
    # one object seen by two tiles: the duplicate goes, the higher score stays; strictly above the threshold only
    r0, r1 = np.asarray([A], np.float32), np.asarray([[0, 0, 10, 10, 0.75, 0]], np.float32)
    rows, idx = tiles.merge([r0, r1], [[0, 0], [10, 10]], 1, 30, 0.5, 'iou')
    assert rows.tolist() == [[10, 10, 20, 20, 0.75, 0]] and idx.tolist() == [1]
    r1 = np.asarray([[0, 0, 10, 10, 0.5, 0]], np.float32)                 # equal scores: the lower candidate index wins
    assert tiles.merge([r0, r1], [[0, 0], [10, 10]], 1, 30, 0.5, 'iou')[1].tolist() == [0]
    half = np.asarray([[10, 10, 20, 15, 0.25, 0]], np.float32)            # inside A, half its area: iou 0.5, ios 1
    assert tiles.merge([r0, half], [[0, 0], [0, 0]], 1, 30, 0.5, 'iou')[1].tolist() == [0, 1]       # exactly at the threshold: kept
    assert tiles.merge([r0, half], [[0, 0], [0, 0]], 1, 30, 0.5, 'ios')[1].tolist() == [0]
    assert tiles.merge([r0, half], [[0, 0], [0, 0]], 1, 30, 0.4375, 'iou')[1].tolist() == [0]
    # rows outside the class range, a NaN score and an empty box
    odd = np.asarray([[0, 0, 5, 5, 0.5, -1], [0, 0, 5, 5, 0.5, 2], [0, 0, 5, 5, np.nan, 0], [30, 30, 30, 40, 0.125, 1]], np.float32)
    rows, idx = tiles.merge([r0, odd], [[0, 0], [0, 0]], 2, 30, 0.5, 'ios')
    assert idx.tolist() == [0, 4] and rows[1].tolist() == [30, 30, 30, 40, 0.125, 1]
    # the cap, and no tiles at all
    many = np.asarray([[0, 20 * i, 10, 20 * i + 10, 0.5, 0] for i in range(7)], np.float32)
    assert tiles.merge([many], [[0, 0]], 1, 3, 0.5, 'ios')[1].tolist() == [0, 1, 2]
    assert tiles.merge([np.zeros((0, 6), np.float32)] * 3, np.zeros((3, 2)), 4, 30, 0.5, 'ios')[0].shape == (0, 6)

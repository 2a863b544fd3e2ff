"""Sliced inference on the GPU: yk_letterbox_tiles_u8 against yk_letterbox_u8 on a contiguous copy of every crop,
yk_merge_tiles against tiles.merge, both bit for bit, and detect.run(tiles=...) against the untiled path composed by hand.

The merge, beyond the cases that came with it (threshold, ties, cap, empty tiles, 1 and 80 classes, 65 tiles of one class on both paths, the
refusals), on the inputs of tests/tile_cases.py, each of which tests/test_tile_cases.py shows to sit where it claims, and each asked of
engine.merge_tiles_lds_candidates for its path before it runs:
  two_classes_global_small    two classes of ONE picture off LDS at lds_cap 64, six more in LDS beside them; rows that are not decode-shaped
  four_classes_global_stride8 the same with 16 classes and classes 0, 1, 8, 9 off LDS: workgroups 8 apart share a cache on a device of 8 dies, and
                              only there do two segments that overlap show (measured: with `seg` dropped from the segment base this case fails and
                              two_classes_global_small passes)
  boundary-64 / -65           n == lds_cap (the last LDS case) and lds_cap + 1 (the first global one; the extra candidate is the picture's best)
  two_classes_global_decode_shaped, three_pictures_mixed
                              2 x 2112 candidates at lds_cap 2048, both metrics; four segments in two list regions around a small picture
  dropped_rows                counted rows with score NaN / -inf and class -1 / C / 1.5 / NaN vanish; +inf wins; -0.0 is a score and keeps its sign
  box_edges                   swapped corners, zero-area boxes, thresh 0 (touching stays, one shared cell goes), thresh +inf (the cap ends it)
  far_origin, far_origin_touch   origins (4000.3, 2999.7), (-0.1, 1e-3): the rows are the float32 sums and the decisions are made on those
  ties                        equal scores across tiles and across one lane's entries i and i + 64, in LDS and in global memory
  clamps                      the C entry point with counts [cap + 5, -3, 7] and first [0, 5, 2] / [-1, 2] / [0, n_tiles + 4]
Rows are compared as int32 patterns (so -0.0 is not 0.0); d_out is filled with a sentinel first and every row beyond a picture's count must
still hold it (the kernel writes the counted rows only).  three_pictures_mixed twice gives the same bytes; the call is captured
in a graph (memset + two kernel nodes, nothing run meanwhile) and replayed on rows A, B, A.
Measured on the MI355X: the whole file (48 tests) 3.0 - 4.0 s, of which 1.6 - 2.7 s is the first test's set-up (library and device); every merge
test under 0.05 s, the largest new ones (three_pictures_mixed, 8.6k rows; the graph replay) 0.02 s."""
import ctypes as C

import numpy as np
import pytest

from k210_yolo_framework_amd import draw, tiles
from tests import tile_cases

pytestmark = pytest.mark.gpu
F = np.float32


# ---------------------------------------------------------------------------------------------------- the tile letterbox
PICTURES = [(1, 1), (5, 7), (33, 47), (64, 48)]
GRIDS = [(1, 1, 0.2), (2, 2, 0.0), (2, 2, 0.2), (3, 1, 0.5)]


def _packed_with_gaps(torch, shapes, seed):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]       # no zero byte: a tap that leaves the tile shows
    packed, table, _ = draw.pack_ragged(imgs, gap=5)
    flat = packed.numpy()
    used = np.zeros(flat.size, bool)
    for r in table:
        used[int(r['offset']):int(r['offset']) + 3 * int(r['h']) * int(r['w'])] = True
    flat[~used] = 255                                                                 # the gaps are not zero either
    return imgs, table, packed.cuda()


@pytest.mark.parametrize('dst', [(32, 48), (224, 320)])
def test_tile_letterbox_equals_letterbox_of_the_contiguous_crop(dst):
    import torch
    from k210_yolo_framework_amd import engine
    shapes = PICTURES + [(9, 9)]
    imgs, table, d_packed = _packed_with_gaps(torch, shapes, 3)
    crops, rows = [], []
    for i, (im, (h, w)) in enumerate(zip(imgs, shapes)):
        for nx, ny, ov in ([(8, 8, 0.2)] if (h, w) == (9, 9) else GRIDS):
            g = tiles.grid(h, w, nx, ny, ov)
            rows.append(tiles.table_rows(g, int(table['offset'][i]), w))
            crops += [np.ascontiguousarray(im[y0:y0 + th, x0:x0 + tw]) for y0, x0, th, tw in g]
    rows = np.concatenate(rows)
    assert len(rows) == len(crops) == 4 * (2 + 5 + 5 + 4) + 65
    out = engine.letterbox_tiles_u8(d_packed, rows, dst)
    torch.cuda.synchronize()
    for t, crop in enumerate(crops):
        ref = engine.letterbox_u8(torch.from_numpy(crop[None]).cuda(), dst)[0]
        assert torch.equal(out[t], ref), (t, crop.shape, dst)


def _device_table(torch, engine, rows, dst):
    t = np.array(rows, dtype=tiles.TILE_DTYPE, copy=True)
    engine.call('yk_letterbox_tiles_params', t, len(t), dst[0], dst[1])
    return t


def test_tile_letterbox_bad_rows_give_zero_frames_next_to_good_ones():
    import torch
    from k210_yolo_framework_amd import engine
    dst = (32, 48)
    imgs, table, d_packed = _packed_with_gaps(torch, [(33, 47), (64, 48)], 4)
    g = tiles.grid(64, 48, 2, 2, 0.2, full=False)
    good = _device_table(torch, engine, tiles.table_rows(g, int(table['offset'][1]), 48), dst)
    want = engine.letterbox_tiles_u8(d_packed, good, dst)
    assert all(want[t].any().item() for t in range(4))
    nbytes = d_packed.numel()
    spoil = [('h', 0), ('w', -3), ('stride', 3 * int(good['w'][2]) - 1), ('offset', nbytes - int(good['stride'][3]) * (int(good['h'][3]) - 1) - 3 * int(good['w'][3]) + 1)]
    for k, (field, value) in enumerate(spoil):
        bad = good.copy()
        bad[field][k] = value
        with pytest.raises(engine.YkError, match=f'tile table: row {k}'):
            engine.check_tile_rows(bad, nbytes)
        d_table = torch.from_numpy(bad.view(np.uint8).reshape(4, 40)).cuda()
        out = engine.letterbox_tiles_u8(d_packed, d_table, dst)
        torch.cuda.synchronize()
        for t in range(4):
            assert torch.equal(out[t], torch.zeros_like(out[t]) if t == k else want[t]), (field, t)
    # the last byte of the buffer itself is a legal last byte
    edge = good.copy()
    edge['offset'][3] = spoil[3][1] - 1
    engine.check_tile_rows(edge, nbytes)
    assert engine.letterbox_tiles_u8(d_packed, edge, dst)[3].any().item()
    L = engine.lib()
    d_table = torch.from_numpy(good.view(np.uint8).reshape(4, 40)).cuda()
    assert L.yk_letterbox_tiles_u8(d_packed, nbytes, d_table, 0, want, 32, 48, None) == -10
    assert L.yk_letterbox_tiles_u8(None, nbytes, d_table, 4, want, 32, 48, None) == -10
    assert L.yk_letterbox_tiles_u8(d_packed, nbytes, d_table, 4, want, 0, 48, None) == -10
    assert L.yk_letterbox_tiles_params(good.copy(), 0, 32, 48) == -10


def test_tile_letterbox_recorded_in_a_graph_and_replayed():
    import torch
    from k210_yolo_framework_amd import engine
    dst = (32, 48)
    imgs, table, d_packed = _packed_with_gaps(torch, [(33, 47), (5, 7)], 5)
    rows = np.concatenate([tiles.table_rows(tiles.grid(33, 47, 2, 2, 0.2), int(table['offset'][0]), 47),
                           tiles.table_rows(tiles.grid(5, 7, 3, 1, 0.5), int(table['offset'][1]), 7)])
    d_table = engine.tile_table_to_device(rows, dst, d_packed.numel(), d_packed.device)
    eager = engine.letterbox_tiles_u8(d_packed, d_table, dst)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    graph = engine.capture(st, lambda: engine.call('yk_letterbox_tiles_u8', d_packed, d_packed.numel(), d_table, len(rows), out, dst[0], dst[1], st))
    try:
        assert graph.kernel_nodes == 1
        stream.synchronize()
        assert not out.any().item()                                 # recorded, not executed
        graph.launch(st)
        stream.synchronize()
        assert torch.equal(out, eager)
    finally:
        graph.close()


# ---------------------------------------------------------------------------------------------------- the merge
def _run_merge(rows_per_tile, origins, first, class_num, max_out, thresh, metric):
    """-> per picture (rows, count) from the device, checked against tiles.merge bit for bit."""
    import torch
    from k210_yolo_framework_amd import engine
    cap = class_num * max_out
    n = len(rows_per_tile)
    dets = np.full((n, cap, 6), np.nan, F)                           # unused rows hold NaN: reading one would show
    counts = np.zeros(n, np.int32)
    for t, r in enumerate(rows_per_tile):
        r = np.asarray(r, F).reshape(-1, 6)
        dets[t, :len(r)] = r
        counts[t] = len(r)
    out, out_counts = engine.merge_tiles(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(), np.asarray(origins, F), np.asarray(first, np.int32),
                                         class_num, max_out, thresh, metric)
    torch.cuda.synchronize()
    got = []
    for p in range(len(first) - 1):
        a, b = first[p], first[p + 1]
        want, _ = tiles.merge([np.asarray(r, F).reshape(-1, 6) for r in rows_per_tile[a:b]], np.asarray(origins, F).reshape(-1, 2)[a:b], class_num, max_out,
                              thresh, metric)
        k = int(out_counts[p])
        assert k == len(want), (p, k, len(want))
        assert torch.equal(out[p, :k].cpu(), torch.from_numpy(want)), p
        got.append(want)
    return got


def _seeded_tiles(seed, n_tiles, k, class_num, side=96):
    """Float coordinates, scores from eight values (ties are common), every tile full."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_tiles):
        t, l = rng.uniform(0, side, k), rng.uniform(0, side, k)
        rows.append(np.stack([t, l, t + rng.uniform(1, 32, k), l + rng.uniform(1, 32, k), rng.integers(1, 9, k) / 8.0,
                              rng.integers(0, class_num, k)], 1).astype(F))
    return rows, rng.integers(0, side, (n_tiles, 2)).astype(F)


def test_merge_one_tile_at_origin_zero_returns_the_decodes_rows():
    """What the decode's own hard NMS kept at iou_thresh survives a second pass of the same rule at the same threshold, in the same order."""
    import torch
    from k210_yolo_framework_amd import engine, softnms
    rng = np.random.default_rng(11)
    class_num, max_out, iou_thresh = 3, 30, 0.3
    t, l = rng.uniform(0, 80, 200), rng.uniform(0, 80, 200)
    boxes = np.stack([t, l, t + rng.uniform(2, 40, 200), l + rng.uniform(2, 40, 200)], 1).astype(F)
    scores = (rng.integers(1, 17, (200, class_num)) / 16.0).astype(F)
    rows, _ = softnms.decode_image(boxes, scores, 0.25, iou_thresh, max_out, 'hard')
    assert 10 < len(rows) <= class_num * max_out
    got = _run_merge([rows], [[0.0, 0.0]], [0, 1], class_num, max_out, iou_thresh, 'iou')[0]
    assert got.shape == rows.shape and bool((got == rows).all())


def test_merge_small_cases():
    A = [10, 10, 20, 20, 0.5, 0]
    half = [10, 10, 20, 15, 0.25, 0]                                 # inside A, half its area: IoU exactly 0.5, IoS 1
    both = lambda r0, r1, thr, metric, o1=(0, 0): _run_merge([[r0], [r1]], [[0, 0], list(o1)], [0, 2], 1, 30, thr, metric)[0].tolist()
    assert both(A, half, 0.4375, 'iou') == [A]                       # above
    assert both(A, half, 0.5625, 'iou') == [A, half]                 # below
    assert both(A, half, 0.5, 'iou') == [A, half]                    # exactly at the threshold: kept, the rule is >
    assert both(A, half, 0.5, 'ios') == [A]                          # a small box inside a large one
    assert both(A, [0, 0, 10, 10, 0.75, 0], 0.5, 'ios', (10, 10)) == [[10, 10, 20, 20, 0.75, 0]]        # one object, two tiles: the better score
    assert both(A, [1, 1, 11, 11, 0.5, 0], 0.5, 'ios', (10, 10)) == [A]                                  # equal scores: the lower candidate index
    assert both([1, 1, 11, 11, 0.5, 0], A, 0.5, 'ios', (-10, -10)) == [[1, 1, 11, 11, 0.5, 0]]
    # more than max_out survivors in a class; a row of class -1 and one of class C; tiles with count 0
    many = [[0, 20 * i, 10, 20 * i + 10, 0.5 + i / 64, 1] for i in range(6)]
    odd = [[0, 0, 5, 5, 0.875, -1], [0, 0, 5, 5, 0.875, 2], A, [50, 50, 60, 60, 0.25, 1.5]]
    got = _run_merge([[], many, [], odd, []], np.zeros((5, 2)), [0, 5], 2, 3, 0.5, 'ios')[0].tolist()
    assert got == [A, many[5], many[4], many[3]]
    assert _run_merge([[], [], []], np.zeros((3, 2)), [0, 3], 2, 3, 0.5, 'ios')[0].shape == (0, 6)


@pytest.mark.parametrize('class_num, metric', [(1, 'ios'), (80, 'iou'), (80, 'ios')])
def test_merge_several_pictures_with_unequal_tile_numbers(class_num, metric):
    max_out = 5
    k = min(class_num * max_out, 60)
    rows, origins = _seeded_tiles(class_num, 71, k, class_num)
    rows[3] = rows[3][:0]                                            # some tiles are empty
    rows[40] = rows[40][:7]
    got = _run_merge(rows, origins, [0, 1, 6, 71], class_num, max_out, 0.5, metric)
    assert [len(g) > 0 for g in got] == [True] * 3
    _run_merge(rows[:5], origins[:5], [0, 5], class_num, max_out, 0.5, metric)       # and one picture alone


@pytest.mark.parametrize('max_out, path', [(30, 'lds'), (100, 'global')])
def test_merge_65_tiles_in_one_class_on_both_paths(max_out, path):
    """65 tiles x max_out candidates, all of one class: 1950 are staged in LDS, 6500 are walked in global memory - asked of the library for
    this device, not assumed."""
    from k210_yolo_framework_amd import engine
    n = 65 * max_out
    lds = engine.merge_tiles_lds_candidates(65, 1, max_out)
    assert (n <= lds) == (path == 'lds'), (n, lds)
    rows, origins = _seeded_tiles(max_out, 65, max_out, 1, side=400)
    got = _run_merge(rows, origins, [0, 65], 1, max_out, 0.5, 'ios')[0]
    assert len(got) == max_out                                       # enough separate objects that the cap is what ends the rounds
    # two such pictures and a small one in one call: the global lists of different pictures and classes do not collide
    if path == 'global':
        rows2, origins2 = _seeded_tiles(7, 65, max_out, 1, side=400)
        _run_merge(rows + rows2 + rows[:2], np.concatenate([origins, origins2, origins[:2]]), [0, 65, 130, 132], 1, max_out, 0.5, 'iou')


def test_merge_bad_arguments_are_refused_by_name():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    dets = torch.zeros((2, 6, 6), dtype=torch.float32, device='cuda')
    counts = torch.zeros(2, dtype=torch.int32, device='cuda')
    origin = torch.zeros((2, 2), dtype=torch.float32, device='cuda')
    first = torch.tensor([0, 2], dtype=torch.int32, device='cuda')
    out = torch.zeros((1, 6, 6), dtype=torch.float32, device='cuda')
    oc = torch.zeros(1, dtype=torch.int32, device='cuda')
    good = dict(d_dets=dets, d_counts=counts, d_origin=origin, d_first=first, n_tiles=2, n_pics=1, class_num=2, max_out=3, thresh=0.5, metric=1,
                d_out=out, d_out_counts=oc, stream=None)
    assert L.yk_merge_tiles(*good.values()) == 0
    for name, value in [('d_dets', None), ('d_counts', None), ('d_origin', None), ('d_first', None), ('d_out', None), ('d_out_counts', None),
                        ('n_tiles', 0), ('n_pics', 0), ('class_num', 0), ('max_out', 0), ('thresh', float('nan')), ('metric', 2), ('metric', -1),
                        ('n_tiles', 1 << 30)]:
        assert L.yk_merge_tiles(*{**good, name: value}.values()) == -10, name
        assert name in L.yk_last_error().decode(), (name, L.yk_last_error())
    torch.cuda.synchronize()
    with pytest.raises(engine.YkError, match='tile_match'):
        engine.merge_tiles(dets, counts, origin, first, 2, 3, 0.5, 'giou')


# ---------------------------------------------------------------------------------------------------- the merge on tests/tile_cases.py
CASES = tile_cases.all_cases()
CLAMPS = tile_cases.clamps()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


class _Device:
    """The buffers of one yk_merge_tiles call: rows beyond a tile's count hold NaN (reading one would show), d_out holds SENTINEL and
    d_out_counts -1 before every call."""

    def __init__(self, case):
        import torch
        self.cap = case.class_num * case.max_out
        self.n_tiles, self.n_pics = len(case.rows), len(case.first) - 1
        self.dets = torch.empty((self.n_tiles, self.cap, 6), dtype=torch.float32, device='cuda')
        self.counts = torch.empty(self.n_tiles, dtype=torch.int32, device='cuda')
        self.origins = torch.empty((self.n_tiles, 2), dtype=torch.float32, device='cuda')
        self.first = torch.from_numpy(np.asarray(case.first, np.int32)).cuda()
        self.out = torch.empty((self.n_pics, self.cap, 6), dtype=torch.float32, device='cuda')
        self.out_counts = torch.empty(self.n_pics, dtype=torch.int32, device='cuda')
        self.load(case)

    def load(self, case):
        import torch
        dets = np.full((self.n_tiles, self.cap, 6), np.nan, F)
        for t, r in enumerate(case.rows):
            dets[t, :len(r)] = r
        self.dets.copy_(torch.from_numpy(dets))
        self.counts.copy_(torch.from_numpy(np.asarray([len(r) for r in case.rows], np.int32)))
        self.origins.copy_(torch.from_numpy(case.origins.copy()))
        self.clear()

    def clear(self):
        self.out.fill_(tile_cases.SENTINEL)
        self.out_counts.fill_(-1)

    def untouched(self):
        return bool((self.out == tile_cases.SENTINEL).all().item()) and bool((self.out_counts == -1).all().item())

    def check(self, want, what):
        """counts and rows equal to the reference bit for bit, and every row beyond a picture's count left as it was"""
        import torch
        assert self.out_counts.tolist() == [len(w) for w in want], (what, self.out_counts.tolist(), [len(w) for w in want])
        for p, w in enumerate(want):
            assert torch.equal(_bits(self.out[p, :len(w)]).cpu(), _bits(torch.from_numpy(np.array(w, F, copy=True)).reshape(-1, 6))), (what, p)
            assert bool((self.out[p, len(w):] == tile_cases.SENTINEL).all().item()), (what, p)


def _path_is_the_claimed_one(engine, case):
    cap = engine.merge_tiles_lds_candidates(len(case.rows), len(case.first) - 1, case.max_out)
    assert cap == tile_cases.case_lds_cap(case) == case.claims['lds_cap'], (case.name, cap)
    assert [[c for c, n in enumerate(per) if n > cap] for per in tile_cases.candidates(case)] == case.claims['over'], case.name


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_merge_cases_equal_the_reference_bit_for_bit(case):
    import torch
    from k210_yolo_framework_amd import engine
    _path_is_the_claimed_one(engine, case)
    d = _Device(case)
    engine.merge_tiles(d.dets, d.counts, d.origins, d.first, case.class_num, case.max_out, case.thresh, case.metric, out=d.out, out_counts=d.out_counts)
    torch.cuda.synchronize()
    want = [rows for rows, _ in tile_cases.reference(case)]
    d.check(want, case.name)
    if 'first_row' in case.claims:                                   # boundary: the candidate at position lds_cap is the picture's best
        assert torch.equal(_bits(d.out[0, 0]).cpu(), _bits(torch.from_numpy(case.claims['first_row'].copy())))
    if 'class2' in case.claims:                                      # dropped_rows: +inf first, -0.0 last and still negative
        got = d.out[0, :len(want[0])].cpu().numpy()
        assert np.array_equal(got[got[:, 5] == 2].view(np.int32), np.asarray(case.claims['class2'], F).view(np.int32))


@pytest.mark.parametrize('case', CLAMPS, ids=[c.name for c in CLAMPS])
def test_merge_clamps_counts_and_first_on_the_device(case):
    """Tables engine.merge_tiles never sees from the pipeline and the C entry point takes: counts [cap + 5, -3, 7] are read as [cap, 0, 7],
    first [0, 5, 2] / [-1, 2] / [0, n_tiles + 4] as [0, 3, 2] (the second picture empty) / [0, 2] / [0, 3].  A row out of reach has the best
    score there is, so one read shows as the first row."""
    import torch
    from k210_yolo_framework_amd import engine
    cap = case.class_num * case.max_out
    dets = torch.from_numpy(case.dets.copy()).cuda()
    counts, origins, first = torch.from_numpy(case.counts.copy()).cuda(), torch.from_numpy(case.origins.copy()).cuda(), torch.from_numpy(case.first.copy()).cuda()
    out = torch.full((case.n_pics, cap, 6), tile_cases.SENTINEL, dtype=torch.float32, device='cuda')
    out_counts = torch.full((case.n_pics,), -1, dtype=torch.int32, device='cuda')
    engine.call('yk_merge_tiles', dets, counts, origins, first, case.n_tiles, case.n_pics, case.class_num, case.max_out, case.thresh,
                tiles.metric_id(case.metric), out, out_counts, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert out_counts.tolist() == [len(w) for w in case.want], case.name
    for p, w in enumerate(case.want):
        assert torch.equal(_bits(out[p, :len(w)]).cpu(), _bits(torch.from_numpy(w.copy()).reshape(-1, 6))), (case.name, p)
        assert bool((out[p, len(w):] == tile_cases.SENTINEL).all().item()), (case.name, p)


def test_merge_two_runs_of_four_global_segments_give_the_same_bytes():
    """three_pictures_mixed twice (twice only): where each class's segment lands in its picture's list depends on which wave reaches the cursor
    first; what comes out does not."""
    import torch
    from k210_yolo_framework_amd import engine
    case = next(c for c in CASES if c.name == 'three_pictures_mixed-ios')
    runs = []
    for _ in range(2):
        d = _Device(case)
        engine.merge_tiles(d.dets, d.counts, d.origins, d.first, case.class_num, case.max_out, case.thresh, case.metric, out=d.out, out_counts=d.out_counts)
        torch.cuda.synchronize()
        runs.append((d.out.cpu(), d.out_counts.cpu()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][1].tolist() == [len(rows) for rows, _ in tile_cases.reference(case)]


def test_merge_recorded_in_a_graph_and_replayed_on_new_rows():
    """The cursor's memset and both kernels are recorded (nothing runs during the capture) and the per-stream scratch survives: the replay reads
    the rows that are in the buffers when it runs - seed A, then B, then A again, each equal to the reference of its own rows."""
    import torch
    from k210_yolo_framework_amd import engine
    a, b = tile_cases.two_classes_global_decode_shaped('ios', seed=3), tile_cases.two_classes_global_decode_shaped('ios', seed=13)
    _path_is_the_claimed_one(engine, a)
    _path_is_the_claimed_one(engine, b)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    with torch.cuda.stream(stream):
        d = _Device(a)
        issue = lambda: engine.call('yk_merge_tiles', d.dets, d.counts, d.origins, d.first, d.n_tiles, d.n_pics, a.class_num, a.max_out, a.thresh,
                                    tiles.metric_id(a.metric), d.out, d.out_counts, st)
        issue()                                                     # eagerly once: the stream's scratch exists before the capture
        stream.synchronize()
        d.check([rows for rows, _ in tile_cases.reference(a)], 'eager')
        d.clear()
        stream.synchronize()
        graph = engine.capture(st, issue)
        try:
            assert graph.kernel_nodes == 2
            stream.synchronize()
            assert d.untouched()                                    # recorded, not executed
            for case in (a, b, a):
                d.load(case)
                stream.synchronize()
                graph.launch(st)
                stream.synchronize()
                d.check([rows for rows, _ in tile_cases.reference(case)], case.name)
        finally:
            graph.close()


# ---------------------------------------------------------------------------------------------------- end to end
SIZES = [(48, 64), (75, 100), (67, 50)]
OBJ, IOU = 0.5, 0.3                 # seeded random weights score high: at 0.5 most classes stay under the cap of 30


@pytest.fixture(scope='module')
def net():
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.yolonet import YoloModel
    from tests.plan_zoo import residual
    spec, weights = residual()
    H, W = spec.in_hw
    model = YoloModel(spec, {'weights': weights, 'precision': 'f16x2'}, False)
    h = Helper(None, 20, VOC_ANCHORS, np.array([[H, W]]), np.array([list(x) for x in spec.out_hw()]))
    rng = np.random.default_rng(21)
    pics = [rng.integers(0, 256, SIZES[i % 3] + (3,), dtype=np.uint8) for i in range(5)]
    yield h, model, pics
    model._drop_plan()


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def test_detect_one_tile_is_the_untiled_path(net, tmp_path):
    import json
    from k210_yolo_framework_amd import detect
    h, model, pics = net
    kw = dict(draw=False, batch=4, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False)
    plain = detect.run(h, model, pics, out_dir=tmp_path / 'plain', **kw)
    one = detect.run(h, model, pics, out_dir=tmp_path / 'one', tiles=(1, 1), tile_full=False, tile_match='iou', tile_thresh=IOU, **kw)
    assert sum(len(d) for d in plain['detections']) > 0
    assert _same(one['detections'], plain['detections'])
    a, b = json.loads((tmp_path / 'plain' / 'detections.json').read_text()), json.loads((tmp_path / 'one' / 'detections.json').read_text())
    assert 'tiles' not in a[0] and b[0]['tiles'] == [1, 1] and b[0]['tile_match'] == 'iou' and b[0]['tile_full'] is False
    assert [d['detections'] for d in a] == [d['detections'] for d in b]
    with pytest.raises(Exception, match="nms 'linear' with tiles"):
        detect.run(h, model, pics, tiles=(2, 2), nms='linear', **kw)


def test_detect_2x2_is_the_untiled_path_on_the_crops_then_the_host_merge(net):
    from k210_yolo_framework_amd import detect
    from tests.test_gpu_draw import paint
    h, model, pics = net
    kw = dict(batch=12, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False)
    got = detect.run(h, model, pics, draw=True, return_arrays=True, tiles=(2, 2), **kw)          # 5 frames a picture: 2 pictures a batch, 3 batches
    grids = [tiles.grid(p.shape[0], p.shape[1], 2, 2, 0.2) for p in pics]
    crops = [np.ascontiguousarray(p[y0:y0 + th, x0:x0 + tw]) for p, g in zip(pics, grids) for y0, x0, th, tw in g]
    per_crop = detect.run(h, model, crops, draw=False, **kw)['detections']
    want = [tiles.merge(per_crop[5 * i:5 * i + 5], grids[i][:, :2].astype(F), 20, 30, 0.5, 'ios')[0] for i in range(len(pics))]
    print('rows per picture, tiled:', [len(w) for w in want], 'of', [sum(len(r) for r in per_crop[5 * i:5 * i + 5]) for i in range(len(pics))], 'candidates')
    assert sum(len(w) for w in want) > 0
    assert _same(got['detections'], want)
    atlas, colours = draw.glyph_atlas(), np.asarray(h.colormap, np.uint8).reshape(-1, 3)
    for i, p in enumerate(pics):
        hh, ww = p.shape[:2]
        assert np.array_equal(got['arrays'][i], paint(p.copy(), want[i], colours, atlas, draw.thickness_of(hh, ww), draw.magnification_of(hh))), i


def test_evaluate_takes_the_same_options(net):
    """evaluate.run with one tile per picture scores the rows it scores without tiles; with 2x2 it scores detect.run's merged rows."""
    from argparse import Namespace
    from k210_yolo_framework_amd import detect, evaluate
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    h, model, pics = net
    items = [(p, np.asarray([[0, 0.5, 0.5, 0.25, 0.25]])) for p in pics]
    base = dict(batch=10, depth=2, precision='f16x2', obj_thresh=OBJ, nms_iou=IOU, nms='hard', nms_sigma=0.5, tile_overlap=0.2, tile_thresh=0.5)

    def rows(**kw):
        ev = MapEvaluator(20, 0.5, False)
        evaluate.run(Namespace(**{**base, **kw}), h, model, items, ev)
        r, img = ev.rows()
        return [r[img == i] for i in range(len(pics))]

    plain = rows(tiles=None, tile_full=True, tile_match='ios')
    assert sum(len(r) for r in plain) > 0
    assert _same(rows(tiles=(1, 1), tile_full=False, tile_match='iou', tile_thresh=IOU), plain)
    want = detect.run(h, model, pics, draw=False, batch=10, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False, tiles=(2, 2))['detections']
    assert _same(rows(tiles=(2, 2), tile_full=True, tile_match='ios'), want)
    with pytest.raises(Exception, match="nms 'diou' with tiles"):
        rows(tiles=(2, 2), tile_full=True, tile_match='ios', nms='diou')

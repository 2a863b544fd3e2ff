"""Training labels built on the GPU (csrc/yk_label.hip: yk_boxes_to_labels_f32; engine.boxes_to_labels; InputPipeline(labels='gpu')): every
comparison is bit for bit against Helper.batch_box_to_label, in both assignment modes, at the smallest shapes where the kernel can go
another way - grids of 6 floats, chunks that begin and end inside a slot, samples at the LDS table's size and one past it, slot
conflicts at every priority, ties, the edges of the clip and the floor - then the status word, determinism, capture, and the pipeline."""
import ctypes as C
import re

import numpy as np
import pytest

from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS

pytestmark = pytest.mark.gpu
CLEAN = 2 ** 31 - 1
MODES = [('best', 0.213), ('multi', 0.213)]


def _define(name):
    from k210_yolo_framework_amd import engine
    return int(re.search(rf'#define {name} (\d+)', engine.HEADER_PATH.read_text()).group(1))


def _helper(out_hw, anchor_num, class_num, seed=0, anchors=None):
    if anchors is None:
        anchors = np.random.default_rng(seed).uniform(0.05, 0.9, (len(out_hw), anchor_num, 2))
    return Helper(None, class_num, np.asarray(anchors, float), [[32 * out_hw[0][0], 32 * out_hw[0][1]]], out_hw)


SHAPES = {'1x1': lambda: _helper([[1, 1]], 1, 1),                                                  # 6 floats per sample
          'voc': lambda: Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]]),          # 25 floats per slot: 5250 and 21000 per sample
          'three': lambda: _helper([[2, 2], [4, 4], [8, 8]], 3, 80, seed=1),                        # 85 floats per slot
          'max': lambda: _helper([[3, 5], [6, 10], [12, 20], [5, 7]], 8, 3, seed=2)}                # YK_MAX_LAYERS x YK_MAX_ANCHORS


def _boxes(rng, k, class_num, wh=(0.02, 0.95)):
    return np.column_stack([rng.integers(0, class_num, k).astype(float), rng.random((k, 2)), rng.uniform(*wh, (k, 2))]).reshape(-1, 5)


def _in_grid(h: Helper, b: np.ndarray) -> np.ndarray:
    """Rows whose numpy cell lies inside every layer's grid (a cell that rounds up to w or h is the one thing [0, 1) does not rule out)."""
    ok = np.ones(len(b), bool)
    for gh, gw in h.out_hw:
        cell = np.floor(b[:, 1:3] * (gw, gh))
        ok &= (cell[:, 0] >= 0) & (cell[:, 0] < gw) & (cell[:, 1] >= 0) & (cell[:, 1] < gh)
    return ok


def _gpu(h, samples, assign, thr, **kw):
    import torch
    from k210_yolo_framework_amd import engine
    first = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int32)
    allb = np.concatenate([np.reshape(s, (-1, 5)) for s in samples]) if first[-1] else np.zeros((0, 5))
    views, status = engine.boxes_to_labels(allb, first, h, assign, thr, **kw)
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in views], int(status.item())


def _same(got, want):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (l, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f'layer {l}: {len(bad)} entries differ, the first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}')


def _check(h, samples, assign, thr):
    want = h.batch_box_to_label(samples, assign, thr)              # must run: no IndexError
    got, status = _gpu(h, samples, assign, thr)
    _same(got, want)
    assert status == CLEAN
    return want


def test_the_constants_are_the_headers():
    from k210_yolo_framework_amd import engine
    assert (_define('YK_MAX_LAYERS'), _define('YK_MAX_ANCHORS')) == (engine.YK_MAX_LAYERS, engine.YK_MAX_ANCHORS) == (4, 8)
    h = SHAPES['max']()
    assert h.anchors.shape == (4, 8, 2)
    assert _define('YK_LABEL_LDS_BOXES') >= 64 and _define('YK_LABEL_CHUNK') % 4 == 0


@pytest.mark.parametrize('assign, thr', MODES, ids=['best', 'multi'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_random_boxes_and_box_counts(shape, assign, thr):
    """0 boxes for every sample, for some, 1, a few: random centres in [0, 1); a row whose numpy cell is out of range is dropped first
    (none is: see test_status_names_the_smallest_box_numpy_could_not_write)."""
    h = SHAPES[shape]()
    rng = np.random.default_rng(5)
    n = 3 if shape == '1x1' else 6
    empty = [np.zeros((0, 5))] * n
    want = _check(h, empty, assign, thr)
    assert not any(w.any() for w in want)
    drawn = kept = 0
    samples = []
    for i, k in enumerate([1, 0, 9, 0, 2, 30][:n]):
        b = _boxes(rng, k, h.class_num)
        ok = _in_grid(h, b)
        drawn, kept = drawn + len(b), kept + int(ok.sum())
        samples.append(b[ok])
    assert kept >= 0.95 * drawn
    want = _check(h, samples, assign, thr)
    assert all(w[1].any() == 0 for w in want) and any(w[0].any() for w in want)
    _check(h, [samples[0]] + empty[1:], assign, thr)                # one box in the whole batch


@pytest.mark.parametrize('assign, thr', MODES, ids=['best', 'multi'])
def test_samples_around_the_lds_table(assign, thr):
    """cap - 1, cap and cap + 1 boxes in one sample, beside small ones: the table in one tile, full, and walked in two."""
    h = SHAPES['voc']()
    cap = _define('YK_LABEL_LDS_BOXES')
    rng = np.random.default_rng(8)
    for k in (cap - 1, cap, cap + 1):
        big = _boxes(rng, k + 40, 20)
        big = big[_in_grid(h, big)][:k]
        assert len(big) == k
        # the last box of the sample wins a slot of its own cell against an earlier one: a key from the second tile beats the first
        big[-1, 1:5] = big[0, 1:5]
        big[-1, 0] = (big[0, 0] + 1) % 20
        want = _check(h, [_boxes(rng, 2, 20) * [1, .99, .99, 1, 1], big, np.zeros((0, 5)), _boxes(rng, 3, 20) * [1, .99, .99, 1, 1]], assign, thr)
        hot = [w[1][w[1][..., 4] == 1] for w in want]
        assert any((s[:, 5:].sum(1) > 1).any() for s in hot)        # class bits did accumulate somewhere


@pytest.mark.parametrize('thr', [0.213, 0.01, 0.99])
def test_collisions_in_one_cell(thr):
    """Many boxes drawn into one cell and near one anchor shape: primaries over primaries, secondaries under primaries, secondaries over
    secondaries, class bits from all.  0.01: almost every (layer, anchor) is a candidate; 0.99: none is."""
    h = SHAPES['voc']()
    rng = np.random.default_rng(13)
    k = 60
    wh = VOC_ANCHORS[1, 1] * rng.uniform(0.5, 2.0, (k, 2))           # around one anchor: the primary moves between it and its neighbours
    xy = np.array([0.52, 0.52]) + rng.uniform(0, 0.04, (k, 2))       # column 5 / 10, row 3 / 7 in both layers
    crowd = np.column_stack([rng.integers(0, 20, k).astype(float), xy, np.clip(wh, 0.01, 1.0)])
    samples = [crowd, _boxes(rng, 4, 20) * [1, .99, .99, 1, 1], crowd[::-1].copy()]
    want = _check(h, samples, 'multi', thr)
    best = _check(h, samples, 'best', thr)
    pos = lambda ws: int(sum((w[..., 4] == 1).sum() for w in ws))
    assert pos(want) == pos(best) if thr == 0.99 else pos(want) > pos(best)
    assert max(int(w[0][..., 5:].sum(-1).max()) for w in want) > 3
    if thr == 0.01:
        assert (want[0][0, 3, 5, :, 4] == 1).all() and (want[1][0, 7, 10, :, 4] == 1).all()          # every anchor of the crowd's cells


@pytest.mark.parametrize('assign, thr', MODES, ids=['best', 'multi'])
def test_ties_take_the_first_argmax(assign, thr):
    anchors = np.array([[[0.3, 0.4], [0.3, 0.4], [0.7, 0.2]], [[0.7, 0.2], [0.3, 0.4], [0.1, 0.1]]])     # equal across anchors and across layers
    h = _helper([[3, 4], [6, 8]], 3, 4, anchors=anchors)
    boxes = np.array([[0, 0.3, 0.3, 0.3, 0.4], [1, 0.6, 0.6, 0.7, 0.2], [2, 0.9, 0.1, 0.35, 0.35], [3, 0.1, 0.9, 0.1, 0.1]])
    want = _check(h, [boxes, boxes[::-1].copy()], assign, thr)
    assert want[0][0, 0, 1, 0, 4] == 1 and want[0][0, 1, 2, 2, 4] == 1            # the first of the equal anchors, the first of the equal layers
    if assign == 'best':
        assert want[0][0, 0, 1, 1, 4] == 0 and want[1][0, 3, 4, 0, 4] == 0


@pytest.mark.parametrize('assign, thr', MODES, ids=['best', 'multi'])
def test_edges_of_the_clip_and_the_floor(assign, thr):
    h = SHAPES['voc']()
    rows = []
    for w, hh in [(0.0, 0.3), (0.3, 0.0), (0.0, 0.0), (1e-9, 0.2), (0.2, 5e-9), (1.5, 0.4), (0.4, 2.0), (1.0, 1.0), (1e-8, 1e-8), (3.0, 3.0)]:
        rows.append([len(rows) % 20, 0.37, 0.81, w, hh])
    for k in range(1, 20):                                           # centres on a cell boundary of the 20-wide layer, and one ulp below it
        for x in (k / 20, np.nextafter(k / 20, 0)):
            rows.append([k, x, min(k / 14, np.nextafter(1.0, 0) * 0.99), 0.2, 0.3])
    for k in range(1, 14):
        for y in (k / 14, np.nextafter(k / 14, 0)):
            rows.append([k, 0.013, y, 0.5, 0.6])
    rows += [[4, np.nextafter(1.0, 0), 0.5, 0.09, 0.15], [5, 0.5, np.nextafter(1.0, 0), 0.7, 0.6]]       # the last column of 20, the last row of 7
    rows += [[0, 0.0, 0.0, 0.3, 0.3], [1, 5e-324, 1e-300, 0.3, 0.3], [2, 0.9999, 0.9999, 0.1, 0.1]]
    b = np.array(rows, float)
    assert _in_grid(h, b).all()
    want = _check(h, [b[:10], b[10:48], b[48:]], assign, thr)
    assert want[0].min() >= 0 and max(w.max() for w in want) == 1
    hot = np.concatenate([w[w[..., 4] == 1][:, :4].ravel() for w in want])
    assert hot.min() == np.float32(1e-8) and hot.max() == 1                       # both ends of the clip were met


@pytest.mark.parametrize('assign, thr', MODES, ids=['best', 'multi'])
def test_status_names_the_smallest_box_numpy_could_not_write(assign, thr):
    h = SHAPES['voc']()
    rng = np.random.default_rng(21)
    # x = nextafter(1, 0) at w = 20 does NOT round to cell 20: x w = w - w 2^-53 lies at least half an ulp below w (exactly half only for a power
    # of two, where the product is exact), so in IEEE double floor(x w) <= w - 1 for every x < 1 and every integer w.  numpy writes that box in
    # column 19, and so must the kernel: it is a clean box here, not an offender
    up = np.nextafter(1.0, 0)
    assert all(np.floor(up * w) == w - 1 for w in (7, 10, 14, 20, 2 ** 20, 2 ** 31 - 1))
    good = [_boxes(rng, k, 20) * [1, .99, .99, 1, 1] for k in (3, 4, 2, 5)]
    # offenders in samples 1, 2 and 3: x = 1.0 (index w: numpy raises), x = -0.1 and y just below 0 (numpy wraps), y = 1.0
    small, large = [7, 0.5, 0.5, 0.09, 0.15], [7, 0.5, 0.5, 0.75, 0.6]            # primary in the 14 x 20 layer / in the 7 x 10 layer
    bad = {1: [[*small[:1], 1.0, *small[2:]]], 2: [[*large[:1], -0.1, *large[2:]], [3, 0.2, -1e-9, 0.3, 0.3]], 3: [[*small[:2], 1.0, *small[3:]]]}
    dirty = [np.concatenate([g[:1], np.array(bad[i], float), g[1:]]) if i in bad else g for i, g in enumerate(good)]
    want = h.batch_box_to_label(good, assign, thr)
    got, status = _gpu(h, dirty, assign, thr)
    _same(got, want)                                                # nothing of an offender is written, everything else is
    assert status == len(good[0]) + 1                               # the first offender's row of the concatenated boxes
    # one offender at the very end of the batch; it is dropped from every layer it would be written to
    one = [g.copy() for g in good]
    one[3] = np.concatenate([good[3], [[5, 1.0, 0.5, *VOC_ANCHORS[1, 1]]]])
    got, status = _gpu(h, one, assign, thr)
    _same(got, want)
    assert status == sum(len(g) for g in good)
    # x = nextafter(1, 0) in the 20-wide and in the 10-wide layer, y likewise: the last column and row, as numpy
    fine = [g.copy() for g in good]
    fine[3] = np.concatenate([good[3], [[5, up, 0.5, *VOC_ANCHORS[1, 1]], [6, up, up, *VOC_ANCHORS[0, 0]], [7, 0.5, up, *VOC_ANCHORS[1, 2]]]])
    last = _check(h, fine, assign, thr)
    assert last[1][3, 7, 19, 1, 4] == 1 and last[0][3, 6, 9, 0, 4] == 1 and last[1][3, 13, 10, 2, 4] == 1
    # a class outside [0, C) is not written either (numpy raises for C, wraps for -1)
    for cls in (20.0, -1.0):
        odd = [g.copy() for g in good]
        odd[0] = np.concatenate([[[cls, 0.5, 0.5, 0.2, 0.2]], good[0]])
        got, status = _gpu(h, odd, assign, thr)
        _same(got, want)
        assert status == 0
    # a fractional class is truncated toward zero, as astype(int) does: -0.5 is class 0 and 19.9 is class 19, both written
    frac = [g.copy() for g in good]
    frac[0] = np.concatenate([[[-0.5, 0.5, 0.5, 0.2, 0.2], [19.9, 0.3, 0.7, 0.6, 0.5]], good[0]])
    _check(h, frac, assign, thr)
    assert _gpu(h, good, assign, thr)[1] == CLEAN


def test_host_arrays_are_checked_before_upload():
    from k210_yolo_framework_amd import engine
    h = SHAPES['voc']()
    b = np.array([[0, 0.5, 0.5, 0.2, 0.2], [1, 0.5, np.nan, 0.2, 0.2]])
    with pytest.raises(engine.YkError, match='box 1 is not finite'):
        engine.boxes_to_labels(b, [0, 1, 2], h)
    with pytest.raises(engine.YkError, match='box 0 is not finite'):
        engine.boxes_to_labels(b[::-1] * [1, 1, 1, np.inf, 1], [0, 2], h)
    for first in ([0, 1], [1, 2], [0, 2, 1, 2], []):
        with pytest.raises(engine.YkError, match='first must ascend'):
            engine.boxes_to_labels(b[:1].repeat(2, 0), first, h)
    with pytest.raises(engine.YkError, match='assign_iou'):
        engine.boxes_to_labels(b[:1], [0, 1], h, 'multi', 1.0)
    views, status = engine.boxes_to_labels(np.zeros((0, 5)), [0], h)           # n = 0: empty views, a clean status
    assert [tuple(v.shape) for v in views] == [(0, 7, 10, 3, 25), (0, 14, 20, 3, 25)] and int(status.item()) == CLEAN


def test_two_streams_a_dirty_buffer_and_a_replayed_capture():
    import torch
    from k210_yolo_framework_amd import engine
    h = SHAPES['voc']()
    rng = np.random.default_rng(34)
    batches = []
    for _ in range(3):
        s = [_boxes(rng, k, 20) * [1, .99, .99, 1, 1] for k in (4, 0, 7, 2)]
        batches.append((np.concatenate(s), np.concatenate([[0], np.cumsum([len(x) for x in s])]).astype(np.int32), s))
    cfg = engine.make_label_cfg(h, 'multi', 0.213)
    want = [h.batch_box_to_label(s, 'multi', 0.213) for _, _, s in batches]
    floats = 4 * (70 + 280) * 75
    # two calls on two streams into buffers full of NaN: the same bits, every element defined
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            out = torch.full((floats,), float('nan'), device='cuda')
            views, status = engine.boxes_to_labels(batches[0][0], batches[0][1], cfg, stream=st, out=out)
        st.synchronize()
        outs.append(out)
        _same([v.cpu().numpy() for v in views], want[0])
        assert int(status.item()) == CLEAN
    assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any()
    # capture one call, replay it on other batches written into the same buffers
    cap = max(len(b) for b, _, _ in batches)
    d_boxes = torch.zeros((cap, 5), dtype=torch.float64, device='cuda')
    d_first = torch.zeros((5,), dtype=torch.int32, device='cuda')
    out = torch.full((floats,), float('nan'), device='cuda')
    status = torch.zeros((1,), dtype=torch.int32, device='cuda')

    def load(k):
        b, f, _ = batches[k]
        d_boxes.zero_()
        d_boxes[:len(b)] = torch.from_numpy(b).cuda()
        d_first.copy_(torch.from_numpy(f).cuda())
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    load(0)
    torch.cuda.synchronize()
    issue = lambda: engine.call('yk_boxes_to_labels_f32', C.byref(cfg), d_boxes, cap, d_first, 4, out, status, st)
    issue()                                                         # eagerly first
    stream.synchronize()
    graph = engine.capture(st, issue)
    try:
        assert graph.kernel_nodes == 1 and graph.nodes >= 2         # the status word's memset, the kernel
        for k in (1, 2, 0):
            load(k)
            out.fill_(float('nan'))
            status.fill_(-5)
            torch.cuda.synchronize()
            graph.launch(st)
            stream.synchronize()
            eager, _ = engine.boxes_to_labels(batches[k][0], batches[k][1], cfg)
            torch.cuda.synchronize()
            at = 0
            for e, w in zip(eager, want[k]):
                assert torch.equal(out[at:at + e.numel()].view(e.shape), e)
                np.testing.assert_array_equal(e.cpu().numpy(), w)
                at += e.numel()
            assert int(status.item()) == CLEAN
    finally:
        graph.close()


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------

HW = (64, 96)
PIPE_MODES = {'plain': dict(), 'augment': dict(augment=True), 'mosaic': dict(mosaic=True), 'mosaic+augment': dict(augment=True, mosaic=True)}


def _pipe_helper():
    return Helper(None, 20, VOC_ANCHORS, [list(HW)], [[2, 3], [4, 6]])


def _items(n=8, seed=6):
    rng = np.random.default_rng(seed)
    items = []
    for k in range(n):
        hw = [(64, 96), (48, 80), (90, 70)][k % 3]
        k_boxes = int(rng.integers(1, 4))
        boxes = np.concatenate([rng.integers(0, 20, (k_boxes, 1)).astype(float), rng.uniform(0.2, 0.8, (k_boxes, 2)), rng.uniform(0.05, 0.3, (k_boxes, 2))], 1)
        items.append((rng.integers(0, 256, (*hw, 3), dtype=np.uint8), boxes))
    return items


def _run(h, items, cache=None, augment=False, mosaic=False, **kw):
    from k210_yolo_framework_amd import pipeline
    from k210_yolo_framework_amd.mosaic import MosaicConfig
    pipe = pipeline.InputPipeline(h, items, 4, seed=3, epoch=1, shuffle=True, workers=2, prefetch=2, augment=augment,
                                  mosaic=MosaicConfig(1.0) if mosaic else None, **({} if cache is None else dict(cache=cache)), **kw)
    try:
        return [(x.clone(), [y.clone() for y in ys]) for x, ys in pipe]
    finally:
        pipe.close()


@pytest.mark.parametrize('cached', [False, True], ids=['nocache', 'cache'])
@pytest.mark.parametrize('mode', list(PIPE_MODES))
def test_pipeline_gpu_labels_equal_host_labels(mode, cached):
    import torch
    from k210_yolo_framework_amd.cache import PictureCache
    h, items = _pipe_helper(), _items()
    cache = PictureCache(1 << 20, stage_bytes=1 << 18) if cached else None
    try:
        for opts in (dict(), dict(assign='multi', assign_iou=0.213)):
            host = _run(h, items, cache, labels='host', **opts, **PIPE_MODES[mode])
            gpu = _run(h, items, cache, labels='gpu', **opts, **PIPE_MODES[mode])
            assert len(host) == len(gpu) == 2
            for (hx, hys), (gx, gys) in zip(host, gpu):
                assert torch.equal(hx, gx) and len(hys) == len(gys) == 2
                for hy, gy in zip(hys, gys):
                    assert gy.is_contiguous() and hy.shape == gy.shape and torch.equal(hy, gy)
                assert sum(int((y[..., 4] == 1).sum()) for y in gys) > 0
        plain = _run(h, items, cache, **PIPE_MODES[mode])                       # no option: the host labels of 'best'
        for (px, pys), (bx, bys) in zip(plain, _run(h, items, cache, labels='gpu', **PIPE_MODES[mode])):
            assert torch.equal(px, bx) and all(torch.equal(a, b) for a, b in zip(pys, bys))
    finally:
        if cache is not None:
            cache.close()


def test_a_pipeline_iterated_twice_gives_the_same_batches_and_checks_each_pass():
    import torch
    from k210_yolo_framework_amd import engine, pipeline
    h, items = _pipe_helper(), _items()
    with pipeline.InputPipeline(h, items, 4, seed=3, epoch=1, shuffle=True, workers=2, labels='gpu', assign='multi') as pipe:
        passes = [[(x.clone(), [y.clone() for y in ys]) for x, ys in pipe] for _ in range(3)]
    want = _run(h, items, labels='host', assign='multi')
    for got in passes:
        assert len(got) == len(want) == 2
        for (gx, gys), (wx, wys) in zip(got, want):
            assert torch.equal(gx, wx) and all(torch.equal(a, b) for a, b in zip(gys, wys))
    bad = list(items)
    bad[5] = (items[5][0], np.array([[2, 0.5, -0.2, 0.2, 0.2]]))
    with pipeline.InputPipeline(h, bad, 4, seed=3, epoch=1, shuffle=True, workers=2, labels='gpu') as pipe:
        for _ in range(2):                                                      # every pass reports it
            with pytest.raises(engine.YkError, match='dataset row 5 '):
                for _ in pipe:
                    pass


def test_pipeline_names_the_row_and_the_box_of_an_out_of_grid_centre():
    from k210_yolo_framework_amd import engine
    h, items = _pipe_helper(), _items()
    bad = list(items)
    bad[5] = (np.zeros((64, 96, 3), np.uint8) + 9, np.array([[1, 0.5, 0.5, 0.2, 0.2], [2, 1.0, 0.5, 0.2, 0.2]]))     # letterboxed 1:1: x stays 1.0
    with pytest.raises(engine.YkError, match=r'dataset row 5 .*box 1 of the sample.*outside the label grid'):
        _run(h, bad, labels='gpu')
    worse = list(items)
    worse[2] = (items[2][0], np.array([[1, 0.5, np.inf, 0.2, 0.2]]))
    with pytest.raises(engine.YkError, match=r'dataset row 2 .*box 0 of the sample.*is not finite'):
        _run(h, worse, labels='gpu')
    for opts, what in ((dict(labels='device'), 'labels'), (dict(assign='all'), 'assign'), (dict(assign='multi', assign_iou=0.0), 'assign_iou')):
        with pytest.raises(engine.YkError, match=what):
            _run(h, items, **opts)


def test_trainer_step_on_gpu_multi_labels_equals_the_step_on_host_multi_labels():
    import torch
    from k210_yolo_framework_amd import netspec
    from k210_yolo_framework_amd.train import Trainer
    spec = netspec.yolo_mobilev1((*HW, 3), 3, 20, alpha=0.5)
    h = Helper(None, 20, VOC_ANCHORS, [list(HW)], [list(x) for x in spec.out_hw()])
    items = _items()
    w = spec.init_weights(seed=4)
    runs = []
    for labels in ('host', 'gpu'):
        x, ys = _run(h, items, labels=labels, assign='multi', assign_iou=0.213)[0]
        tr = Trainer(spec, w, h.anchors, 4, use_graph=False)
        out = tr.step(x, ys)
        torch.cuda.synchronize()
        runs.append((out['loss'], tr.G.cpu().numpy().copy(), tr.P.cpu().numpy().copy(), [y.cpu().numpy() for y in ys]))
    best = _run(h, items, labels='host')[0][1]
    assert any(not np.array_equal(a, b.cpu().numpy()) for a, b in zip(runs[0][3], best))       # multi did change the labels of this batch
    assert runs[0][0] == runs[1][0] and np.isfinite(runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])

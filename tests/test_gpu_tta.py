"""Test-time augmentation on the GPU: yk_letterbox_views_u8 against yk_letterbox_u8 of every view's canvas built on the
host, yk_fuse_views against tta.fuse, both bit for bit, and detect.run / evaluate.run with tta= against the plain path run on the canvases
followed by the host fusion.

The fusion runs on the cases of tests/tta_cases.py (tests/test_tta.py holds tta.fuse itself to a second statement and to hand-derived answers
on the same cases).  Rows are compared as int32 patterns; rows beyond a frame's count hold NaN (reading one would show); d_out is filled with
a sentinel first and every row beyond a picture's count must still hold it.

The end-to-end network is tests/plan_zoo.py::residual, as in tests/test_gpu_tiles.py and tests/test_gpu_softnms.py: both nets of
tests/mini_net.py are refused by the inference plans (an 8-filter stem; 8 channels through the upsample)."""
import ctypes as C
import json

import numpy as np
import pytest

from k210_yolo_framework_amd import draw, softnms, tta
from tests import tta_cases

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = -12345.0


# ---------------------------------------------------------------------------------------------------- the view letterbox
PICTURES = [(1, 1), (5, 7), (33, 64)]                                       # mirrored widths 1, odd and even
SPEC = ((1, False), (1, True), (0.83, False), (0.83, True), (0.67, False), (0.67, True))


def _packed_with_gaps(shapes, seed):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]       # no zero byte: a tap that leaves the picture shows
    packed, table, _ = draw.pack_ragged(imgs, gap=5)
    flat = packed.numpy()
    used = np.zeros(flat.size, bool)
    for r in table:
        used[int(r['offset']):int(r['offset']) + 3 * int(r['h']) * int(r['w'])] = True
    flat[~used] = 255                                                                 # the gaps are not zero either
    return imgs, table, packed.cuda()


def _views_of(h, w):
    """The six views of SPEC, then the picture at hand-set places touching each edge of a canvas 4 rows and 6 columns larger."""
    hand = [(h + 4, w + 6, 0, 0, 0), (h + 4, w + 6, 4, 6, 1), (h + 4, w + 6, 0, 6, 0), (h + 4, w + 6, 4, 0, 1), (h + 4, w + 6, 1, 2, 1)]
    return np.concatenate([tta.views(h, w, SPEC), np.asarray(hand, np.int32)])


@pytest.mark.parametrize('dst', [(7, 10), (224, 320)])
def test_view_letterbox_equals_letterbox_of_the_canvas(dst):
    import torch
    from k210_yolo_framework_amd import engine
    imgs, table, d_packed = _packed_with_gaps(PICTURES, 3)
    canvases, rows = [], []
    for i, (im, (h, w)) in enumerate(zip(imgs, PICTURES)):
        v = _views_of(h, w)
        assert v[0].tolist() == [h, w, 0, 0, 0] and v[1].tolist() == [h, w, 0, 0, 1]   # the picture equal to its canvas, plain and mirrored
        rows.append(tta.table_rows(v, int(table['offset'][i]), h, w))
        canvases += [tta.canvas(im, view) for view in v]
    rows = np.concatenate(rows)
    assert len(rows) == len(canvases) == 33
    out = engine.letterbox_views_u8(d_packed, rows, dst)
    torch.cuda.synchronize()
    for k, cv in enumerate(canvases):
        ref = engine.letterbox_u8(torch.from_numpy(cv[None]).cuda(), dst)[0]
        assert torch.equal(out[k], ref), (k, cv.shape, dst)
    # the identity view is the ragged letterbox's frame
    ragged = engine.letterbox_ragged_u8(d_packed, table, dst)
    for i in range(len(PICTURES)):
        assert torch.equal(out[11 * i], ragged[i]), i


def _filled_table(engine, rows, dst):
    t = np.array(rows, dtype=tta.VIEW_DTYPE, copy=True)
    engine.call('yk_letterbox_views_params', t, len(t), dst[0], dst[1])
    return t


def test_view_letterbox_bad_rows_give_zero_frames_next_to_good_ones():
    import torch
    from k210_yolo_framework_amd import engine
    dst = (32, 48)
    imgs, table, d_packed = _packed_with_gaps([(33, 47), (20, 24)], 4)
    v = np.asarray([(24, 30, 2, 3, 0), (24, 30, 4, 6, 1), (20, 24, 0, 0, 1), (30, 24, 10, 0, 0), (20, 40, 0, 16, 1), (25, 25, 5, 1, 0)], np.int32)
    good = _filled_table(engine, tta.table_rows(v, int(table['offset'][1]), 20, 24), dst)
    want = engine.letterbox_views_u8(d_packed, good, dst)
    assert all(want[k].any().item() for k in range(len(v)))
    nbytes = d_packed.numel()
    spoil = [('h', 0, 'is 0 x 24'), ('w', -3, 'is 20 x -3'), ('oy', -1, 'outside its canvas'), ('oy', 11, 'outside its canvas'), ('ox', 17, 'outside its canvas'),
             ('offset', nbytes - 3 * 20 * 24 + 1, 'ends at byte')]
    for k, (field, value, why) in enumerate(spoil):
        bad = good.copy()
        bad[field][k] = value
        with pytest.raises(engine.YkError, match=f'view table: row {k} .*{why}'):
            engine.check_view_rows(bad, nbytes)
        d_table = torch.from_numpy(bad.view(np.uint8).reshape(len(v), 56)).cuda()
        out = engine.letterbox_views_u8(d_packed, d_table, dst)
        torch.cuda.synchronize()
        for j in range(len(v)):
            assert torch.equal(out[j], torch.zeros_like(out[j]) if j == k else want[j]), (field, value, j)
    wide = good.copy()                                                   # ox + w leaves the canvas only in 64 bits
    wide['ox'][0] = 2 ** 31 - 1
    assert not engine.letterbox_views_u8(d_packed, torch.from_numpy(wide.view(np.uint8).reshape(len(v), 56)).cuda(), dst)[0].any().item()
    edge = good.copy()                                                   # the last byte of the buffer itself is a legal last byte
    edge['offset'][5] = spoil[5][1] - 1
    engine.check_view_rows(edge, nbytes)
    assert engine.letterbox_views_u8(d_packed, edge, dst)[5].any().item()
    L = engine.lib()
    d_table = torch.from_numpy(good.view(np.uint8).reshape(len(v), 56)).cuda()
    assert L.yk_letterbox_views_u8(d_packed, nbytes, d_table, 0, want, 32, 48, None) == -10
    assert L.yk_letterbox_views_u8(None, nbytes, d_table, 6, want, 32, 48, None) == -10
    assert L.yk_letterbox_views_u8(d_packed, nbytes, None, 6, want, 32, 48, None) == -10
    assert L.yk_letterbox_views_u8(d_packed, 0, d_table, 6, want, 32, 48, None) == -10
    assert L.yk_letterbox_views_u8(d_packed, nbytes, d_table, 6, want, 0, 48, None) == -10
    assert L.yk_letterbox_views_params(good.copy(), 0, 32, 48) == -10
    assert L.yk_letterbox_views_params(None, 6, 32, 48) == -10
    nocanvas = good.copy()
    nocanvas['cw'][2] = 0
    assert L.yk_letterbox_views_params(nocanvas, 6, 32, 48) == -10 and b'row 2' in L.yk_last_error()
    # the helper's arithmetic is the ragged helper's on (ch, cw)
    rag = np.zeros(len(v), draw.RAGGED_DTYPE)
    rag['h'], rag['w'] = v[:, 0], v[:, 1]
    engine.call('yk_letterbox_ragged_params', rag, len(rag), 32, 48)
    assert all(good[f].tolist() == rag[f].tolist() for f in ('scale', 'tx', 'ty'))


def test_view_letterbox_recorded_in_a_graph_and_replayed_on_changed_pixels():
    import torch
    from k210_yolo_framework_amd import engine
    dst = (32, 48)
    imgs, table, d_packed = _packed_with_gaps([(33, 47), (5, 7)], 5)
    rows = np.concatenate([tta.table_rows(tta.views(33, 47, 'v5'), int(table['offset'][0]), 33, 47),
                           tta.table_rows(tta.views(5, 7, 'flip'), int(table['offset'][1]), 5, 7)])
    d_table = engine.view_table_to_device(rows, dst, d_packed.numel(), d_packed.device)
    out = torch.zeros((len(rows), *dst, 3), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()
    graph = engine.capture(st, lambda: engine.call('yk_letterbox_views_u8', d_packed, d_packed.numel(), d_table, len(rows), out, dst[0], dst[1], st))
    try:
        assert graph.kernel_nodes == 1
        stream.synchronize()
        assert not out.any().item()                                 # recorded, not executed
        for _ in range(2):
            eager = engine.letterbox_views_u8(d_packed, d_table, dst)
            torch.cuda.synchronize()
            graph.launch(st)
            stream.synchronize()
            assert eager.any().item() and torch.equal(out, eager)
            d_packed.copy_(255 - d_packed)                          # the replay reads the pixels that are there when it runs
            torch.cuda.synchronize()
    finally:
        graph.close()


# ---------------------------------------------------------------------------------------------------- the fusion
def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


class _Device:
    """The buffers of one yk_fuse_views call over pictures (cases) of equal views, class_num and max_out."""

    def __init__(self, cases):
        import torch
        c = cases[0]
        self.views, self.class_num, self.max_out, self.thresh = len(c.rows), c.class_num, c.max_out, c.thresh
        assert all((len(k.rows), k.class_num, k.max_out, k.thresh) == (self.views, self.class_num, self.max_out, self.thresh) for k in cases)
        self.cap = self.class_num * self.max_out
        self.n_pics = len(cases)
        n = self.n_pics * self.views
        self.dets = torch.empty((n, self.cap, 6), dtype=torch.float32, device='cuda')
        self.counts = torch.empty(n, dtype=torch.int32, device='cuda')
        self.xforms = torch.empty((n, 3), dtype=torch.float32, device='cuda')
        self.out = torch.empty((self.n_pics, self.cap, 6), dtype=torch.float32, device='cuda')
        self.out_counts = torch.empty(self.n_pics, dtype=torch.int32, device='cuda')
        self.load(cases)

    def load(self, cases):
        import torch
        rows = [r for c in cases for r in c.rows]
        dets = np.full((len(rows), self.cap, 6), np.nan, F)
        for f, r in enumerate(rows):
            dets[f, :len(r)] = r
        self.dets.copy_(torch.from_numpy(dets))
        self.counts.copy_(torch.from_numpy(np.asarray([len(r) for r in rows], np.int32)))
        self.xforms.copy_(torch.from_numpy(np.concatenate([c.xforms for c in cases]).astype(F)))
        self.clear()

    def clear(self):
        self.out.fill_(SENTINEL)
        self.out_counts.fill_(-1)

    def untouched(self):
        return bool((self.out == SENTINEL).all().item()) and bool((self.out_counts == -1).all().item())

    def args(self, stream=None):
        return (self.dets, self.counts, self.xforms, self.views, self.n_pics, self.class_num, self.max_out, self.thresh, self.out, self.out_counts, stream)

    def check(self, want, what):
        import torch
        assert self.out_counts.tolist() == [len(w) for w in want], (what, self.out_counts.tolist(), [len(w) for w in want])
        for p, w in enumerate(want):
            assert torch.equal(_bits(self.out[p, :len(w)]).cpu(), _bits(torch.from_numpy(np.array(w, F, copy=True)).reshape(-1, 6))), (what, p)
            assert bool((self.out[p, len(w):] == SENTINEL).all().item()), (what, p)


def _reference(cases):
    return [tta.fuse(c.rows, c.xforms, c.class_num, c.max_out, c.thresh)[0] for c in cases]


def _run(cases, what=None):
    import torch
    from k210_yolo_framework_amd import engine
    d = _Device(cases)
    engine.fuse_views(d.dets, d.counts, d.xforms, d.views, d.class_num, d.max_out, d.thresh, out=d.out, out_counts=d.out_counts)
    torch.cuda.synchronize()
    want = _reference(cases)
    d.check(want, what or cases[0].name)
    return want


HAND = tta_cases.hand_cases()


@pytest.mark.parametrize('case', HAND, ids=[c.name for c in HAND])
def test_fuse_hand_cases_equal_the_rule_and_the_answer_by_hand(case):
    want = _run([case])[0]
    assert want.tolist() == np.asarray(case.want, F).reshape(-1, 6).tolist()


@pytest.mark.parametrize('n, views', [(0, 1), (1, 1), (63, 1), (64, 1), (65, 1), (63, 2), (64, 2), (65, 2), (65, 3)])
def test_fuse_classes_at_the_wave_boundaries(n, views):
    case = tta_cases.one_class_counts(n, views)
    assert sum(int((r[:, 5] == 1).sum()) for r in case.rows) == n
    want = _run([case])[0]
    assert (want[:, 5] == 0).sum() in (1, 2) and (n == 0) == (not (want[:, 5] == 1).any())


@pytest.mark.parametrize('views, class_num, k, max_out', [(1, 1, 40, 40), (2, 3, 25, 30), (3, 80, 3, 5), (8, 4, 6, 4), (8, 1, 30, 30), (3, 20, 10, 30)])
def test_fuse_seeded_views_and_classes(views, class_num, k, max_out):
    cases = [tta_cases.random_case(10 * views + s, views, k, class_num, max_out) for s in range(2)]
    want = _run(cases)
    assert all(0 < len(w) for w in want)
    if views > 1:
        assert any(len(w) < sum(len(r) for r in c.rows) for w, c in zip(want, cases))        # something was fused


def test_fuse_three_pictures_of_which_one_has_no_rows():
    a, b = tta_cases.random_case(71, 3, 12, 5, 6, thresh=0.3), tta_cases.random_case(72, 3, 12, 5, 6, thresh=0.3)
    empty = a._replace(name='empty', rows=[r[:0] for r in a.rows])
    want = _run([a, empty, b])
    assert [len(w) > 0 for w in want] == [True, False, True]


def test_fuse_exactly_the_lds_capacity_and_one_more_refused():
    """views * max_out == the capacity, every candidate of one class; one more is refused by name with nothing written."""
    import torch
    from k210_yolo_framework_amd import engine
    cap = engine.fuse_views_lds_candidates(30)
    assert cap >= 8 * 30 and cap % 64 == 0
    rng = np.random.default_rng(5)
    t, l = rng.integers(0, 600, cap).astype(np.float64), rng.integers(0, 600, cap).astype(np.float64)
    rows = np.stack([t, l, t + rng.integers(4, 40, cap), l + rng.integers(4, 40, cap), rng.integers(1, 65, cap) / 64.0, np.zeros(cap)], 1)
    case = tta_cases._case('capacity', [rows[np.argsort(-rows[:, 4], kind='stable')]], [tta_cases.NO], 1, cap, 0.55)
    want = _run([case])[0]
    assert 64 < len(want) < cap
    d = _Device([case])
    L = engine.lib()
    good = d.args()
    assert L.yk_fuse_views(*good) == 0
    torch.cuda.synchronize()
    d.clear()
    torch.cuda.synchronize()
    # (the buffers are those of the capacity case: the refusal comes before anything is read)
    assert L.yk_fuse_views(*good[:6], cap + 1, *good[7:]) == -10
    msg = L.yk_last_error().decode()
    assert 'views' in msg and 'max_out' in msg and str(cap + 1) in msg and str(cap) in msg, msg
    assert L.yk_fuse_views(*good[:3], 2, 1, 1, cap // 2 + 1, *good[7:]) == -10
    torch.cuda.synchronize()
    assert d.untouched()
    assert L.yk_fuse_views_lds_candidates(0) == -10


def test_fuse_clamps_counts_on_the_device():
    """counts [cap + 5, -3, 2] are read as [cap, 0, 2]: the C entry point on a table engine.fuse_views never sees from the pipeline."""
    import torch
    from k210_yolo_framework_amd import engine
    full = tta_cases.random_case(81, 3, [4, 4], 2, 4)
    d = _Device([full])
    cap = d.cap
    rng = np.random.default_rng(9)
    t = rng.integers(0, 90, (3, cap)).astype(np.float64)
    dets = np.stack([t, t, t + 20, t + 20, rng.integers(1, 17, (3, cap)) / 16.0, np.tile(np.repeat([0, 1], 4), (3, 1))], 2).astype(F)
    d.dets.copy_(torch.from_numpy(dets))
    d.counts.copy_(torch.tensor([cap + 5, -3, 2], dtype=torch.int32))
    engine.call('yk_fuse_views', *d.args(C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    want = tta.fuse([dets[0], dets[1][:0], dets[2][:2]], full.xforms, 2, 4, full.thresh)[0]
    d.check([want], 'clamps')


def test_fuse_two_runs_give_the_same_bytes():
    import torch
    from k210_yolo_framework_amd import engine
    cases = [tta_cases.random_case(90 + s, 3, 10, 20, 30) for s in range(3)]
    runs = []
    for _ in range(2):
        d = _Device(cases)
        engine.fuse_views(d.dets, d.counts, d.xforms, d.views, d.class_num, d.max_out, d.thresh, out=d.out, out_counts=d.out_counts)
        torch.cuda.synchronize()
        runs.append((d.out.cpu(), d.out_counts.cpu()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][1].tolist() == [len(w) for w in _reference(cases)]


def test_fuse_recorded_in_a_graph_and_replayed_on_new_rows():
    """Both kernels are recorded (nothing runs during the capture) and the per-stream scratch survives: the replay reads the rows that are in
    the buffers when it runs - seed A, then B, then A again, each equal to the rule on its own rows."""
    import torch
    from k210_yolo_framework_amd import engine
    a = [tta_cases.random_case(100 + s, 3, 10, 20, 30) for s in range(2)]
    b = [tta_cases.random_case(200 + s, 3, 10, 20, 30) for s in range(2)]
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    with torch.cuda.stream(stream):
        d = _Device(a)
        issue = lambda: engine.call('yk_fuse_views', *d.args(st))
        issue()                                                     # eagerly once: the stream's scratch exists before the capture
        stream.synchronize()
        d.check(_reference(a), 'eager')
        d.clear()
        stream.synchronize()
        graph = engine.capture(st, issue)
        try:
            assert graph.kernel_nodes == 2
            stream.synchronize()
            assert d.untouched()                                    # recorded, not executed
            for cases in (a, b, a):
                d.load(cases)
                stream.synchronize()
                graph.launch(st)
                stream.synchronize()
                d.check(_reference(cases), cases[0].name)
        finally:
            graph.close()


def test_fuse_bad_arguments_are_refused_by_name_with_nothing_written():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    d = _Device([tta_cases.random_case(7, 2, 3, 2, 3)])
    good = dict(d_dets=d.dets, d_counts=d.counts, d_xform=d.xforms, views=2, n_pics=1, class_num=2, max_out=3, thresh=0.5, d_out=d.out,
                d_out_counts=d.out_counts, stream=None)
    assert L.yk_fuse_views(*good.values()) == 0
    torch.cuda.synchronize()
    d.clear()
    torch.cuda.synchronize()
    for name, value in [('d_dets', None), ('d_counts', None), ('d_xform', None), ('d_out', None), ('d_out_counts', None), ('views', 0), ('views', -1),
                        ('views', 9), ('n_pics', 0), ('class_num', 0), ('max_out', 0), ('thresh', float('nan')), ('thresh', -0.25), ('n_pics', 1 << 30),
                        ('class_num', 1 << 30)]:
        assert L.yk_fuse_views(*{**good, name: value}.values()) == -10, name
        assert name in L.yk_last_error().decode(), (name, L.yk_last_error())
    torch.cuda.synchronize()
    assert d.untouched()
    with pytest.raises(engine.YkError, match='not whole pictures of 3 views'):
        engine.fuse_views(d.dets, d.counts, d.xforms, 3, 2, 3)


# ---------------------------------------------------------------------------------------------------- end to end
SIZES = [(48, 64), (75, 100), (67, 50)]
OBJ, IOU, THRESH = 0.5, 0.5, 0.55


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


@pytest.fixture(scope='module')
def plain(net, tmp_path_factory):
    """The default run, once: no tta argument at all."""
    from k210_yolo_framework_amd import detect
    h, model, pics = net
    out = tmp_path_factory.mktemp('plain')
    res = detect.run(h, model, pics, out_dir=out, draw=False, batch=4, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False)
    return res, (out / 'detections.json').read_bytes()


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def test_detect_with_tta_none_writes_the_bytes_of_the_default_run(net, plain, tmp_path):
    from k210_yolo_framework_amd import detect
    h, model, pics = net
    res = detect.run(h, model, pics, out_dir=tmp_path, draw=False, batch=4, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False, tta=None, tta_thresh=0.55)
    assert _same(res['detections'], plain[0]['detections'])
    assert (tmp_path / 'detections.json').read_bytes() == plain[1]
    assert b'tta' not in plain[1]


def test_detect_one_plain_view_is_the_plain_path(net, plain, tmp_path):
    from k210_yolo_framework_amd import detect
    h, model, pics = net
    dets = plain[0]['detections']
    assert sum(len(d) for d in dets) > 0
    # the premise: the decode's own NMS at 0.5 leaves no same-class pair above 0.55, so every row stays a cluster of its own
    worst = 0.0
    for d in dets:
        for m in range(len(d)):
            o = softnms.iou_to_all(d[:, :4], m)[0]
            o[m] = 0
            worst = max(worst, float(o[d[:, 5] == d[m, 5]].max(initial=0)))
    assert worst <= THRESH, worst
    one = detect.run(h, model, pics, out_dir=tmp_path, draw=False, batch=4, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False, tta=((1, False),),
                     tta_thresh=THRESH)
    assert _same(one['detections'], dets)
    a, b = json.loads(plain[1]), json.loads((tmp_path / 'detections.json').read_text())
    assert b[0]['tta'] == '1' and b[0]['tta_views'] == [[1.0, False]] and b[0]['tta_thresh'] == THRESH
    assert [d['detections'] for d in a] == [d['detections'] for d in b]


@pytest.mark.parametrize('spec', ['flip', 'v5'])
def test_detect_tta_is_the_plain_path_on_the_canvases_then_the_host_fusion(net, spec):
    from k210_yolo_framework_amd import detect
    from tests.test_gpu_draw import paint
    h, model, pics = net
    kw = dict(batch=7, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False)
    got = detect.run(h, model, pics, draw=True, return_arrays=True, tta=spec, tta_thresh=THRESH, **kw)   # 2 or 3 frames a picture: 3 or 2 pictures a batch
    vws = [tta.views(p.shape[0], p.shape[1], spec) for p in pics]
    V = len(vws[0])
    canvases = [tta.canvas(p, view) for p, v in zip(pics, vws) for view in v]
    per = detect.run(h, model, canvases, draw=False, **kw)['detections']
    want = [tta.fuse(per[V * i:V * i + V], tta.xforms(vws[i]), 20, 30, THRESH)[0] for i in range(len(pics))]
    print(spec, 'rows per picture, fused:', [len(w) for w in want], 'of', [sum(len(r) for r in per[V * i:V * i + V]) for i in range(len(pics))], 'candidates')
    assert sum(len(w) for w in want) > 0
    assert any(len(w) < sum(len(r) for r in per[V * i:V * i + V]) for i, w in enumerate(want))            # the views agreed on something
    assert _same(got['detections'], want)
    atlas, colours = draw.glyph_atlas(), np.asarray(h.colormap, np.uint8).reshape(-1, 3)
    for i, p in enumerate(pics):
        hh, ww = p.shape[:2]
        assert np.array_equal(got['arrays'][i], paint(p.copy(), want[i], colours, atlas, draw.thickness_of(hh, ww), draw.magnification_of(hh))), i


def test_detect_refuses_what_tta_cannot_be_combined_with(net):
    from k210_yolo_framework_amd import detect
    h, model, pics = net
    kw = dict(draw=False, batch=4, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False)
    with pytest.raises(Exception, match='tta with tiles'):
        detect.run(h, model, pics, tta='flip', tiles=(2, 2), **kw)
    with pytest.raises(Exception, match="nms 'linear' with tta"):
        detect.run(h, model, pics, tta='flip', nms='linear', **kw)
    with pytest.raises(Exception, match='a picture is 3 frames and a batch holds 2'):
        detect.run(h, model, pics, tta='v5', **{**kw, 'batch': 2})
    with pytest.raises(Exception, match='above 1'):
        detect.run(h, model, pics, tta=((1.25, False),), **kw)


def test_evaluate_takes_the_same_options_and_names_them(net, plain):
    """evaluate.run with one plain view scores the rows it scores without; with v5 it scores detect.run's fused rows; the options may come in
    the namespace or as arguments."""
    from argparse import Namespace
    from k210_yolo_framework_amd import detect, evaluate
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    h, model, pics = net
    items = [(p, np.asarray([[0, 0.5, 0.5, 0.25, 0.25]])) for p in pics]
    base = dict(batch=7, depth=2, precision='f16x2', obj_thresh=OBJ, nms_iou=IOU, nms='hard', nms_sigma=0.5, tiles=None, tile_overlap=0.2, tile_full=True,
                tile_match='ios', tile_thresh=0.5)

    def rows(ns=None, **kw):
        ev = MapEvaluator(20, 0.5, False)
        evaluate.run(Namespace(**{**base, **(ns or {})}), h, model, items, ev, **kw)
        r, img = ev.rows()
        return [r[img == i] for i in range(len(pics))]

    assert _same(rows(), plain[0]['detections'])                     # a namespace from before the option: off
    assert _same(rows(dict(tta=((1, False),), tta_thresh=THRESH)), plain[0]['detections'])
    want = detect.run(h, model, pics, draw=False, batch=7, depth=2, obj_thresh=OBJ, iou_thresh=IOU, verbose=False, tta='v5', tta_thresh=THRESH)['detections']
    assert _same(rows(dict(tta='v5', tta_thresh=THRESH)), want)
    assert _same(rows(tta='v5', tta_thresh=THRESH), want)
    with pytest.raises(Exception, match="nms 'diou' with tta"):
        rows(dict(nms='diou'), tta='flip')
    with pytest.raises(Exception, match='tta with tiles'):
        rows(dict(tiles=(2, 2)), tta='flip')
    assert tta.rule_of(tta.check('v5'), THRESH) == dict(tta='1,0.83f,0.67', tta_views=[[1.0, False], [0.83, True], [0.67, False]], tta_thresh=THRESH)   # eval.json's keys

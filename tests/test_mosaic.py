"""Mosaic augmentation, host side (k210_yolo_framework_amd/mosaic.py): the draws, the plan, the box rule on hand-computed cases, the host
copy of the kernel against helper.letterbox_bilinear, and yk_mosaic_params (C, needs no device) against the Python geometry."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import mosaic

ROOT = Path(__file__).resolve().parents[1]
HW = (224, 320)
SHAPES = [(240, 320), (375, 500), (333, 500), (224, 320), (17, 23), (500, 375), (1, 1), (5, 200)]


def _h(hw=HW):
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    return Helper(None, 20, VOC_ANCHORS, [list(hw)], [[7, 10], [14, 20]])


def _items(n, seed=0, pixels=False):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        hw = SHAPES[k % len(SHAPES)]
        m = int(rng.integers(1, 4))
        boxes = np.concatenate([rng.integers(0, 20, (m, 1)).astype(float), rng.uniform(0.05, 0.95, (m, 2)), rng.uniform(0.05, 0.6, (m, 2))], 1)
        out.append((rng.integers(1, 256, (*hw, 3), dtype=np.uint8) if pixels else hw, boxes))
    return out


def test_table_is_a_function_of_seed_epoch_and_row_only():
    t = mosaic.param_table(3, 5, 40)
    assert t.shape == (40, 11) and t.dtype == np.float64
    np.testing.assert_array_equal(t, np.random.default_rng([3, 5, 2]).random((40, 11)))
    np.testing.assert_array_equal(t, mosaic.param_table(3, 5, 40))
    np.testing.assert_array_equal(t[:17], mosaic.param_table(3, 5, 17))            # a row's draws do not depend on the rows after it
    assert not np.array_equal(t, mosaic.param_table(3, 6, 40)) and not np.array_equal(t, mosaic.param_table(4, 5, 40))
    from k210_yolo_framework_amd import augment
    assert not np.array_equal(t[:, :5], augment.param_table(3, 5, 40))             # its own stream, not the augmentation's


def test_decode_follows_the_written_rule():
    u = np.array([[0.3, 0.0, 0.999999, 0.0, 0.5, 0.999999, 0.0, 0.5, 1.0, 0.25, 0.74],
                  [0.7, 0.5, 0.5, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2, 0.2, 0.999999]])
    is_m, seam, partners, gains, q0 = mosaic.decode(u, 10, HW, prob=0.5)
    assert is_m.tolist() == [True, False]
    assert seam.dtype == np.int32 and seam.tolist() == [[80, 167], [160, 112]]     # floor(320*0.25), floor(224*0.749999..)
    assert partners.tolist() == [[0, 5, 9], [1, 1, 1]]
    np.testing.assert_array_equal(gains[0], [0.5, 0.75, 1.0, 0.625])
    assert q0.tolist() == [2, 3]
    items, _ = mosaic.members([4, 7], np.concatenate([np.zeros((4, 11)), u[:1], np.zeros((2, 11)), u[1:], np.zeros((2, 11))]), HW, prob=0.5)
    assert items.tolist() == [[0, 5, 4, 9], [7, 7, 7, 7]]                          # own picture in quadrant q0, partners fill the others in order


def test_plan_is_the_same_for_any_rank_or_world_split():
    items = _items(24)
    table = mosaic.param_table(1, 2, len(items))
    rows = np.random.default_rng(0).permutation(len(items))[:16]
    shapes_of, boxes_of = (lambda i: items[i][0]), (lambda i: items[i][1])
    q, c, b = mosaic.plan(rows, table, shapes_of, HW, boxes_of=boxes_of, prob=0.8)
    assert q.shape == (16, 4) and c.shape == (16, 2) and len(b) == 16
    for world in (2, 4):
        per = 16 // world
        parts = [mosaic.plan(rows[r * per:(r + 1) * per], table, shapes_of, HW, boxes_of=boxes_of, prob=0.8) for r in range(world)]
        np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), q)
        np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), c)
        for got, want in zip([x for p in parts for x in p[2]], b):
            np.testing.assert_array_equal(got, want)
    is_m = mosaic.members(rows, table, HW, prob=0.8)[1]
    assert is_m.any() and not is_m.all()


def test_a_non_mosaic_sample_is_the_plain_letterbox_bit_for_bit():
    from k210_yolo_framework_amd import pipeline
    h = _h()
    items = _items(16, seed=4)
    table = mosaic.param_table(9, 0, len(items))
    rows = np.arange(len(items))
    dropped = []
    q, c, b = mosaic.plan(rows, table, lambda i: items[i][0], HW, boxes_of=lambda i: items[i][1], prob=0.0, dropped=dropped)
    assert dropped == [0] * len(items)
    for i in rows:
        scale, tr = h.letterbox_params(items[i][0])
        for k in range(4):
            assert q[i, k]['item'] == i and (q[i, k]['h'], q[i, k]['w']) == items[i][0]
            assert q[i, k]['scale'] == scale[0] and (q[i, k]['tx'], q[i, k]['ty']) == tuple(tr)
        want = pipeline.letterbox_boxes(h, items[i][0], items[i][1])
        assert b[i].shape == want.shape
        np.testing.assert_array_equal(b[i], want)
    assert (c[:, 0] >= 80).all() and (c[:, 0] < 240).all() and (c[:, 1] >= 56).all() and (c[:, 1] < 168).all()


# Hand-computed: frame 100 x 200, picture 50 x 100 (letterbox scale 2).  In quadrant 1 (top right) of the seam (100, 50) with gain 1.0 the
# scale is 2, the picture is 200 x 100 px, tx = cx = 100, ty = cy - 100 = -50: source fraction (fx, fy) lands at (100 + 200 fx, -50 + 100 fy)
# and the quadrant is [100, 200] x [0, 50].
Q1 = dict(img_hw=(50, 100), scale=2.0, tx=100, ty=-50, k=1, cx=100, cy=50, hw=(100, 200))


def test_box_wholly_inside_its_quadrant():
    # quadrant 0, gain 0.5: scale 1, tx = 100 - 100 = 0, ty = 50 - 50 = 0: the picture is the quadrant.  x 40..60, y 15..35
    got, lost = mosaic.quadrant_boxes(np.array([[3, 0.5, 0.5, 0.2, 0.4]]), (50, 100), 1.0, 0, 0, 0, 100, 50, (100, 200))
    assert lost == 0
    np.testing.assert_allclose(got, [[3, 0.25, 0.25, 0.1, 0.2]], rtol=1e-12, atol=0)


def test_box_cut_by_the_frame_to_half_its_area_is_kept_and_clipped():
    # x 180..220 -> 180..200 (half), y 15..35
    got, lost = mosaic.quadrant_boxes(np.array([[1, 0.5, 0.75, 0.2, 0.2]]), **Q1)
    assert lost == 0
    np.testing.assert_allclose(got, [[1, 0.95, 0.25, 0.1, 0.2]], rtol=1e-12, atol=0)


def test_box_cut_by_the_seam_is_clipped_at_the_seam():
    # quadrant 0 of the same seam, gain 1.0: tx = 100 - 200 = -100, ty = -50; x = -100 + 200 fx.  x 80..120 -> 80..100, y 15..35
    got, lost = mosaic.quadrant_boxes(np.array([[2, 1.0, 0.75, 0.2, 0.2]]), (50, 100), 2.0, -100, -50, 0, 100, 50, (100, 200))
    assert lost == 0
    np.testing.assert_allclose(got, [[2, 0.45, 0.25, 0.1, 0.2]], rtol=1e-12, atol=0)


def test_box_cut_below_a_tenth_of_its_area_is_dropped():
    # x 197..230 -> 197..200: 3 px of 33 wide (>= 2 px, but 0.0909 of the area), y 15..35 whole
    got, lost = mosaic.quadrant_boxes(np.array([[1, 0.5675, 0.75, 0.165, 0.2]]), **Q1)
    assert lost == 1 and got.shape == (0, 5)
    # one pixel more to the left, 4 of 34 = 0.1176: kept
    got, lost = mosaic.quadrant_boxes(np.array([[1, 0.565, 0.75, 0.17, 0.2]]), **Q1)
    assert lost == 0
    np.testing.assert_allclose(got, [[1, 0.99, 0.25, 0.02, 0.2]], rtol=1e-12, atol=0)


def test_box_clipped_to_under_two_pixels_is_dropped():
    # x 199..203 -> 199..200: a quarter of the area, but 1 px wide
    got, lost = mosaic.quadrant_boxes(np.array([[1, 0.505, 0.75, 0.02, 0.2]]), **Q1)
    assert lost == 1 and got.shape == (0, 5)
    # y 49..53 of the quadrant's 0..50 (fy 0.99..1.03): 1 px high
    got, lost = mosaic.quadrant_boxes(np.array([[1, 0.2, 1.01, 0.2, 0.04]]), **Q1)
    assert lost == 1 and got.shape == (0, 5)


def test_boxes_come_in_quadrant_order_then_source_order():
    hw = (100, 200)
    # row 0: mosaic, seam (100, 50), partners 1, 2, 3, every gain 0.5, own picture in quadrant 2 -> quadrants hold items 1, 2, 0, 3
    u = np.zeros((4, 11))
    u[0] = [0.0, 0.5, 0.5, 0.3, 0.55, 0.8, 0, 0, 0, 0, 0.6]
    boxes_of = lambda i: np.array([[10 * i, 0.3, 0.3, 0.2, 0.2], [10 * i + 1, 0.7, 0.7, 0.2, 0.2]])
    dropped = []
    q, c, b = mosaic.plan([0], u, lambda i: (50, 100), hw, boxes_of=boxes_of, dropped=dropped)
    assert c.tolist() == [[100, 50]] and q[0]['item'].tolist() == [1, 2, 0, 3] and dropped == [0]
    assert b[0][:, 0].tolist() == [10, 11, 20, 21, 0, 1, 30, 31]
    # each picture at scale 1 exactly fills its quadrant: the first box of quadrant 3 is at (100 + 30, 50 + 15)
    assert [(int(r['tx']), int(r['ty'])) for r in q[0]] == [(0, 0), (100, 0), (0, 50), (100, 50)]
    np.testing.assert_allclose(b[0][6], [30, 130 / 200, 65 / 100, 0.1, 0.1], rtol=1e-12, atol=0)


def test_each_quadrant_of_the_host_copy_is_the_letterbox_of_its_picture():
    from k210_yolo_framework_amd.helper import letterbox_bilinear
    items = _items(12, seed=2, pixels=True)
    table = mosaic.param_table(5, 1, len(items))
    rows = np.arange(len(items))
    q, c, _ = mosaic.plan(rows, table, lambda i: items[i][0].shape[:2], HW, prob=0.75)
    negative = 0
    for b in rows:
        frame = mosaic.compose_u8([items[int(i)][0] for i in q[b]['item']], q[b], c[b], HW)
        assert frame.shape == (*HW, 3) and frame.dtype == np.uint8
        cx, cy = int(c[b, 0]), int(c[b, 1])
        for k, (ys, xs) in enumerate([(slice(0, cy), slice(0, cx)), (slice(0, cy), slice(cx, None)), (slice(cy, None), slice(0, cx)),
                                      (slice(cy, None), slice(cx, None))]):
            r = q[b, k]
            want = letterbox_bilinear(items[int(r['item'])][0], HW, float(r['scale']), (int(r['tx']), int(r['ty'])))
            np.testing.assert_array_equal(frame[ys, xs], want[ys, xs], err_msg=f'sample {b} quadrant {k}')
            negative += int(r['tx'] < 0 or r['ty'] < 0)
    assert negative
    # a sample that is not a mosaic: the plain letterbox, wherever the seam is
    h = _h()
    plain = [int(b) for b in rows[~mosaic.members(rows, table, HW, prob=0.75)[1]]]
    assert plain
    for b in plain[:2]:
        s, t = h.letterbox_params(items[b][0].shape[:2])
        for seam in (c[b], (0, 0), (HW[1], HW[0]), (1, HW[0] - 1)):
            np.testing.assert_array_equal(mosaic.compose_u8([items[b][0]] * 4, q[b], seam, HW), letterbox_bilinear(items[b][0], HW, float(s[0]), t))
    # a missing picture leaves its quadrant zero and the others as they were
    b = int(rows[0])
    full = mosaic.compose_u8([items[int(i)][0] for i in q[b]['item']], q[b], c[b], HW)
    cut = mosaic.compose_u8([None] + [items[int(i)][0] for i in q[b]['item'][1:]], q[b], c[b], HW)
    assert not cut[:c[b, 1], :c[b, 0]].any()
    cut[:c[b, 1], :c[b, 0]] = full[:c[b, 1], :c[b, 0]]
    np.testing.assert_array_equal(cut, full)


@pytest.fixture(scope='module')
def lib():
    from k210_yolo_framework_amd import engine
    if not engine.library_path().exists():
        import __graft_entry__ as g
        g.build()
    return engine.lib()


def test_yk_mosaic_params_agrees_with_the_plan(lib):
    from k210_yolo_framework_amd.draw import RAGGED_DTYPE
    items = _items(32, seed=7)
    for hw in (HW, (24, 40), (416, 416)):
        table = mosaic.param_table(2, 3, len(items))
        rows = np.arange(len(items))
        q, c, _ = mosaic.plan(rows, table, lambda i: items[i][0], hw)
        _, _, _, gains, _ = mosaic.decode(table[rows], len(items), hw)
        for b in rows:
            t = np.zeros(4, RAGGED_DTYPE)
            t['h'], t['w'] = q[b]['h'], q[b]['w']
            assert lib.yk_mosaic_params(t, int(c[b, 0]), int(c[b, 1]), np.ascontiguousarray(gains[b]), hw[0], hw[1]) == 0
            assert (t['scale'] == q[b]['scale']).all(), (b, t['scale'], q[b]['scale'])           # exact equality
            assert (t['tx'] == q[b]['tx']).all() and (t['ty'] == q[b]['ty']).all()
            assert (t['offset'] == 0).all() and (t['thickness'] == 0).all()


def test_yk_mosaic_params_refuses_bad_arguments(lib):
    from k210_yolo_framework_amd.draw import RAGGED_DTYPE
    t = np.zeros(4, RAGGED_DTYPE)
    t['h'], t['w'] = 10, 20
    g = np.full(4, 0.75)
    assert lib.yk_mosaic_params(t, 5, 5, g, 24, 40) == 0
    bad_row = t.copy()
    bad_row[2]['w'] = 0
    for args in [(None, 5, 5, g, 24, 40), (t, 5, 5, None, 24, 40), (t, 5, 5, g, 0, 40), (t, 5, 5, g, 24, -1), (bad_row, 5, 5, g, 24, 40),
                 (t, 5, 5, np.array([0.5, 0.0, 0.5, 0.5]), 24, 40), (t, 5, 5, np.array([0.5, 0.5, np.nan, 0.5]), 24, 40)]:
        assert lib.yk_mosaic_params(*args) == -10
        assert b'yk_mosaic_params' in lib.yk_last_error()


def test_cli_knows_the_three_options_and_refuses_them_without_a_device():
    import torch
    from k210_yolo_framework_amd import engine, training
    a = training.parser().parse_args([])
    assert (a.mosaic, a.mosaic_prob, a.mosaic_off_epochs) == ('False', 1.0, 0)
    a = training.parser().parse_args(['--mosaic', 'True', '--mosaic_prob', '0.5', '--mosaic_off_epochs', '2'])
    assert (a.mosaic, a.mosaic_prob, a.mosaic_off_epochs) == ('True', 0.5, 2)
    mk = (ROOT / 'Makefile').read_text()
    assert '--mosaic $(MOSAIC) --mosaic_prob $(MOSAICPROB) --mosaic_off_epochs $(MOSAICOFF)' in mk
    if not torch.cuda.is_available():
        with pytest.raises(engine.YkError, match='--mosaic True'):
            training.cli(['--synthetic', '16', '--mosaic', 'True', '--max_steps', '1'])

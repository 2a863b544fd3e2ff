"""yk_draw_dets_u8 against a painter written HERE: a sequential numpy loop that follows the rule of include/yolo_hip.h primitive by
primitive, later paint over earlier.  Whole pictures of seeded noise are compared with ==, so every pixel no primitive covers is held too.
Nothing of the package's drawing code is used by the painter except the glyph bitmaps it is given."""
import numpy as np
import pytest

from k210_yolo_framework_amd import draw

pytestmark = pytest.mark.gpu
COLOURS = np.asarray([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [128, 64, 32]], np.uint8)


def corners(row, h, w):
    """Step 1 of the rule, in fp32 as NumPy evaluates inference.py's expression on a float32 row.  None: the row draws nothing."""
    top, left, bottom, right = (np.float32(v) for v in row[:4])
    half = np.float32(0.5)
    t, l = max(0, int(np.floor(top + half))), max(0, int(np.floor(left + half)))
    b, r = min(h, int(np.floor(bottom + half))), min(w, int(np.floor(right + half)))
    return None if (b <= t or r <= l) else (t, l, b, r)


def paint(img, rows, colours, atlas, thickness, mag, label=True):
    """The painter's rule on one picture, in place: rows in order; per row outline rings, label background, label text."""
    h, w = img.shape[:2]
    gh, gw = atlas.shape[1:]

    def put(y, x, c):
        if 0 <= y < h and 0 <= x < w:                              # clipped: row h / column w are simply not painted
            img[y, x] = c

    for row in rows:
        c4 = corners(row, h, w)
        if c4 is None:
            continue
        t, l, b, r = c4
        colour = colours[int(row[5]) % len(colours)]
        for j in range(thickness):
            if not (r - j > l + j and b - j > t + j):
                break
            for x in range(l + j, r - j + 1):
                put(t + j, x, colour)
                put(b - j, x, colour)
            for y in range(t + j, b - j + 1):
                put(y, l + j, colour)
                put(y, r - j, colour)
        if not label or gh == 0:
            continue
        x0, y0 = l, t + 1
        img[y0:min(h, y0 + gh * mag), x0:min(w, x0 + 7 * gw * mag)] = colour
        text = '{:2d} {:.2f}'.format(int(row[5]), float(np.float32(row[4])))
        assert len(text) == 7
        for slot, ch in enumerate(text):
            glyph = atlas['0123456789. '.index(ch)]
            for gy in range(gh):
                for gx in range(gw):
                    if glyph[gy, gx]:
                        ya, xa = y0 + gy * mag, x0 + (slot * gw + gx) * mag
                        img[min(h, ya):min(h, ya + mag), min(w, xa):min(w, xa + mag)] = 0
    return img


def run_gpu(imgs, rows_per_image, atlas, cap=None, thickness=None, mag=None, colours=COLOURS, counts=None):
    """imgs / rows through engine.draw_detections_u8 -> (drawn pictures, table)."""
    import torch
    from k210_yolo_framework_amd import engine
    packed, table, _ = draw.pack_ragged(imgs)
    if thickness is not None:
        table['thickness'] = thickness
    if mag is not None:
        table['mag'] = mag
    n = len(imgs)
    cap = cap or max(1, max(len(r) for r in rows_per_image))
    dets = np.full((n, cap, 6), np.nan, np.float32)                 # rows past the count are never read: NaN would show as paint
    for i, r in enumerate(rows_per_image):
        if len(r):
            dets[i, :len(r)] = np.asarray(r, np.float32)
    cnt = np.asarray([len(r) for r in rows_per_image] if counts is None else counts, np.int32)
    d_packed = packed.cuda()
    engine.draw_detections_u8(d_packed, table, torch.from_numpy(dets).cuda(), torch.from_numpy(cnt).cuda(), torch.from_numpy(colours).cuda(),
                              torch.from_numpy(np.ascontiguousarray(atlas)).cuda())
    torch.cuda.synchronize()
    flat = d_packed.cpu().numpy()
    return [v.copy() for v in draw.unpack_ragged(flat, table)], table


def check(imgs, rows_per_image, atlas=None, **kw):
    atlas = draw.glyph_atlas() if atlas is None else atlas
    got, table = run_gpu(imgs, rows_per_image, atlas, **kw)
    want = []
    for im, rows, trow in zip(imgs, rows_per_image, table):
        want.append(paint(im.copy(), rows, kw.get('colours', COLOURS), atlas, int(trow['thickness']), int(trow['mag'])))
    for i, (g, r) in enumerate(zip(got, want)):
        bad = np.argwhere((g != r).any(-1))
        assert not len(bad), (i, g.shape, len(bad), bad[:5].tolist())
    return got


def noise(seed, *shapes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def test_overlapping_boxes_in_both_orders_differ_and_match_the_painter():
    a, b = [20.2, 30.7, 90.4, 180.0, 0.91, 3], [24.0, 100.0, 120.6, 260.3, 0.55, 12]       # b's label lies on a's outline and label
    img = noise(1, (240, 320))
    ab = check(img, [[a, b]])[0]
    ba = check(img, [[b, a]])[0]
    assert (ab != ba).any()
    assert (ab != img[0]).any()


def test_boxes_over_each_edge_and_on_the_far_edges():
    h, w = 97, 131
    rows = [[-20.0, 10.0, 30.0, 60.0, 0.8, 0], [40.0, -15.5, 80.0, 40.0, 0.7, 1], [70.0, 50.0, 140.0, 100.0, 0.6, 2],
            [10.0, 100.0, 50.0, 400.0, 0.5, 3], [-1e9, -1e9, 1e9, 1e9, 0.4, 4]]
    check(noise(2, (h, w)), [rows])
    for row in rows:                                                # one at a time too: an edge case hidden under a later box would not show
        check(noise(2, (h, w)), [[row]])
    check(noise(3, (h, w)), [[[60.0, 70.0, float(h), float(w), 0.9, 5]]])                   # bottom == h and right == w exactly
    check(noise(3, (h, w)), [[[60.0, 70.0, h + 0.4, w - 0.6, 0.9, 5]]])


def test_degenerate_boxes_paint_nothing_not_even_a_label():
    img = noise(4, (60, 80))
    rows = [[30.0, 10.0, 30.2, 50.0, 0.9, 1], [40.0, 20.0, 20.0, 50.0, 0.9, 2], [10.0, 50.0, 40.0, 50.4, 0.9, 3], [70.0, 10.0, 90.0, 40.0, 0.9, 4],
            [10.0, 95.0, 40.0, 99.0, 0.9, 5]]
    assert all(corners(r, 60, 80) is None for r in rows)
    got = check(img, [rows])[0]
    assert np.array_equal(got, img[0])
    check(img, [rows[:2] + [[5.0, 5.0, 40.0, 60.0, 0.5, 6]] + rows[2:]])                    # between them a box that does draw


def test_thickness_beyond_half_the_box_stops_where_the_rule_says():
    img = noise(5, (64, 96))
    rows = [[8.0, 8.0, 15.0, 60.0, 0.9, 1], [30.0, 20.0, 40.0, 26.0, 0.3, 2], [50.0, 70.0, 51.0, 71.0, 0.2, 3]]
    check(img, [rows], thickness=9, atlas=np.zeros((12, 0, 8), np.uint8))                   # outlines alone: the rings fill the box
    check(img, [rows], thickness=9)
    check(img, [rows], thickness=2)


def test_label_clipped_by_the_right_and_bottom_edges():
    check(noise(6, (30, 40)), [[[20.0, 25.0, 30.0, 40.0, 0.77, 19]]])
    check(noise(6, (30, 40)), [[[25.6, 36.0, 29.0, 39.0, 0.77, 8]]])
    check(noise(6, (30, 40)), [[[20.0, 25.0, 30.0, 40.0, 0.77, 19]]], mag=2)


def test_count_zero_leaves_the_picture_alone_and_count_cap_draws_every_row():
    imgs = noise(7, (50, 70), (50, 70))
    rng = np.random.default_rng(8)
    cap = 300                                                       # more rows than one staging chunk of the kernel
    rows = []
    for _ in range(cap):
        t, l = rng.uniform(-5, 45), rng.uniform(-5, 65)
        rows.append([t, l, t + rng.uniform(0, 25), l + rng.uniform(0, 30), rng.uniform(0, 1), int(rng.integers(0, 20))])
    got = check(imgs, [[], rows], cap=cap)
    assert np.array_equal(got[0], imgs[0])
    # counts outside [0, cap] are clamped
    got2, _ = run_gpu(imgs, [[], rows], draw.glyph_atlas(), cap=cap, counts=[-4, cap + 1000])
    assert np.array_equal(got2[0], imgs[0]) and np.array_equal(got2[1], got[1])


def test_a_batch_of_different_sizes_thickness_and_magnification():
    shapes = [(30, 40), (97, 131), (240, 320), (1100, 64)]
    imgs = noise(9, *shapes)
    rng = np.random.default_rng(10)
    rows = []
    for h, w in shapes:
        r = []
        for _ in range(5):
            t, l = rng.uniform(-0.1 * h, 0.8 * h), rng.uniform(-0.1 * w, 0.8 * w)
            r.append([t, l, t + rng.uniform(0.05, 0.5) * h, l + rng.uniform(0.05, 0.9) * w, rng.uniform(0, 1), int(rng.integers(0, 20))])
        rows.append(r)
    _, table = run_gpu(imgs, rows, draw.glyph_atlas())
    assert table['mag'].tolist() == [1, 1, 1, 2] and table['thickness'].tolist() == [1, 1, 1, 3]
    check(imgs, rows)
    check(imgs, rows, thickness=np.asarray([1, 2, 3, 4], np.int32))


def test_label_digits_are_pythons_for_ties_and_ends():
    scores = [0.0, 0.005, 0.125, 0.285, 0.995, 1.0]
    atlas = draw.glyph_atlas()
    for cls in (0, 7, 19):
        rows = [[4.0 + 20 * k, 3.0, 22.0 + 20 * k, 70.0, s, cls] for k, s in enumerate(scores)]
        got = check(noise(11, (130, 80)), [rows], atlas=atlas)[0]
        for k, s in enumerate(scores):                              # read the glyph indices back out of the drawn label
            t, l = 4 + 20 * k, 3
            cells = got[t + 1:t + 17, l:l + 56].reshape(16, 7, 8, 3)
            text = '{:2d} {:.2f}'.format(cls, float(np.float32(s)))
            for slot in range(7):
                ink = (cells[:, slot] == 0).all(-1).astype(np.uint8)
                assert np.array_equal(ink, atlas['0123456789. '.index(text[slot])]), (cls, s, slot)
            assert draw.label_glyphs(cls, s) == ['0123456789. '.index(ch) for ch in text]


def test_outlines_alone_equal_pils_rectangle_loop():
    """With the label off (gh = 0) the picture is what inference.py's ImageDraw.rectangle loop paints."""
    from PIL import Image, ImageDraw
    for seed, (h, w) in ((12, (240, 320)), (13, (375, 500)), (14, (61, 47))):
        img = noise(seed, (h, w))[0]
        rng = np.random.default_rng(seed)
        rows = []
        for _ in range(8):
            t, l = rng.uniform(-0.1 * h, 0.9 * h), rng.uniform(-0.1 * w, 0.9 * w)
            rows.append([t, l, t + rng.uniform(0, 0.6) * h, l + rng.uniform(0, 0.6) * w, 0.5, int(rng.integers(0, 20))])
        rows += [[10.0, 10.0, 12.0, 30.0, 0.5, 1], [20.0, 5.0, 21.0, 6.0, 0.5, 2], [h - 10.0, w - 10.0, float(h), float(w), 0.5, 3]]
        got, table = run_gpu([img], [rows], np.zeros((12, 0, 8), np.uint8))
        pil = Image.fromarray(img.copy())
        d = ImageDraw.Draw(pil)
        thickness = max(1, (h + w) // 300)
        assert int(table['thickness'][0]) == thickness
        for row in rows:                                            # inference.py:68-75
            c4 = corners(row, h, w)
            if c4 is None:
                continue
            t, l, b, r = c4
            for j in range(thickness):
                if r - j > l + j and b - j > t + j:
                    d.rectangle([l + j, t + j, r - j, b - j], outline=tuple(int(v) for v in COLOURS[int(row[5]) % len(COLOURS)]))
        assert np.array_equal(got[0], np.asarray(pil)), (h, w)


def test_two_runs_give_the_same_bytes_and_bad_arguments_are_refused():
    import ctypes as C
    import torch
    from k210_yolo_framework_amd import engine
    imgs = noise(15, (97, 131), (30, 40))
    rows = [[[5.0, 5.0, 60.0, 100.0, 0.5, 1], [20.0, 30.0, 90.0, 120.0, 0.25, 2]], [[2.0, 2.0, 20.0, 30.0, 0.1, 3]]]
    a, _ = run_gpu(imgs, rows, draw.glyph_atlas())
    b, _ = run_gpu(imgs, rows, draw.glyph_atlas())
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    L = engine.lib()
    buf = torch.zeros(64, dtype=torch.uint8, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    good = [p, C.c_size_t(64), p, C.c_int(1), p, C.c_int(1), p, p, C.c_int(1), p, C.c_int(16), C.c_int(8), C.c_size_t(1), None]
    for pos, bad in ((0, None), (2, None), (4, None), (6, None), (7, None), (9, None), (3, C.c_int(0)), (5, C.c_int(0)), (8, C.c_int(0)),
                     (10, C.c_int(-1)), (11, C.c_int(0)), (1, C.c_size_t(0)), (12, C.c_size_t(0))):
        args = list(good)
        args[pos] = bad
        assert L.yk_draw_dets_u8(*args) == -10, pos                 # YK_ERR_ARG: refused before anything is launched
        assert b'yk_draw_dets_u8' in L.yk_last_error()
    torch.cuda.synchronize()

"""HSV colour jitter, host side (k210_yolo_framework_amd/colour.py): the draws, the configuration, the exact properties of the pixel rule on
a lattice of colours and over all 2^24, hand-computed pixels, the host generator `training.batches(hsv=)`, the arguments yk_hsv_jitter_u8
refuses before it needs a device, and the CLI."""
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import augment, colour, mosaic

ROOT = Path(__file__).resolve().parents[1]
LEVELS = sorted(set(range(0, 256, 8)) | {1, 2, 127, 128, 254, 255})


def lattice() -> np.ndarray:
    """[37^3, 3] u8 (128 is a multiple of 8 already, so 37 levels): every combination of LEVELS - every grey level of LEVELS, every sector boundary of the hue circle, both ends."""
    a = np.array(LEVELS, np.uint8)
    return np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)


def _one(colours, dh, gs, gv):
    return colour.jitter_u8(np.ascontiguousarray(colours, np.uint8).reshape(1, -1, 3), (dh, gs, gv)).reshape(-1, 3)


def test_lattice_is_what_the_tests_say():
    L = lattice()
    assert len(LEVELS) == 37 and L.shape == (37 ** 3, 3)
    greys = L[(L[:, 0] == L[:, 1]) & (L[:, 1] == L[:, 2])][:, 0]
    assert sorted(greys.tolist()) == LEVELS and {0, 255} <= set(LEVELS)
    # sector boundaries: pure primaries and secondaries (h = 0, 1, .. 5) at full and at partial saturation
    for c in [(255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255), (128, 8, 8), (8, 128, 128)]:
        assert (L == np.array(c, np.uint8)).all(1).any(), c


def test_table_is_a_function_of_seed_epoch_and_row_only():
    cfg = colour.HsvConfig()
    t = colour.param_table(5, 2, 100, cfg)
    assert t.shape == (100, 3) and t.dtype == np.float64
    np.testing.assert_array_equal(t, colour.param_table(5, 2, 100, cfg))
    np.testing.assert_array_equal(colour.uniforms(5, 2, 100), np.random.default_rng([5, 2, 3]).random((100, 6)))
    assert not np.array_equal(t, colour.param_table(6, 2, 100, cfg)) and not np.array_equal(t, colour.param_table(5, 3, 100, cfg))
    # a stream of its own: not the augmentation's, not the mosaic's
    u = colour.uniforms(5, 2, 100)
    assert not np.array_equal(u[:, :5], augment.param_table(5, 2, 100)) and not np.array_equal(u, mosaic.param_table(5, 2, 100)[:, :6])
    # however the rows are split between ranks, a row finds the same parameters
    rows = np.random.default_rng(0).permutation(100)
    for world in (1, 2, 4):
        got = np.concatenate([t[rows[r::world]] for r in range(world)])
        want = np.concatenate([colour.param_table(5, 2, 100, cfg)[rows[r::world]] for r in range(world)])
        np.testing.assert_array_equal(got, want)


def test_decode_follows_the_written_rule():
    u = np.array([[0.3, 0.75, 0.5, 0.9, 0.25, 0.1],
                  [0.95, 0.75, 0.5, 0.9, 0.25, 0.1],                 # u0 >= prob: neutral
                  [0.0, 0.0, 1.0, 0.2, 0.0, 0.7]])
    p = colour.decode(u, colour.HsvConfig(hue=0.1, sat=1.5, exposure=2.0, prob=0.9))
    np.testing.assert_array_equal(p[0], [0.1 * (2.0 * 0.75 - 1.0), 1.0 + 0.5 * 0.5, 1.0 / (1.0 + 1.0 * 0.25)])
    np.testing.assert_array_equal(p[1], [0.0, 1.0, 1.0])
    np.testing.assert_array_equal(p[2], [0.1 * -1.0, 1.0 / 1.5, 1.0])


def test_neutral_configurations_give_neutral_rows():
    np.testing.assert_array_equal(colour.param_table(1, 0, 500, colour.HsvConfig(prob=0.0)), np.tile([0.0, 1.0, 1.0], (500, 1)))
    np.testing.assert_array_equal(colour.param_table(1, 0, 500, colour.HsvConfig(hue=0.0, sat=1.0, exposure=1.0)), np.tile([0.0, 1.0, 1.0], (500, 1)))


def test_draws_stay_in_their_ranges_over_ten_thousand_rows():
    cfg = colour.HsvConfig(hue=0.1, sat=1.5, exposure=2.5, prob=0.7)
    p = colour.param_table(3, 1, 10 ** 4, cfg)
    assert (np.abs(p[:, 0]) <= cfg.hue).all()
    assert (p[:, 1] >= 1.0 / cfg.sat).all() and (p[:, 1] <= cfg.sat).all()
    assert (p[:, 2] >= 1.0 / cfg.exposure).all() and (p[:, 2] <= cfg.exposure).all()
    neutral = (p == np.array([0.0, 1.0, 1.0])).all(1)
    assert 0.25 < neutral.mean() < 0.35                              # 1 - prob of the rows
    live = p[~neutral]
    assert (live[:, 0] < 0).any() and (live[:, 0] > 0).any() and (live[:, 1] < 1).any() and (live[:, 1] > 1).any()
    assert (live[:, 2] < 1).any() and (live[:, 2] > 1).any()


@pytest.mark.parametrize('bad', [dict(hue=-0.01), dict(hue=0.51), dict(hue=np.nan), dict(hue=np.inf), dict(sat=0.99), dict(sat=0.0),
                                 dict(sat=-2.0), dict(sat=np.nan), dict(sat=np.inf), dict(exposure=0.5), dict(exposure=np.nan),
                                 dict(exposure=np.inf), dict(prob=-0.1), dict(prob=1.1), dict(prob=np.nan)])
def test_every_bad_configuration_value_is_refused(bad):
    with pytest.raises(ValueError, match=next(iter(bad))):
        colour.param_table(0, 0, 4, colour.HsvConfig(**bad))
    with pytest.raises(ValueError, match=next(iter(bad))):
        colour.validate(colour.HsvConfig(**bad))


def test_good_configuration_edges_are_accepted():
    for cfg in (colour.HsvConfig(0.0, 1.0, 1.0, 0.0), colour.HsvConfig(0.5, 1.0, 100.0, 1.0)):
        assert colour.validate(cfg) == cfg


def test_jitter_refuses_rows_it_must_not_follow_and_wrong_inputs():
    img = np.zeros((2, 3, 4, 3), np.uint8)
    for row in [(np.nan, 1, 1), (0, np.inf, 1), (0, 1, -np.inf), (0, -0.5, 1), (0, 1, -1e-9)]:
        with pytest.raises(ValueError):
            colour.jitter_u8(img, np.array([(0.0, 1.0, 1.0), row]))
    with pytest.raises(ValueError):
        colour.jitter_u8(img, np.ones((3, 3)))                      # three rows for two frames
    with pytest.raises(ValueError):
        colour.jitter_u8(img.astype(np.float32), (0, 1, 1))
    with pytest.raises(ValueError):
        colour.jitter_u8(np.zeros((3, 4, 4), np.uint8), (0, 1, 1))


def test_a_neutral_row_returns_every_colour_of_the_lattice():       # property (a)
    L = lattice()
    np.testing.assert_array_equal(colour._jitter_one(L[None], 0.0, 1.0, 1.0)[0], L)         # the arithmetic itself, not the shortcut
    np.testing.assert_array_equal(_one(L, 0.0, 1.0, 1.0), L)
    np.testing.assert_array_equal(_one(L, -0.0, 1.0, 1.0), L)


def test_a_neutral_row_returns_every_one_of_the_2_to_24_colours():  # property (a) on every colour: one pass of the arithmetic
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    for r0 in range(0, 256, 32):
        block = np.empty((32, 256, 256, 3), np.uint8)
        block[..., 0] = np.arange(r0, r0 + 32, dtype=np.uint8)[:, None, None]
        block[..., 1], block[..., 2] = g, b
        flat = block.reshape(1, -1, 3)
        assert np.array_equal(colour._jitter_one(flat, 0.0, 1.0, 1.0), flat), r0


def test_a_whole_turn_returns_every_colour():                       # property (b)
    L = lattice()
    np.testing.assert_array_equal(_one(L, 1.0, 1.0, 1.0), L)
    np.testing.assert_array_equal(_one(L, -1.0, 1.0, 1.0), L)


def test_a_third_of_a_turn_rotates_the_channels():                   # property (c)
    L = lattice()
    np.testing.assert_array_equal(_one(L, 1.0 / 3.0, 1.0, 1.0), L[:, [2, 0, 1]])


@pytest.mark.parametrize('row', [(0.07, 1.5, 0.8), (-0.3, 0.0, 1.5), (0.5, 3.0, 4.0), (0.1, 1.0 / 1.5, 1.0 / 1.5), (0.0371, 1.234, 0.777)])
def test_grey_stays_grey(row):                                       # property (d)
    g = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    out = _one(g, *row)
    want = np.minimum(255, np.floor(np.arange(256, dtype=np.float64) * row[2] + 0.5)).astype(np.uint8)
    np.testing.assert_array_equal(out, np.repeat(want[:, None], 3, 1))


@pytest.mark.parametrize('dh, gv', [(0.03, 1.0), (-0.21, 1.0), (0.5, 0.5), (0.0, 1.7)])
def test_no_saturation_gives_the_value_in_all_three_channels(dh, gv):     # property (e)
    L = lattice()
    v = np.minimum(255, np.floor(L.max(1).astype(np.float64) * gv + 0.5)).astype(np.uint8)
    np.testing.assert_array_equal(_one(L, dh, 0.0, gv), np.repeat(v[:, None], 3, 1))


def test_hand_computed_pixels():
    one = lambda rgb, row: tuple(int(v) for v in colour.jitter_u8(np.array([[rgb]], np.uint8), row)[0, 0])
    # red, h = 0, a sixth of a turn on: h = 1, i = 1, f = 0: (q, V, p) = (255(1 - 0), 255, 255(1 - 1)) - yellow
    assert one((255, 0, 0), (1.0 / 6.0, 1.0, 1.0)) == (255, 255, 0)
    # gs = 0: S' = 0, p = q = t = V' = 200
    assert one((200, 100, 50), (0.0, 0.0, 1.0)) == (200, 200, 200)
    # (100, 50, 25): V = 100, d = 75, S = 0.75, h = (50 - 25)/75 = 1/3 (sector 0, f = 1/3).  gv = 4: V' = min(255, 400) = 255, hue and
    # saturation kept: (V', t, p) with t = 255(1 - 0.75 * 2/3) = 127.5 -> 128 and p = 255 * 0.25 = 63.75 -> 64
    assert one((100, 50, 25), (0.0, 1.0, 4.0)) == (255, 128, 64)
    # black is a fixed point
    for row in [(0.0, 1.0, 1.0), (0.37, 2.5, 4.0), (-0.5, 0.0, 0.1), (1.0, 1e6, 1e6)]:
        assert one((0, 0, 0), row) == (0, 0, 0)
    # frames of a batch each follow their own row; a single frame takes one row
    img = np.array([[[(255, 0, 0)]], [[(200, 100, 50)]], [[(9, 8, 7)]]], np.uint8)
    out = colour.jitter_u8(img, np.array([(1.0 / 6.0, 1.0, 1.0), (0.0, 0.0, 1.0), (0.0, 1.0, 1.0)]))
    assert out.shape == img.shape and out.dtype == np.uint8
    assert [tuple(int(v) for v in o[0, 0]) for o in out] == [(255, 255, 0), (200, 200, 200), (9, 8, 7)]
    assert img[0, 0, 0].tolist() == [255, 0, 0]                     # not in place


def _h(hw):
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    return Helper(None, 20, VOC_ANCHORS, [list(hw)], [[7, 10], [14, 20]])


def _items(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        hw = [(30, 40), (47, 61), (24, 40), (17, 23)][k % 4]
        m = int(rng.integers(1, 4))
        boxes = np.concatenate([rng.integers(0, 20, (m, 1)).astype(float), rng.uniform(0.2, 0.8, (m, 2)), rng.uniform(0.1, 0.4, (m, 2))], 1)
        out.append((rng.integers(1, 256, (*hw, 3), dtype=np.uint8), boxes))
    return out


class _Fixed:
    def __init__(self, order):
        self.order = order

    def permutation(self, n):
        return self.order


@pytest.mark.parametrize('augmented, mosaicked', [(False, False), (True, False), (False, True), (True, True)])
def test_host_generator_jitters_the_finished_frame_and_leaves_the_labels(augmented, mosaicked):
    from k210_yolo_framework_amd import training
    hw = (28, 40)
    h, items = _h(hw), _items(12, seed=4)
    seed, epoch, cfg = 3, 1, colour.HsvConfig()
    order = np.random.default_rng(9).permutation(len(items))
    kw = dict(augment=(seed, epoch) if augmented else None, mosaic=(seed, epoch, 0.7) if mosaicked else None)
    got = list(training.batches(h, items, 4, _Fixed(order), shuffle=True, hsv=(seed, epoch, cfg), **kw))
    table = colour.param_table(seed, epoch, len(items), cfg)
    plain = list(training.batches(h, items, 4, _Fixed(order), shuffle=True, **kw))
    assert len(got) == len(plain) == 3
    changed = 0
    for b, ((gx, gys), (px, pys)) in enumerate(zip(got, plain)):
        for gy, py in zip(gys, pys):
            np.testing.assert_array_equal(gy, py)                   # labels: identical to the run without
        for k in range(4):
            row = order[4 * b + k]
            frame = _frame_u8(h, items, row, seed, epoch, hw, augmented, mosaicked)
            np.testing.assert_array_equal(px[k], (frame / np.max(frame)).astype(np.float32))       # (the reconstruction is the generator's)
            jit = colour.jitter_u8(frame, table[row])
            np.testing.assert_array_equal(gx[k], (jit / np.max(jit)).astype(np.float32), err_msg=f'batch {b} sample {k}')
            changed += not np.array_equal(jit, frame)
    assert changed == 12


def _frame_u8(h, items, row, seed, epoch, hw, augmented, mosaicked):
    """The finished u8 frame of dataset row `row`: letterbox or mosaic, then the warp - what `batches` hands to the jitter."""
    from k210_yolo_framework_amd.helper import letterbox_bilinear
    if mosaicked:
        mt = mosaic.param_table(seed, epoch, len(items))
        quads, centres, _ = mosaic.plan([row], mt, lambda i: items[i][0].shape[:2], hw, boxes_of=lambda i: items[i][1], prob=0.7)
        frame = mosaic.compose_u8([items[int(j)][0] for j in quads[0]['item']], quads[0], centres[0], hw)
    else:
        scale, translation = h.letterbox_params(items[row][0].shape[:2])
        frame = letterbox_bilinear(items[row][0], hw, float(scale[0]), translation)
    if augmented:
        frame = augment.warp_u8(frame, augment.matrices(augment.param_table(seed, epoch, len(items))[row].reshape(1, 5), hw)[2][0])
    return frame


def test_prob_zero_is_the_run_without():
    from k210_yolo_framework_amd import training
    h, items = _h((28, 40)), _items(8, seed=2)
    order = np.arange(8)
    a = list(training.batches(h, items, 4, _Fixed(order), shuffle=True, hsv=(1, 0, colour.HsvConfig(prob=0.0))))
    b = list(training.batches(h, items, 4, _Fixed(order), shuffle=True))
    for (ax, ays), (bx, bys) in zip(a, b):
        np.testing.assert_array_equal(ax, bx)
        for ay, by in zip(ays, bys):
            np.testing.assert_array_equal(ay, by)


@pytest.fixture(scope='module')
def lib():
    from k210_yolo_framework_amd import engine
    if not engine.library_path().exists():
        import __graft_entry__ as g
        g.build()
    return engine.lib()


def test_yk_hsv_jitter_u8_refuses_bad_arguments_before_it_needs_a_device(lib):
    frames, params = np.zeros((2, 3, 4, 3), np.uint8), np.tile([0.0, 1.0, 1.0], (2, 1))
    assert lib.yk_hsv_jitter_u8(frames, 0, 3, 4, params, None) == 0                  # n = 0: a successful no-op
    assert lib.yk_hsv_jitter_u8(None, 0, 3, 4, None, None) == 0
    for args in [(None, 2, 3, 4, params), (frames, 2, 3, 4, None), (frames, -1, 3, 4, params), (frames, 2, 0, 4, params),
                 (frames, 2, 3, 0, params), (frames, 2, -3, 4, params), (frames, 0, 0, 4, params),
                 (frames, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, params)]:      # 3 n h w does not fit a size_t
        assert lib.yk_hsv_jitter_u8(*args, None) == -10               # YK_ERR_ARG
        assert b'yk_hsv_jitter_u8' in lib.yk_last_error()
    assert not frames.any()


def test_cli_knows_the_five_options_and_refuses_them_without_a_device():
    import torch
    from k210_yolo_framework_amd import engine, training
    a = training.parser().parse_args([])
    assert (a.hsv, a.hsv_hue, a.hsv_sat, a.hsv_exposure, a.hsv_prob) == ('False', 0.1, 1.5, 1.5, 1.0)
    a = training.parser().parse_args(['--hsv', 'True', '--hsv_hue', '0.05', '--hsv_sat', '2', '--hsv_exposure', '1.2', '--hsv_prob', '0.5'])
    assert (a.hsv, a.hsv_hue, a.hsv_sat, a.hsv_exposure, a.hsv_prob) == ('True', 0.05, 2.0, 1.2, 0.5)
    mk = (ROOT / 'Makefile').read_text()
    assert '--hsv $(HSV) --hsv_hue $(HSVHUE) --hsv_sat $(HSVSAT) --hsv_exposure $(HSVEXP) --hsv_prob $(HSVPROB)' in mk
    for flag, value in [('--hsv_hue', '0.6'), ('--hsv_hue', '-0.1'), ('--hsv_sat', '0.5'), ('--hsv_exposure', '0.9'), ('--hsv_prob', '1.5'),
                        ('--hsv_sat', 'nan'), ('--hsv_exposure', 'inf')]:
        with pytest.raises(engine.YkError, match=flag + ' '):       # refused by name, before anything needs a device
            training.cli(['--synthetic', '16', '--hsv', 'True', flag, value, '--max_steps', '1'])
    if not torch.cuda.is_available():
        with pytest.raises(engine.YkError, match='--hsv True'):
            training.cli(['--synthetic', '16', '--hsv', 'True', '--max_steps', '1'])

"""Positive assignment of the label builder, host side (Helper.box_to_label / batch_box_to_label, assign='best' | 'multi'): the multi rule
against a literal per-box restatement written here, on crafted cases; the batched and the per-sample form agree; 'best' is the code as it
stood; the host generator `training.batches(assign=)`; the arguments yk_boxes_to_labels_f32 refuses before it needs a device; the CLI."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS

ROOT = Path(__file__).resolve().parents[1]
OUT_HW = [[7, 10], [14, 20]]


def _h(class_num=20, anchors=VOC_ANCHORS, out_hw=OUT_HW, in_hw=(224, 320)):
    return Helper(None, class_num, np.asarray(anchors, float), [list(in_hw)], out_hw)


def fit_of(wh, anchor):
    """Helper._fake_iou for one box and one anchor, in Python floats (IEEE doubles, one rounding per operation, numpy's order)."""
    overlap = max(min(wh[0], anchor[0]), 0.0) * max(min(wh[1], anchor[1]), 0.0)
    return overlap / (wh[0] * wh[1] + anchor[0] * anchor[1] - overlap)


def restated(h: Helper, samples, assign, assign_iou):
    """The issue's rule, box by box: all secondary candidates in box order, then all primary candidates in box order."""
    grids = [np.zeros((len(samples), int(gh), int(gw), len(h.anchors[l]), 5 + h.class_num), np.float32) for l, (gh, gw) in enumerate(h.out_hw)]

    def write(s, l, a, box):
        gh, gw = (int(v) for v in h.out_hw[l])
        cx, cy = int(np.floor(box[1] * gw)), int(np.floor(box[2] * gh))
        assert 0 <= cx < gw and 0 <= cy < gh
        slot = grids[l][s, cy, cx, a]
        slot[:4] = np.clip(box[1:5], 1e-8, 1.0)
        slot[4] = 1.0
        slot[5 + int(box[0])] = 1.0
    todo = []
    for s, boxes in enumerate(samples):
        for box in np.asarray(boxes, float).reshape(-1, 5):
            fits = [(fit_of(box[3:5], h.anchors[l][a]), l, a) for l in range(len(h.anchors)) for a in range(len(h.anchors[l]))]
            best = max(f for f, _, _ in fits)
            primary = next((l, a) for f, l, a in fits if f == best)                       # the first of equal maxima
            todo.append((s, box, primary, [(l, a) for f, l, a in fits if (l, a) != primary and f > assign_iou] if assign == 'multi' else []))
    for s, box, _, second in todo:
        for l, a in second:
            write(s, l, a, box)
    for s, box, (l, a), _ in todo:
        write(s, l, a, box)
    return grids


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


def positives(grids):
    return int(sum((g[..., 4] == 1).sum() for g in grids))


# anchors made for the crafted cases: layer 0 holds a big and a small anchor, layer 1 a copy of the big one and a wide one
CRAFT = np.array([[[0.5, 0.5], [0.1, 0.1]], [[0.5, 0.5], [0.5, 0.25]]])


def test_a_box_without_secondary_slots_equals_best():
    h = _h(3, CRAFT)
    box = [np.array([[1, 0.31, 0.62, 0.1, 0.1]])]                    # fits (0, 1) exactly; every other fit is 0.04 or 0.08
    multi = h.batch_box_to_label(box, 'multi', 0.213)
    same(multi, h.batch_box_to_label(box))
    same(multi, restated(h, box, 'multi', 0.213))
    assert positives(multi) == 1


def test_a_box_above_the_threshold_in_both_layers():
    h = _h(3, CRAFT)
    box = [np.array([[2, 0.31, 0.62, 0.5, 0.5]])]                    # fits (0, 0) and (1, 0) with 1.0 (primary: the first), (1, 1) with 0.5
    multi = h.batch_box_to_label(box, 'multi', 0.213)
    same(multi, restated(h, box, 'multi', 0.213))
    assert positives(multi) == 3 and positives(h.batch_box_to_label(box)) == 1
    assert multi[0][0, 4, 3, 0, 4] == 1 and multi[1][0, 8, 6, 0, 4] == 1 and multi[1][0, 8, 6, 1, 4] == 1
    np.testing.assert_array_equal(multi[1][0, 8, 6, 1, :4], np.float32([0.31, 0.62, 0.5, 0.5]))
    assert multi[1][0, 8, 6, 1, 5:].tolist() == [0, 0, 1]


def test_a_fit_equal_to_the_threshold_is_not_taken():
    h = _h(3, CRAFT)
    box = [np.array([[0, 0.5, 0.5, 0.5, 0.5]])]
    thr = fit_of((0.5, 0.5), CRAFT[1][1])                            # 0.5, exactly
    assert thr == 0.5
    at = h.batch_box_to_label(box, 'multi', thr)
    below = h.batch_box_to_label(box, 'multi', np.nextafter(thr, 0))
    same(at, restated(h, box, 'multi', thr))
    same(below, restated(h, box, 'multi', np.nextafter(thr, 0)))
    assert at[1][0, 7, 10, 1, 4] == 0 and below[1][0, 7, 10, 1, 4] == 1
    assert positives(at) == 2 and positives(below) == 3


def test_a_later_secondary_meets_an_earlier_primary():
    h = _h(3, CRAFT)
    # box 0: primary (1, 1).  box 1 (later): primary (0, 0), secondary (1, 0) and (1, 1) - the same cell of layer 1, anchor 1
    boxes = [np.array([[0, 0.52, 0.52, 0.5, 0.25], [2, 0.53, 0.53, 0.5, 0.5]])]
    multi = h.batch_box_to_label(boxes, 'multi', 0.213)
    same(multi, restated(h, boxes, 'multi', 0.213))
    slot = multi[1][0, 7, 10, 1]
    np.testing.assert_array_equal(slot[:5], np.float32([0.52, 0.52, 0.5, 0.25, 1]))      # the primary's xywh stays
    assert slot[5:].tolist() == [1, 0, 1]                                                # both class bits


def test_two_primaries_in_one_slot_the_last_wins():
    h = _h(3, CRAFT)
    boxes = [np.array([[0, 0.52, 0.6, 0.5, 0.5], [1, 0.58, 0.58, 0.45, 0.5]])]      # both in column 5, row 4 of layer 0, anchor 0
    for mode in ('best', 'multi'):
        got = h.batch_box_to_label(boxes, mode, 0.9)
        same(got, restated(h, boxes, mode, 0.9))
        np.testing.assert_array_equal(got[0][0, 4, 5, 0, :5], np.float32([0.58, 0.58, 0.45, 0.5, 1]))
        assert got[0][0, 4, 5, 0, 5:].tolist() == [1, 1, 0]


def test_an_empty_sample_between_full_ones():
    h = _h(3, CRAFT)
    boxes = [np.array([[2, 0.31, 0.62, 0.5, 0.5]]), np.zeros((0, 5)), np.array([[1, 0.9, 0.1, 0.1, 0.1], [0, 0.2, 0.2, 0.5, 0.3]])]
    multi = h.batch_box_to_label(boxes, 'multi', 0.213)
    same(multi, restated(h, boxes, 'multi', 0.213))
    assert not any(g[1].any() for g in multi) and all(g[0].any() or g[2].any() for g in multi)


def _random_samples(rng, n, class_num, most=6):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, most + 1))
        b = np.column_stack([rng.integers(0, class_num, k), rng.uniform(0.0, 0.999, (k, 2)), rng.uniform(0.02, 0.9, (k, 2))])
        out.append(b.reshape(-1, 5))
    return out


@pytest.mark.parametrize('assign', ['best', 'multi'])
def test_stacked_box_to_label_equals_the_batched_form_and_the_restatement(assign):
    h = _h()
    samples = _random_samples(np.random.default_rng(3), 24, 20)
    samples += [np.tile([[3, 0.55, 0.45, 0.3, 0.6]], (5, 1)) * [1, 1, 1, 1, 1] + np.arange(5)[:, None] * [1, 0, 0, 0.01, 0]]   # one cell, many classes
    for thr in (0.213, 0.01, 0.6):
        batched = h.batch_box_to_label(samples, assign, thr)
        single = [h.box_to_label(b, assign=assign, assign_iou=thr) for b in samples]
        same(batched, [np.stack([s[l] for s in single]) for l in range(2)])
        same(batched, restated(h, samples, assign, thr))
    if assign == 'multi':
        assert positives(h.batch_box_to_label(samples, 'multi', 0.01)) > positives(h.batch_box_to_label(samples, 'multi', 0.6)) >= \
            positives(h.batch_box_to_label(samples))


def _best_as_it_stood(h: Helper, boxes_per_sample):
    """Helper.batch_box_to_label before it had an `assign` argument, kept here word for word."""
    n = len(boxes_per_sample)
    grids = [np.zeros((n, *map(int, h.out_hw[l]), len(h.anchors[l]), 5 + h.class_num), np.float32) for l in range(h.output_number)]
    per = [np.asarray(b, float).reshape(-1, 5) for b in boxes_per_sample]
    counts = [len(b) for b in per]
    if sum(counts) == 0:
        return grids
    allb = np.concatenate(per)
    sid = np.repeat(np.arange(n), counts)
    fit = Helper._fake_iou(allb[:, None, None, 3:5], h.anchors[None])
    layer, anchor = np.unravel_index(fit.reshape(len(allb), -1).argmax(1), fit.shape[1:])
    xywh = np.clip(allb[:, 1:5], 1e-8, 1.0)
    cls = allb[:, 0].astype(int)
    for l in range(h.output_number):
        m = np.nonzero(layer == l)[0]
        if not len(m):
            continue
        gh, gw = h.out_hw[l]
        cell = np.floor(allb[m, 1:3] * (gw, gh)).astype(int)
        s_, cy, cx, a = sid[m], cell[:, 1], cell[:, 0], anchor[m]
        grids[l][s_, cy, cx, a, :4] = xywh[m]
        grids[l][s_, cy, cx, a, 4] = 1.0
        grids[l][s_, cy, cx, a, 5 + cls[m]] = 1.0
    return grids


def test_best_with_any_assign_iou_is_the_present_output():
    h = _h()
    samples = _random_samples(np.random.default_rng(11), 40, 20, most=12)
    want = _best_as_it_stood(h, samples)
    same(h.batch_box_to_label(samples), want)
    for thr in (0.213, 0.0, 1.0, -3.0, 7.5, float('nan')):
        same(h.batch_box_to_label(samples, 'best', thr), want)
        same(h.batch_box_to_label(samples, assign='best', assign_iou=thr), want)
    same([np.stack([h.box_to_label(b, assign_iou=9.0)[l] for b in samples]) for l in range(2)], want)


def test_bad_options_are_refused_by_name():
    h = _h()
    box = [np.array([[0, 0.5, 0.5, 0.2, 0.2]])]
    for thr in (0.0, 1.0, -0.1, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='assign_iou'):
            h.batch_box_to_label(box, 'multi', thr)
        with pytest.raises(ValueError, match='assign_iou'):
            h.box_to_label(box[0], assign='multi', assign_iou=thr)
    for mode in ('all', '', None, 'Best'):
        with pytest.raises(ValueError, match='assign '):
            h.batch_box_to_label(box, mode)
        with pytest.raises(ValueError, match='assign '):
            h.box_to_label(box[0], assign=mode)


def test_training_batches_yields_these_labels():
    from k210_yolo_framework_amd import training
    hw = (28, 40)
    h = Helper(None, 5, VOC_ANCHORS, [list(hw)], [[2, 3], [4, 5]])
    items = training.synthetic_list(8, hw, 5, seed=2)
    plain = list(training.batches(h, items, 4, None, shuffle=False, with_boxes=True))
    best = list(training.batches(h, items, 4, None, shuffle=False, assign='best', assign_iou=0.5))
    multi = list(training.batches(h, items, 4, None, shuffle=False, with_boxes=True, assign='multi', assign_iou=0.213))
    assert len(plain) == len(best) == len(multi) == 2
    more = 0
    for (px, pys, pbs), (bx, bys), (mx, mys, mbs) in zip(plain, best, multi):
        np.testing.assert_array_equal(px, mx)
        same(bys, pys)
        same(mys, h.batch_box_to_label(mbs, 'multi', 0.213))
        same(mys, restated(h, mbs, 'multi', 0.213))
        more += positives(mys) - positives(pys)
    assert more > 0


# ---- the C entry point: every refusal comes before a device is needed -------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    from k210_yolo_framework_amd import engine
    if not engine.library_path().exists():
        import __graft_entry__ as g
        g.build()
    return engine.lib()


def test_label_cfg_is_the_headers_struct():
    from k210_yolo_framework_amd import engine
    assert C.sizeof(engine.LabelCfg) == 4 * 4 + 3 * 4 * 4 + 4 * 8 * 2 * 8 + 8 == 584
    assert engine.LabelCfg.anchors.offset == 64 and engine.LabelCfg.assign_iou.offset == 576
    cfg = engine.make_label_cfg(_h(), 'multi', 0.3)
    assert (cfg.n_layers, cfg.class_num, cfg.assign, cfg.assign_iou) == (2, 20, 1, 0.3)
    assert list(cfg.out_h)[:2] == [7, 14] and list(cfg.out_w)[:2] == [10, 20] and list(cfg.anchor_num)[:2] == [3, 3]
    assert cfg.anchors[1][2][0] == VOC_ANCHORS[1][2][0] and cfg.anchors[0][1][1] == VOC_ANCHORS[0][1][1]
    header = engine.HEADER_PATH.read_text()
    assert 'YK_ASSIGN_BEST = 0, YK_ASSIGN_MULTI = 1' in header and '#define YK_LABEL_LDS_BOXES 512' in header
    with pytest.raises(engine.YkError, match='assign_iou'):
        engine.make_label_cfg(_h(), 'multi', 1.0)


def test_yk_boxes_to_labels_f32_refuses_bad_arguments_before_it_needs_a_device(lib):
    from k210_yolo_framework_amd import engine
    h = _h()
    boxes = np.array([[0, 0.5, 0.5, 0.2, 0.2], [1, 0.2, 0.2, 0.5, 0.5]])
    first = np.array([0, 1, 2], np.int32)
    labels = np.zeros(2 * (7 * 10 + 14 * 20) * 3 * 25, np.float32)
    status = np.array([5], np.int32)

    def cfg(**change):
        c = engine.make_label_cfg(h, 'multi', 0.213)
        for k, v in change.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return C.byref(c)
    ok = (cfg(), boxes, 2, first, 2, labels, status)
    assert lib.yk_boxes_to_labels_f32(cfg(), boxes, 2, first, 0, labels, status, None) == 0          # n = 0: a successful no-op
    assert lib.yk_boxes_to_labels_f32(None, None, 0, None, 0, None, None, None) == 0
    bad = [(None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:3] + (None,) + ok[4:], ok[:5] + (None, status), ok[:6] + (None,),   # NULL with n > 0
           ok[:4] + (-1,) + ok[5:], ok[:2] + (-1,) + ok[3:], ok[:2] + (2 ** 30,) + ok[3:],
           (cfg(n_layers=0),) + ok[1:], (cfg(n_layers=engine.YK_MAX_LAYERS + 1),) + ok[1:],
           (cfg(anchor_num=(1, 0)),) + ok[1:], (cfg(anchor_num=(0, engine.YK_MAX_ANCHORS + 1)),) + ok[1:],
           (cfg(out_h=(0, 0)),) + ok[1:], (cfg(out_w=(1, -4)),) + ok[1:], (cfg(class_num=0),) + ok[1:], (cfg(assign=2),) + ok[1:],
           (cfg(assign_iou=0.0),) + ok[1:], (cfg(assign_iou=1.0),) + ok[1:], (cfg(assign_iou=float('nan')),) + ok[1:],
           (cfg(out_h=(0, 2 ** 31 - 1), out_w=(0, 2 ** 31 - 1)),) + ok[1:],                              # a layer beyond size_t
           (cfg(out_h=(0, 2 ** 15), out_w=(0, 2 ** 15), class_num=2 ** 24),) + ok[1:4] + (2 ** 31 - 1,) + ok[5:]]   # n of them beyond size_t
    for args in bad:
        assert lib.yk_boxes_to_labels_f32(*args, None) == -10        # YK_ERR_ARG
        assert b'yk_boxes_to_labels_f32' in lib.yk_last_error()
    # a threshold outside (0, 1) is only refused where it is read
    best = engine.make_label_cfg(h)
    best.assign_iou = 7.0
    import torch
    if not torch.cuda.is_available():
        assert lib.yk_boxes_to_labels_f32(C.byref(best), boxes, 2, first, 2, labels, status, None) == -13      # YK_ERR_NO_DEVICE: every check passed
        assert lib.yk_boxes_to_labels_f32(*ok, None) == -13
    assert not labels.any() and status[0] == 5


def test_cli_knows_the_three_options_and_refuses_them_without_a_device():
    import torch
    from k210_yolo_framework_amd import engine, training
    a = training.parser().parse_args([])
    assert (a.labels, a.assign, a.assign_iou) == ('host', 'best', 0.213)
    a = training.parser().parse_args(['--labels', 'gpu', '--assign', 'multi', '--assign_iou', '0.3'])
    assert (a.labels, a.assign, a.assign_iou) == ('gpu', 'multi', 0.3)
    mk = (ROOT / 'Makefile').read_text()
    assert '$(if $(filter-out host,$(LABELS)),--labels $(LABELS))' in mk
    assert '$(if $(filter-out best,$(ASSIGN)),--assign $(ASSIGN) --assign_iou $(ASSIGNIOU))' in mk
    for value in ('0', '1', '-0.2', 'nan'):
        with pytest.raises(engine.YkError, match='--assign_iou '):
            training.cli(['--synthetic', '16', '--assign', 'multi', '--assign_iou', value, '--max_steps', '1'])
    if not torch.cuda.is_available():
        with pytest.raises(engine.YkError, match='--labels gpu'):
            training.cli(['--synthetic', '16', '--labels', 'gpu', '--max_steps', '1'])

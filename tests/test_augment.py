"""Training augmentation on the host (augment.py, Helper.data_augmenter): the per-(seed, epoch, row) parameter table, the inverse
maps, the host copy of the warp the GPU kernel is checked against, and the box transform."""
import numpy as np
import pytest

from k210_yolo_framework_amd import augment, pipeline, training
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS, letterbox_bilinear

HW = (224, 320)


def _h():
    return Helper(None, 20, VOC_ANCHORS, [list(HW)], [[7, 10], [14, 20]])


def _rot(theta_deg):
    r = np.radians(theta_deg)
    return np.array([[np.cos(r), -np.sin(r)], [np.sin(r), np.cos(r)]])


def test_parameter_table_is_deterministic_rank_independent_and_well_distributed():
    n = 30000
    tab = augment.param_table(3, 7, n)
    assert tab.shape == (n, 5)
    np.testing.assert_array_equal(tab, augment.param_table(3, 7, n))
    assert not np.array_equal(tab, augment.param_table(3, 8, n)) and not np.array_equal(tab, augment.param_table(4, 7, n))
    # a row's draws are those of the row, whichever rank / world size takes it
    order = pipeline.epoch_order(n, 3, 7, True)
    want = {int(i): tab[int(i)] for i in order[:64]}
    for world in (1, 2, 4):
        for rank in range(world):
            for rows in pipeline.rank_rows(order[:64], 16, rank, world):
                for i in rows:
                    np.testing.assert_array_equal(tab[i], want[int(i)])
    branch, flip, theta, fx, fy = augment.decode(tab)
    for b in range(3):
        assert abs((branch == b).mean() - 1 / 3) < 0.015
    assert abs(flip[branch == augment.FLIP].mean() - 0.5) < 0.02
    assert theta.min() >= -10 and theta.max() <= 10 and fx.min() >= -0.1 and fx.max() <= 0.1 and fy.min() >= -0.1 and fy.max() <= 0.1
    A, t = augment.forward_maps(tab, HW)
    assert np.abs(t[:, 0]).max() <= 0.1 * HW[1] and np.abs(t[:, 1]).max() <= 0.1 * HW[0]
    assert (t[branch != augment.TRANSLATE] == 0).all()
    rot = branch == augment.ROTATE
    ang = np.degrees(np.arctan2(A[rot, 1, 0], A[rot, 0, 0]))
    np.testing.assert_allclose(ang, theta[rot], atol=1e-9)
    assert np.allclose(np.linalg.det(A), [1.0 if b != augment.FLIP or not f else -1.0 for b, f in zip(branch, flip)])


def test_branch_edges():
    u = np.array([[0.0, 0.49, 0, 0, 0], [1 / 3 - 1e-12, 0.5, 0, 0, 0], [1 / 3, 0, 0, 0, 0], [0.9999999, 0, 1.0, 0.0, 1.0]])
    branch, flip, theta, fx, fy = augment.decode(u)
    assert branch.tolist() == [0, 0, 1, 2] and flip.tolist()[:2] == [True, False]
    assert theta[3] == 10.0 and fx[3] == -0.1 and np.isclose(fy[3], 0.1)


def test_identity_and_flip_matrices_are_exact_integers():
    A = np.stack([np.eye(2), np.diag([-1.0, 1.0])])
    M = augment.inverse_matrices(A, np.zeros((2, 2)), HW)
    np.testing.assert_array_equal(M[0], [[1, 0, 0], [0, 1, 0]])
    np.testing.assert_array_equal(M[1], [[-1, 0, HW[1] - 1], [0, 1, 0]])


def test_inverse_matrix_inverts_the_forward_map():
    A, t, M = augment.matrices(augment.param_table(0, 0, 64), HW)
    idx = np.array([[0.0, 0.0], [319.0, 223.0], [17.25, 101.5]])
    for a, tt, m in zip(A, t, M):
        p = idx + 0.5                                                            # pixel centres
        q = (p - (160, 112)) @ a.T + (160, 112) + tt                             # forward, continuous coordinates
        src = (q - 0.5) @ m[:, :2].T + m[:, 2]                                  # inverse, pixel-index coordinates
        np.testing.assert_allclose(src, idx, atol=1e-9)


def test_warp_identity_is_an_exact_copy_and_two_flips_give_back_the_original():
    img = np.random.default_rng(0).integers(0, 256, (*HW, 3), dtype=np.uint8)
    A = np.stack([np.eye(2), np.diag([-1.0, 1.0])])
    M = augment.inverse_matrices(A, np.zeros((2, 2)), HW)
    np.testing.assert_array_equal(augment.warp_u8(img, M[0]), img)
    once = augment.warp_u8(img, M[1])
    np.testing.assert_array_equal(once, img[:, ::-1])
    np.testing.assert_array_equal(augment.warp_u8(once, M[1]), img)


def test_warp_translation_by_whole_pixels_shifts_and_zero_fills():
    img = np.random.default_rng(1).integers(1, 256, (*HW, 3), dtype=np.uint8)
    M = augment.inverse_matrices(np.eye(2)[None], np.array([[5.0, -3.0]]), HW)[0]
    out = augment.warp_u8(img, M)
    np.testing.assert_array_equal(out[:HW[0] - 3, 5:], img[3:, :HW[1] - 5])
    assert (out[:, :5] == 0).all() and (out[HW[0] - 3:] == 0).all()


def test_flip_maps_box_x_to_one_minus_x():
    boxes = np.array([[1, 0.3, 0.4, 0.2, 0.1], [4, 0.75, 0.5, 0.1, 0.3]])
    out = augment.augment_boxes(boxes, np.diag([-1.0, 1.0]), np.zeros(2), HW)
    np.testing.assert_allclose(out[:, 1], 1 - boxes[:, 1], atol=1e-12)
    np.testing.assert_allclose(out[:, [0, 2, 3, 4]], boxes[:, [0, 2, 3, 4]], atol=1e-12)


@pytest.mark.parametrize('theta', [10.0, -7.5, 3.0])
def test_rotating_a_centred_square_gives_the_analytic_bounding_box(theta):
    s = 60.0
    boxes = np.array([[2, 0.5, 0.5, s / HW[1], s / HW[0]]])
    out = augment.augment_boxes(boxes, _rot(theta), np.zeros(2), HW)
    r = np.radians(theta)
    side = s * (abs(np.cos(r)) + abs(np.sin(r)))
    np.testing.assert_allclose(out[0], [2, 0.5, 0.5, side / HW[1], side / HW[0]], atol=1e-12)


def test_a_box_translated_out_of_the_image_is_dropped_and_classes_stay_with_their_boxes():
    """Deviation (a): utils.py:336 would pair classes [3, 7] with the boxes of 7 and 9 here."""
    boxes = np.array([[3, 0.97, 0.5, 0.04, 0.2], [7, 0.5, 0.5, 0.2, 0.2], [9, 0.3, 0.6, 0.1, 0.1]])
    u = np.array([[0.9, 0.0, 0.0, 1.0, 0.5]])                                    # translation, tx = +0.1 W, ty = 0
    A, t = augment.forward_maps(u, HW)
    assert np.isclose(t[0, 0], 32.0) and t[0, 1] == 0
    out = augment.augment_boxes(boxes, A[0], t[0], HW)
    assert out[:, 0].tolist() == [7, 9]
    np.testing.assert_allclose(out[:, 1], boxes[1:, 1] + t[0, 0] / HW[1], atol=1e-12)
    np.testing.assert_allclose(out[:, 2:], boxes[1:, 2:], atol=1e-12)
    # partly out: clipped to the image, centre / size recomputed
    part = augment.augment_boxes(np.array([[5, 0.9, 0.5, 0.2, 0.2]]), A[0], t[0], HW)
    x0, x1 = (0.8 * 320 + 32), 320.0
    np.testing.assert_allclose(part[0], [5, (x0 + x1) / 2 / 320, 0.5, (x1 - x0) / 320, 0.2], atol=1e-12)
    # a box that only touches the border (no positive-area overlap) goes too
    edge = augment.augment_boxes(np.array([[1, 0.95, 0.5, 0.1, 0.1]]), A[0], t[0], HW)
    assert edge.shape == (0, 5)


def test_pixels_and_boxes_agree():
    img = np.zeros((*HW, 3), np.uint8)
    img[60:140, 100:200] = (200, 120, 40)
    box = np.array([[0, 150 / 320, 100 / 224, 100 / 320, 80 / 224]])
    A, t = _rot(10.0)[None], np.array([[20.0, -12.0]])
    M = augment.inverse_matrices(A, t, HW)[0]
    out = augment.warp_u8(img, M)
    got = augment.augment_boxes(box, A[0], t[0], HW)[0]
    x0, x1 = (got[1] - got[3] / 2) * HW[1], (got[1] + got[3] / 2) * HW[1]
    y0, y1 = (got[2] - got[4] / 2) * HW[0], (got[2] + got[4] / 2) * HW[0]
    ys, xs = np.nonzero(out.max(-1))
    assert len(ys) > 8000                                                        # the rectangle is still there
    assert (xs + 0.5 >= x0 - 1).all() and (xs + 0.5 <= x1 + 1).all() and (ys + 0.5 >= y0 - 1).all() and (ys + 0.5 <= y1 + 1).all()
    # and the box is tight: the content reaches each side to within 1.5 px
    assert xs.min() + 0.5 - x0 < 1.5 and x1 - (xs.max() + 0.5) < 1.5 and ys.min() + 0.5 - y0 < 1.5 and y1 - (ys.max() + 0.5) < 1.5


def test_batch_box_transform_is_bit_identical_to_the_per_sample_function():
    rng = np.random.default_rng(4)
    tab = augment.param_table(11, 2, 40)
    A, t, _ = augment.matrices(tab, HW)
    boxes = []
    for k in range(40):
        n = int(rng.integers(0, 5))
        b = np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.0, 1.0, (n, 2)), rng.uniform(0.01, 0.5, (n, 2))], 1)
        if n:
            b[0] = [k % 20, 0.996, 0.996, 0.004, 0.004]                          # leaves the image under most translations
        boxes.append(b)
    got = augment.augment_boxes_batch(boxes, A, t, HW)
    assert len(got) == 40
    dropped = 0
    for k in range(40):
        want = augment.augment_boxes(boxes[k], A[k], t[k], HW)
        assert got[k].shape == want.shape
        assert got[k].tobytes() == want.tobytes()
        dropped += len(boxes[k]) - len(want)
    assert dropped > 0                                                           # the drop path is exercised
    assert [b.shape for b in augment.augment_boxes_batch([np.zeros((0, 5))] * 3, A[:3], t[:3], HW)] == [(0, 5)] * 3


def test_every_kept_box_fits_the_label_encoder():
    rng = np.random.default_rng(8)
    h = _h()
    tab = augment.param_table(1, 0, 500)
    A, t, _ = augment.matrices(tab, HW)
    boxes = [np.concatenate([rng.integers(0, 20, (3, 1)).astype(float), rng.uniform(0.0, 1.0, (3, 2)), rng.uniform(0.01, 0.9, (3, 2))], 1)
             for _ in range(500)]
    out = augment.augment_boxes_batch(boxes, A, t, HW)
    allb = np.concatenate(out)
    assert (allb[:, 1:3] >= 0).all() and (allb[:, 1:3] < 1).all() and (allb[:, 3:5] > 0).all() and (allb[:, 3:5] <= 1).all()
    h.batch_box_to_label(out)


def test_process_img_with_aug_is_letterbox_then_data_augmenter():
    h = _h()
    rng = np.random.default_rng(3)
    tab = augment.param_table(5, 1, 6)
    tab[:, 0] = [0.1, 0.1, 0.5, 0.5, 0.9, 0.9]                                  # every branch twice
    tab[:2, 1] = [0.2, 0.7]                                                      # flip and no flip
    for k, src_hw in enumerate([(375, 500), (224, 320), (333, 500), (100, 100), (240, 320), (375, 500)]):
        img = rng.integers(0, 256, (*src_hw, 3), dtype=np.uint8)
        boxes = np.array([[2, 0.5, 0.5, 0.3, 0.4], [6, 0.1, 0.9, 0.15, 0.15]])
        got, gb = h._process_img(img, boxes.copy(), is_training=True, is_resize=True, aug=tab[k])
        lb, lbox = h._process_img(img, boxes.copy(), is_training=False, is_resize=True)
        s, tr = h.letterbox_params(src_hw)
        letterboxed = letterbox_bilinear(img, HW, float(s[0]), tr)
        want, wb = h.data_augmenter(letterboxed, lbox, tab[k])
        np.testing.assert_array_equal(got, want / np.max(want))
        np.testing.assert_array_equal(gb, wb)
        A, t, M = augment.matrices(tab[k:k + 1], HW)
        np.testing.assert_array_equal(want, augment.warp_u8(letterboxed, M[0]))
        if k == 1:
            assert np.array_equal(want, letterboxed)                             # no-flip: unchanged
        if k == 0:
            assert np.array_equal(want, letterboxed[:, ::-1])


def test_process_img_training_without_aug_says_to_pass_it():
    h = _h()
    with pytest.raises(NotImplementedError, match='aug'):
        h._process_img(np.zeros((224, 320, 3), np.uint8), None, is_training=True, is_resize=True)


def test_host_generator_augments_per_epoch_and_row():
    h = _h()
    items = training.synthetic_list(12, HW, 20, 2)
    order = np.arange(12)

    class _Fixed:
        def permutation(self, n):
            return order
    plain = list(training.batches(h, items, 4, _Fixed(), shuffle=True))
    a = list(training.batches(h, items, 4, _Fixed(), shuffle=True, augment=(3, 0)))
    b = list(training.batches(h, items, 4, _Fixed(), shuffle=True, augment=(3, 0)))
    c = list(training.batches(h, items, 4, _Fixed(), shuffle=True, augment=(3, 1)))
    for (ax, ay), (bx, by) in zip(a, b):
        np.testing.assert_array_equal(ax, bx)
        for u, v in zip(ay, by):
            np.testing.assert_array_equal(u, v)
    assert any(not np.array_equal(ax, px) for (ax, _), (px, _) in zip(a, plain))
    assert any(not np.array_equal(ax, cx) for (ax, _), (cx, _) in zip(a, c))
    # a row's augmentation does not depend on the batch it lands in
    order = np.arange(12)[::-1].copy()
    rev = list(training.batches(h, items, 4, _Fixed(), shuffle=True, augment=(3, 0)))
    np.testing.assert_array_equal(rev[0][0][3], a[2][0][0])                      # row 8


def test_training_dataset_is_augmented_per_pass_and_row():
    h = _h()
    items = training.synthetic_list(10, HW, 20, 4)
    h.train_list, h.test_list = items[2:], items[:2]
    h.train_total_data, h.test_total_data = 8, 2
    h.set_dataset(4, 6, is_training=True)
    x1, y1 = h.get_iter(True)
    assert x1.shape == (4, 224, 320, 3) and np.isfinite(x1).all() and [y.shape for y in y1] == [(4, 7, 10, 3, 25), (4, 14, 20, 3, 25)]
    h2 = _h()
    h2.train_list, h2.test_list, h2.train_total_data, h2.test_total_data = items[2:], items[:2], 8, 2
    h2.set_dataset(4, 6, is_training=True)
    np.testing.assert_array_equal(h2.get_iter(True)[0], x1)                      # keyed by (rand_seed, pass, row): reproducible
    # the first batch of pass 0 is the host generator's epoch 0 on the same order
    order = np.random.default_rng(6).permutation(8)

    class _Fixed:
        def permutation(self, n):
            return order
    want = next(training.batches(h, items[2:], 4, _Fixed(), shuffle=True, augment=(6, 0)))
    np.testing.assert_array_equal(x1, want[0])
    # small lists (fewer rows than a batch) repeat before batching and still augment
    h3 = _h()
    h3.train_list, h3.test_list, h3.train_total_data, h3.test_total_data = items[:3], items[3:5], 3, 2
    h3.set_dataset(4, 1, is_training=True)
    for _ in range(3):
        assert h3.get_iter(True)[0].shape == (4, 224, 320, 3)

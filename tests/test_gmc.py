"""gmc.py, the rule of camera-motion compensation, on generated pictures whose motion is known; and what the motion does in track.Tracker."""
import numpy as np
import pytest

from k210_yolo_framework_amd import gmc
from k210_yolo_framework_amd import track as tk
from tests.gmc_cases import CONTENT, view

F = np.float32


@pytest.mark.parametrize('name', list(CONTENT))
def test_the_rule_on_known_motion(name):
    frames, want = CONTENT[name]
    e = gmc.Estimator()
    first, got = e.update(frames[0]), e.update(frames[1])
    assert first.tolist() == [0, 0] and got.dtype == F and len(e.blocks) == 18
    if want is not None:
        assert got.tolist() == list(want)
    if name == 'beyond':                                  # 40 px is past the +-32 the search reaches: whatever wins, it is not the shift
        assert got.tolist() != [40, 0] and np.array_equal(got, gmc.motion_of(e.blocks))
    if name == 'flat':
        assert not e.blocks[:, 3].any() and (e.blocks[:, :3] == 0).all()        # every candidate ties at SAD 0: (0, 0) wins, nothing kept
    if name == 'period_4_ties':
        assert (e.blocks[:, 2] == 0).all() and (e.blocks[:, :2] == (0, -2)).all()
    if name == 'a_third_moves_away':
        assert (e.blocks[:, 1] == 4).sum() == 6 and (e.blocks[:, 1] == -2).sum() == 12


def test_shrink_grey_rounding_partial_cells_and_the_lower_median():
    img = np.zeros((9, 7, 3), np.uint8)
    img[:4, :4] = (255, 255, 255)
    img[0, 0] = (1, 2, 3)                                 # g = (77 + 300 + 87 + 128) >> 8 = 2
    img[4:8, :4] = (0, 1, 0)                              # g = 278 >> 8 = 1 everywhere: the cell is 1
    small = gmc.shrink(img, 4)
    assert small.shape == (2, 1) and small[:, 0].tolist() == [(15 * 255 + 2 + 8) // 16, 1]
    blocks = np.asarray([[1, 5, 0, 1], [2, -3, 0, 1], [3, 7, 0, 1], [4, 0, 0, 1], [9, 9, 0, 0]], np.int32)
    assert gmc.motion_of(blocks, 4, 4).tolist() == [0, 8] and gmc.motion_of(blocks, 4, 5).tolist() == [0, 0]


def test_a_first_frame_and_a_change_of_size_give_no_motion():
    e = gmc.Estimator()
    got = [e.update(p).tolist() for p in (view(), view(8, 0), view(16, 0, h=252), view(24, 0, h=252))]
    assert got == [[0, 0], [8, 0], [0, 0], [8, 0]]


@pytest.mark.parametrize('kw, name', [(dict(block=10), 'gmc_block'), (dict(range=0), 'gmc_range'), (dict(scale=0), 'gmc_scale'),
                                      (dict(step=0), 'gmc_step'), (dict(texture=-1), 'gmc_texture')])
def test_bad_options_are_refused_by_name(kw, name):
    with pytest.raises(ValueError, match=name):
        gmc.check(**kw)


def pan_rows(t):
    """Three static objects seen by a camera that pans 40 px to and fro: every box jumps by +-40 on alternating frames (2, 4, 6)."""
    off = 40 * ((t // 2) % 2)
    return np.asarray([[50, 100 + off + 120 * k, 110, 140 + off + 120 * k, 0.9, k] for k in range(3)], F)


@pytest.mark.parametrize('assign', tk.ASSIGNS)
def test_a_panning_camera_keeps_every_id_with_the_motion_and_loses_them_without(assign):
    with_motion, without = tk.Tracker(20, gmc=True, assign=assign), tk.Tracker(20, assign=assign)
    ids, plain = [], []
    for t in range(8):
        motion = (0, 0) if t == 0 or t % 2 else (40 if (t // 2) % 2 else -40, 0)
        rows, i = with_motion.update(pan_rows(t), motion=motion)
        ids.append(i.tolist())
        plain.append(without.update(pan_rows(t))[1].tolist())
        assert np.array_equal(rows[:, :4], pan_rows(t)[:, :4])       # static objects, exact motion: the filter never sees a residual
    assert ids == [[1, 2, 3]] * 8
    assert plain[0] == [1, 2, 3] and plain[3] == [4, 5, 6]                 # a 40-px jump of a 40-px box: IoU 0, new tracks where they landed
    with pytest.raises(ValueError, match='gmc'):
        without.update(pan_rows(0), motion=(1, 1))

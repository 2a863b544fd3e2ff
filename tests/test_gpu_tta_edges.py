"""yk_fuse_views (csrc/yk_tta.hip) on the inputs of tests/tta_edge_cases.py, which tests/test_tta_edge_cases.py vets on the CPU: classes of more
candidates than views * max_out (the guards `pos < nmax` and `n = min(n, nmax)` of the ballot compaction, never taken by decode-shaped rows),
rows inside a frame's count that are no candidates, more clusters than max_out with equal final scores on both sides of the cut, and
mw = 0.0 / -0.0 / the smallest negative float32 at the mirror switch.

As in tests/test_gpu_tta.py: rows are compared with tta.fuse as int32 patterns, rows beyond a frame's count hold NaN, d_out is filled with a
sentinel first and every row beyond a picture's count must still hold it.  Every case runs as one picture of its own and as the middle one of
three, between two seeded decode-shaped pictures whose whole output rows (sentinels included) must be what the two give in a call without it:
a write that leaves the case's LDS or its slice of the staging buffer lands in a neighbour."""
import numpy as np
import pytest

from k210_yolo_framework_amd import tta
from tests import tta_edge_cases as te
from tests.test_gpu_tta import SENTINEL, _bits, _Device, _reference

pytestmark = pytest.mark.gpu
F = np.float32
CASES = te.cases()


def _fused(cases):
    """One yk_fuse_views call over `cases`, checked against tta.fuse of each -> (the device buffers, the rule's rows)."""
    import torch
    from k210_yolo_framework_amd import engine
    d = _Device(cases)
    engine.fuse_views(d.dets, d.counts, d.xforms, d.views, d.class_num, d.max_out, d.thresh, out=d.out, out_counts=d.out_counts)
    torch.cuda.synchronize()
    want = _reference(cases)
    d.check(want, cases[0].name)
    return d, want


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_edge_case_as_one_picture_equals_the_rule_and_the_answer_by_hand(case):
    d, (want,) = _fused([case])
    assert not (want == SENTINEL).any()
    if case.want is not None:
        assert np.array_equal(want.view(np.int32), np.asarray(case.want, F).reshape(-1, 6).view(np.int32))
    if case.name in te.OVERFULL:
        c, total = te.OVERFULL[case.name]
        assert total > d.views * d.max_out
        alone = tta.fuse(te.without_class(case, c).rows, case.xforms, case.class_num, case.max_out, case.thresh)[0]
        assert np.array_equal(want[want[:, 5] != c].view(np.int32), alone.view(np.int32))          # the other classes do not feel it


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_edge_case_between_two_pictures_leaves_them_what_they_are_alone(case):
    import torch
    left, right = te.neighbours(case)
    pair, _ = _fused([left, right])
    trio, want = _fused([left, case, right])
    assert all(len(w) > 0 for w in (want[0], want[2]))
    for at, alone in ((0, 0), (2, 1)):
        assert torch.equal(_bits(trio.out[at]), _bits(pair.out[alone])) and trio.out_counts[at].item() == pair.out_counts[alone].item(), (case.name, at)

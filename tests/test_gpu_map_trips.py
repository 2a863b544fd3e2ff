"""The evaluator kernels of csrc/yk_map.hip past one grid of workgroups: match_kernel and coco_match_kernel with more (image, class) groups than
65536 workgroups x 4 waves, confusion_kernel and append_padded_kernel with more images than 65536 workgroups - so that a workgroup goes round
its grid-stride loop a second time - and both matchers on equal IoUs whose boxes lie in different 64-box chunks of one group.  Cases and
references: tests/grid_trip_cases.py (checked on their own by tests/test_grid_trip_cases.py, which also shows that the images without rows and
boxes, left out of the references here, change none of their outputs).  The comparisons are those of tests/test_gpu_map_eval.py,
tests/test_gpu_coco_eval.py and tests/test_gpu_oppoint.py: integers and flags exactly, AP within their 1e-12."""
import numpy as np
import pytest

from tests import grid_trip_cases as gt

pytestmark = pytest.mark.gpu

MAP_MAX_GRID = gt.MAP_MAX_GRID                       # csrc/yk_map.hip:33, grid_for: `if (g > 65536) g = 65536`
MAP_GROUPS = gt.MAP_GROUPS                           # x MAP_WAVES (csrc/yk_map.hip:27) groups per trip of the matchers


def _evaluator(c):
    """A MapEvaluator holding every image of the case, the empty ones too."""
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    from tests.test_gpu_map_eval import pack
    dets, gts, diff = gt.spread(c)
    ev = MapEvaluator(c['class_num'])
    rows, off = pack(dets)
    ev.add(rows, off, gts, diff)
    assert ev.n_img == c['n_img'] and ev.n_rows == sum(len(d) for d in c['dets'])
    return ev


# ---- the matchers past MAP_GROUPS groups ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def many_groups():
    c = gt.match_case()
    assert c['n_img'] * c['class_num'] > MAP_GROUPS                                                # a second trip of the group loop
    return c, _evaluator(c)


def test_voc_matcher_past_one_grid_of_groups(many_groups):
    from tests.test_gpu_map_eval import compare
    c, ev = many_groups
    got = ev.result()
    ref = compare(got, c['dets'], c['gts'], c['class_num'], difficult=c['diff'])
    assert (ref['tp'] >= 4).all() and (ref['fp'] >= 4).all()                                      # every class, in every image with rows


def test_coco_matcher_past_one_grid_of_groups(many_groups):
    from tests.test_gpu_coco_eval import compare
    c, ev = many_groups
    ref = gt.match_reference('coco')
    compare(ev.coco_result(), ref)
    assert (ref['n_det'] >= 16).all()


# ---- one workgroup per image, more images than workgroups ----------------------------------------------------------------------------
def test_confusion_past_one_grid_of_images():
    """Workgroup k matches image k, then image 65536 + k out of the same LDS: other numbers of rows and boxes, in one pair more of both."""
    from tests.test_gpu_oppoint import same_confusion
    c = gt.confusion_case()
    assert c['n_img'] > MAP_MAX_GRID                                                               # a second trip of the image loop
    got = _evaluator(c).confusion(c['conf'])
    same_confusion(got, gt.confusion_reference())
    assert got['match'].max() >= 0 and (got['match'] == -1).any()


def test_padded_append_past_one_grid_of_images_and_past_one_stride_of_the_count_sum():
    """65540 images, cap 3, counts from {-1, 0, 1, 3, 5}: every row and image index against a cumsum of the clamped counts; then one row
    fewer than there are - nothing past it may be written."""
    import torch
    from k210_yolo_framework_amd import engine
    c = gt.append_case()
    B, cap, base = gt.APPEND_BATCH, gt.APPEND_CAP, gt.APPEND_BASE
    assert B > MAP_MAX_GRID and B > gt.APPEND_BLOCK                                                # csrc/yk_map.hip:89 and :93
    total, have, fill = len(c['rows']), 5, -7
    d, cnt = torch.from_numpy(np.array(c['dets'])).cuda(), torch.from_numpy(np.array(c['counts'])).cuda()
    for n_new in (total, total - 1):
        capacity = have + total + 4
        rows = torch.full((capacity, 6), float(fill), dtype=torch.float32, device='cuda')
        img = torch.full((capacity,), fill, dtype=torch.int32, device='cuda')
        engine.call('yk_map_append_padded', d, cnt, B, cap, base, n_new, rows, img, have, capacity, engine._stream())
        torch.cuda.synchronize()
        r, i = rows.cpu().numpy(), img.cpu().numpy()
        bad = np.nonzero((r[have:have + n_new] != c['rows'][:n_new]).any(1) | (i[have:have + n_new] != c['img'][:n_new]))[0]
        assert len(bad) == 0, (n_new, len(bad), bad[:8], i[have + bad[:8]], c['img'][bad[:8]])
        assert (r[:have] == fill).all() and (i[:have] == fill).all()                               # sentinels in front
        assert (r[have + n_new:] == fill).all() and (i[have + n_new:] == fill).all()               # and behind: nothing past n_new


# ---- equal IoU across 64-box chunks ----------------------------------------------------------------------------------------------------
def test_voc_matcher_breaks_ties_across_chunks_toward_the_lower_box():
    from tests.test_gpu_map_eval import check
    c = gt.tie_case()
    got = check(c['dets'], c['gts'], 1, difficult=c['diff'])
    assert tuple(got['flags'][:12]) == gt.TIE_VOC_FLAGS and (got['flags'][12:] == 1).all()


def test_coco_matcher_breaks_ties_across_chunks_toward_the_higher_box():
    from k210_yolo_framework_amd import coco_eval
    from tests.test_gpu_coco_eval import compare, evaluator
    c = dict(gt.tie_case())
    got = evaluator(c).coco_result()
    compare(got, coco_eval.evaluate(c['dets'], c['gts'], 1, difficult=c['diff']))
    assert tuple(got['flags'][0, 0, :12]) == gt.TIE_COCO_FLAGS

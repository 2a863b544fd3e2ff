"""The case builders of tests/region_cases.py and the CPU oracle on them, checked on their own (no GPU): each family must really sit on the edge it
is named after, or tests/test_gpu_region_edges.py would compare the kernels with the oracle somewhere harmless."""
import numpy as np
import pytest

import oracle
from tests import region_cases as rc

F = np.float32
TINY = np.finfo(F).tiny


def _subnormal(a):
    return (a != 0) & (np.abs(a) < TINY)


def _candidates(case):
    """Non-zero probabilities per (image, class) before any suppression (nms = 1e9: no IoU exceeds it)."""
    C = rc.dims(case)[4]
    return [tuple(int(n) for n in (p[:, :C] != 0).sum(0)) for _, _, p in rc.reference(case, nms=1e9)]


def _survivors(case):
    C = rc.dims(case)[4]
    return [tuple(int(n) for n in (p[:, :C] != 0).sum(0)) for _, _, p in rc.reference(case)]


def test_every_case_is_finite_and_the_oracle_makes_no_nan():
    cases = [rc.expf_sweep(), rc.softmax_tail(), rc.lds_boundary(), rc.saturating()] + rc.image_sizes() + rc.ties() + rc.small()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.x.dtype == F and np.isfinite(c.x).all(), c.name
        for out, boxes, probs in rc.reference(c):
            assert not (np.isnan(out).any() or np.isnan(boxes).any() or np.isnan(probs).any()), c.name


def test_expf_sweep_sits_on_the_limits():
    c = rc.expf_sweep()
    B, W, H, A, C = rc.dims(c)
    assert (B, W, H, A, C) == (2, 52, 52, 3, 1) and c.net_wh == c.image_wh == (320, 224) and (c.anchor == 1).all() and c.thr == 2.0
    pts = rc.expf_points()
    assert pts.size == 17 * len(rc.EXPF_CENTRES) == len(set(pts.view(np.uint32).tolist()))
    over, under = F(rc.EXPF_OVERFLOW), F(rc.EXPF_UNDERFLOW)
    for edge in (over, under):                                           # the thresholds themselves and the floats on either side of them
        assert {np.nextafter(edge, F(-np.inf)), edge, np.nextafter(edge, F(np.inf))} <= set(pts.tolist())
    for b, (out, boxes, probs) in enumerate(rc.reference(c)):
        tw, th = c.x[b, :, 2].ravel(), c.x[b, :, 3].ravel()
        assert set(pts.view(np.uint32).tolist()) <= set(tw.view(np.uint32).tolist())
        np.testing.assert_array_equal(th, -tw[::-1])
        for t in (c.x[b, :, 0], c.x[b, :, 1], c.x[b, :, 4]):
            assert set(t.ravel().view(np.uint32).tolist()) in (set(tw.view(np.uint32).tolist()), set(th.view(np.uint32).tolist()))
        e = boxes[:, 2]
        assert _subnormal(e).sum() >= 100 and (e == 0).sum() >= 100 and np.isinf(e).sum() >= 100      # here: 692/222/259 and 720/249/241
        assert _subnormal(out).sum() >= 100                               # logistic's 1 / (1 + inf-sized e) quotients: subnormal objectness
        assert (probs[:, :C] == 0).all()                                  # thr = 2: NMS has nothing to do
        # the oracle's (glibc's) expf against float64: at most 1 ulp (here: max 1 ulp, 6 and 3 of 8112 values differ)
        rc.check_expf_f64(boxes[:, 2], tw, f'expf(tw) image {b}')
        rc.check_expf_f64(boxes[:, 3], th, f'expf(th) image {b}')
        assert (e[tw > over] == np.inf).all() and np.isfinite(e[tw <= over]).all()
        assert (e[tw < under] == 0).all() and (e[tw >= under] > 0).all()


def test_softmax_tail_makes_subnormal_quotients_and_products():
    c = rc.softmax_tail()
    B, W, H, A, C = rc.dims(c)
    assert (W, H, A, C, c.thr) == (52, 52, 3, 3, 0.0)
    (out, boxes, probs), = rc.reference(c)
    cls = out.reshape(A, 5 + C, H, W)[:, 5:]
    assert _subnormal(cls[:, 1]).all() and (cls[:, 2] == 0).all() and (cls[:, 0] == 1).all()        # here: all 8112 subnormal
    assert _subnormal(probs[:, 1]).sum() > 0                                                          # here: 1212 survive NMS
    assert (probs[:, 2] == 0).all()
    (cand,) = _candidates(c)
    assert cand[0] == A * H * W and cand[1] > rc.YK_NMS_MAXC and cand[2] == 0       # subnormal candidates go down the global-memory path


# tolerances of the oracle's fp32 un-letterbox against float64: 8 x the worst error seen over these five cases when this was written,
# 1.95e-7 absolute on x / y (values up to 1.52) and 1.98e-7 relative on w / h
XY_ATOL = 8 * 1.95e-7
WH_RTOL = 8 * 1.98e-7


def test_image_sizes_reach_both_branches_and_truncate():
    cases = rc.image_sizes()
    assert [(c.net_wh, c.image_wh) for c in cases] == [(n, i) for n, i, _ in rc.IMAGE_SIZES]
    seen = set()
    for c, (_, _, want) in zip(cases, rc.IMAGE_SIZES):
        new_w, new_h, branch, truncated = rc.letterbox_dims(c.net_wh, c.image_wh)
        assert (new_w, new_h) == want, c.name
        seen.add((branch, truncated, new_w < c.net_wh[0], new_h < c.net_wh[1]))
    assert ('fit_h', True, True, False) in seen       # the else branch with a truncated new_w < net_w
    assert ('fit_w', True, False, True) in seen       # the first branch with a truncated new_h
    assert ('fit_w', False, False, True) in seen      # and an exact division


@pytest.mark.parametrize('i', range(len(rc.IMAGE_SIZES)))
def test_image_sizes_oracle_against_float64(i):
    """The reference hard-codes 320 x 224, so the oracle's image_wh has no upstream to be compared with: float64 numpy stands in."""
    c = rc.image_sizes()[i]
    B, W, H, A, C = rc.dims(c)
    assert (W, H, A, C) == (10, 7, 3, 2)
    want = rc.unletterbox_f64(c)
    for b, (_, boxes, probs) in enumerate(rc.reference(c)):
        err_xy = np.abs(boxes[:, :2] - want[b, :, :2]).max()
        err_wh = (np.abs(boxes[:, 2:] - want[b, :, 2:]) / want[b, :, 2:]).max()
        print(c.name, b, 'xy abs', err_xy, 'wh rel', err_wh)
        assert err_xy <= XY_ATOL and err_wh <= WH_RTOL, (c.name, b, err_xy, err_wh)
        assert (probs[:, :C] != 0).sum() > 20                  # NMS has work to do on these boxes


def test_ties_have_one_probability():
    small, large = rc.ties()
    for c, nb in ((small, 210), (large, 8112)):
        B, W, H, A, C = rc.dims(c)
        assert A * H * W == nb and C == 2 and c.net_wh == (416, 416)
        (_, _, p), = rc.reference(c, nms=1e9)
        assert len(np.unique(p[:, :C][p[:, :C] != 0])) == 1     # any disagreement with the oracle is a tie-break disagreement
        assert _candidates(c) == [(nb, nb)]
    assert 210 <= rc.YK_NMS_MAXC < 8112                         # one grid per NMS path
    assert _survivors(small) == [(70, 70)] and _survivors(large) == [(117, 117)]


def test_lds_boundary_candidate_counts():
    c = rc.lds_boundary()
    M = rc.YK_NMS_MAXC
    assert rc.dims(c) == (3, 52, 52, 3, 2)
    assert _candidates(c) == [(M - 1, M + 1), (M, M + 1), (M + 1, M + 1)]
    for s in _survivors(c):
        assert min(s) > 1000                                    # most boxes survive: the greedy loop runs long on both paths
    for b in range(3):                                          # the "on" boxes are scattered over the whole index range
        on = np.flatnonzero(c.x[b, :, 4].ravel() > 0)
        assert on.size == M + 1 and on[0] < 64 and on[-1] > 8112 - 64


def test_small_cases_have_empty_and_single_candidate_images():
    cases = rc.small()
    assert [rc.dims(c)[1:] + (c.thr,) for c in cases] == [s for s in rc.SMALL]
    assert rc.dims(cases[-1])[3] == rc.YK_MAX_ANCHORS
    for c in cases:
        cand = _candidates(c)
        assert set(cand[0]) == {0} and set(cand[1]) == {1} and max(cand[2]) >= 1, (c.name, cand)
    assert sum(rc.dims(c)[1] * rc.dims(c)[2] * rc.dims(c)[3] < 64 for c in cases) == 2


def test_saturating_boxes_and_their_draw_casts():
    c = rc.saturating()
    B, W, H, A, C = rc.dims(c)
    assert (W, H, A, C, c.thr) == (5, 3, 2, 2, 0.3)
    (out, boxes, probs), = rc.reference(c)
    assert np.isinf(boxes).sum() == 7 and (boxes[:, 3] == 0).sum() == 5 and not np.isnan(boxes).any()
    dets = oracle.region_draw(boxes, probs, c.thr)
    assert len(dets) >= 20
    drawn = np.flatnonzero(probs[:, :C].max(1) > c.thr)
    wide = np.isinf(boxes[drawn, 2])
    assert wide.sum() >= 5
    assert (dets[wide, 0] == 0).all() and (dets[wide, 2] == 0).all()       # -inf and +inf both convert to 0
    assert (dets[~wide, 2] != 0).all()


def test_to_u32_outside_the_int64_range_is_zero():
    """The draw casts on their own: NaN, +-inf and +-2^63 give 0, as cvttss2si's integer indefinite truncates to; inside the range it wraps."""
    probs = np.array([[0.9, 0.9]], F)
    inside = F(2.0 ** 40 + 2.0 ** 20)
    for w, x1, x2 in ((np.inf, 0, 0), (2.0 ** 63, 0, 0), (2.0 ** 65, 0, 0), (inside, (-int(inside)) & 0xFFFFFFFF, int(inside) & 0xFFFFFFFF)):
        # centre 0 in a 2 x 2 image: x1 = 0 * 2 - w * 2 / 2 = -w and x2 = +w, exactly
        d = oracle.region_draw(np.array([[0, 0.5, w, 0.5]], F), probs, 0.5, (2, 2))
        assert (d[0, 0], d[0, 2]) == (x1, x2), (w, d)
    assert int(inside) & 0xFFFFFFFF == 2 ** 20
    d = oracle.region_draw(np.array([[np.nan, 0.5, 0.5, 0.5]], F), probs, 0.5, (2, 2))
    assert d[0, 0] == 0 and d[0, 2] == 0

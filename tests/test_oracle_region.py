"""Pin oracle/region_layer_ref.c against the reference's own region_layer.c.

(a) committed golden vectors produced by the compiled reference (tests/golden/make_region_golden.py)
(b) stored outputs of the compiled reference on seeded inputs of several shapes (tests/golden/make_region_live_golden.py),
    re-checked against the live oracle/_ref build when it is present
"""
import numpy as np
import pytest

import oracle


def _cases(golden_dir):
    g = np.load(golden_dir / 'region_golden.npz')
    names = sorted({k.split('/')[0] for k in g.files if '/' in k})
    return g, names


def test_golden_cases_bit_exact(golden_dir):
    g, names = _cases(golden_dir)
    assert len(names) >= 6
    for n in names:
        W, H, A, C, li, nw, nh = g[n + '/meta']
        thr, nms = g[n + '/thr']
        out, boxes, probs = oracle.region_run(g[n + '/input'], g['anchors'][li], W, H, A, C, thr, nms, (nw, nh))
        # same glibc expf on the generating and the checking side -> bit-exact expected
        np.testing.assert_array_equal(out, g[n + '/output'], err_msg=n)
        np.testing.assert_array_equal(boxes, g[n + '/boxes'], err_msg=n)
        np.testing.assert_array_equal(probs, g[n + '/probs'], err_msg=n)
        dets = oracle.region_draw(boxes, probs, thr)
        np.testing.assert_array_equal(dets, g[n + '/dets'], err_msg=n)


@pytest.mark.parametrize('W,H,A,C,thr,nms,net', [
    (10, 7, 3, 20, 0.6, 0.3, (320, 224)), (20, 14, 3, 20, 0.1, 0.3, (320, 224)),
    (13, 13, 3, 20, 0.2, 0.5, (416, 416)), (5, 3, 5, 2, 0.05, 0.2, (160, 224)), (1, 1, 1, 1, 0.0, 0.5, (320, 224)),
    (20, 14, 3, 1, 0.3, 0.3, (320, 224)),
])
def test_live_reference_bit_exact(W, H, A, C, thr, nms, net, golden_dir):
    """The reference's outputs on these seeded inputs are stored (tests/golden/make_region_live_golden.py); where oracle/_ref is built,
    the live reference must still produce them."""
    g = np.load(golden_dir / 'region_live_golden.npz')
    key = f'{W}x{H}x{A}x{C}_{thr}_{nms}_{net[0]}x{net[1]}'
    anchor = g[key + '/anchor']
    for scale in (6.0, 2.0):
        k = f'{key}/s{scale:g}'
        x = g[k + '/input']
        ro, rb, rp, rd = g[k + '/output'], g[k + '/boxes'], g[k + '/probs'], g[k + '/dets']
        if oracle.have_ref():
            for live, stored in zip(oracle.ref_region_run(x, anchor, W, H, A, C, thr, nms, net), (ro, rb, rp, rd)):
                np.testing.assert_array_equal(live, stored)
        out, boxes, probs = oracle.region_run(x, anchor, W, H, A, C, thr, nms, net)
        np.testing.assert_array_equal(out, ro)
        np.testing.assert_array_equal(boxes, rb)
        np.testing.assert_array_equal(probs, rp)
        np.testing.assert_array_equal(oracle.region_draw(boxes, probs, thr), rd)


def test_live_reference_saturating_boxes(golden_dir):
    """Infinite widths and zero heights (tests/region_cases.py saturating()): the stored outputs are the reference's own, draw casts of +-inf
    included, and pin the oracle's to_u32 on them.  (The key format above does not fit: the input is built, not drawn at a scale.)"""
    from tests import region_cases
    g = np.load(golden_dir / 'region_live_golden.npz')
    c = region_cases.saturating()
    _, W, H, A, C = region_cases.dims(c)
    x, anchor = g['saturating/input'], g['saturating/anchor']
    np.testing.assert_array_equal(x, c.x[0])                  # the fixture was made from the builder as it is now
    np.testing.assert_array_equal(anchor, c.anchor)
    stored = tuple(g[f'saturating/{k}'] for k in ('output', 'boxes', 'probs', 'dets'))
    assert np.isinf(stored[1]).sum() == 7 and not np.isnan(stored[1]).any()
    if oracle.have_ref():
        for live, want in zip(oracle.ref_region_run(x, anchor, W, H, A, C, c.thr, c.nms, c.net_wh), stored):
            np.testing.assert_array_equal(live, want)
    out, boxes, probs = oracle.region_run(x, anchor, W, H, A, C, c.thr, c.nms, c.net_wh)
    for got, want in zip((out, boxes, probs, oracle.region_draw(boxes, probs, c.thr)), stored):
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_negative_coordinate_cast_is_defined():
    # region_layer.c:397-400 converts possibly-negative floats to uint32 (UB); the restatement and the
    # new ABI define it as (uint32_t)(int64_t)x.  A box hanging over the left/top edge exercises it.
    boxes = np.array([[0.01, 0.01, 0.5, 0.5]], np.float32)
    probs = np.array([[0.9, 0.9]], np.float32)
    d = oracle.region_draw(boxes, probs, 0.5)
    x1 = np.float32(0.01) * np.float32(320) - (np.float32(0.5) * np.float32(320) / np.float32(2))
    assert d[0, 0] == np.uint32(np.int64(x1) & 0xFFFFFFFF)
    assert d[0, 0] > 4_000_000_000

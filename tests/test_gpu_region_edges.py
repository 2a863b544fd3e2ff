"""GPU: the C-mode region layer (csrc/yk_region.hip, yk_expf_glibc of csrc/yk_common.h, csrc/yk_nms.h) on the cases of tests/region_cases.py, where
random logits in (-6, 6) never take it: expf at its overflow / underflow thresholds and in the subnormal band, subnormal softmax quotients, image
sizes on both letterbox branches, exact ties on both NMS paths, the 2048-candidate LDS limit from either side, grids below one wavefront,
arbitrary input strides, and the drop-in ABI on infinite boxes and on its -5 failure.

Unless said otherwise every comparison is on the BIT PATTERNS of output, boxes and probs against the CPU oracle (oracle.region_run) per image;
tests/test_region_cases.py checks, without a GPU, that each case sits where it claims to and holds the oracle itself to float64."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import region_cases as rc

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope='module')
def hip():
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    return engine.lib()


def _run(case, layout='chw', want_output=True):
    """engine.region_batched on the whole batch of the case -> numpy (output | None, boxes, probs)."""
    import torch
    from k210_yolo_framework_amd import engine
    B, W, H, A, Cn = rc.dims(case)
    xin = torch.from_numpy(rc.layout(case.x, layout)).cuda()
    out, boxes, probs = engine.region_batched(xin, W, H, A, Cn, case.anchor, case.thr, case.nms, case.net_wh, case.image_wh, layout, want_output)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), boxes.cpu().numpy(), probs.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _assert_bit_equal(case, got, what=''):
    out, boxes, probs = got
    for b, (wo, wb, wp) in enumerate(rc.reference(case)):
        tag = f'{case.name} {what} image {b}'
        # boxes first: they do not depend on NMS, so a failure here is the decode's, a failure in probs alone is (almost surely) the NMS's
        np.testing.assert_array_equal(_bits(boxes[b]), _bits(wb), err_msg=tag + ' boxes')
        if out is not None:
            np.testing.assert_array_equal(_bits(out[b]).ravel(), _bits(wo), err_msg=tag + ' output')
        np.testing.assert_array_equal(_bits(probs[b]), _bits(wp), err_msg=tag + ' probs')


@pytest.mark.parametrize('layout', ['chw', 'hwc'])
def test_expf_limits(hip, layout):
    """(a) the overflow and underflow branches of yk_expf_glibc to the float, the subnormal band (the final double -> float conversion must round
    to subnormals, not flush), and logistic's divisions with subnormal quotients."""
    c = rc.expf_sweep()
    got = _run(c, layout)
    boxes = got[1]
    for b in range(boxes.shape[0]):
        # against float64 as well, so that the test still means something on a host whose libm differs from glibc
        rc.check_expf_f64(boxes[b, :, 2], c.x[b, :, 2], f'expf(tw) image {b}')
        rc.check_expf_f64(boxes[b, :, 3], c.x[b, :, 3], f'expf(th) image {b}')
    _assert_bit_equal(c, got, layout)


def test_softmax_tail_subnormals(hip):
    """(b) e / total and obj * e subnormal: an fp32 division or product that flushes denormals, or an approximate division, shows here; the
    subnormal probabilities are candidates (thr = 0) and go through the global-memory NMS path."""
    c = rc.softmax_tail()
    _assert_bit_equal(c, _run(c))


@pytest.mark.parametrize('layout', ['chw', 'hwc'])
@pytest.mark.parametrize('i', range(len(rc.IMAGE_SIZES)))
def test_image_sizes(hip, i, layout):
    """(c) both branches of fill_args with truncating divisions; boxes that change with image_wh feed the IoUs of NMS."""
    c = rc.image_sizes()[i]
    _assert_bit_equal(c, _run(c, layout), layout)


@pytest.mark.parametrize('i', [0, 1])
def test_exact_ties_break_by_ascending_box_index(hip, i):
    """(d) every candidate has the same probability: 210 of them (LDS path) and 8112 (global-memory path)."""
    c = rc.ties()[i]
    _assert_bit_equal(c, _run(c))


@pytest.mark.parametrize('want_output', [True, False])
def test_lds_boundary_both_paths_in_one_launch(hip, want_output):
    """(e) 2047, 2048 and 2049 candidates of class 0 next to 2049 of class 1: the LDS path one short of full and full, the global-memory path
    at its smallest, both in one launch.  Values, not masks: the kept boxes of the global path are parked as -p and must come back as p."""
    c = rc.lds_boundary()
    got = _run(c, 'chw', want_output)
    assert (got[0] is None) == (not want_output)
    _assert_bit_equal(c, got, f'want_output={want_output}')


@pytest.mark.parametrize('i', range(len(rc.SMALL)))
def test_small_grids(hip, i):
    """(f) fewer boxes than one wavefront, YK_MAX_ANCHORS anchors, threshold 0, images with no candidate and with exactly one."""
    c = rc.small()[i]
    _assert_bit_equal(c, _run(c))
    _assert_bit_equal(c, _run(c, 'hwc', False), 'hwc, no output')


def _strided_call(case, strides, lead, tail):
    """yk_region_batched through engine.call with a hand-filled RegionCfg: the input is a view, `lead` floats into a buffer poisoned with 1e30 (large and
    finite: read as a logit it changes every result, and it cannot make a NaN that compares unequal to itself), element strides as given."""
    import torch
    from k210_yolo_framework_amd import engine
    B, W, H, A, Cn = rc.dims(case)
    E, nb = 5 + Cn, A * H * W
    span = sum((n - 1) * s for n, s in zip(case.x.shape, strides)) + 1
    buf = np.full(lead + span + tail, 1e30, F)
    view = np.lib.stride_tricks.as_strided(buf[lead:], case.x.shape, tuple(4 * s for s in strides))
    view[...] = case.x
    assert int((buf != F(1e30)).sum()) == case.x.size            # the strides overlap nowhere, every other float is poison
    cfg = engine.RegionCfg()
    cfg.layer_w, cfg.layer_h, cfg.anchor_num, cfg.classes = W, H, A, Cn
    cfg.net_w, cfg.net_h, cfg.image_w, cfg.image_h = case.net_wh + case.image_wh
    cfg.threshold, cfg.nms_value = case.thr, case.nms
    for j, v in enumerate(case.anchor):
        cfg.anchor[j] = float(v)
    cfg.stride_b, cfg.stride_n, cfg.stride_e, cfg.stride_y, cfg.stride_x = strides
    dbuf = torch.from_numpy(buf).cuda()
    out = torch.empty((B, A * E, H, W), dtype=torch.float32, device='cuda')
    boxes = torch.empty((B, nb, 4), dtype=torch.float32, device='cuda')
    probs = torch.empty((B, nb, Cn + 1), dtype=torch.float32, device='cuda')
    engine.call('yk_region_batched', C.byref(cfg), dbuf[lead:], B, out, boxes, probs, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy(), boxes.cpu().numpy(), probs.cpu().numpy()


@pytest.mark.parametrize('kind', ['chw_padded', 'hwc_padded'])
def test_strided_input_equals_dense(hip, kind):
    """Strides no dense tensor has: padded rows (stride_y = W + 3), planes, anchors and images in CHW order; padded pixels
    (stride_x = A*E + 5), rows and images in HWC order."""
    c = rc.image_sizes()[3]
    B, W, H, A, Cn = rc.dims(c)
    E = 5 + Cn
    if kind == 'chw_padded':
        sx, sy = 1, W + 3
        se = H * sy + 7
        sn = E * se + 11
        sb = A * sn + 13
    else:
        se, sn, sx = 1, E, A * E + 5
        sy = W * sx + 2
        sb = H * sy + 9
    got = _strided_call(c, (sb, sn, se, sy, sx), lead=17, tail=29)
    dense = _run(c, 'chw' if kind == 'chw_padded' else 'hwc')
    for g, d, name in zip(got, dense, ('output', 'boxes', 'probs')):
        np.testing.assert_array_equal(_bits(g), _bits(d), err_msg=f'{kind} {name}')
    _assert_bit_equal(c, got, kind)


def test_dropin_abi_on_saturating_boxes(hip):
    """(g) infinite widths, zero heights: init / run / draw / deinit as main.c calls them; the draw casts see -inf and +inf (to_u32 -> 0)."""
    c = rc.saturating()
    _, W, H, A, Cn = rc.dims(c)
    out, boxes, probs, dets = oracle.drive_region_abi(hip, c.x[0], c.anchor, W, H, A, Cn, c.thr, c.nms, c.net_wh)
    (wo, wb, wp), = rc.reference(c)
    assert np.isinf(wb).sum() == 7
    np.testing.assert_array_equal(_bits(boxes), _bits(wb))
    np.testing.assert_array_equal(_bits(out), _bits(wo))
    np.testing.assert_array_equal(_bits(probs), _bits(wp))
    want = oracle.region_draw(wb, wp, c.thr)
    assert len(want) >= 20 and (want[np.isinf(wb[wp[:, :Cn].max(1) > c.thr, 2]), 2] == 0).all()
    np.testing.assert_array_equal(dets, want)                    # ordered callback rows (x1, y1, x2, y2, class, probability bits)


@pytest.mark.parametrize('anchors,channels', [(rc.YK_MAX_ANCHORS + 1, (rc.YK_MAX_ANCHORS + 1) * 7), (3, 3 * 5)])
def test_region_layer_init_refuses_with_minus_5(hip, anchors, channels):
    """More anchors than YK_MAX_ANCHORS, or zero classes: an error return that leaves the four host buffers freed and null, and a struct that
    region_layer_deinit takes without harm.  (region_layer_run on such a struct aborts by design and is not called.)"""
    rl = oracle.RegionLayerT()
    anc = np.full(2 * anchors, 0.5, F)
    rl.anchor_number = anchors
    rl.anchor = anc.ctypes.data_as(oracle.f32p)
    rl.threshold, rl.nms_value = 0.5, 0.3
    assert hip.region_layer_init(C.byref(rl), 5, 3, channels, 320, 224) == -5
    assert not rl.output and not rl.boxes and not rl.probs_buf and not rl.probs
    assert int(rl.classes) == channels // anchors - 5 and int(rl.boxes_number) == 5 * 3 * anchors
    hip.region_layer_deinit(C.byref(rl))
    # and the library is as usable as before: a layer with a valid configuration initialises, runs and matches
    good = rc.small()[2]
    _, W, H, A, Cn = rc.dims(good)
    got = oracle.drive_region_abi(hip, good.x[2], good.anchor, W, H, A, Cn, good.thr, good.nms, good.net_wh)
    for g, w in zip(got[:3], rc.reference(good)[2]):
        np.testing.assert_array_equal(_bits(g), _bits(w))

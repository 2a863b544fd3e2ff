"""The fused calibration kernels of csrc/yk_calib.hip (yk_scale_act_range_f32, yk_scale_act_hist_f32) past one grid of work items, on the
16-byte path and on the scalar path: a workgroup goes round its grid-stride loop a second time, and the channel of an item in the second trip
is not the channel of the item one trip before it.  Shapes and inputs: tests/grid_trip_cases.py.  The criteria are the ones
tests/test_gpu_quantize.py::test_scale_act_range_kernel and tests/test_gpu_hist.py::test_fused_kernel_writes_the_range_kernels_y_and_histograms_it
hold the same kernels to at smaller shapes."""
import ctypes as C

import numpy as np
import pytest

from tests import calib_ref
from tests import grid_trip_cases as gt

pytestmark = pytest.mark.gpu

CAL_ITEMS = gt.CAL_ITEMS                             # csrc/yk_range.h:13-15, grid_for: CAL_MAX_GRID x CAL_BLOCK = 2048 x 256 items per trip
_Y0 = {}                                             # path -> (z, scale, bias on the device, y of yk_scale_act_range_f32 on the host): computed once


def _range_run(path):
    import torch
    from k210_yolo_framework_amd import engine
    from tests.test_gpu_quantize import Slots
    if path not in _Y0:
        M, Cn = gt.CALIB_SHAPES[path]
        zd, sd, bd = (torch.from_numpy(np.array(v)).cuda() for v in gt.calib_case(path))
        yd = torch.full_like(zd, float('nan'))
        assert all(t.data_ptr() % 16 == 0 for t in (zd, sd, bd, yd))                               # the dispatch is decided by C alone
        S = Slots()
        assert S.L.yk_scale_act_range_f32(engine._ptr(zd), C.c_longlong(M), Cn, engine._ptr(sd), engine._ptr(bd), gt.CALIB_ACT, C.c_float(gt.CALIB_ALPHA),
                                          engine._ptr(yd), engine._ptr(S.d), 3, S._s()) == 0
        _Y0[path] = (zd, sd, bd, yd.cpu().numpy(), S.read())
    return _Y0[path]


@pytest.mark.parametrize('path', ['vector', 'scalar'])
def test_scale_act_range_kernel_past_one_grid(path):
    from tests.test_gpu_quantize import FP32_TOL, np_min_max
    M, Cn = gt.CALIB_SHAPES[path]
    assert gt.calib_vec(M, Cn) == (path == 'vector') and gt.calib_items(M, Cn) > CAL_ITEMS        # csrc/yk_calib.hip, scale_act_vec; a second trip
    _, _, _, y, (lo, hi, fl) = _range_run(path)
    z, sc, bi = gt.calib_case(path)
    v = z * sc + bi                                        # fp32, one rounding per operation
    want = np.where(v >= 0, v, v * np.float32(gt.CALIB_ALPHA)).astype(np.float32)
    err = np.abs(y.astype(np.float64) - want)
    print('max |y - numpy|', float(err.max()), 'elements with other bits', int((y.view(np.uint32) != want.view(np.uint32)).sum()), 'of', y.size)
    assert not np.isnan(y).any()                                                                   # every element was written
    assert float(err.max()) <= FP32_TOL * max(1e-6, float(np.abs(want).max()))
    w = np_min_max(y)                                      # the range is that of the y it stored, bit for bit
    assert (lo[3].tobytes(), hi[3].tobytes(), fl[3]) == (w[0].tobytes(), w[1].tobytes(), 0)
    assert np.isposinf(lo[:3]).all() and np.isneginf(hi[:3]).all()


@pytest.mark.parametrize('path', ['vector', 'scalar'])
def test_fused_histogram_kernel_past_one_grid(path):
    import torch
    from tests.test_gpu_hist import Hists
    M, Cn = gt.CALIB_SHAPES[path]
    assert gt.calib_vec(M, Cn) == (path == 'vector') and gt.calib_items(M, Cn) > CAL_ITEMS        # csrc/yk_calib.hip, scale_act_vec; a second trip
    zd, sd, bd, want_y, _ = _range_run(path)
    lo, hi = calib_ref.widen(want_y.min(), want_y.max())
    H = Hists(2048)
    p = H.engine._ptr
    y = torch.full_like(zd, float('nan'))
    assert y.data_ptr() % 16 == 0
    assert H.L.yk_scale_act_hist_f32(p(zd), C.c_longlong(M), Cn, p(sd), p(bd), gt.CALIB_ACT, C.c_float(gt.CALIB_ALPHA), p(y), C.c_float(lo),
                                     C.c_float(calib_ref.inv_of(lo, hi, 2048)), 2048, p(H.d), p(H.f), 1, H._s()) == 0
    counts, fl = H.read()
    got_y = y.cpu().numpy()
    assert got_y.tobytes() == want_y.tobytes()                                 # bit for bit the y of yk_scale_act_range_f32
    assert np.array_equal(counts[1], calib_ref.hist(got_y, lo, hi, 2048)[0]) and counts[1].sum() == M * Cn
    assert not counts[0].any() and not counts[2].any() and not fl.any()

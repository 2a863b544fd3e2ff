"""The dispatch of csrc/yk_calib.hip between its 16-byte and its scalar kernels (scale_act_vec and plain_grid there): every fused call
(yk_scale_act_range_f32, _hist_f32, _chrange_f32, _chsum_f32) and both plain ones (yk_range_f32, yk_hist_f32) once with every pointer 16-byte
aligned and once with the tensors one float into a larger allocation.  Both calls must store the same y bytes and leave the same accumulator
contents, and those must be the numpy float32 reference's: which kernel ran must not show."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import calib_ref

pytestmark = pytest.mark.gpu

M, CN, ACT, ALPHA = 7, 8, 3, 0.3                          # YK_ACT_LEAKY
NB = 64
YK_ERR_ARG = -10                                          # include/yolo_hip.h


def _case():
    rng = np.random.default_rng(78)
    z = (rng.standard_normal((M, CN)) * 3).astype(np.float32)
    sc = (rng.uniform(0.2, 2.0, CN) * rng.choice([-1, 1], CN)).astype(np.float32)
    bi = rng.standard_normal(CN).astype(np.float32)
    p = (z * sc + bi).astype(np.float32)                   # fp32, one rounding per operation
    y = np.where(p >= 0, p, p * np.float32(ALPHA)).astype(np.float32)
    assert (p < 0).any() and (p > 0).any()
    return z, sc, bi, p, y


def _placed(a, offset):
    """`a` on the device, `offset` floats into an allocation of its own (whole allocations are 16-byte aligned)."""
    import torch
    big = torch.zeros(a.size + 4, dtype=torch.float32, device='cuda')
    v = big[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * offset
    return v


def _both(run):
    """run(z, scale, bias, y) with everything aligned, then with z and y one float in: -> [(y bytes, what run returned)] x 2"""
    import torch
    z, sc, bi, _, _ = _case()
    out = []
    for off in (0, 1):
        zd, yd = _placed(z, off), _placed(np.full_like(z, np.nan), off)
        got = run(zd, _placed(sc, 0), _placed(bi, 0), yd)
        torch.cuda.synchronize()
        out.append((yd.cpu().numpy().tobytes(), got))
    return out


def _same_y_and(out, want_y):
    (y0, a0), (y1, a1) = out
    assert y0 == want_y.tobytes() and y1 == want_y.tobytes()
    assert a0 == a1
    return a0


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_scale_act_range_aligned_and_offset():
    from k210_yolo_framework_amd import engine
    from tests.test_gpu_quantize import Slots, np_min_max
    want_y = _case()[4]

    def run(z, sc, bi, y):
        S = Slots()
        engine.call('yk_scale_act_range_f32', z, M, CN, sc, bi, ACT, ALPHA, y, S.d, 2, _stream())
        S.torch.cuda.synchronize()
        return S.d.cpu().numpy().tobytes()                 # the range words as they are
    words = np.frombuffer(_same_y_and(_both(run), want_y), np.uint32).reshape(4, 4)
    S = Slots()
    S.fold(_placed(want_y, 0), 2)                          # the words of the reference's y; yk_range_f32 is held to numpy below
    S.torch.cuda.synchronize()
    assert words.tobytes() == S.d.cpu().numpy().tobytes()
    lo, hi, fl = S.read()
    w = np_min_max(want_y)
    assert (lo[2].tobytes(), hi[2].tobytes(), fl[2]) == (w[0].tobytes(), w[1].tobytes(), 0)


def test_scale_act_hist_aligned_and_offset():
    from k210_yolo_framework_amd import engine
    from tests.test_gpu_hist import Hists
    want_y = _case()[4]
    lo, hi = calib_ref.widen(want_y.min(), want_y.max())

    def run(z, sc, bi, y):
        H = Hists(NB)
        engine.call('yk_scale_act_hist_f32', z, M, CN, sc, bi, ACT, ALPHA, y, float(lo), float(calib_ref.inv_of(lo, hi, NB)), NB, H.d, H.f, 1, _stream())
        counts, fl = H.read()
        return counts.tobytes(), fl.tobytes()
    counts, fl = _same_y_and(_both(run), want_y)
    counts = np.frombuffer(counts, np.uint64).reshape(3, NB)
    assert np.array_equal(counts[1], calib_ref.hist(want_y, lo, hi, NB)[0]) and counts[1].sum() == M * CN
    assert not counts[0].any() and not counts[2].any() and not np.frombuffer(fl, np.int32).any()


def test_scale_act_chrange_aligned_and_offset():
    from k210_yolo_framework_amd import engine
    from tests.test_gpu_quantize import Slots, np_min_max
    want_y = _case()[4]

    def run(z, sc, bi, y):
        S = Slots(CN + 2)
        engine.call('yk_scale_act_chrange_f32', z, M, CN, sc, bi, ACT, ALPHA, y, S.d, 1, _stream())
        lo, hi, fl = S.read()
        return S.d.cpu().numpy().tobytes(), lo.tobytes(), hi.tobytes(), fl.tobytes()
    _, lo, hi, fl = _same_y_and(_both(run), want_y)
    lo, hi, fl = np.frombuffer(lo, np.float32), np.frombuffer(hi, np.float32), np.frombuffer(fl, np.int32)
    for c in range(CN):
        w = np_min_max(want_y[:, c])
        assert (lo[1 + c].tobytes(), hi[1 + c].tobytes()) == (w[0].tobytes(), w[1].tobytes()), c
    assert not fl.any() and lo[0] == np.inf and lo[CN + 1] == np.inf


def test_scale_act_chsum_aligned_and_offset():
    from tests.test_gpu_chsum import Sums
    _, _, _, p, want_y = _case()

    def run(z, sc, bi, y):
        S = Sums(CN + 2)
        S.run(z, sc, bi, ACT, ALPHA, y, 1)
        s, f = S.read()
        return s.tobytes(), f.tobytes()                    # the float64 sums bit for bit
    s, f = _same_y_and(_both(run), want_y)
    s = np.frombuffer(s, np.float64)
    p64 = p.astype(np.float64)
    exact = np.array([math.fsum(col) for col in p64.T])
    # seven float32 of these magnitudes: every partial sum fits in float64's 53 bits, so any order of additions gives the exact sum
    assert all(np.ldexp(np.abs(col).max(), 3) / np.abs(col).min() < 2.0 ** 28 for col in p64.T)
    assert s[1:1 + CN].tobytes() == exact.tobytes() and s[0] == 0 and s[CN + 1] == 0 and not np.frombuffer(f, np.int32).any()


def test_plain_range_and_hist_of_nine_floats_aligned_and_offset():
    """n = 9: two float4 and a tail of one when aligned, no float4 and a tail of nine when not."""
    from tests.test_gpu_hist import Hists
    from tests.test_gpu_quantize import Slots, np_min_max
    x = np.array([0.5, -2.25, 3e-41, -0.0, 7.75, 1.0, -1e-3, 6.5, -9.5], np.float32)
    lo, hi = calib_ref.widen(x.min(), x.max())
    got = []
    for off in (0, 1):
        xd = _placed(x, off)
        S, H = Slots(), Hists(NB)
        S.fold(xd, 1)
        assert H.add(xd, lo, hi, 1) == 0
        counts, hfl = H.read()
        got.append((S.d.cpu().numpy().tobytes(), counts.tobytes(), hfl.tobytes()))
        rlo, rhi, rfl = S.read()
        w = np_min_max(x)
        assert (rlo[1].tobytes(), rhi[1].tobytes(), rfl[1]) == (w[0].tobytes(), w[1].tobytes(), 0)
        assert np.array_equal(counts[1], calib_ref.hist(x, lo, hi, NB)[0]) and counts[1].sum() == 9 and not hfl.any()
        assert not counts[0].any() and not counts[2].any() and rlo[0] == np.inf and rlo[2] == np.inf
    assert got[0] == got[1]


def test_scale_act_range_refuses_a_size_past_2_63():
    import torch
    from k210_yolo_framework_amd import engine
    from tests.test_gpu_quantize import Slots
    S = Slots()
    z = torch.zeros(16, dtype=torch.float32, device='cuda')
    y = torch.full_like(z, 7.0)
    p = engine._ptr
    rc = S.L.yk_scale_act_range_f32(p(z), C.c_longlong(2 ** 62), 4, p(z), p(z), ACT, C.c_float(ALPHA), p(y), p(S.d), 0, S._s())
    assert rc == YK_ERR_ARG and b'yk_scale_act_range_f32' in S.L.yk_last_error()
    lo, hi, fl = S.read()
    assert (lo == np.inf).all() and (y == 7.0).all()       # nothing launched

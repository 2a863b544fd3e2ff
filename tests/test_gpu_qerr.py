"""yk_qerr_u8_f32, yk_dequant_u8_f32 (csrc/yk_qerr.hip) and yk_kpu_layer_ptr against the numpy rule of qerror.py.

The bound: kernel and numpy compute every term the same way (float64, one rounding per operation), and add the n terms of a channel in different
orders; a float64 sum of n terms is, in any order, within (n - 1) 2^-53 sum|term| of the exact sum, so n 2^-53 sum|term| bounds the distance
to the numpy figure's worst case of reordering.  Derived, not measured.  Counts, flags and the largest |e| do not depend on the order: exact."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from k210_yolo_framework_amd import qerror

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SUMS = ('syy', 'see', 'se', 'syh', 'shh')
EXACT = ('n', 'n0', 'n255', 'emax')


@pytest.fixture(scope='module', autouse=True)
def _give_the_memory_back():
    """The tensors of this file are returned to the driver when it is done, so that later files meet the device as they did before it existed."""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _define(name):
    from k210_yolo_framework_amd import engine
    return int(re.search(rf'#define {name} (\d+)', engine.HEADER_PATH.read_text()).group(1))


def _tile_rows(Cn):
    """Rows of one workgroup, and workgroups one pass of the finishing launch takes (include/yolo_hip.h)."""
    block = _define('YK_QERR_BLOCK')
    return -(-_define('YK_QERR_TILE') // Cn), max(1, block // min(Cn, block))


class Slots:
    def __init__(self, n):
        import torch
        from k210_yolo_framework_amd import engine
        engine.require_gpu()
        self.torch, self.engine, self.n = torch, engine, n
        self.d = torch.full((n * _define('YK_QERR_WORDS'),), -1, dtype=torch.int64, device='cuda')
        self.work = {}
        engine.call('yk_qerr_reset', self.d, n, self.stream())

    def stream(self, s=None):
        return C.c_void_p((s or self.torch.cuda.current_stream()).cuda_stream)

    def run(self, q, y, step, s_y, zp, slot0, s=None):
        B, qh, qw, Cn = q.shape
        M = B * -(-qh // step) * -(-qw // step)
        assert tuple(y.shape) == (B, -(-qh // step), -(-qw // step), Cn)
        need = C.c_size_t()
        self.engine.call('yk_qerr_workspace_bytes', M, Cn, C.byref(need))
        assert need.value == 8 * 7 * Cn * -(-M // _tile_rows(Cn)[0])
        key = (need.value, s)
        if key not in self.work:
            self.work[key] = self.torch.empty(need.value // 8, dtype=self.torch.int64, device='cuda')
        self.engine.call('yk_qerr_u8_f32', q, y, B, qh, qw, Cn, step, float(s_y), int(zp), self.d, slot0, self.work[key], self.stream(s))

    def read(self):
        counts, sums = np.empty((self.n, 4), np.int64), np.empty((self.n, 6), np.float64)
        self.torch.cuda.synchronize()
        self.engine.call('yk_qerr_read', self.d, self.n, counts, sums)
        return counts, sums

    def layer(self, got, slot0, Cn):
        return qerror.sums_of_slots(got[0][slot0:slot0 + Cn], got[1][slot0:slot0 + Cn])


def _inputs(B, qh, qw, Cn, step, s_y, zp, seed, codes=None):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (B, qh, qw, Cn)).astype(np.uint8) if codes is None else np.full((B, qh, qw, Cn), codes, np.uint8)
    y = ((q[:, ::step, ::step].astype(np.float32) - zp) * np.float32(s_y) + rng.normal(0, 2.0 * s_y, q[:, ::step, ::step].shape)).astype(np.float32)
    return q, y


def _bounds(q, y, step, s_y, zp):
    """n 2^-53 sum|term| per channel and sum."""
    ok = np.isfinite(y)
    yd = np.where(ok, y, 0).astype(np.float64)
    yh = np.where(ok, qerror.dequantise(q[:, ::step, ::step], s_y, zp), 0.0)
    e = yd - yh
    n = ok.sum(axis=(0, 1, 2)).astype(np.float64)
    terms = dict(syy=yd * yd, see=e * e, se=e, syh=yd * yh, shh=yh * yh)
    return {k: n * U * np.abs(v).sum(axis=(0, 1, 2)) for k, v in terms.items()}


def _check(got, want, bound, what):
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert np.array_equal(got['flag'], want['flag']), (what, got['flag'])
    for k in SUMS:
        err = np.abs(got[k] - want[k])
        print(f'{what} {k}: max |gpu - numpy| / bound = {float((err / np.maximum(bound[k], 1e-300)).max()):.3g}')
        assert (err <= bound[k]).all(), (what, k, err, bound[k])


def _same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in SUMS + EXACT)


def _offset_copy(t, elements=1):
    """A copy of the device tensor that starts `elements` items past a 16-byte boundary."""
    import torch
    big = torch.empty(t.numel() + elements, dtype=t.dtype, device='cuda')
    v = big[elements:].view(t.shape)
    v.copy_(t)
    return v


def _row_cases():
    """(B, qH, qW, C, step): a single row of qW positions just below, at and above one workgroup's tile, and - where that is still small -
    one pass of the finishing launch; then step 2 with odd and even sizes, and every C of the issue past one workgroup."""
    out = []
    for Cn, finish in ((1, False), (3, False), (4, True), (5, False), (256, True), (257, True)):
        T, R = _tile_rows(Cn)
        for M in sorted({T - 1, T, T + 1} | ({R * T - 1, R * T, R * T + 1} if finish else set())):
            if M > 0:
                out.append((1, 1, M, Cn, 1))
    out += [(3, 5, 6, 4, 2), (3, 6, 5, 5, 2), (2, 7, 7, 3, 2), (2, 8, 8, 256, 2), (3, 13, 10, 257, 2), (2, 65, 67, 8, 2), (1, 9, 4, 1, 2),
            (3, 33, 31, 12, 1), (2, 40, 41, 260, 1)]
    return out


@pytest.mark.parametrize('B,qh,qw,Cn,step', _row_cases())
def test_sums_against_numpy_on_both_paths(B, qh, qw, Cn, step):
    import torch
    s_y, zp = 0.0371, (B * 7 + qw + Cn) % 256
    q, y = _inputs(B, qh, qw, Cn, step, s_y, zp, seed=qw * 31 + Cn)
    want, bound = qerror.channel_sums(y, q, s_y, zp, step), _bounds(q, y, step, s_y, zp)
    S = Slots(2 * Cn + 3)
    held = torch.from_numpy(np.concatenate([q, np.zeros_like(q[:1])])).cuda()      # one image more than is compared, as a plan's arena has
    qd, yd = held[:B], torch.from_numpy(y).cuda()
    S.run(qd, yd, step, s_y, zp, 2)
    yo = _offset_copy(yd)                                                          # y 4 bytes past a 16-byte boundary: the scalar path
    assert yo.data_ptr() % 16 == 4
    S.run(qd, yo, step, s_y, zp, Cn + 3)
    got = S.read()
    a, b = S.layer(got, 2, Cn), S.layer(got, Cn + 3, Cn)
    _check(a, want, bound, 'aligned')
    _check(b, want, bound, 'offset')
    assert _same_bits(a, b)                                                        # the order follows from the shape alone, not from the alignment
    assert not got[0][[0, 1, Cn + 2]].any() and not got[1][[0, 1, Cn + 2]].any()   # the neighbouring slots are untouched


@pytest.mark.parametrize('zp,codes', [(0, None), (255, None), (0, 0), (255, 0), (0, 255), (255, 255), (128, 0), (3, 255)])
def test_zero_point_ends_and_constant_codes(zp, codes):
    import torch
    B, qh, qw, Cn, step, s_y = 2, 9, 11, 20, 1, 0.113
    q, y = _inputs(B, qh, qw, Cn, step, s_y, zp, seed=zp + 1, codes=codes)
    want, bound = qerror.channel_sums(y, q, s_y, zp), _bounds(q, y, step, s_y, zp)
    S = Slots(Cn)
    S.run(torch.from_numpy(q).cuda(), torch.from_numpy(y).cuda(), step, s_y, zp, 0)
    got = S.layer(S.read(), 0, Cn)
    _check(got, want, bound, f'zp {zp} codes {codes}')
    if codes is not None:
        n = B * qh * qw
        assert got['n0'].tolist() == [n * (codes == 0)] * Cn and got['n255'].tolist() == [n * (codes == 255)] * Cn


@pytest.mark.parametrize('Cn,bad_c,step', [(48, 17, 1), (5, 4, 1), (8, 3, 2)])
def test_a_planted_nan_and_infinity_flag_their_channel_only_and_are_not_added(Cn, bad_c, step):
    import torch
    B, qh, qw, s_y, zp = 2, 12, 10, 0.05, 40
    q, y = _inputs(B, qh, qw, Cn, step, s_y, zp, seed=9)
    y[0, 3, 2, bad_c], y[1, 0, 4, bad_c] = np.nan, np.inf
    want, bound = qerror.channel_sums(y, q, s_y, zp, step), _bounds(q, y, step, s_y, zp)
    assert want['flag'].tolist() == [c == bad_c for c in range(Cn)] and want['n'][bad_c] == want['n'][0] - 2
    # (that the numpy rule equals the sums without the element is tests/test_qerror.py's; the other channels here are those of the clean tensor)
    clean = y.copy()
    clean[0, 3, 2, bad_c] = clean[1, 0, 4, bad_c] = 0.0
    without = qerror.channel_sums(clean, q, s_y, zp, step)
    S = Slots(Cn)
    S.run(torch.from_numpy(q).cuda(), torch.from_numpy(y).cuda(), step, s_y, zp, 0)
    got = S.layer(S.read(), 0, Cn)
    _check(got, want, bound, 'planted')
    others = [c for c in range(Cn) if c != bad_c]
    for k in SUMS:
        assert np.array_equal(want[k][others], without[k][others])


def test_two_streams_give_the_same_bits_and_two_calls_accumulate():
    import torch
    B, qh, qw, Cn, s_y, zp = 6, 30, 29, 48, 0.021, 77
    q, y = _inputs(B, qh, qw, Cn, 1, s_y, zp, seed=5)
    want, bound = qerror.channel_sums(y, q, s_y, zp), _bounds(q, y, 1, s_y, zp)
    S = Slots(3 * Cn)
    qd, yd = torch.from_numpy(q).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    for k, st in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        with torch.cuda.stream(st):
            S.run(qd, yd, 1, s_y, zp, k * Cn, st)
    torch.cuda.synchronize()
    S.run(qd[:2], yd[:2], 1, s_y, zp, 2 * Cn)                                      # two batches of one set, into the third run of slots
    S.run(qd[2:], yd[2:], 1, s_y, zp, 2 * Cn)
    got = S.read()
    a, b, c = (S.layer(got, k * Cn, Cn) for k in range(3))
    assert _same_bits(a, b)
    _check(a, want, bound, 'one call')
    _check(c, want, bound, 'two calls')


def test_bad_arguments_are_refused():
    import torch
    from k210_yolo_framework_amd import engine
    S = Slots(4)
    q, y = torch.zeros((1, 2, 2, 4), dtype=torch.uint8, device='cuda'), torch.zeros((1, 2, 2, 4), dtype=torch.float32, device='cuda')
    for step, s_y, zp in ((3, 1.0, 0), (0, 1.0, 0), (1, float('inf'), 0), (1, float('nan'), 0), (1, 1.0, 256), (1, 1.0, -1)):
        with pytest.raises(engine.YkError):
            engine.call('yk_qerr_u8_f32', q, y, 1, 2, 2, 4, step, s_y, zp, S.d, 0, S.d, S.stream())
    with pytest.raises(engine.YkError):
        engine.call('yk_qerr_u8_f32', q, y, 1, 2, 2, 0, 1, 1.0, 0, S.d, 0, S.d, S.stream())
    with pytest.raises(engine.YkError):
        engine.call('yk_dequant_u8_f32', q, 1, 2, 2, 4, 0, 1.0, 0, y, S.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize('B,qh,qw,Cn,step,zp', [(2, 5, 7, 3, 1, 0), (3, 6, 5, 4, 2, 255), (2, 7, 9, 8, 2, 100), (1, 4, 4, 257, 1, 31), (2, 31, 33, 16, 1, 9)])
def test_dequantise_is_exact(B, qh, qw, Cn, step, zp):
    import torch
    from k210_yolo_framework_amd import engine
    s_y = 0.0457
    q = np.random.default_rng(qh * 10 + Cn).integers(0, 256, (B + 1, qh, qw, Cn)).astype(np.uint8)
    want = (q[:B, ::step, ::step].astype(np.int32) - zp).astype(np.float32) * np.float32(s_y)      # one fp32 rounding
    qd = torch.from_numpy(q).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for off in (0, 1):
        y = torch.full((want.size + off,), np.nan, dtype=torch.float32, device='cuda')
        engine.call('yk_dequant_u8_f32', qd, B, qh, qw, Cn, step, s_y, zp, y[off:], st)
        assert y[off:].cpu().numpy().tobytes() == want.tobytes(), off


def test_layer_ptr_equals_read_layer_byte_for_byte():
    import torch
    from k210_yolo_framework_amd import engine, quantize, yolonet
    model, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 20, alpha=0.5)
    w = model.spec.init_weights(seed=3)
    frames = quantize.synthetic_frames(3, (32, 32), seed=4)
    km, rep = quantize.quantize(model.spec, w, quantize.calibrate(model.spec, w, frames, 3))
    with engine.KpuPlan(km, max_batch=4) as plan:                                  # B below max_batch
        plan.run_u8(torch.from_numpy(frames).cuda())
        torch.cuda.synchronize()
        for name, r in rep['layers'].items():
            view = plan.layer_view(r['index'])
            assert view.dtype == torch.uint8 and view.shape[0] == 4
            got = view[:3].permute(0, 3, 1, 2).cpu().numpy()
            for i in range(3):
                assert got[i].tobytes() == plan.read_layer(r['index'], i).tobytes(), (name, i)
        with pytest.raises(engine.YkError):
            plan.layer_view(10 ** 6)

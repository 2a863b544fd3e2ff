"""yk_normalise_u8 (`img / np.max(img)` of the training input pipeline: u8_image_max_kernel + u8_normalise_kernel) on its own, bit for bit
against numpy: every quotient v / m, the maximum in every place the max kernel treats differently (byte lanes of a 16-byte load, lanes and
waves of the block, a thread's second trip, the tail after the last whole vector, the byte path of an unaligned image), a black image
between two others, and rejected arguments.  The pipeline tests only ever feed it images whose maximum is 255."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

YK_ERR_ARG = -10
M_VALUES = [1, 2, 128, 254, 255, 3, 77]


def _ref(f):
    with np.errstate(invalid='ignore'):
        return (f.astype(np.float64) / f.reshape(len(f), -1).max(1)[:, None]).astype(np.float32)


def _normalise(f, shift=0):
    """f: uint8 [B, per_image] -> float32 [B, per_image]; `shift` bytes into a larger device buffer."""
    import torch
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    buf = torch.zeros(f.size + shift, dtype=torch.uint8, device='cuda')
    d = buf[shift:]
    d.copy_(torch.from_numpy(np.ascontiguousarray(f)).reshape(-1))
    assert d.data_ptr() % 16 == shift % 16
    out = torch.full(f.shape, -7.0, dtype=torch.float32, device='cuda')
    rc = engine.lib().yk_normalise_u8(engine._ptr(d), C.c_int(f.shape[0]), C.c_size_t(f.shape[1]), engine._ptr(out), engine._stream())
    assert rc == 0, engine.lib().yk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits_equal(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:5], [(got[tuple(i)], want[tuple(i)]) for i in bad[:5]])


def test_every_quotient_is_the_float64_quotient_rounded_once():
    per_image = 259                                                 # 16 * 16 + 3: most images start unaligned, all have a tail
    rng = np.random.default_rng(0)
    f = np.empty((255, per_image), np.uint8)
    for k, m in enumerate(range(1, 256)):
        row = np.concatenate([np.arange(m + 1), rng.integers(0, m + 1, per_image - m - 1)])
        f[k] = rng.permutation(row)
    assert sum(len(np.unique(r)) for r in f) == 32895              # every pair (v, m), v <= m
    _bits_equal(_normalise(f), _ref(f))


def _positions(per_image):
    """Byte offsets the maximum is put at, one image each.  With a tail, images 0 and 16 (16-byte aligned whenever the batch is) get its
    first and last byte: only an aligned image has a tail at all, an unaligned one is read byte by byte throughout."""
    nv = per_image // 16
    want = list(range(80, 96)) if nv > 5 else list(range(min(16, per_image)))            # the 16 byte lanes of one vector
    want += [16 * v + v % 16 for v in (0, 63, 64, 1023, 1024) if v < nv]                 # lane 0 | 63, wave 1, wave 15, second trip
    if nv:
        want.append(16 * nv - 1)                                                         # end of the last whole vector
    want = list(dict.fromkeys(want))
    if per_image % 16:
        first, last = 16 * nv, per_image - 1
        want = [p for p in want if p not in (first, last)]
        want = [first] + (want * 16)[:15] + [last] + want
    return want


def _max_at_one_place(per_image):
    rng = np.random.default_rng(per_image)
    pos = _positions(per_image)
    while len(pos) < len(M_VALUES):
        pos = pos + pos
    f = np.empty((len(pos), per_image), np.uint8)
    for k, p in enumerate(pos):
        m = M_VALUES[k % len(M_VALUES)]
        f[k] = rng.integers(0, m, per_image)                       # strictly below m everywhere else
        f[k, p] = m
    assert (f.max(1) == [M_VALUES[k % len(M_VALUES)] for k in range(len(pos))]).all() and ((f == f.max(1)[:, None]).sum(1) == 1).all()
    return f


@pytest.mark.parametrize('per_image', [16 * 2049, 16 * 2049 + 5, 48, 17, 16, 15, 7, 1])
def test_the_maximum_is_found_wherever_it_sits(per_image):
    f = _max_at_one_place(per_image)
    assert len(set(f.max(1))) == len(M_VALUES)
    _bits_equal(_normalise(f), _ref(f))


@pytest.mark.parametrize('per_image', [16 * 2049, 48])
def test_a_base_that_is_not_16_byte_aligned_takes_the_byte_path(per_image):
    f = _max_at_one_place(per_image)
    _bits_equal(_normalise(f, shift=3), _ref(f))


@pytest.mark.parametrize('per_image', [48, 100])
def test_a_black_image_is_nan_and_leaves_its_neighbours_alone(per_image):
    rng = np.random.default_rng(3)
    f = np.stack([rng.integers(0, 200, per_image), np.zeros(per_image), rng.integers(0, 31, per_image)]).astype(np.uint8)
    got, want = _normalise(f), _ref(f)
    assert np.isnan(want[1]).all() and np.isfinite(want[0::2]).all() and want[0].max() == 1 and want[2].max() == 1
    _bits_equal(got, want)                                         # numpy's 0 / 0 and the kernel's are the same NaN


def test_bad_arguments_are_rejected_and_nothing_is_written():
    import torch
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    L, P, s = engine.lib(), engine._ptr, engine._stream()
    f = torch.full((2, 48), 9, dtype=torch.uint8, device='cuda')
    out = torch.full((2, 48), -7.0, dtype=torch.float32, device='cuda')
    for args in ((None, 2, 48, P(out)), (P(f), 2, 48, None), (P(f), 0, 48, P(out)), (P(f), -1, 48, P(out)), (P(f), 2, 0, P(out))):
        assert L.yk_normalise_u8(args[0], C.c_int(args[1]), C.c_size_t(args[2]), args[3], s) == YK_ERR_ARG, args
        assert 'bad argument' in L.yk_last_error().decode()
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert L.yk_normalise_u8(P(f), C.c_int(2), C.c_size_t(48), P(out), s) == 0
    torch.cuda.synchronize()
    assert (out == 1.0).all()

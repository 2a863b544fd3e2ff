"""yk_l2_segments_f32 (keras.regularizers.l2 over segments of the flat parameter buffer: l2_seg_kernel + dot_finish_kernel) on its own
against float64 numpy: segment boundaries of the per-element binary search (lengths 1, 255 | 256 | 257, an empty segment), segments out of
order with gaps between them, more elements than one pass of the 512 x 256 grid, the value / gradient switches, and rejected arguments.

Tolerances come from the count of roundings.  Gradient: G + fl(2 * weight * w) is one rounding of the product and one of the sum, each
at most 2^-24 of its result: 2^-23 * (|G| + |2 * weight * w|) per element.  Value: the squares are summed in double, the sum is cast to
float and multiplied by the weight once: two roundings of 2^-24, held to 4 * 2^-24 relative."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

YK_ERR_ARG = -10
WEIGHT = float(np.float32(5e-4))                                   # what the C entry point receives (a float)
LENGTHS = [1, 255, 256, 257, 3, 0, 70001, 65000]


@functools.lru_cache(maxsize=None)
def _layout(lengths=tuple(LENGTHS), seed=0):
    """-> P, G (float32, flat), prefix and offset tables built as TrainNet.regulariser builds them, mask of the segment elements.
    The segments lie in the buffer in another order than in the table, 1 to 1000 floats apart, with slack at both ends."""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths), np.int64)
    cur = 37
    for k in rng.permutation(len(lengths)):
        off[k] = cur
        cur += lengths[k] + int(rng.integers(1, 1001))
    size = cur + 53
    pre = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    P = rng.uniform(0.5, 2.0, size).astype(np.float32) * rng.choice([-1, 1], size).astype(np.float32)
    G = rng.normal(0, 1e-3, size).astype(np.float32)
    inside = np.zeros(size, bool)
    for o, n in zip(off, lengths):
        assert not inside[o:o + n].any()
        inside[o:o + n] = True
    assert inside.sum() == pre[-1] and not inside[:37].any() and not inside[-53:].any()
    for a in (P, G, pre, off, inside):
        a.setflags(write=False)
    return P, G, pre, off, inside


def _reference(P, G, inside):
    w = np.where(inside, P.astype(np.float64), 0.0)
    return WEIGHT * np.sum(w * w), G.astype(np.float64) + 2 * WEIGHT * w


def _call(P, G, pre, off, want_value, want_grad, out0=-7.0):
    import torch
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    p, g, dp, do = (torch.from_numpy(np.array(a)).cuda() for a in (P, G, pre, off))
    out = torch.full((1,), out0, dtype=torch.float32, device='cuda')
    rc = engine.lib().yk_l2_segments_f32(engine._ptr(p), engine._ptr(g), engine._ptr(dp), engine._ptr(do), C.c_int(len(off)),
                                         C.c_longlong(int(pre[-1])), C.c_float(WEIGHT), C.c_int(want_value), C.c_int(want_grad),
                                         engine._ptr(out), engine._stream())
    assert rc == 0, engine.lib().yk_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy().view(np.uint32), P.view(np.uint32))           # the parameters are only read
    return out.cpu().numpy(), g.cpu().numpy()


def _check_grad(got, P, G, inside):
    _, ref = _reference(P, G, inside)
    assert np.array_equal(got[~inside].view(np.uint32), G[~inside].view(np.uint32))      # gaps, slack and everything else: untouched
    bound = 2.0 ** -23 * (np.abs(G.astype(np.float64)) + np.abs(2 * WEIGHT * P.astype(np.float64)))
    err = np.abs(got.astype(np.float64) - ref)
    bad = np.flatnonzero(inside & (err > bound))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], ref[bad[:5]])
    assert (got[inside] != G[inside]).mean() > 0.99                                      # ... and the segments were


def _check_value(got, P, G, inside):
    ref, _ = _reference(P, G, inside)
    print('value', got, ref, abs(float(got) - ref) / ref / 2.0 ** -24)
    assert abs(float(got) - ref) <= 4 * 2.0 ** -24 * ref, (got, ref)


def test_value_and_gradient_over_scattered_segments():
    P, G, pre, off, inside = _layout()
    assert pre[-1] > 512 * 256 and 0 in np.diff(pre) and list(np.argsort(off)) != list(range(len(off)))   # the grid wraps; empty; unordered
    out, g = _call(P, G, pre, off, 1, 1)
    _check_value(out[0], P, G, inside)
    _check_grad(g, P, G, inside)


def test_switches_and_determinism():
    P, G, pre, off, inside = _layout()
    both, g_both = _call(P, G, pre, off, 1, 1)
    value, g_value = _call(P, G, pre, off, 1, 0)
    nothing, g_grad = _call(P, G, pre, off, 0, 1)
    assert np.array_equal(g_value.view(np.uint32), G.view(np.uint32))                   # value only: no gradient written
    _check_value(value[0], P, G, inside)
    assert nothing[0] == -7.0                                                           # gradient only: no value written
    _check_grad(g_grad, P, G, inside)
    assert value.view(np.uint32) == both.view(np.uint32) and np.array_equal(g_grad.view(np.uint32), g_both.view(np.uint32))
    again, _ = _call(P, G, pre, off, 1, 0)
    assert again.view(np.uint32) == value.view(np.uint32)                               # fixed-order sum


@pytest.mark.parametrize('n', [1, 257])
def test_a_single_segment(n):
    P, G, pre, off, inside = _layout(lengths=(n,), seed=n)
    out, g = _call(P, G, pre, off, 1, 1)
    _check_value(out[0], P, G, inside)
    _check_grad(g, P, G, inside)


def test_bad_arguments_are_rejected_and_nothing_is_written():
    import torch
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    L, ptr, s = engine.lib(), engine._ptr, engine._stream()
    P, G, pre, off, inside = _layout(lengths=(3, 5), seed=1)
    p, g, dp, do = (torch.from_numpy(np.array(a)).cuda() for a in (P, G, pre, off))
    out = torch.full((1,), -7.0, dtype=torch.float32, device='cuda')
    ok = dict(params=ptr(p), grads=ptr(g), pre=ptr(dp), off=ptr(do), nseg=2, total=8, want_value=1, want_grad=1, out=ptr(out))

    def call(**kw):
        a = {**ok, **kw}
        return L.yk_l2_segments_f32(a['params'], a['grads'], a['pre'], a['off'], C.c_int(a['nseg']), C.c_longlong(a['total']), C.c_float(WEIGHT),
                                    C.c_int(a['want_value']), C.c_int(a['want_grad']), a['out'], s)
    for bad in (dict(nseg=0), dict(nseg=-1), dict(total=0), dict(total=-8), dict(params=None), dict(grads=None), dict(out=None),
                dict(pre=None), dict(off=None)):
        assert call(**bad) == YK_ERR_ARG, bad
        assert 'bad argument' in L.yk_last_error().decode()
    torch.cuda.synchronize()
    assert out.item() == -7.0 and np.array_equal(g.cpu().numpy().view(np.uint32), G.view(np.uint32))
    assert call(grads=None, want_grad=0) == 0 and call(out=None, want_value=0) == 0     # a null pointer nobody asked to fill is fine
    torch.cuda.synchronize()
    assert out.item() != -7.0 and not np.array_equal(g.cpu().numpy(), G)

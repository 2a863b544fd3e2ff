"""The small calls of csrc/yk_train.hip that every training step runs - yk_maxpool2_{fwd,bwd}_f32, yk_upsample2x_bwd_f32, yk_bias_add_f32,
yk_colsum_f32, yk_axpy_f32, yk_adam_f32 - at the shapes, values and arguments where they can go wrong (tests/train_cases.py holds the
cases and references; tests/test_train_cases.py checks those on the CPU).

yk_train.o is built without FMA contraction, so every written operation is one IEEE rounding and most of this is held BIT FOR BIT against a
numpy float32 restatement of the kernel's written order: the pool's y and argmax, the pool's gradient on integer dy, the upsample adjoint,
bias add, axpy, the column sum on integer data, and Adam's m, v and p (float32 divide and sqrtf are correctly rounded on the device, as
they are in numpy).  Where sums of normal data are compared with float64 the bound counts roundings: 3 * 2^-24 * sum|terms| for the at
most four terms of the pool gradient and the upsample adjoint; 2^-24 |ref| + M 2^-53 sum|x| for the column sum (accumulated in double on
the device); per Adam step 2^-23 (|p| + 4 |update|), 3 * 2^-24 (|b1 m| + |(1 - b1) g|) and likewise for v, accumulated over four steps.

Every output carries a tail of sentinels (64 floats; 64 bytes of 0xA5 behind the uint8 argmax) that must come back untouched.

Sensitivity: what fails first under each mutation.  The pool and Adam mutations were applied to the numpy restatements and run against
this file's data (the device kernels equal those restatements bit for bit, which is what the tests assert); the last two follow from
reading the code.  None was run on a device.
  `>=` for `>` in maxpool_fwd_kernel          test_maxpool...: `arg` differs on data (a) in 26 of the 28 cases (the 1 x 1 inputs cannot tie);
                                              y does not differ, the tied values being equal
  a dropped tap (t < 3) in maxpool_bwd_kernel test_maxpool...: dx differs bit for bit on integer dy wherever a window's arg is 3
  swapped tap order (t >> 1 <-> t & 1)        test_maxpool...: `arg` differs in 75 of the 84 case x data pairs (forward mutated); dx then
                                              differs wherever arg is 1 or 2 (backward mutated)
  a dropped `i < total` guard                 `written past its end` from _tails_intact in the test of that call, at every size that is no
                                              multiple of 256
  b2 for b1 in adam_kernel's m                test_adam_single_step...: m differs in the 15 cases that start from a previous state
  gi for gi * gi in adam_kernel's v           test_adam_single_step...: v differs in all 30 cases
  grad_scale ignored                          test_adam_single_step... at grad_scale 1/8 and 1/3: m and v differ in all 20 cases; and
                                              test_adam_grad_scale_equals_scaling_the_gradient
  lane_split's other side at C = 17 and 33    nothing fails, and nothing should: bn_colreduce_kernel takes the split as an argument and
                                              sums correctly under either, in double, so integer data give the same bits.  What the
                                              C = 16 | 17 and 32 | 33 cases pin is the geometry built FROM the split: a grid sized by the
                                              neighbouring split leaves columns of C = 130 unwritten, and the column sum test fails there."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_cases as tc

pytestmark = pytest.mark.gpu

YK_ERR_ARG = -10                                                  # include/yolo_hip.h
SENTINEL, TAIL, TAIL_U8 = 12345.0, 64, 0xA5


def _lib():
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    return engine, engine.lib()


def _cu(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).cuda()                       # (a copy: the shared problems are read-only)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(*shape, init=None, dtype=torch.float32):
    """An output tensor as a view of a sentinel-filled buffer with TAIL elements more behind it (see _tails_intact); init: its contents."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), TAIL_U8 if dtype == torch.uint8 else SENTINEL, dtype=dtype, device='cuda')
    view = buf[:n].view(*shape)
    if init is not None:
        view.copy_(torch.from_numpy(np.array(init)).view(*shape))             # (a copy: the shared problems are read-only)
    return view, buf


def _tails_intact(*bufs):
    for k, b in enumerate(bufs):
        want = TAIL_U8 if b.dtype == torch.uint8 else SENTINEL
        assert bool((b[-TAIL:] == want).all()), f'output {k}: written past its end'


def _untouched(*bufs):
    for k, b in enumerate(bufs):
        want = TAIL_U8 if b.dtype == torch.uint8 else SENTINEL
        assert bool((b == want).all()), f'output {k}: written by a refused call'


def _same_bits(got, want, what):
    """got (device tensor or array) equals want (float32 values) bit for bit: -0 is not 0, and -inf must be -inf."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    w32 = want.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == w32.shape, (what, got.dtype, got.shape, w32.shape)
    if want.dtype != np.float32:
        assert np.array_equal(w32.astype(np.float64), want, equal_nan=True), what     # the reference is a float32 value
    bad = np.flatnonzero(got.view(np.uint32).ravel() != w32.view(np.uint32).ravel())
    assert bad.size == 0, (what, int(bad.size), bad[:4], got.ravel()[bad[:4]], w32.ravel()[bad[:4]])


def _within(got, ref, bound, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    err, bound = np.abs(got.astype(np.float64) - ref), np.broadcast_to(bound, np.shape(ref))
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print('margin', what, f'{float(ratio.max()) if ratio.size else 0.0:.3g}')
    assert (err <= bound).all(), (what, int(np.argmax(ratio)), float(ratio.max()))


# --------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize('case', tc.POOL_CASES, ids=str)
def test_maxpool_forward_argmax_and_backward(case):
    """Forward: y bit for bit (a selection) and argmax equal to 'first maximum in tap order' on every element - on {0, 6} data most
    windows tie, on data (b) a whole plane is -inf (y = -inf, arg = 0).  Backward, driven by the reference's arg and by the device's own:
    bit for bit on integer dy (also where one input wins four windows at stride 1), three roundings on normal dy."""
    engine, L = _lib()
    B, Hi, Wi, Cc, Ho, Wo, s = tc.pool_geom(case)
    for kind in tc.POOL_KINDS:
        p = tc.pool_problem(case, kind)
        xd, dyd = _cu(p['x']), _cu(p['dy'])
        (y, yb), (arg, argb) = _out(B, Ho, Wo, Cc), _out(B, Ho, Wo, Cc, dtype=torch.uint8)
        assert L.yk_maxpool2_fwd_f32(engine._ptr(xd), B, Hi, Wi, Cc, Ho, Wo, s, engine._ptr(y), engine._ptr(arg), _st()) == 0, L.yk_last_error()
        torch.cuda.synchronize()
        _tails_intact(yb, argb)
        _same_bits(y, p['y'], ('y', kind))
        got_arg = arg.cpu().numpy()
        assert np.array_equal(got_arg, p['arg']), ('arg', kind, np.argwhere(got_arg != p['arg'])[:4])
        for who, a in (('reference arg', _cu(p['arg'], np.uint8)), ('device arg', arg)):
            dx, dxb = _out(B, Hi, Wi, Cc)
            assert L.yk_maxpool2_bwd_f32(engine._ptr(dyd), engine._ptr(a), B, Hi, Wi, Cc, Ho, Wo, s, engine._ptr(dx), _st()) == 0, L.yk_last_error()
            torch.cuda.synchronize()
            _tails_intact(dxb)
            if kind == 'c':
                _within(dx, p['dx'], 3 * tc.U * p['dx_abs'], ('pool dx', kind, who))
            else:
                assert p['abs_sum'] < 2 ** 24
                _same_bits(dx, p['dx'], ('dx', kind, who))


# --------------------------------------------------------------------------------------------- upsample adjoint, bias add, axpy
@pytest.mark.parametrize('case', tc.UPSAMPLE_CASES, ids=str)
def test_upsample_adjoint_is_bitwise_the_written_order(case):
    engine, L = _lib()
    B, H, W, Cc = case
    p = tc.upsample_problem(case)
    dx, dxb = _out(B, H, W, Cc)
    assert L.yk_upsample2x_bwd_f32(engine._ptr(_cu(p['dy'])), B, H, W, Cc, engine._ptr(dx), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(dxb)
    _same_bits(dx, p['dx32'], 'dx')
    _within(dx, p['dx64'], 3 * tc.U * p['dx_abs'], ('upsample dx', case))


@pytest.mark.parametrize('case', tc.BIAS_CASES, ids=str)
def test_bias_add_is_bitwise_one_rounded_sum(case):
    engine, L = _lib()
    M, Cc = case
    p = tc.bias_problem(case)
    y, yb = _out(M, Cc, init=p['y'])
    assert L.yk_bias_add_f32(engine._ptr(y), C.c_longlong(M), Cc, engine._ptr(_cu(p['bias'])), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(yb)
    _same_bits(y, p['out32'], 'y')


@pytest.mark.parametrize('case', tc.AXPY_CASES, ids=str)
def test_axpy_is_bitwise_product_then_sum_also_on_a_misaligned_view(case):
    """y += a * x with the product rounded before the sum; once on an aligned y, once in place on a view that starts one float behind a
    16-byte boundary (the element in front of it and the tail behind it stay)."""
    engine, L = _lib()
    n, a = case
    p = tc.axpy_problem(case)
    xd = _cu(p['x'])
    y, yb = _out(n, init=p['y'])
    assert L.yk_axpy_f32(C.c_longlong(n), C.c_float(a), engine._ptr(xd), engine._ptr(y), _st()) == 0, L.yk_last_error()
    buf = torch.full((1 + n + TAIL,), SENTINEL, device='cuda')
    view = buf[1:1 + n]
    view.copy_(torch.from_numpy(np.array(p['y'])))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    assert L.yk_axpy_f32(C.c_longlong(n), C.c_float(a), engine._ptr(xd), engine._ptr(view), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(yb, buf)
    assert float(buf[0]) == SENTINEL
    _same_bits(y, p['out32'], 'y')
    _same_bits(view, p['out32'], 'y, misaligned')


# --------------------------------------------------------------------------------------------- column sum
@pytest.mark.parametrize('case', tc.COLSUM_CASES, ids=str)
def test_colsum_on_every_route(case):
    """bn_chunking -> bn_colreduce_kernel<true> -> colsum_from_stats_kernel with 16 / 32 / 64 channel lanes, fewer rows than row lanes, a
    last chunk of one row, more chunks than one pass of the finishing wave: integers -3..3 bit for bit (|sum| <= 3 M < 2^24: exact in any
    order), normal data within one float32 rounding of the float64 sum plus the float64 reordering error."""
    engine, L = _lib()
    M, Cc = case
    assert M * 3 < 2 ** 24
    for lattice in (True, False):
        p = tc.colsum_problem(case, lattice)
        out, outb = _out(Cc)
        assert L.yk_colsum_f32(engine._ptr(_cu(p['x'])), C.c_longlong(M), Cc, engine._ptr(out), _st()) == 0, L.yk_last_error()
        torch.cuda.synchronize()
        _tails_intact(outb)
        if lattice:
            _same_bits(out, p['sum'], ('colsum', case))
        else:
            _within(out, p['sum'], tc.colsum_bound(M, p['sum'], p['abs_sum']), ('colsum', case))


# --------------------------------------------------------------------------------------------- Adam
def _adam(engine, L, n, p, g, m, v, iterations, gscale, decay):
    """yk_adam_f32 with the Trainer's constants on sentinel-tailed device tensors p, m, v (updated in place)."""
    rc = L.yk_adam_f32(C.c_longlong(n), engine._ptr(p), engine._ptr(g), engine._ptr(m), engine._ptr(v), C.c_float(tc.ADAM_LR), C.c_float(decay),
                       C.c_longlong(iterations), C.c_float(tc.ADAM_B1), C.c_float(tc.ADAM_B2), C.c_float(tc.ADAM_EPS), C.c_float(gscale), _st())
    assert rc == 0, L.yk_last_error()


def _ulps_of_update(got_p, pr):
    """The largest |p - restatement| in units in the last place of the update term p_old - p_new (printed before p is asserted)."""
    upd = np.abs(pr['p'].astype(np.float64) - pr['p32'].astype(np.float64))
    ulp = np.spacing(np.maximum(upd, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(got_p.astype(np.float64) - pr['p32'].astype(np.float64)) / ulp).max())


@pytest.mark.parametrize('case', tc.ADAM_CASES, ids=str)
def test_adam_single_step_is_bitwise_the_written_order(case):
    """m, v (products and sums) and p (one correctly rounded divide and square root more) bit for bit against the float32 restatement,
    with lr_t formed in double as the host code writes it: at iterations up to 100 000, with and without decay, grad_scale 1, 1/8 and
    1/3, from a fresh and from a previous state, with exact-zero gradients (0 / (0 + eps): p unchanged to the bit, m = v = 0) and
    gradients of 1e-20 whose squares are subnormal."""
    engine, L = _lib()
    n, iterations, gscale, decay, warm = case
    pr = tc.adam_problem(case)
    (p, pb), (m, mb), (v, vb) = _out(n, init=pr['p']), _out(n, init=pr['m']), _out(n, init=pr['v'])
    _adam(engine, L, n, p, _cu(pr['g']), m, v, iterations, gscale, decay)
    torch.cuda.synchronize()
    _tails_intact(pb, mb, vb)
    _same_bits(m, pr['m32'], 'm')
    _same_bits(v, pr['v32'], 'v')
    got_p = p.cpu().numpy()
    print('adam p: largest difference in ulps of the update', _ulps_of_update(got_p, pr))
    _same_bits(got_p, pr['p32'], 'p')
    z = (pr['g'] == 0) & (pr['v'] == 0) & (pr['m'] == 0)
    assert n < 255 or warm or z.any()
    assert np.array_equal(got_p[z].view(np.uint32), pr['p'][z].view(np.uint32))
    assert not m.cpu().numpy()[z].any() and not v.cpu().numpy()[z].any()


@pytest.mark.parametrize('warm', [False, True])
def test_adam_grad_scale_equals_scaling_the_gradient(warm):
    """grad_scale = 1/8 on g is grad_scale = 1 on g / 8 (an exact product), bit for bit in p, m and v."""
    engine, L = _lib()
    case = next(c for c in tc.ADAM_CASES if c[2] == 0.125 and c[0] == 10007)
    n, iterations, _, decay, _ = case
    rng = np.random.default_rng(3)
    p0, m0, v0 = tc.adam_state(rng, n, warm)
    g = tc.adam_gradients(rng, n)
    runs = []
    for gs, gd in ((0.125, _cu(g)), (1.0, _cu(g * np.float32(0.125)))):
        (p, pb), (m, mb), (v, vb) = _out(n, init=p0), _out(n, init=m0), _out(n, init=v0)
        _adam(engine, L, n, p, gd, m, v, iterations, gs, decay)
        torch.cuda.synchronize()
        _tails_intact(pb, mb, vb)
        runs.append([t.cpu().numpy() for t in (p, m, v)])
    for a, b, k in zip(runs[0], runs[1], 'pmv'):
        _same_bits(a, b, k)
    assert not np.array_equal(runs[0][1], m0)


@pytest.mark.parametrize('case', tc.ADAM_RUN_CASES, ids=str)
def test_adam_four_steps_against_float64(case):
    """Four consecutive steps against oracle.train_ref.AdamRef (float64, with the gradient scale in front): p, m and v after every step
    within the accumulated per-step bounds of tests/train_cases.py (ScaledAdamRef.step)."""
    engine, L = _lib()
    n, it0, gscale, decay, warm = case
    pr = tc.adam_run_problem(case)
    (p, pb), (m, mb), (v, vb) = _out(n, init=pr['p']), _out(n, init=pr['m']), _out(n, init=pr['v'])
    for k, s in enumerate(pr['steps']):
        _adam(engine, L, n, p, _cu(s['g']), m, v, it0 + k, gscale, decay)
        torch.cuda.synchronize()
        _tails_intact(pb, mb, vb)
        for t, a in ((p, 'p'), (m, 'm'), (v, 'v')):
            _within(t, s[a + '64'], s['b' + a], (a, 'step', k, case))


# --------------------------------------------------------------------------------------------- refusals
def test_the_small_calls_refuse_bad_arguments_on_the_host():
    """A null pointer, a non-positive size, a pool stride outside {1, 2}, pool output sizes that are not ceil(input / stride), and negative
    Adam iterations: YK_ERR_ARG with a text that names the call, and no launch - every output stays sentinel-filled."""
    engine, L = _lib()
    f = torch.zeros(4096, device='cuda')
    u8 = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    o, ob = _out(4096)
    o2, o2b = _out(4096)
    o3, o3b = _out(4096)
    a8, a8b = _out(4096, dtype=torch.uint8)
    F, U8, O, O2, O3, A8 = (engine._ptr(t) for t in (f, u8, o, o2, o3, a8))
    ll, fl, st = C.c_longlong, C.c_float, _st()
    adam = lambda n=16, p=O, g=F, m=O2, v=O3, it=0: (ll(n), p, g, m, v, fl(5e-4), fl(0.0), ll(it), fl(0.9), fl(0.999), fl(1e-7), fl(1.0), st)
    pf = lambda x=F, B=2, Hi=5, Wi=7, Cc=3, Ho=3, Wo=4, s=2, y=O, arg=A8: (x, B, Hi, Wi, Cc, Ho, Wo, s, y, arg, st)
    pb = lambda dy=F, arg=U8, B=2, Hi=5, Wi=7, Cc=3, Ho=3, Wo=4, s=2, dx=O: (dy, arg, B, Hi, Wi, Cc, Ho, Wo, s, dx, st)
    bad = {
        'yk_bias_add_f32': [(None, ll(4), 3, F, st), (O, ll(4), 3, None, st), (O, ll(0), 3, F, st), (O, ll(-1), 3, F, st), (O, ll(4), 0, F, st)],
        'yk_colsum_f32': [(None, ll(4), 3, O, st), (F, ll(4), 3, None, st), (F, ll(0), 3, O, st), (F, ll(4), 0, O, st), (F, ll(4), -2, O, st)],
        'yk_upsample2x_bwd_f32': [(None, 1, 2, 2, 3, O, st), (F, 1, 2, 2, 3, None, st), (F, 0, 2, 2, 3, O, st), (F, 1, 0, 2, 3, O, st),
                                  (F, 1, 2, -1, 3, O, st), (F, 1, 2, 2, 0, O, st)],
        'yk_axpy_f32': [(ll(8), fl(1.0), None, O, st), (ll(8), fl(1.0), F, None, st), (ll(0), fl(1.0), F, O, st), (ll(-8), fl(1.0), F, O, st)],
        'yk_adam_f32': [adam(p=None), adam(g=None), adam(m=None), adam(v=None), adam(n=0), adam(n=-16), adam(it=-1)],
        'yk_maxpool2_fwd_f32': [pf(x=None), pf(y=None), pf(arg=None), pf(B=0), pf(Hi=0), pf(Wi=-1), pf(Cc=0), pf(Ho=0), pf(Wo=0), pf(s=0),
                                pf(s=3), pf(s=-1), pf(Ho=2), pf(Wo=3), pf(Ho=5, Wo=7), pf(s=1)],
        'yk_maxpool2_bwd_f32': [pb(dy=None), pb(arg=None), pb(dx=None), pb(B=0), pb(Hi=0), pb(Wi=-1), pb(Cc=0), pb(Ho=0), pb(Wo=0), pb(s=0),
                                pb(s=3), pb(s=-1), pb(Ho=2), pb(Wo=3), pb(Ho=5, Wo=7), pb(s=1)],
    }
    for name, calls in bad.items():
        for k, args in enumerate(calls):
            assert getattr(L, name)(*args) == YK_ERR_ARG, (name, k)
            text = L.yk_last_error()
            assert text and name.encode() in text, (name, k, text)
    torch.cuda.synchronize()
    _untouched(ob, o2b, o3b, a8b)
    # and the same argument lists, valid, are accepted: the refusals above are about the one argument each of them changes
    assert L.yk_maxpool2_fwd_f32(*pf()) == 0 and L.yk_maxpool2_bwd_f32(*pb()) == 0 and L.yk_adam_f32(*adam()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(ob, o2b, o3b, a8b)

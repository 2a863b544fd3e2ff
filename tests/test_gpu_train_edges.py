"""The depthwise and BatchNorm training kernels of csrc/yk_train.hip on every dispatch path and edge of their host wrappers, each against
a float64 reference (tests/train_cases.py holds the cases, the references and the tolerances; tests/test_train_cases.py checks those on
the CPU).  tests/test_gpu_train.py reaches most of these paths at one shape each or only through a whole training step.

Tolerances (fp32 HIP vs float64): depthwise on integer data bit for bit, on normal data 1e-4 of the tensor's maximum; BatchNorm statistics
1e-5, y within 2e-5 of max|pre|, dbeta / dgamma per column within 2e-4 of the column's sum of |terms| plus the kink slack, dz within 2e-4
of its maximum plus the widening the kink slack implies (tests/train_cases.py: kink_slack).

Every output buffer carries a tail of sentinel values that must come back untouched: a store that loses its row or channel guard shows
there.  With YK_TRAIN_EDGES_MARGINS=<file> every BatchNorm test appends its largest err / bound per output to that file
(tools/train_edges_margins.py folds it into profiles/train_edges_margins.txt)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import netspec as ns
from tests import train_cases as tc

pytestmark = pytest.mark.gpu

YK_ERR_ARG = -10                                                  # include/yolo_hip.h
SENTINEL, TAIL = 12345.0, 64                                      # TAIL floats behind every output


def _lib():
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    return engine, engine.lib()


def _cu(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()                  # (a copy: the shared problems are read-only)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(*shape):
    """An output tensor as a view of a sentinel-filled buffer with TAIL floats more behind it (see _tails_intact)."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), SENTINEL, device='cuda')
    return buf[:n].view(*shape), buf


def _tails_intact(*bufs):
    for k, b in enumerate(bufs):
        assert bool((b[-TAIL:] == SENTINEL).all()), f'output {k}: written past its end'


def _close(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref).max()
    assert err <= tol * max(1e-6, np.abs(ref).max()), (err, np.abs(ref).max())


def _margin(path, case, **ratios):
    print('margins', path, case, ' '.join(f'{k}={v:.3g}' for k, v in ratios.items()))
    f = os.environ.get('YK_TRAIN_EDGES_MARGINS')
    if f:
        with open(f, 'a') as fh:
            for k, v in ratios.items():
                fh.write(f'{path} {k} {v:.6g} {case}\n')


def _ratio(err, bound):
    """Largest err / bound; a zero bound (exact result required) counts as 0 when met and inf when missed."""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    if err.size == 0:
        return 0.0
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# --------------------------------------------------------------------------------------------- depthwise 3x3
def _dw_run(engine, L, case, p):
    """yk_dw3x3_fwd_f32, yk_dw3x3_bwd_data_f32, yk_dw3x3_bwd_weight_f32 on one problem: (y, dx, dw) as numpy."""
    geom, _ = tc.dw_geom(case)
    B, Hi, Wi, Cc, Ho, Wo = geom[:6]
    g = [C.c_int(v) for v in geom]
    xd, wd, dyd = _cu(p['x']), _cu(p['w'].reshape(9, Cc)), _cu(p['dy'])
    (y, yb), (dx, dxb), (dw, dwb) = _out(B, Ho, Wo, Cc), _out(B, Hi, Wi, Cc), _out(9, Cc)
    assert L.yk_dw3x3_fwd_f32(engine._ptr(xd), engine._ptr(wd), *g, engine._ptr(y), _st()) == 0, L.yk_last_error()
    assert L.yk_dw3x3_bwd_data_f32(engine._ptr(dyd), engine._ptr(wd), *g, engine._ptr(dx), _st()) == 0, L.yk_last_error()
    assert L.yk_dw3x3_bwd_weight_f32(engine._ptr(xd), engine._ptr(dyd), *g, engine._ptr(dw), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(yb, dxb, dwb)
    return y.cpu().numpy(), dx.cpu().numpy(), dw.cpu().numpy().reshape(3, 3, Cc)


@pytest.mark.parametrize('case', tc.DW_CASES, ids=str)
def test_depthwise_on_integer_data_is_bitwise_the_float64_reference(case):
    """Inputs, weights and dy are integers -3..3 and every sum of |terms| stays below 2^24 (asserted from the reference), so fp32 is exact in
    any summation order: one missing or doubled tap at a border, a segment start or a cut channel group fails outright."""
    engine, L = _lib()
    p = tc.dw_problem(case, True)
    assert p['abs_sum'] < 2 ** 24
    y, dx, dw = _dw_run(engine, L, case, p)
    assert np.array_equal(y, p['y']), np.argwhere(y != p['y'])[:4]
    assert np.array_equal(dx, p['dx']), np.argwhere(dx != p['dx'])[:4]
    assert np.array_equal(dw, p['dw']), np.argwhere(dw != p['dw'])[:4]


def test_grouped_depthwise_weight_gradients_on_integer_data_are_bitwise_the_float64_reference():
    """The same problems through yk_dw3x3_bwd_weight_grouped_f32 in one call, against the reference and not against the separate calls."""
    engine, L = _lib()
    ps = [tc.dw_problem(case, True) for case in tc.DW_CASES]
    n = len(ps)
    xs, dys = [_cu(p['x']) for p in ps], [_cu(p['dy']) for p in ps]
    outs = [_out(9, case[3]) for case in tc.DW_CASES]
    geo = [v for case in tc.DW_CASES for v in tc.dw_geom(case)[0]]
    pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    assert L.yk_dw3x3_bwd_weight_grouped_f32(n, pa(xs), pa(dys), (C.c_int * (9 * n))(*geo), pa([o for o, _ in outs]), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    for case, p, (o, buf) in zip(tc.DW_CASES, ps, outs):
        _tails_intact(buf)
        assert np.array_equal(o.cpu().numpy().reshape(3, 3, case[3]), p['dw']), case


@pytest.mark.parametrize('case', tc.DW_CASES, ids=str)
def test_depthwise_on_normal_data(case):
    engine, L = _lib()
    p = tc.dw_problem(case, False)
    y, dx, dw = _dw_run(engine, L, case, p)
    _close(y, p['y'], 1e-4)
    _close(dx, p['dx'], 1e-4)
    _close(dw, p['dw'], 1e-4)


@pytest.mark.parametrize('case', tc.IM2COL_CASES, ids=str)
def test_im2col_and_col2im_with_asymmetric_padding_on_integer_data(case):
    """yk_im2col3x3_f32 (C = 4: float4 kernel, C = 3: scalar kernel) copies, yk_col2im3x3_f32 sums at most 9 integers: both exact."""
    engine, L = _lib()
    geom, _ = tc.dw_geom(case)
    B, Hi, Wi, Cc, Ho, Wo = geom[:6]
    g = [C.c_int(v) for v in geom]
    rng = np.random.default_rng(sum(case))
    x = rng.integers(-3, 4, (B, Hi, Wi, Cc)).astype(np.float32)
    cm = rng.integers(-3, 4, (B * Ho * Wo, 9 * Cc)).astype(np.float32)
    (col, colb), (dx, dxb) = _out(B * Ho * Wo, 9 * Cc), _out(B, Hi, Wi, Cc)
    assert L.yk_im2col3x3_f32(engine._ptr(_cu(x)), *g, engine._ptr(col), _st()) == 0
    assert L.yk_col2im3x3_f32(engine._ptr(_cu(cm)), *g, engine._ptr(dx), _st()) == 0
    torch.cuda.synchronize()
    _tails_intact(colb, dxb)
    assert np.array_equal(col.cpu().numpy(), tc.im2col_ref(case, x))
    assert np.array_equal(dx.cpu().numpy(), tc.col2im_ref(case, cm))


# --------------------------------------------------------------------------------------------- BatchNorm forward + backward
def _bn_fwd_bwd(engine, L, zd, gd, bd, dyd, M, Cc, act, alpha):
    """yk_bn_train_fwd_f32 then yk_bn_train_bwd_f32 on device tensors; every output as a device tensor."""
    (y, yb), (dz, dzb) = _out(M, Cc), _out(M, Cc)
    (sm, smb), (si, sib), (dg, dgb), (db, dbb), (mm, mmb), (mv, mvb) = (_out(Cc) for _ in range(6))
    mm.zero_()
    mv.fill_(1.0)
    assert L.yk_bn_train_fwd_f32(engine._ptr(zd), C.c_longlong(M), Cc, engine._ptr(gd), engine._ptr(bd), C.c_float(tc.EPS), act, C.c_float(alpha),
                                 engine._ptr(y), engine._ptr(sm), engine._ptr(si), engine._ptr(mm), engine._ptr(mv), C.c_float(tc.MOMENTUM),
                                 _st()) == 0, L.yk_last_error()
    assert L.yk_bn_train_bwd_f32(engine._ptr(zd), engine._ptr(dyd), C.c_longlong(M), Cc, engine._ptr(gd), engine._ptr(bd), engine._ptr(sm),
                                 engine._ptr(si), act, C.c_float(alpha), engine._ptr(dz), engine._ptr(dg), engine._ptr(db), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(yb, dzb, smb, sib, dgb, dbb, mmb, mvb)
    return dict(y=y, dz=dz, mean=sm, invstd=si, dgamma=dg, dbeta=db, moving_mean=mm, moving_var=mv)


def _exact_dbeta(engine, L, case, zd, gd, bd, out, ref, amb, cols=None):
    """dbeta once more, exactly.  The per-column bound above is 2e-4 of the sum of |terms|: at 50 000 rows one dropped or doubled row moves
    dbeta by 2e-5 of that and passes.  With dy on the integers -3..3 and a gate of 0 or 1 (none, relu, relu6) every g is an integer and
    sum |g| <= 3 M < 2^24, so fp32 gives sum g exactly in any order: dbeta must EQUAL the float64 sum.  dy is 0 at the ambiguous elements, so
    their gate does not matter; everywhere else fp32 and float64 gate alike (the fp32 pre-activation is off by ~1e-6, the band is 1e-4).
    cols: the columns that ref and amb hold (all by default); only these are compared."""
    M, Cc, act, alpha = case
    if act == ns.ACT_LEAKY:
        return
    assert 3 * M < 2 ** 24
    gen = torch.Generator(device='cuda').manual_seed(M + Cc)
    dyi = torch.randint(-3, 4, (M, Cc), device='cuda', generator=gen).float()
    idx = torch.arange(Cc, device='cuda') if cols is None else torch.tensor(cols, device='cuda')
    dyi[:, idx] = dyi[:, idx] * torch.from_numpy(~amb).cuda()
    (dz, dzb), (dg, dgb), (db, dbb) = _out(M, Cc), _out(Cc), _out(Cc)
    assert L.yk_bn_train_bwd_f32(engine._ptr(zd), engine._ptr(dyi), C.c_longlong(M), Cc, engine._ptr(gd), engine._ptr(bd), engine._ptr(out['mean']),
                                 engine._ptr(out['invstd']), act, C.c_float(alpha), engine._ptr(dz), engine._ptr(dg), engine._ptr(db), _st()) == 0
    torch.cuda.synchronize()
    _tails_intact(dzb, dgb, dbb)
    want = (dyi[:, idx].cpu().numpy().astype(np.float64) * tc.act_gate(ref['pre'], act, alpha)).sum(0)
    got = db[idx].cpu().numpy().astype(np.float64)
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8], (got - want)[got != want][:8])


def _bn_check(case, got, ref, amb, s_db, s_dg, widen):
    """got: numpy arrays of the compared columns.  The assertions of the module docstring; prints and records err / bound first."""
    M, Cc, act, alpha = case
    path = tc.bn_bwd_path(M, Cc)
    assert tc.kink_cap_holds(amb), (int(amb.sum(0).max()), M)                 # a condition on the data: else the slack is no small thing
    e_db, b_db = np.abs(got['dbeta'] - ref['dbeta']), tc.GRAD_TOL * ref['S_dbeta'] + s_db
    e_dg, b_dg = np.abs(got['dgamma'] - ref['dgamma']), tc.GRAD_TOL * ref['S_dgamma'] + s_dg
    e_dz, b_dz = np.abs(got['dz'] - ref['dz'])[~amb], (tc.GRAD_TOL * np.abs(ref['dz']).max() + widen)[~amb]
    e_y, b_y = np.abs(got['y'] - ref['y']).max(), 2e-5 * np.abs(ref['pre']).max()
    _margin(path, case, dbeta=_ratio(e_db, b_db), dgamma=_ratio(e_dg, b_dg), dz=_ratio(e_dz, b_dz), y=_ratio(e_y, b_y))
    _close(got['mean'], ref['mean'], 1e-5)
    _close(got['invstd'], ref['invstd'], 1e-5)
    _close(got['moving_mean'], ref['moving_mean'], 1e-5)
    _close(got['moving_var'], ref['moving_var'], 1e-5)     # fed the UNBIASED batch variance; the biased one (here 0) for a single row
    assert e_y <= b_y, (e_y, b_y)
    assert (e_db <= b_db).all(), (int(np.argmax(e_db - b_db)), e_db.max(), b_db.min())
    assert (e_dg <= b_dg).all(), (int(np.argmax(e_dg - b_dg)), e_dg.max(), b_dg.min())
    # one row: dz is identically 0 in exact arithmetic and max|ref dz| = 0, so this asks |dz| <= the widening alone
    assert (e_dz <= b_dz).all(), (e_dz.max(), b_dz.min())


# The longest sequential fp32 addition chain behind one dbeta / dgamma (tests/train_cases.py: bn_bwd_chain), per path at these shapes:
#   cols    3 rows per thread + a 9-step tree over the 512 row lanes                                                     = 12 adds
#   scalar  rows per thread (1 .. 13) + row lanes (4 .. 16) + chunks / 64 (1 .. 8) + the 6-step wave tree              <= 35 adds
#   v4      rows per thread (8 .. 25) + row lanes (1 .. 64) + chunks / 64 (2 .. 32) + the 6-step wave tree             <= 80 adds
# so the a-priori bound chain * 2^-24 * S_c is at most 4.8e-6 * S_c: 40 times below the 2e-4 * S_c asserted (the products g * xhat and
# xhat itself add a few more roundings of 2^-24 each, far inside that room).  tests/test_train_cases.py asserts the factor of ten.
@pytest.mark.parametrize('case', tc.BN_HOST_CASES, ids=str)
def test_batchnorm_forward_backward_on_every_path(case):
    engine, L = _lib()
    M, Cc, act, alpha = case
    p = tc.bn_problem(case)
    zd, gd, bd = _cu(p['z']), _cu(p['gamma']), _cu(p['beta'])
    out = _bn_fwd_bwd(engine, L, zd, gd, bd, _cu(p['dy']), M, Cc, act, alpha)
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
    _bn_check(case, got, p['ref'], p['amb'], p['slack_dbeta'], p['slack_dgamma'], p['dz_widen'])
    _exact_dbeta(engine, L, case, zd, gd, bd, out, p['ref'], p['amb'])


@pytest.mark.parametrize('case', [c for c in tc.BN_CASES if c[:2] in tc.BN_WIDE], ids=str)
def test_batchnorm_forward_backward_wide_v4(case):
    """C = 1024 (256 channel-quad lanes, one row lane) and C = 1028 (a second channel group of one lane): 51 M elements, generated on the
    GPU; the first 8 and the last 16 columns come to the host and are compared (BatchNorm is per column, so the subset is exact)."""
    engine, L = _lib()
    M, Cc, act, alpha = case
    cols = tc.BN_WIDE[(M, Cc)]
    rng = np.random.default_rng(Cc)
    scale, shift = _cu(rng.uniform(0.5, 3, Cc)), _cu(rng.normal(size=Cc) * 2)
    gamma, beta = rng.uniform(0.5, 3, Cc).astype(np.float32), rng.normal(size=Cc).astype(np.float32)
    gen = torch.Generator(device='cuda').manual_seed(Cc)
    zd = torch.randn(M, Cc, device='cuda', generator=gen).mul_(scale).add_(shift)
    dyd = torch.randn(M, Cc, device='cuda', generator=gen)
    gd, bd = _cu(gamma), _cu(beta)
    out = _bn_fwd_bwd(engine, L, zd, gd, bd, dyd, M, Cc, act, alpha)
    idx = torch.tensor(cols, device='cuda')
    take = lambda t: t.index_select(t.dim() - 1, idx).cpu().numpy().astype(np.float64)
    dy = take(dyd)
    ref = tc.bn_ref(take(zd), gamma, beta, dy, act, alpha, cols=cols)
    amb, s_db, s_dg, widen = tc.kink_slack(ref, dy)
    _bn_check(case, {k: take(v) for k, v in out.items()}, ref, amb, s_db, s_dg, widen)
    _exact_dbeta(engine, L, case, zd, gd, bd, out, ref, amb, cols)


def test_batchnorm_backward_refuses_a_null_dgamma_on_the_host():
    """bn_apply_bwd_kernel reads dgamma unconditionally, so a NULL is an argument error: refused by the host check at the top of
    yk_bn_train_bwd_f32, before the device is asked for and before any launch."""
    engine, L = _lib()
    M, Cc = 8, 4
    z, dy, dz = torch.zeros(M, Cc, device='cuda'), torch.zeros(M, Cc, device='cuda'), torch.zeros(M, Cc, device='cuda')
    v = [torch.ones(Cc, device='cuda') for _ in range(5)]
    rc = L.yk_bn_train_bwd_f32(engine._ptr(z), engine._ptr(dy), C.c_longlong(M), Cc, engine._ptr(v[0]), engine._ptr(v[1]), engine._ptr(v[2]),
                               engine._ptr(v[3]), ns.ACT_RELU, C.c_float(0.0), engine._ptr(dz), None, engine._ptr(v[4]), _st())
    assert rc == YK_ERR_ARG and b'yk_bn_train_bwd_f32' in L.yk_last_error()
    rc = L.yk_bn_train_bwd_f32(engine._ptr(z), engine._ptr(dy), C.c_longlong(0), Cc, engine._ptr(v[0]), engine._ptr(v[1]), engine._ptr(v[2]),
                               engine._ptr(v[3]), ns.ACT_RELU, C.c_float(0.0), engine._ptr(dz), engine._ptr(v[4]), engine._ptr(v[4]), _st())
    assert rc == YK_ERR_ARG


# --------------------------------------------------------------------------------------------- the fused forwards vs float64
def _fused_check(out, z_ref, ref, ztol):
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
    _close(got['z'], z_ref, ztol)
    for k in ('mean', 'invstd', 'moving_mean', 'moving_var'):
        _close(got[k], ref[k], 1e-5)
    e_y, b_y = np.abs(got['y'] - ref['y']).max(), 2e-5 * np.abs(ref['pre']).max()
    print('fused y err / bound', e_y / b_y)
    assert e_y <= b_y, (e_y, b_y)


def _bn_outs(M, N):
    o = dict(z=_out(M, N), y=_out(M, N), mean=_out(N), invstd=_out(N), moving_mean=_out(N), moving_var=_out(N))
    o['moving_mean'][0].zero_()
    o['moving_var'][0].fill_(1.0)
    return {k: v[0] for k, v in o.items()}, [v[1] for v in o.values()]


@pytest.mark.parametrize('i', range(len(tc.GEMM_BN_CASES)), ids=[str(c) for c in tc.GEMM_BN_CASES])
def test_gemm_bn_forward_against_float64(i):
    """yk_gemm_bn_fwd_f32 around bn_fwd_cols_kernel<3>: M = 512 / 513 / 1536 rows take it (one / two / three rows per thread, C % 8 == 0
    and == 4), M = 1537 is the first to miss it.  Against X W^T and BatchNorm in float64, not against the separate calls."""
    engine, L = _lib()
    M, N, K, with_res = tc.GEMM_BN_CASES[i]
    act, alpha = tc.ACTS[i % 4]
    rng = np.random.default_rng(M + N)
    X, W = (rng.normal(size=(M, K)) + 0.3).astype(np.float32), rng.normal(size=(N, K)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 2, N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    r = rng.normal(size=(M, N)).astype(np.float32) if with_res else None
    z_ref = X.astype(np.float64) @ W.astype(np.float64).T
    ref = tc.bn_ref(z_ref, gamma, beta, None, act, alpha, res=r)
    xd, wd, gd, bd, rd = _cu(X), _cu(W), _cu(gamma), _cu(beta), (_cu(r) if with_res else None)
    o, bufs = _bn_outs(M, N)
    assert L.yk_gemm_bn_fwd_f32(M, N, K, engine._ptr(xd), K, engine._ptr(wd), K, engine._ptr(o['z']), engine._ptr(gd), engine._ptr(bd),
                                C.c_float(tc.EPS), act, C.c_float(alpha), engine._ptr(o['y']), engine._ptr(o['mean']), engine._ptr(o['invstd']),
                                engine._ptr(o['moving_mean']), engine._ptr(o['moving_var']), C.c_float(tc.MOMENTUM),
                                engine._ptr(rd) if with_res else None, _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(*bufs)
    _fused_check(o, z_ref, ref, 2e-5)


@pytest.mark.parametrize('i', range(len(tc.DW_BN_CASES)), ids=[str(c) for c in tc.DW_BN_CASES])
def test_depthwise_bn_forward_against_float64(i):
    """yk_dw3x3_bn_fwd_f32 (dw_fwd_stats_kernel + bn_fwd_cols_kernel<3>) with a cut channel-lane group and with asymmetric padding."""
    engine, L = _lib()
    case = tc.DW_BN_CASES[i]
    geom, _ = tc.dw_geom(case)
    B, Hi, Wi, Cc, Ho, Wo = geom[:6]
    M = B * Ho * Wo
    act, alpha = tc.ACTS[i + 1]
    p = tc.dw_problem(case, False)
    rng = np.random.default_rng(Cc)
    gamma, beta = rng.uniform(0.5, 2, Cc).astype(np.float32), rng.normal(size=Cc).astype(np.float32)
    z_ref = p['y'].reshape(M, Cc)
    ref = tc.bn_ref(z_ref, gamma, beta, None, act, alpha)
    xd, wd, gd, bd = _cu(p['x']), _cu(p['w'].reshape(9, Cc)), _cu(gamma), _cu(beta)
    o, bufs = _bn_outs(M, Cc)
    assert L.yk_dw3x3_bn_fwd_f32(engine._ptr(xd), engine._ptr(wd), *[C.c_int(v) for v in geom], engine._ptr(o['z']), engine._ptr(gd), engine._ptr(bd),
                                 C.c_float(tc.EPS), act, C.c_float(alpha), engine._ptr(o['y']), engine._ptr(o['mean']), engine._ptr(o['invstd']),
                                 engine._ptr(o['moving_mean']), engine._ptr(o['moving_var']), C.c_float(tc.MOMENTUM), None, _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(*bufs)
    _fused_check(o, z_ref, ref, 1e-4)


# --------------------------------------------------------------------------------------------- the 16-byte rule of the host wrappers
# A V = 4 kernel is launched only when C % 4 == 0 AND every tensor it touches 16 bytes at a time starts on a 16-byte boundary (vec4_ok in
# yk_train.hip); otherwise the scalar kernel runs.  Each entry point is called with every tensor aligned and once per tensor argument with
# that tensor 4 bytes past a boundary (a [1:] view of a buffer one float longer); every call meets the float64 reference within the bound
# the tests above apply to that entry point.
def _placed(which, ins, outs):
    """Device tensors of one call: inputs from numpy arrays, outputs as views of sentinel-filled buffers with TAIL floats behind them.  The
    tensor named `which` starts 4 bytes past a 16-byte boundary (one sentinel float in front), every other one on a boundary."""
    t, bufs = {}, {}
    for k, a in ins.items():
        a, off = np.array(a, np.float32), int(k == which)               # (a copy: the shared problems are read-only)
        buf = torch.zeros(a.size + off, device='cuda')
        buf[off:] = torch.from_numpy(a.reshape(-1)).cuda()
        t[k] = buf[off:].view(*a.shape)
    for k, shape in outs.items():
        n, off = int(np.prod(shape)), int(k == which)
        bufs[k] = torch.full((off + n + TAIL,), SENTINEL, device='cuda')
        t[k] = bufs[k][off:off + n].view(*shape)
    for k, v in t.items():
        assert v.data_ptr() % 16 == (4 if k == which else 0), k
    assert which is None or which in t, which
    return t, bufs


def _guards_intact(bufs, which):
    _tails_intact(*bufs.values())
    if which in bufs:
        assert float(bufs[which][0]) == SENTINEL, f'{which}: written before its start'


def _dw_align_call(engine, L, fn, case, which, p, a, out):
    """One of the two three-tensor depthwise calls (a, w -> out) with `which` misaligned: the output as numpy."""
    geom, _ = tc.dw_geom(case)
    B, Hi, Wi, Cc, Ho, Wo = geom[:6]
    shape = (B, Ho, Wo, Cc) if out == 'y' else (B, Hi, Wi, Cc)
    t, bufs = _placed(which, {a: p[a], 'w': p['w'].reshape(9, Cc)}, {out: shape})
    assert fn(engine._ptr(t[a]), engine._ptr(t['w']), *[C.c_int(v) for v in geom], engine._ptr(t[out]), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _guards_intact(bufs, which)
    return t[out].cpu().numpy()


@pytest.mark.parametrize('which', [None, 'x', 'w', 'y'], ids=str)
@pytest.mark.parametrize('case', tc.ALIGN_DW_CASES, ids=str)
def test_depthwise_forward_with_a_misaligned_tensor(case, which):
    """yk_dw3x3_fwd_f32: exact on integer data, 1e-4 on normal data; dw_fwd_kernel<1> and <4> add the taps in one order, so the call with a
    misaligned tensor returns the bits of the aligned call."""
    engine, L = _lib()
    p = tc.dw_problem(case, True)
    assert p['abs_sum'] < 2 ** 24
    assert np.array_equal(_dw_align_call(engine, L, L.yk_dw3x3_fwd_f32, case, which, p, 'x', 'y'), p['y'])
    p = tc.dw_problem(case, False)
    y = _dw_align_call(engine, L, L.yk_dw3x3_fwd_f32, case, which, p, 'x', 'y')
    _close(y, p['y'], 1e-4)
    if which:
        assert np.array_equal(y, _dw_align_call(engine, L, L.yk_dw3x3_fwd_f32, case, None, p, 'x', 'y'))


@pytest.mark.parametrize('which', [None, 'dy', 'w', 'dx'], ids=str)
@pytest.mark.parametrize('case', tc.ALIGN_DW_CASES, ids=str)
def test_depthwise_data_gradient_with_a_misaligned_tensor(case, which):
    """yk_dw3x3_bwd_data_f32: exact on integer data, 1e-4 on normal data."""
    engine, L = _lib()
    p = tc.dw_problem(case, True)
    assert p['abs_sum'] < 2 ** 24
    assert np.array_equal(_dw_align_call(engine, L, L.yk_dw3x3_bwd_data_f32, case, which, p, 'dy', 'dx'), p['dx'])
    p = tc.dw_problem(case, False)
    _close(_dw_align_call(engine, L, L.yk_dw3x3_bwd_data_f32, case, which, p, 'dy', 'dx'), p['dx'], 1e-4)


_BN_FWD_OUTS = ('y', 'mean', 'invstd', 'moving_mean', 'moving_var')


def _bn_fwd_tensors(which, ins, M, Cc, z_out):
    """_placed for a BatchNorm forward: y [M][Cc] (and z when the call produces it), four vectors, the moving statistics at (0, 1)."""
    outs = dict({'z': (M, Cc)} if z_out else {}, y=(M, Cc), mean=(Cc,), invstd=(Cc,), moving_mean=(Cc,), moving_var=(Cc,))
    t, bufs = _placed(which, ins, outs)
    t['moving_mean'].zero_()
    t['moving_var'].fill_(1.0)
    return t, bufs


@pytest.mark.parametrize('which', [None, 'x', 'w', 'z', 'gamma', 'beta', 'y', 'mean', 'invstd', 'moving_mean', 'moving_var', 'res'], ids=str)
@pytest.mark.parametrize('case', tc.ALIGN_DW_CASES, ids=str)
def test_depthwise_bn_forward_with_a_misaligned_tensor(case, which):
    """yk_dw3x3_bn_fwd_f32 with a residual, against the depthwise reference and BatchNorm in float64: the bounds of
    test_depthwise_bn_forward_against_float64."""
    engine, L = _lib()
    geom, _ = tc.dw_geom(case)
    B, Hi, Wi, Cc, Ho, Wo = geom[:6]
    M = B * Ho * Wo
    act, alpha = tc.ACTS[2]
    p = tc.dw_problem(case, False)
    rng = np.random.default_rng(Cc + M)
    gamma, beta = rng.uniform(0.5, 2, Cc).astype(np.float32), rng.normal(size=Cc).astype(np.float32)
    r = rng.normal(size=(M, Cc)).astype(np.float32)
    z_ref = p['y'].reshape(M, Cc)
    ref = tc.bn_ref(z_ref, gamma, beta, None, act, alpha, res=r)
    t, bufs = _bn_fwd_tensors(which, dict(x=p['x'], w=p['w'].reshape(9, Cc), gamma=gamma, beta=beta, res=r), M, Cc, True)
    assert L.yk_dw3x3_bn_fwd_f32(engine._ptr(t['x']), engine._ptr(t['w']), *[C.c_int(v) for v in geom], engine._ptr(t['z']), engine._ptr(t['gamma']),
                                 engine._ptr(t['beta']), C.c_float(tc.EPS), act, C.c_float(alpha), engine._ptr(t['y']), engine._ptr(t['mean']),
                                 engine._ptr(t['invstd']), engine._ptr(t['moving_mean']), engine._ptr(t['moving_var']), C.c_float(tc.MOMENTUM),
                                 engine._ptr(t['res']), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _guards_intact(bufs, which)
    _fused_check({k: t[k] for k in ('z',) + _BN_FWD_OUTS}, z_ref, ref, 1e-4)


@pytest.mark.parametrize('which', [None, 'z', 'gamma', 'beta', 'y', 'mean', 'invstd', 'moving_mean', 'moving_var', 'res'], ids=str)
def test_batchnorm_forward_with_residual_and_a_misaligned_tensor(which):
    """yk_bn_train_fwd_res_f32 at M = 30, C = 4: statistics within 1e-5, y within 2e-5 of max|pre|, as _bn_check asks of the forward."""
    engine, L = _lib()
    M, Cc, act, alpha = tc.ALIGN_BN_CASE
    p = tc.bn_problem(tc.ALIGN_BN_CASE)
    r = np.random.default_rng(M + Cc).normal(size=(M, Cc)).astype(np.float32)
    ref = tc.bn_ref(p['z'], p['gamma'], p['beta'], None, act, alpha, res=r)
    t, bufs = _bn_fwd_tensors(which, dict(z=p['z'], gamma=p['gamma'], beta=p['beta'], res=r), M, Cc, False)
    assert L.yk_bn_train_fwd_res_f32(engine._ptr(t['z']), C.c_longlong(M), Cc, engine._ptr(t['gamma']), engine._ptr(t['beta']), C.c_float(tc.EPS), act,
                                     C.c_float(alpha), engine._ptr(t['y']), engine._ptr(t['mean']), engine._ptr(t['invstd']),
                                     engine._ptr(t['moving_mean']), engine._ptr(t['moving_var']), C.c_float(tc.MOMENTUM), engine._ptr(t['res']),
                                     _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _guards_intact(bufs, which)
    got = {k: t[k].cpu().numpy().astype(np.float64) for k in _BN_FWD_OUTS}
    for k in ('mean', 'invstd', 'moving_mean', 'moving_var'):
        _close(got[k], ref[k], 1e-5)
    e_y, b_y = np.abs(got['y'] - ref['y']).max(), 2e-5 * np.abs(ref['pre']).max()
    print('y err / bound', e_y / b_y)
    assert e_y <= b_y, (e_y, b_y)


@pytest.mark.parametrize('which', [None, 'z', 'dy', 'gamma', 'beta', 'mean', 'invstd', 'dz', 'dgamma', 'dbeta'], ids=str)
def test_batchnorm_backward_with_a_misaligned_tensor(which):
    """yk_bn_train_bwd_f32 at M = 30, C = 4 (aligned: bn_bwd_cols_kernel<3>; any tensor misaligned: the scalar reduction and apply pass) on
    the statistics an aligned yk_bn_train_fwd_f32 saved: the bounds of _bn_check."""
    engine, L = _lib()
    case = tc.ALIGN_BN_CASE
    M, Cc, act, alpha = case
    p = tc.bn_problem(case)
    fwd = _bn_fwd_bwd(engine, L, _cu(p['z']), _cu(p['gamma']), _cu(p['beta']), _cu(p['dy']), M, Cc, act, alpha)
    ins = dict(z=p['z'], dy=p['dy'], gamma=p['gamma'], beta=p['beta'], mean=fwd['mean'].cpu().numpy(), invstd=fwd['invstd'].cpu().numpy())
    t, bufs = _placed(which, ins, dict(dz=(M, Cc), dgamma=(Cc,), dbeta=(Cc,)))
    assert L.yk_bn_train_bwd_f32(engine._ptr(t['z']), engine._ptr(t['dy']), C.c_longlong(M), Cc, engine._ptr(t['gamma']), engine._ptr(t['beta']),
                                 engine._ptr(t['mean']), engine._ptr(t['invstd']), act, C.c_float(alpha), engine._ptr(t['dz']), engine._ptr(t['dgamma']),
                                 engine._ptr(t['dbeta']), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _guards_intact(bufs, which)
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in fwd.items()}
    got.update({k: t[k].cpu().numpy().astype(np.float64) for k in ('dz', 'dgamma', 'dbeta')})
    _bn_check(case, got, p['ref'], p['amb'], p['slack_dbeta'], p['slack_dgamma'], p['dz_widen'])


def test_depthwise_entry_points_refuse_a_null_tensor_and_an_empty_batch():
    """yk_dw3x3_fwd_f32, yk_dw3x3_bwd_data_f32, yk_dw3x3_bwd_weight_f32 and yk_dw3x3_bn_fwd_f32: a NULL tensor or B = 0 is YK_ERR_ARG with a
    message that names the entry point, from the host check at the top of each: nothing is launched."""
    engine, L = _lib()
    geom, _ = tc.dw_geom(tc.ALIGN_DW_CASES[0])
    B, Hi, Wi, Cc, Ho, Wo = geom[:6]
    M = B * Ho * Wo
    x, y, w = torch.zeros(B, Hi, Wi, Cc, device='cuda'), torch.zeros(B, Ho, Wo, Cc, device='cuda'), torch.zeros(9, Cc, device='cuda')
    v = [torch.ones(Cc, device='cuda') for _ in range(6)]
    z, r = torch.zeros(M, Cc, device='cuda'), torch.zeros(M, Cc, device='cuda')
    g = lambda b: [C.c_int(b)] + [C.c_int(k) for k in geom[1:]]
    bn = lambda zz: [engine._ptr(zz) if zz is not None else None, engine._ptr(v[0]), engine._ptr(v[1]), C.c_float(tc.EPS), ns.ACT_RELU, C.c_float(0.0),
                     engine._ptr(y), engine._ptr(v[2]), engine._ptr(v[3]), engine._ptr(v[4]), engine._ptr(v[5]), C.c_float(tc.MOMENTUM), engine._ptr(r)]
    calls = {
        b'yk_dw3x3_fwd_f32': (lambda: L.yk_dw3x3_fwd_f32(engine._ptr(x), engine._ptr(w), *g(B), None, _st()),
                              lambda: L.yk_dw3x3_fwd_f32(engine._ptr(x), engine._ptr(w), *g(0), engine._ptr(y), _st())),
        b'yk_dw3x3_bwd_data_f32': (lambda: L.yk_dw3x3_bwd_data_f32(None, engine._ptr(w), *g(B), engine._ptr(x), _st()),
                                   lambda: L.yk_dw3x3_bwd_data_f32(engine._ptr(y), engine._ptr(w), *g(0), engine._ptr(x), _st())),
        b'yk_dw3x3_bwd_weight_f32': (lambda: L.yk_dw3x3_bwd_weight_f32(engine._ptr(x), None, *g(B), engine._ptr(w), _st()),
                                     lambda: L.yk_dw3x3_bwd_weight_f32(engine._ptr(x), engine._ptr(y), *g(0), engine._ptr(w), _st())),
        b'yk_dw3x3_bn_fwd_f32': (lambda: L.yk_dw3x3_bn_fwd_f32(engine._ptr(x), engine._ptr(w), *g(B), *bn(None), _st()),
                                 lambda: L.yk_dw3x3_bn_fwd_f32(engine._ptr(x), engine._ptr(w), *g(0), *bn(z), _st())),
    }
    for name, (null_tensor, empty_batch) in calls.items():
        for call in (null_tensor, empty_batch):
            assert call() == YK_ERR_ARG, name
            assert name in L.yk_last_error(), (name, L.yk_last_error())
    torch.cuda.synchronize()

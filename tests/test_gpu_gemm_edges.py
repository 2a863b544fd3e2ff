"""The fp32 MFMA GEMM family (yk_gemm_f32, yk_gemm_f32_grouped, yk_gemm_bn_fwd_f32) and the implicit-GEMM 3x3 convolutions (yk_conv3x3_*) on
every layout, loader, epilogue, K-slice and finishing-pass path of their host wrappers, each against a float64 reference
(tests/gemm_cases.py holds the cases, the references and the path labels in the test ids; tests/test_gemm_cases.py checks those on the CPU).

Lattice data (integers -3..3, (alpha, beta) in {(1, 0), (0.5, 2)}) is exact in fp32 in any summation order: the result must EQUAL the
float64 reference, so one dropped, doubled or misplaced term, an unwritten slab or a mis-scaled epilogue fails outright.  Normal data (K <= 320)
is held per element to gamma(K + 4) (|alpha| |A| |B| + |beta| |C0|), the any-order fp32 summation bound: a product in less than fp32 misses
it.  Every test prints its largest err / bound (`gemm-margins path output ratio case`; tools/gemm_edges_margins.py folds `pytest -s` output
into profiles/gemm_edges_margins.txt).

Every operand of yk_gemm_f32 lives in a larger buffer: leading dimensions exceed the rows, an operand may start one float past a 16-byte
boundary, and every float that is no matrix element holds one NaN pattern.  C's buffer holds that pattern everywhere when beta == 0;
afterwards the guards are compared as int32 and must be untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_cases as gc
from tests import train_cases as tc
from tests.test_gpu_train_edges import _bn_outs, _cu, _fused_check, _lib, _out, _ratio, _st, _tails_intact

pytestmark = pytest.mark.gpu

YK_ERR_ARG, YK_ERR_UNSUPPORTED = -10, -12                        # include/yolo_hip.h


def _dev(buf):
    """A flat float32 host buffer on the device, bit for bit (NaN payloads included)."""
    t = torch.from_numpy(np.array(buf).view(np.int32)).cuda().view(torch.float32)
    assert t.data_ptr() % 16 == 0
    return t


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _margin(path, output, ratio, case):
    print('gemm-margins', path, output, f'{ratio:.6g}', case)


def _check_c(got, p, M, N, pc, oc, lattice, path, case):
    """got: C's whole buffer back on the host.  Guards untouched (as int32); the logical region equal to the float64 reference (lattice) or
    within the per-element bound (normal)."""
    bits = got.view(np.int32)
    touched = np.flatnonzero(p['guard'] & (bits != gc.NAN_BITS))
    assert touched.size == 0, ('written outside C', touched[:8], got[touched[:8]])
    out = gc.logical(got, M, N, pc, oc).astype(np.float64)
    if lattice:
        assert np.array_equal(out, p['ref']), (np.argwhere(out != p['ref'])[:4], out[out != p['ref']][:4], p['ref'][out != p['ref']][:4])
        return
    err = np.abs(out - p['ref'])
    _margin(path, 'c', _ratio(np.nan_to_num(err, nan=np.inf), p['bound']), case)
    assert (err <= p['bound']).all(), (np.argwhere(~(err <= p['bound']))[:4], float(np.nanmax(err / p['bound'])))


# --------------------------------------------------------------------------------------------- yk_gemm_f32
def _gemm(c, lattice):
    engine, L = _lib()
    p = gc.gemm_problem(c, lattice)
    tA, tB = gc.LAYOUTS[c.layout]
    a, b, cc = _dev(p['bufA']), _dev(p['bufB']), _dev(p['bufC'])
    assert L.yk_gemm_f32(tA, tB, c.M, c.N, c.K, C.c_float(p['alpha']), _p(a, c.oa), p['lda'], _p(b, c.ob), p['ldb'], C.c_float(p['beta']),
                         _p(cc, c.oc), p['ldc'], _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _check_c(cc.cpu().numpy(), p, c.M, c.N, c.pc, c.oc, lattice, gc.gemm_path(c), gc.gemm_id(c))


@pytest.mark.parametrize('c', gc.GEMM_CASES, ids=gc.gemm_id)
def test_gemm_on_lattice_data_is_bitwise_the_float64_reference(c):
    assert gc.gemm_problem(c, True)['abs_sum'] < 2 ** 24
    _gemm(c, True)


@pytest.mark.parametrize('c', gc.GEMM_NORMAL_CASES, ids=gc.gemm_id)
def test_gemm_on_normal_data_within_the_fp32_summation_bound(c):
    _gemm(c, False)


def test_gemm_refuses_bad_arguments_on_the_host():
    engine, L = _lib()
    t = torch.zeros(64, device='cuda')
    for M, N, K, a in [(0, 4, 4, t), (4, -1, 4, t), (4, 4, 0, t), (4, 4, 4, None)]:
        rc = L.yk_gemm_f32(0, 1, M, N, K, C.c_float(1), _p(a) if a is not None else None, 4, _p(t), 4, C.c_float(0), _p(t), 4, _st())
        assert rc == YK_ERR_ARG and b'yk_gemm_f32' in L.yk_last_error()
    assert L.yk_gemm_f32_grouped(-1, 0, 1, None, None, None, C.c_float(1), None, None, None, None, C.c_float(0), None, None, _st()) == YK_ERR_ARG
    assert L.yk_gemm_f32_grouped(2, 0, 1, None, None, None, C.c_float(1), None, None, None, None, C.c_float(0), None, None, _st()) == YK_ERR_ARG
    assert (t == 0).all()


# --------------------------------------------------------------------------------------------- yk_gemm_f32_grouped
@pytest.mark.parametrize('layout,count', gc.GROUP_CASES, ids=[f'{l}-{n}' for l, n in gc.GROUP_CASES])
def test_grouped_gemms_on_lattice_data_are_bitwise_the_float64_reference(layout, count):
    """Against the float64 reference of every problem and not against the separate calls (same tile code); then a second call, bit for bit
    the first.  `count` problems ride in grouped launches (1, 36, 37, 73: one launch, exactly full, one over, three launches), the ones that
    cannot take 16-byte loads go through their own launch in between; TT: every problem falls back."""
    engine, L = _lib()
    tA, tB = gc.LAYOUTS[layout]
    ps = gc.group_problem(layout, count)
    n = len(ps)
    alpha, beta = gc.ALPHA_BETA[gc.group_ab(count)]
    As, Bs, Cs = [_cu(p['A']) for p in ps], [_cu(p['B']) for p in ps], [_dev(p['bufC']) for p in ps]
    ia = lambda v: (C.c_int * n)(*v)
    pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    args = (n, tA, tB, ia([p['M'] for p in ps]), ia([p['N'] for p in ps]), ia([p['K'] for p in ps]), C.c_float(alpha), pa(As), ia([a.shape[1] for a in As]),
            pa(Bs), ia([b.shape[1] for b in Bs]), C.c_float(beta), pa(Cs), ia([p['ldc'] for p in ps]), _st())
    assert L.yk_gemm_f32_grouped(*args) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    first = [c.cpu().numpy() for c in Cs]
    for i, (p, got) in enumerate(zip(ps, first)):
        _check_c(got, p, p['M'], p['N'], p['pc'], 0, True, None, (layout, count, i, p['M'], p['N'], p['K']))
    for c, p in zip(Cs, ps):
        c.copy_(_dev(p['bufC']))
    assert L.yk_gemm_f32_grouped(*args) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    for i, (c, f) in enumerate(zip(Cs, first)):
        assert np.array_equal(c.cpu().numpy().view(np.int32), f.view(np.int32)), (i, ps[i]['M'], ps[i]['N'], ps[i]['K'])


def test_grouped_gemm_of_no_problems_does_nothing():
    engine, L = _lib()
    for tA, tB in gc.LAYOUTS.values():
        assert L.yk_gemm_f32_grouped(0, tA, tB, None, None, None, C.c_float(1), None, None, None, None, C.c_float(0), None, None, _st()) == 0


# --------------------------------------------------------------------------------------------- GEMM + BatchNorm
def _bn_args(engine, o, gd, bd, act, alpha, rd):
    return (engine._ptr(gd), engine._ptr(bd), C.c_float(tc.EPS), act, C.c_float(alpha), engine._ptr(o['y']), engine._ptr(o['mean']), engine._ptr(o['invstd']),
            engine._ptr(o['moving_mean']), engine._ptr(o['moving_var']), C.c_float(tc.MOMENTUM), engine._ptr(rd) if rd is not None else None, _st())


def _z_exact_then_bn(o, bufs, z_ref, gamma, beta, act, alpha, res):
    _tails_intact(*bufs)
    z = o['z'].cpu().numpy().astype(np.float64)
    assert np.array_equal(z, z_ref), (np.argwhere(z != z_ref)[:4], z[z != z_ref][:4], z_ref[z != z_ref][:4])
    _fused_check(o, z_ref, tc.bn_ref(z_ref, gamma, beta, None, act, alpha, res=res), 2e-5)


@pytest.mark.parametrize('i', range(len(gc.GEMM_BN_CASES)), ids=[gc.gemm_bn_id(c) for c in gc.GEMM_BN_CASES])
def test_gemm_bn_forward_on_lattice_data(i):
    """yk_gemm_bn_fwd_f32: z bitwise X W^T in float64; the batch statistics, the moving statistics and y to the bounds of
    test_gemm_bn_forward_against_float64.  The STATS epilogue with rows past M and a ragged column tile, the scalar STATS kernel,
    ldx > K, and the split route with an empty slice."""
    engine, L = _lib()
    c = gc.GEMM_BN_CASES[i]
    act, alpha = tc.ACTS[i % 4]
    p = gc.gemm_bn_problem(c)
    assert p['abs_sum'] < 2 ** 24
    xd, wd, gd, bd, rd = _dev(p['bufX']), _dev(p['bufW']), _cu(p['gamma']), _cu(p['beta']), (_cu(p['res']) if c.res else None)
    o, bufs = _bn_outs(c.M, c.N)
    assert L.yk_gemm_bn_fwd_f32(c.M, c.N, c.K, _p(xd, c.ox), p['ldx'], _p(wd), p['ldw'], engine._ptr(o['z']), *_bn_args(engine, o, gd, bd, act, alpha, rd)) == 0, \
        L.yk_last_error()
    torch.cuda.synchronize()
    _z_exact_then_bn(o, bufs, p['z'], p['gamma'], p['beta'], act, alpha, p['res'])


# --------------------------------------------------------------------------------------------- implicit 3x3 convolutions
NOBN = [None, None, C.c_float(0), 0, C.c_float(0), None, None, None, None, None, C.c_float(0), None]


def _conv(c, lattice, run):
    """The calls of `run` that the case's channel counts and stride allow; the others must be refused on the host."""
    engine, L = _lib()
    geom, _ = gc.conv_geom(c)
    B, Hi, Wi, Ci, Ho, Wo = geom[:6]
    g = [C.c_int(v) for v in geom]
    M = B * Ho * Wo
    p = gc.conv_problem(c, lattice)
    xd, wd, dzd = _cu(p['x']), _cu(p['wd']), _cu(p['dz'])
    (z, zb), (dw, dwb), (dx, dxb) = _out(M, c.Co), _out(c.Co, 9 * Ci), _out(B, Hi, Wi, Ci)
    on = gc.conv_calls(c)
    if run['fwd']:
        assert L.yk_conv3x3_bn_fwd_f32(engine._ptr(xd), engine._ptr(wd), *g, c.Co, engine._ptr(z), *NOBN, _st()) == 0, L.yk_last_error()
    if run['bwd_weight']:
        assert L.yk_conv3x3_bwd_weight_f32(engine._ptr(xd), engine._ptr(dzd), *g, c.Co, engine._ptr(dw), _st()) == 0, L.yk_last_error()
    if run['bwd_data']:
        assert L.yk_conv3x3_bwd_data_f32(engine._ptr(dzd), engine._ptr(wd), *g, c.Co, engine._ptr(dx), _st()) == 0, L.yk_last_error()
    if not on['bwd_weight']:                                     # Co % 4 != 0: both gradients are refused
        assert L.yk_conv3x3_bwd_weight_f32(engine._ptr(xd), engine._ptr(dzd), *g, c.Co, engine._ptr(dw), _st()) == YK_ERR_UNSUPPORTED
        assert L.yk_conv3x3_bwd_data_f32(engine._ptr(dzd), engine._ptr(wd), *g, c.Co, engine._ptr(dx), _st()) == YK_ERR_UNSUPPORTED
    elif not on['bwd_data']:                                     # stride 2: the data gradient is refused
        assert L.yk_conv3x3_bwd_data_f32(engine._ptr(dzd), engine._ptr(wd), *g, c.Co, engine._ptr(dx), _st()) == YK_ERR_UNSUPPORTED
        assert b'stride' in L.yk_last_error()
    torch.cuda.synchronize()
    _tails_intact(zb, dwb, dxb)
    got = dict(fwd=z.cpu().numpy().reshape(B, Ho, Wo, c.Co), bwd_weight=dw.cpu().numpy(), bwd_data=dx.cpu().numpy())
    for call, key, bound in (('fwd', 'y', 'bound_y'), ('bwd_weight', 'dw', 'bound_dw'), ('bwd_data', 'dx', 'bound_dx')):
        if not run[call]:
            assert (got[call] == 12345.0).all(), call            # a refused call wrote nothing
            continue
        out = got[call].astype(np.float64)
        if lattice:
            assert np.array_equal(out, p[key]), (call, np.argwhere(out != p[key])[:4], out[out != p[key]][:4], p[key][out != p[key]][:4])
        else:
            err = np.abs(out - p[key])
            _margin(f'conv_{call}', key, _ratio(np.nan_to_num(err, nan=np.inf), p[bound]), gc.conv_id(c))
            assert (err <= p[bound]).all(), (call, np.argwhere(~(err <= p[bound]))[:4], float(np.nanmax(err / np.maximum(p[bound], 1e-300))))


@pytest.mark.parametrize('c', gc.CONV_CASES, ids=gc.conv_id)
def test_conv3x3_on_lattice_data_is_bitwise_the_float64_reference(c):
    assert gc.conv_problem(c, True)['abs_sum'] < 2 ** 24
    _conv(c, True, gc.conv_calls(c))


@pytest.mark.parametrize('c', [c for c in gc.CONV_CASES if any(gc.conv_normal_calls(c).values())], ids=gc.conv_id)
def test_conv3x3_on_normal_data_within_the_fp32_summation_bound(c):
    _conv(c, False, gc.conv_normal_calls(c))


@pytest.mark.parametrize('i', range(len(gc.CONV_BN_CASES)), ids=[gc.conv_id(c) for c in gc.CONV_BN_CASES])
def test_conv3x3_bn_forward_on_lattice_data(i):
    """yk_conv3x3_bn_fwd_f32 with BatchNorm: the STATS epilogue (105 rows: a ragged second tile) and the split route through
    splitk_sum_stats_kernel.  z bitwise the float64 convolution, the rest as for yk_gemm_bn_fwd_f32."""
    engine, L = _lib()
    c = gc.CONV_BN_CASES[i]
    geom, _ = gc.conv_geom(c)
    B, Hi, Wi, Ci, Ho, Wo = geom[:6]
    M = B * Ho * Wo
    act, alpha = tc.ACTS[(i + 1) % 4]
    p = gc.conv_problem(c, True)
    rng = np.random.default_rng(c.Co)
    gamma, beta, res = rng.uniform(0.5, 2, c.Co).astype(np.float32), rng.normal(size=c.Co).astype(np.float32), rng.normal(size=(M, c.Co)).astype(np.float32)
    res = res if i else None
    xd, wd, gd, bd, rd = _cu(p['x']), _cu(p['wd']), _cu(gamma), _cu(beta), (_cu(res) if res is not None else None)
    o, bufs = _bn_outs(M, c.Co)
    assert L.yk_conv3x3_bn_fwd_f32(engine._ptr(xd), engine._ptr(wd), *[C.c_int(v) for v in geom], c.Co, engine._ptr(o['z']),
                                   *_bn_args(engine, o, gd, bd, act, alpha, rd)) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _z_exact_then_bn(o, bufs, p['y'].reshape(M, c.Co), gamma, beta, act, alpha, res)

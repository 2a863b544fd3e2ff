"""Adaptive rounding on the GPU: the kernels of csrc/yk_adaround.hip against the float64 rule of adaround.py, adaround.gpu_optimise on the mini
network of tests/biascorrect_cases.py, and save_kmodel(adaround=True) on yolo_mobilev1-0.5 at 32 x 32 with 8 generated frames.

The step kernel's tolerance is measured, not derived: expf and powf of the device have documented errors of a few ulp, but the step divides by
sqrt(v) + 1e-8, which has no useful a-priori bound.  tests/adaround_cases.step_float32_figure restates the step in float32 numpy (statement by
statement what the kernel does) and compares it, on the CPU, with the float64 rule fed the same P on exactly the inputs below, over 3 steps.
Measured there, relative to the largest magnitude of each array: V 2.8e-07, m 4.2e-07, v 1.3e-05, D 2.3e-05.  The kernel is allowed FOUR
times that figure (the device's transcendental functions differ from numpy's by a few ulp each); the figure is recomputed when the test runs.

Like tests/test_gpu_yolo_biascorrect.py this file sorts behind tests/test_gpu_shared_weights.py, which compares differences of the device's free
memory a few 2 MiB blocks wide, and returns its memory to the driver when it is done."""
import ctypes as C

import numpy as np
import pytest

from k210_yolo_framework_amd import adaround, biascorrect, kmodel, netspec as ns, quantize
from tests import adaround_cases as ac

pytestmark = pytest.mark.gpu
U64, U32 = 2.0 ** -53, 2.0 ** -24
STEP_FACTOR = 4.0
YK_ERR_ARG = -10


@pytest.fixture(scope='module', autouse=True)
def _give_the_memory_back():
    """The tensors of this file are returned to the driver when it is done, so that later files meet the device as they did before it existed."""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---- yk_dw3x3_gram_f32 -------------------------------------------------------------------------------------------------------------------
def _gram_call(x, stride, pt, pl, ho, wo, G):
    import torch
    from k210_yolo_framework_amd import engine
    B, H, W, Cn = x.shape
    need = C.c_size_t()
    engine.call('yk_dw3x3_gram_workspace_bytes', B, ho, wo, Cn, C.byref(need))
    assert need.value % 8 == 0 and need.value >= 45 * 8 * Cn
    work = torch.full((need.value // 8,), float('nan'), dtype=torch.float64, device='cuda')           # contents undefined before: poison
    engine.call('yk_dw3x3_gram_f32', x, B, H, W, Cn, ho, wo, stride, pt, pl, G, work, _stream())


# (C, B, H, W, stride, pad_t, pad_l, pad_b, pad_r): 1 x 1, 5 x 7 and 8 x 8 inputs, the stride-2 padding whose bottom / right part is unused on
# an even size ((1, 1, 1, 1)) or absent at the top / left ((0, 0, 1, 1)), one chunk of rows, several, and 19200 rows: past the
# YK_DWGRAM_ROWS * YK_DWGRAM_MAX_CHUNKS = 16384 at which a chunk grows beyond 64 rows
GRAM_CASES = [(1, 1, 1, 1, 1, 1, 1, 1, 1), (3, 1, 5, 7, 1, 1, 1, 1, 1), (4, 3, 8, 8, 2, 1, 1, 1, 1), (5, 3, 5, 7, 2, 1, 1, 1, 1),
              (68, 1, 8, 8, 1, 1, 1, 1, 1), (68, 3, 8, 8, 2, 0, 0, 1, 1), (4, 1, 1, 1, 2, 1, 1, 1, 1), (5, 3, 8, 8, 1, 1, 1, 1, 1),
              (1, 3, 5, 7, 1, 1, 1, 1, 1), (3, 3, 80, 80, 1, 1, 1, 1, 1)]


@pytest.mark.parametrize('case', GRAM_CASES, ids=lambda c: 'C{}_B{}_{}x{}_s{}_p{}{}{}{}'.format(*c))
def test_dw_gram_against_float64_two_batches_accumulated_and_equal_bits(case):
    import torch
    Cn, B, H, W, stride, pt, pl, pb, pr = case
    rng = np.random.default_rng(Cn * 1000 + B * 100 + H)
    xs = [rng.normal(0.0, 1.0, (B, H, W, Cn)).astype(np.float32) for _ in range(2)]
    ho, wo = (H + pt + pb - 3) // stride + 1, (W + pl + pr - 3) // stride + 1
    M = B * ho * wo
    got = []
    for _ in range(2):
        G = torch.zeros((Cn, 9, 9), dtype=torch.float64, device='cuda')
        firsts = []
        for x in xs:                                                               # two batches accumulated
            _gram_call(_dev(x), stride, pt, pl, ho, wo, G)
            firsts.append(G.cpu().numpy().copy())
        got.append(firsts)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])               # two calls: equal bits
    want1 = ac.dw_gram(xs[0], stride, pt, pl, pb, pr)
    want2 = want1 + ac.dw_gram(xs[1], stride, pt, pl, pb, pr)
    abs1 = ac.dw_gram_abs(xs[0], stride, pt, pl, pb, pr)
    abs2 = abs1 + ac.dw_gram_abs(xs[1], stride, pt, pl, pb, pr)
    # every product is exact in float64: what is left is the float64 summation of n terms (+ the adds into the output), in any order
    for g, want, ab, n in ((got[0][0], want1, abs1, M + 1), (got[0][1], want2, abs2, 2 * M + 2)):
        err = np.abs(g - want)
        print(f'{case}: M {M}, worst error {err.max():.3g}, bound at it {(n * U64 * ab).flat[int(err.argmax())]:.3g}')
        assert (err <= n * U64 * ab).all()
        assert np.array_equal(g, g.transpose(0, 2, 1))                             # full symmetric, both halves from the same sums


# ---- the dense Gram path: yk_im2col3x3_f32 / the tensor itself into yk_gemm_f32(transA) ------------------------------------------------------
# (k, Ci, B, H, W, stride)
DENSE_CASES = [(1, 3, 1, 5, 7, 1), (1, 16, 3, 9, 11, 1), (1, 68, 2, 8, 8, 1), (3, 3, 2, 8, 8, 2), (3, 3, 1, 5, 7, 1), (3, 8, 3, 7, 9, 1),
               (3, 20, 2, 8, 8, 2)]


@pytest.mark.parametrize('case', DENSE_CASES, ids=lambda c: 'k{}_Ci{}_B{}_{}x{}_s{}'.format(*c))
def test_dense_gram_path_against_float64(case):
    import torch
    from k210_yolo_framework_amd import engine
    k, ci, B, H, W, stride = case
    x = np.random.default_rng(k * 100 + ci).normal(0.0, 1.0, (B, H, W, ci)).astype(np.float32)
    pad = (k - 1) // 2
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    M, K = B * ho * wo, k * k * ci
    xd = _dev(x)
    if k == 1:
        X = xd
    else:
        X = torch.empty((M, K), dtype=torch.float32, device='cuda')
        engine.call('yk_im2col3x3_f32', xd, B, H, W, ci, ho, wo, stride, pad, pad, X, _stream())
    G = torch.empty((K, K), dtype=torch.float32, device='cuda')
    engine.call('yk_gemm_f32', 1, 0, K, K, M, 1.0, X, K, X, K, 0.0, G, K, _stream())
    col = ac.columns(x, k, stride, pad, pad, pad, pad)
    assert col.shape == (M, K)
    want, ab = col.T @ col, np.abs(col).T @ np.abs(col)
    err = np.abs(G.cpu().numpy().astype(np.float64) - want)
    # an fp32 dot product of length M: every product and every add rounds once, |error| <= M 2^-24 sum |x_i x_j| (to first order; the
    # comparison's own float64 error is 2^-29 of that)
    bound = M * U32 * ab
    print(f'{case}: M {M}, K {K}, worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}')
    assert (err <= bound).all()


# ---- yk_adaround_step_f32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(ac.STEP_MODES))
@pytest.mark.parametrize('shape', ac.STEP_SHAPES, ids=lambda s: f'Co{s[0]}_K{s[1]}')
def test_step_after_1_and_3_steps_against_the_float64_rule_fed_the_devices_own_p(shape, mode):
    import torch
    from k210_yolo_framework_amd import engine
    Co, K = shape
    lam, beta = ac.STEP_MODES[mode]
    case = ac.step_case(Co, K)
    figure = ac.step_float32_figure()
    V, r, D, inv_e = (_dev(case[k]) for k in ('V', 'r', 'D', 'inv_e'))
    m, v, P = torch.zeros_like(V), torch.zeros_like(V), torch.empty_like(V)
    frozen = _dev(case['frozen'], np.uint8)
    G32 = _dev(case['G'])
    used, got = [], []
    for t in range(3):
        engine.call('yk_gemm_f32', 0, 0, Co, K, K, 1.0, D, K, G32, K, 0.0, P, K, _stream())
        used.append(P.cpu().numpy().astype(np.float64))
        engine.call('yk_adaround_step_f32', V, m, v, r, frozen, P, inv_e, D, Co, K, case['n_free'], case['s_w'], lam, beta, ac.STEP_LR, t + 1,
                    _stream())
        got.append(tuple(a.cpu().numpy().astype(np.float64) for a in (V, m, v, D)))
    want, _ = ac.run_steps(case, lam, beta, 3, np.float64, used)
    fz = case['frozen']
    for t in (0, 2):
        for k, what in enumerate(('V', 'm', 'v', 'D')):
            assert np.isfinite(got[t][k]).all()
            tol = STEP_FACTOR * figure[k] * float(np.abs(want[t][k]).max())
            err = float(np.abs(got[t][k] - want[t][k]).max())
            print(f'{shape} {mode} step {t + 1} {what}: error {err:.3g}, allowed {tol:.3g}')
            assert err <= tol, (what, t)
        assert np.array_equal(got[t][0][fz], case['V'].astype(np.float32)[fz]) and not got[t][3][fz].any()       # frozen: V kept, D = 0
        clipped = np.abs(case['V']) == 20.0
        assert np.array_equal(got[t][0][clipped], case['V'][clipped])                                         # h clipped: no gradient, V kept


# ---- yk_adaround_dw_quad_f32, yk_adaround_rowerr_f64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cn', [1, 3, 29, 68, 300])
def test_dw_quad_against_float64(Cn):
    import torch
    from k210_yolo_framework_amd import engine
    rng = np.random.default_rng(Cn)
    A = rng.normal(0.0, 1.0, (Cn, 12, 9))
    G = np.einsum('cmi,cmj->cij', A, A)
    D = rng.normal(0.0, 0.01, (Cn, 9)).astype(np.float32)
    P = torch.empty((Cn, 9), dtype=torch.float32, device='cuda')
    engine.call('yk_adaround_dw_quad_f32', _dev(G, np.float64), _dev(D), Cn, P, _stream())
    want = adaround.quad(D.astype(np.float64), G)
    ab = adaround.quad(np.abs(D).astype(np.float64), np.abs(G))
    # 9 float64 products and adds, then one rounding to fp32
    assert (np.abs(P.cpu().numpy().astype(np.float64) - want) <= 10 * U64 * ab + U32 * np.abs(want)).all()


@pytest.mark.parametrize('shape', [(1, 1), (3, 9), (2, 63), (5, 65), (3, 257), (2, 1000)], ids=lambda s: f'Co{s[0]}_K{s[1]}')
def test_rowerr_against_float64_to_the_summation_bound_and_equal_bits(shape):
    import torch
    from k210_yolo_framework_amd import engine
    Co, K = shape
    rng = np.random.default_rng(K)
    D, P = rng.normal(0.0, 1.0, (Co, K)).astype(np.float32), rng.normal(0.0, 1.0, (Co, K)).astype(np.float32)
    out = []
    for _ in range(2):
        E = torch.full((Co,), float('nan'), dtype=torch.float64, device='cuda')
        engine.call('yk_adaround_rowerr_f64', _dev(D), _dev(P), Co, K, E, _stream())
        out.append(E.cpu().numpy())
    terms = D.astype(np.float64) * P.astype(np.float64)                                                       # exact
    assert np.array_equal(out[0], out[1])
    assert (np.abs(out[0] - terms.sum(1)) <= K * U64 * np.abs(terms).sum(1)).all()


def test_bad_arguments_are_refused_before_anything_is_launched():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    f = torch.zeros(64, dtype=torch.float32, device='cuda')
    d, dwork = (torch.zeros(128, dtype=torch.float64, device='cuda') for _ in range(2))
    u = torch.zeros(64, dtype=torch.uint8, device='cuda')
    need = C.c_size_t()
    s = _stream()
    assert L.yk_dw3x3_gram_workspace_bytes(1, 2, 2, 1, None) == YK_ERR_ARG
    for sizes in ((0, 2, 2, 1), (1, 0, 2, 1), (1, 2, 0, 1), (1, 2, 2, 0)):
        assert L.yk_dw3x3_gram_workspace_bytes(*sizes, C.byref(need)) == YK_ERR_ARG
    good = [f, 1, 2, 2, 1, 2, 2, 1, 1, 1, d, dwork, s]
    assert L.yk_dw3x3_gram_f32(*good) == 0
    for at in (0, 10, 11):
        assert L.yk_dw3x3_gram_f32(*[None if i == at else a for i, a in enumerate(good)]) == YK_ERR_ARG
    for at in (1, 2, 3, 4, 5, 6, 7):
        assert L.yk_dw3x3_gram_f32(*[0 if i == at else a for i, a in enumerate(good)]) == YK_ERR_ARG
    good = [f, f, f, f, u, f, f, f, 2, 3, 6, 0.01, 0.01, 2.0, 0.01, 1, s]
    assert L.yk_adaround_step_f32(*good) == 0
    for at in range(8):
        assert L.yk_adaround_step_f32(*[None if i == at else a for i, a in enumerate(good)]) == YK_ERR_ARG
    for at in (8, 9, 10, 15):
        assert L.yk_adaround_step_f32(*[0 if i == at else a for i, a in enumerate(good)]) == YK_ERR_ARG
    good = [d, f, 1, f, s]
    assert L.yk_adaround_dw_quad_f32(*good) == 0
    for at in (0, 1, 3):
        assert L.yk_adaround_dw_quad_f32(*[None if i == at else a for i, a in enumerate(good)]) == YK_ERR_ARG
    assert L.yk_adaround_dw_quad_f32(d, f, 0, f, s) == YK_ERR_ARG
    good = [f, f, 2, 3, d, s]
    assert L.yk_adaround_rowerr_f64(*good) == 0
    for at in (0, 1, 4):
        assert L.yk_adaround_rowerr_f64(*[None if i == at else a for i, a in enumerate(good)]) == YK_ERR_ARG
    for at in (2, 3):
        assert L.yk_adaround_rowerr_f64(*[0 if i == at else a for i, a in enumerate(good)]) == YK_ERR_ARG
    torch.cuda.synchronize()


# ---- gpu_optimise on the mini case the CPU test vetted -------------------------------------------------------------------------------------
def test_gpu_optimise_on_the_mini_network():
    import torch
    spec, w, fr, G_np = ac.mini_case()
    frames = np.array(fr)
    codes, rep = adaround.gpu_optimise(spec, w, frames, batch=2, iters=ac.MINI_ITERS, lam=ac.MINI_LAMBDA, lr=ac.MINI_LR, report_every=50)
    G_dev, skipped = adaround.gpu_grams(spec, w, frames, batch=2)                     # 3 frames in batches of 2 and 1; the same calls: the same bits
    assert not skipped and set(codes) == {l.name for l in spec.layers} == set(rep['layers'])
    twin = ac.mini_optimised()
    improved = {ns.OP_CONV: 0, ns.OP_DWCONV: 0}
    for op in spec.ops:
        if op['type'] not in (ns.OP_CONV, ns.OP_DWCONV):
            continue
        name, dw = op['layer'], op['type'] == ns.OP_DWCONV
        kern = np.asarray(w[name + '/kernel'], np.float64)
        st = adaround.setup(kern)
        lo, hi = adaround.allowed_codes(kern)
        c = codes[name]
        assert c.dtype == np.uint8 and c.shape == kern.shape and ((c == lo) | (c == hi)).all(), name        # every code a down or an up code
        assert np.array_equal(c[st['frozen']], st['nearest'][st['frozen']]), name                          # frozen weights at nearest
        G = G_dev[name].cpu().numpy()
        rows, crow = adaround.rows_of(kern, dw), adaround.rows_of(c, dw)
        rst = adaround.setup(rows)
        e_near = adaround.row_errors(adaround.hard_error(rst['nearest'], rst), G)
        e_new = adaround.row_errors(adaround.hard_error(crow, rst), G)
        info = rep['layers'][name]
        assert np.array_equal(info['e_rows_nearest'], e_near) and info['e_nearest'] == float(e_near.sum())    # float64 from the device Gram
        assert (e_new <= e_near).all() and info['e_adaround'] == float(e_new.sum()), name
        assert info['flipped'] == int((c != st['nearest']).sum()) and info['rows_changed'] == int((e_new < e_near).sum())
        assert not info['skipped'] and info['frozen'] == int(st['frozen'].sum()) and info['soft'][-1][0] == ac.MINI_ITERS
        improved[op['type']] += int((e_new < e_near).sum())
        print(f"{name}: GPU E {info['e_nearest']:.6g} -> {info['e_adaround']:.6g} ({info['flipped']} flipped), numpy twin "
              f"{twin[name][1]['e_nearest']:.6g} -> {twin[name][1]['e_adaround']:.6g} ({twin[name][1]['flipped']} flipped)")
    assert improved[ns.OP_CONV] >= 1 and improved[ns.OP_DWCONV] >= 1, improved
    # conv1 reads the frames themselves (exact in fp32 up to the rounding of x / 255), so its device Gram matrix differs from numpy's only by
    # the fp32 dot product of length M and the two roundings of each input (the scale 1 / 255, the product): E(nearest) within
    # sum |d_i| |d_j| (M + 4) 2^-24 sum |x_i x_j|
    op = spec.ops[0]
    col = ac.columns(frames.astype(np.float64) * quantize.INPUT_SCALE, 3, op['stride'], op['pad_t'], op['pad_l'], op.get('pad_b', op['pad_t']),
                     op.get('pad_r', op['pad_l']))
    rst = adaround.setup(adaround.rows_of(np.asarray(w['conv1/kernel'], np.float64), False))
    d = np.abs(adaround.hard_error(rst['nearest'], rst))
    bound = (len(col) + 4) * U32 * ((d @ (np.abs(col).T @ np.abs(col))) * d).sum(1)
    assert (np.abs(rep['layers']['conv1']['e_rows_nearest'] - twin['conv1'][1]['e_rows_nearest']) <= bound).all()
    # a cap below a layer's need leaves it at nearest and names it
    codes2, rep2 = adaround.gpu_optimise(spec, w, frames, batch=2, iters=2, max_gram_mb=0.004)             # 4 KiB: K <= 22
    left = {n for n, r in rep2['layers'].items() if r['skipped']}
    assert left and left == {op['layer'] for op in spec.ops if op['type'] == ns.OP_CONV and (op['k'] ** 2 * op['cin']) ** 2 * 8 > 0.004 * 2 ** 20
                             } | {op['layer'] for op in spec.ops if op['type'] == ns.OP_DWCONV and op['cout'] * 81 * 8 > 0.004 * 2 ** 20}
    assert not left & set(codes2) and 'SKIPPED' in adaround.format_report(rep2)
    torch.cuda.synchronize()


# ---- save_kmodel(adaround=True) ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_yolo():
    from k210_yolo_framework_amd import yolonet
    model, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 20, alpha=0.5)
    model.set_weights(model.spec.init_weights(seed=3))
    frames = quantize.synthetic_frames(8, (32, 32), seed=4)
    return model, frames


ADA = dict(adaround=True, ada_iters=100, ada_lr=5e-2)


def test_save_kmodel_adaround_moves_weight_bytes_by_one_and_nothing_else(small_yolo, tmp_path):
    from k210_yolo_framework_amd import yolonet
    model, frames = small_yolo
    spec, w = model.spec, model.get_weights()
    off, off2, on = (str(tmp_path / n) for n in ('off.kmodel', 'off2.kmodel', 'on.kmodel'))
    rep_off = model.save_kmodel(off, frames, batch=8, adaround=False)
    model.save_kmodel(off2, frames, batch=8)
    rep_on = model.save_kmodel(on, frames, batch=8, **ADA)
    a, a2, b = (open(p, 'rb').read() for p in (off, off2, on))
    want, _ = quantize.quantize(spec, w, quantize.calibrate(spec, w, frames, 8))
    assert a == a2 == kmodel.serialise(want)                                                  # off: the bytes of the unchanged functions
    assert 'adaround' not in rep_off and 'adaround ' not in quantize.format_report(rep_off)
    ka, kb = kmodel.parse(a), kmodel.parse(b)
    moved = 0
    for la, lb in zip(ka.convs, kb.convs):
        diff = lb.weights.astype(np.int64) - la.weights.astype(np.int64)
        assert np.abs(diff).max() <= 1, la.index                                              # +-1 per weight
        moved += int((diff != 0).sum())
    ab, bb = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    assert len(ab) == len(bb)
    assert moved > 0 and int((ab != bb).sum()) == moved                                       # every other byte is equal
    arep = rep_on['adaround']
    assert moved == sum(r['flipped'] for r in arep['layers'].values()) and set(arep['layers']) == {l.name for l in spec.layers}
    assert all(r['e_adaround'] <= r['e_nearest'] for r in arep['layers'].values())
    text = quantize.format_report(rep_on)
    assert text.count('adaround ') == len(spec.layers) and 'adaptive rounding:' in text
    print(text[text.index('adaround '):].split('main memory')[0])
    fresh, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 20, alpha=0.5, precision='kpu')
    fresh.load_weights(on)
    outs = fresh.predict(frames[:2])
    assert len(outs) == 2 and all(np.isfinite(o).all() for o in outs)


def test_save_kmodel_adaround_with_bias_correct_keeps_the_residual_bound(small_yolo, tmp_path):
    model, frames = small_yolo
    spec, w = model.spec, model.get_weights()
    on = str(tmp_path / 'both.kmodel')
    rep = model.save_kmodel(on, frames, batch=8, bias_correct=True, **ADA)
    brep = rep['biascorrect']
    fm = quantize.calibrate_means(spec, w, frames, 8)
    res = biascorrect.residuals(rep, fm, biascorrect.gpu_measure(frames, 8)(kmodel.parse(open(on, 'rb').read())))
    worst = {}
    for name, v in res.items():
        keep = np.setdiff1d(np.arange(len(v)), brep['layers'][name]['limited'])
        worst[name] = float(v[keep].max())
    print('residuals with adaround + bias correction', worst)
    assert set(res) == {l.name for l in spec.layers}
    assert max(worst.values()) <= 0.5 + 1e-6                                                  # the bound of tests/test_gpu_yolo_biascorrect.py
    assert sum(len(r['limited']) for r in brep['layers'].values()) <= 2
    assert sum(r['flipped'] for r in rep['adaround']['layers'].values()) > 0

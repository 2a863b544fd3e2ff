"""The kernels of csrc/yk_adaround.hip on the inputs of tests/adaround_edge_cases.py and adaround_cases.step_edge_case, which
tests/test_adaround_edge_cases.py vets on the CPU: yk_dw3x3_gram_f32 with several chunks of rows AND several groups of 64 channels at once
(the partial index (chunk * 45 + e) * C + c with chunk >= 1 and c >= 64), a last chunk of 1, 2 and 4 rows, chunks grown to 65 rows on two
groups, stride 2 on odd sizes with more than 64 channels; yk_adaround_step_f32 at V == 0 exactly, at K = 1 across a workgroup boundary, on
tensors with nothing and with everything frozen and at t = 10000; yk_adaround_rowerr_f64 at K = 255, 256, 512 and on 70000 rows.

The Gram and row-error bounds are the derived ones of tests/test_gpu_yolo_adaround.py.  The step kernel's tolerance is measured the way that
file measures it, on exactly the inputs below: adaround_cases.step_edge_figure restates the step in float32 numpy and compares it on the CPU
with the float64 rule fed the same P, over 3 steps from each case's first t, the worst over the four cases and four modes.  Measured there,
relative to the largest magnitude of each array: V 1.3e-07, m 4.2e-07, v 1.3e-05, D 4.2e-07.  The kernel is allowed STEP_FACTOR = 4 times that
figure, which is recomputed when the test runs.  Beside the tolerance four properties are exact: every output is finite; where V == 0 and
P == 0 the gradient is exactly 0 and m, v and V keep their bits; frozen elements keep V, m and v and get D = 0; a tensor with everything frozen
comes back with m and v untouched.

Like tests/test_gpu_yolo_adaround.py this file sorts behind tests/test_gpu_shared_weights.py, which compares differences of the device's free
memory a few 2 MiB blocks wide, and returns its memory to the driver when it is done."""
import numpy as np
import pytest

from tests import adaround_cases as ac
from tests import adaround_edge_cases as ae
from tests.test_gpu_yolo_adaround import STEP_FACTOR, U32, U64, _dev, _gram_call, _stream

pytestmark = pytest.mark.gpu
assert U64 == ae.U64 and U32 == 2.0 ** -24


@pytest.fixture(scope='module', autouse=True)
def _give_the_memory_back():
    """The tensors of this file are returned to the driver when it is done, so that later files meet the device as they did before it existed."""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- yk_dw3x3_gram_f32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c, _ in ae.GRAM_EDGES], ids=ae.GRAM_IDS)
def test_dw_gram_on_several_chunks_and_groups_against_float64_two_batches_accumulated_and_equal_bits(case):
    import torch
    Cn, B, H, W, stride, pt, pl, pb, pr = case
    xs = ae.gram_inputs(case)
    ho, wo = ae.out_hw(case)
    M = B * ho * wo
    got = []
    for _ in range(2):
        G = torch.zeros((Cn, 9, 9), dtype=torch.float64, device='cuda')
        firsts = []
        for x in xs:                                                               # two batches accumulated
            _gram_call(_dev(x), stride, pt, pl, ho, wo, G)                         # (its workspace is NaN before the call)
            firsts.append(G.cpu().numpy().copy())
        got.append(firsts)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])               # two calls: equal bits
    want1 = ac.dw_gram(xs[0], stride, pt, pl, pb, pr)
    want2 = want1 + ac.dw_gram(xs[1], stride, pt, pl, pb, pr)
    abs1 = ac.dw_gram_abs(xs[0], stride, pt, pl, pb, pr)
    abs2 = abs1 + ac.dw_gram_abs(xs[1], stride, pt, pl, pb, pr)
    # every product is exact in float64: what is left is the float64 summation of n terms (+ the adds into the output), in any order
    for g, want, ab, n in ((got[0][0], want1, abs1, M + 1), (got[0][1], want2, abs2, 2 * M + 2)):
        assert np.isfinite(g).all()
        err = np.abs(g - want)
        print(f'{case}: M {M}, worst error {err.max():.3g}, bound at it {(n * U64 * ab).flat[int(err.argmax())]:.3g}')
        assert ae.within_bound(g, want, ab, n)
        assert np.array_equal(g, g.transpose(0, 2, 1))                             # full symmetric, both halves from the same sums


# ---- yk_adaround_step_f32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(ac.STEP_MODES))
@pytest.mark.parametrize('kind', ac.STEP_EDGES)
def test_step_on_edge_inputs_against_the_float64_rule_fed_the_devices_own_p(kind, mode):
    import torch
    from k210_yolo_framework_amd import engine
    lam, beta = ac.STEP_MODES[mode]
    case = ac.step_edge_case(kind)
    Co, K = case['V'].shape
    t0 = case['first_t']
    figure = ac.step_edge_figure()
    zero = np.zeros_like(case['V'])
    V, r, D, inv_e, m, v = (_dev(a) for a in (case['V'], case['r'], case['D'], case['inv_e'], case.get('m', zero), case.get('v', zero)))
    P = torch.empty_like(V)
    V0, m0, v0 = (a.cpu().numpy() for a in (V, m, v))
    frozen = _dev(case['frozen'], np.uint8)
    G32 = _dev(case['G'])
    p_zero = torch.from_numpy(case['p_zero']).cuda() if 'p_zero' in case else None
    used, got = [], []
    for t in range(3):
        engine.call('yk_gemm_f32', 0, 0, Co, K, K, 1.0, D, K, G32, K, 0.0, P, K, _stream())
        if p_zero is not None:
            P[p_zero] = 0.0
        used.append(P.cpu().numpy().astype(np.float64))
        engine.call('yk_adaround_step_f32', V, m, v, r, frozen, P, inv_e, D, Co, K, case['n_free'], case['s_w'], lam, beta, ac.STEP_LR, t0 + t, _stream())
        got.append(tuple(a.cpu().numpy() for a in (V, m, v, D)))
    want, _ = ac.run_steps(case, lam, beta, 3, np.float64, used, first_t=t0)
    fz = case['frozen']
    for t in (0, 2):
        for k, what in enumerate(('V', 'm', 'v', 'D')):
            assert np.isfinite(got[t][k]).all(), (what, t)
            tol = STEP_FACTOR * figure[k] * float(np.abs(want[t][k]).max())
            err = float(np.abs(got[t][k].astype(np.float64) - want[t][k]).max())
            print(f'{kind} {mode} step {t0 + t} {what}: error {err:.3g}, allowed {tol:.3g}')
            assert err <= tol, (what, t)
        Vt, mt, vt, Dt = (a.view(np.int32) for a in got[t])
        # frozen: V, m and v keep their bits, D = 0 (with everything frozen that is the whole tensor)
        assert np.array_equal(Vt[fz], V0.view(np.int32)[fz]) and np.array_equal(mt[fz], m0.view(np.int32)[fz]) and np.array_equal(vt[fz], v0.view(np.int32)[fz])
        assert not Dt[fz].any()
        if kind == 'zeros':                                                        # V == 0 and P == 0: the gradient is exactly 0
            still = case['p_zero'] & ~fz
            assert still.sum() == 3 and not Vt[still].any() and not mt[still].any() and not vt[still].any()
    if kind == 'zeros':
        moved = ~fz & ~case['p_zero'] & (case['V'] == 0.0)
        assert moved.sum() == 4 and (got[0][0][moved] != 0).all()                  # the other zeros, with P != 0, do move
    if kind == 'rows_of_one':
        assert (got[0][0] != V0).mean() > 0.5


# ---- yk_adaround_rowerr_f64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ae.ROWERR_EDGES, ids=lambda s: f'Co{s[0]}_K{s[1]}')
def test_rowerr_on_the_strides_of_256_and_past_65535_rows_to_the_summation_bound_and_equal_bits(shape):
    import torch
    from k210_yolo_framework_amd import engine
    Co, K = shape
    D, P = ae.rowerr_inputs(Co, K)
    out = []
    for _ in range(2):
        E = torch.full((Co,), float('nan'), dtype=torch.float64, device='cuda')
        engine.call('yk_adaround_rowerr_f64', _dev(D), _dev(P), Co, K, E, _stream())
        out.append(E.cpu().numpy())
    terms = D.astype(np.float64) * P.astype(np.float64)                                                       # exact
    assert np.array_equal(out[0], out[1])
    assert (np.abs(out[0] - terms.sum(1)) <= K * U64 * np.abs(terms).sum(1)).all()

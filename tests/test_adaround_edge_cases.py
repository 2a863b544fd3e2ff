"""tests/adaround_edge_cases.py and adaround_cases.step_edge_case checked on their own, without a GPU.

  * every Gram case reaches what it is in the table for, by gram_split restated from YK_DWGRAM_ROWS and YK_DWGRAM_MAX_CHUNKS of
    include/yolo_hip.h, and yk_dw3x3_gram_workspace_bytes (host code: no device needed) asks for 8 * 45 * chunks * C bytes;
  * the test of the test, as tests/test_x2_bound.py: the bound of the Gram test, n * 2^-53 * sum |x_i x_j|, is n times wider than one
    rounding, so it is shown to ACCEPT the sums taken in the kernels' order and to REJECT the float64 reference damaged the way each index
    mistake the first case is there for would damage it;
  * the step cases hold the values they claim (V exactly 0 where h is exactly 0.5 in float32, K = 1 past one workgroup, everything frozen,
    c1 and c2 about 1 at t = 10000), and the float32 restatement of the step has the exact properties the kernel is then held to;
  * the row-error shapes sit on the strides of 256 threads and past 65535 rows."""
import ctypes as C

import numpy as np
import pytest

from k210_yolo_framework_amd import adaround
from tests import adaround_cases as ac
from tests import adaround_edge_cases as ae


@pytest.fixture(scope='module')
def lib():
    from k210_yolo_framework_amd import engine
    if not engine.library_path().exists():
        import __graft_entry__ as g
        g.build()
    return engine.lib()


# ---- yk_dw3x3_gram_f32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case, reaches', ae.GRAM_EDGES, ids=ae.GRAM_IDS)
def test_gram_case_reaches_what_it_is_in_the_table_for(case, reaches, lib):
    Cn, B, H, W, stride, pt, pl, pb, pr = case
    rows, most = ae.define('YK_DWGRAM_ROWS'), ae.define('YK_DWGRAM_MAX_CHUNKS')
    ho, wo = ae.out_hw(case)
    M = B * ho * wo
    rpc, chunks = ae.gram_split(M)
    groups = -(-Cn // 64)
    last = M - (chunks - 1) * rpc
    assert dict(M=M, chunks=chunks, groups=groups, last=last, grown=rpc > rows) == {k: v for k, v in reaches.items() if k != 'pad_read'}
    assert chunks >= 2 and groups >= 2 and 0 < last <= rpc and chunks <= most           # both grid dimensions above 1 at once
    assert (M > rows * most) == reaches['grown']
    if reaches['grown']:
        assert rpc == rows + 1 and M % rpc and last < 4                                # chunks of 65 rows, the last one ragged
    if stride == 2:
        assert H % 2 and W % 2 and 'pad_read' in reaches
        read = ((ho - 1) * 2 - pt + 2 >= H, (wo - 1) * 2 - pl + 2 >= W)                # the last window's last tap lies in the padding
        assert read == (reaches['pad_read'],) * 2 and (pt, pl) == ((1, 1) if reaches['pad_read'] else (0, 0))
    need = C.c_size_t()
    assert lib.yk_dw3x3_gram_workspace_bytes(B, ho, wo, Cn, C.byref(need)) == 0
    assert need.value == 8 * 45 * chunks * Cn
    assert B * H * W * Cn * 4 <= 4.5e6                                                  # the largest input is 4.3 MB


def test_gram_table_holds_each_of_the_paths():
    r = [x for _, x in ae.GRAM_EDGES]
    assert any(x['last'] == 1 and x['groups'] == 3 for x in r)                          # row lanes 1 .. 3 idle, three groups
    assert any(x['last'] == 4 and c[0] % 64 == 0 for c, x in ae.GRAM_EDGES)             # exactly four rows, exactly two groups
    assert [x.get('pad_read') for x in r if 'pad_read' in x] == [True, False]
    assert sum(x['grown'] for x in r) == 1


@pytest.fixture(scope='module')
def first_case():
    case, reaches = ae.GRAM_EDGES[0]
    Cn, B, H, W, stride, *pads = case
    x = ae.gram_inputs(case)[0]
    win = ae.taps(x, stride, *pads)
    M = win.shape[1]
    assert M == reaches['M'] and Cn == 65
    want, ab = ac.dw_gram(x, stride, *pads), ac.dw_gram_abs(x, stride, *pads)
    rpc, chunks = ae.gram_split(M)
    return win, want, ab, M, rpc


def test_bound_accepts_the_sums_in_the_kernels_order(first_case):
    win, want, ab, M, rpc = first_case
    assert np.array_equal(ae.gram_of_rows(win, np.arange(M)), want) and np.array_equal(ae.gram_of_rows(np.abs(win), np.arange(M)), ab)
    model = ae.gram_in_kernel_order(win, rpc)
    err = np.abs(model - want) / np.maximum((M + 1) * ae.U64 * ab, 1e-300)
    print(f'kernel-order sums against the reference: worst error / bound {err.max():.3g}')
    assert ae.within_bound(model, want, ab, M + 1)
    assert err.max() <= 0.25                                                            # with room: the bound is not met by a hair


@pytest.mark.parametrize('damage', ['second_chunk_dropped_from_channel_64_on', 'second_chunk_of_channel_c_added_to_c_minus_64', 'last_row_dropped'])
def test_bound_rejects_the_damaged_reference(first_case, damage):
    win, want, ab, M, rpc = first_case
    second = ae.gram_of_rows(win, np.arange(rpc, M))                                   # chunk 1: rows 64 .. 80
    bad = want.copy()
    if damage == 'second_chunk_dropped_from_channel_64_on':                           # blockIdx.x >= 1 with blockIdx.y >= 1 never stored, or never read
        bad[64:] -= second[64:]
        hit = slice(64, None)
    elif damage == 'second_chunk_of_channel_c_added_to_c_minus_64':                   # the chunk stride taken for 64 instead of C
        bad[0:1] += second[64:65]
        hit = slice(0, 1)
    else:                                                                             # m1 one short
        bad -= ae.gram_of_rows(win, np.arange(M - 1, M))
        hit = slice(None)
    assert not ae.within_bound(bad, want, ab, M + 1)
    over = np.abs(bad - want)[hit] / ((M + 1) * ae.U64 * ab[hit])
    print(f'{damage}: smallest error / bound at the squared centre tap of the channels hit {over[:, 4, 4].min():.3g}')
    assert (over[:, 4, 4] > 1e6).all()                                                 # the centre tap is never padding: every channel hit shows it, by far
    untouched = np.ones(len(want), bool)
    untouched[hit] = False
    assert ae.within_bound(bad[untouched], want[untouched], ab[untouched], M + 1)


# ---- yk_adaround_step_f32 ----------------------------------------------------------------------------------------------------------------
def test_step_edge_cases_hold_what_they_claim():
    F = np.float32
    z = ac.step_edge_case('zeros')
    base = ac.step_case(3, 86)
    assert (z['V'][0, :8] == 0.0).all() and np.array_equal(z['V'].ravel()[8:], base['V'].ravel()[8:]) and z['first_t'] == 1
    V32 = z['V'].astype(F)
    h = adaround.h_of(V32)
    assert (h[0, :8] == F(0.5)).all() and (F(2) * h[0, :8] - F(1) == 0).all()           # float32: h = 0.5, x = 0, |x| = 0, sign 0
    assert z['p_zero'].sum() == 4 and z['p_zero'][0, :4].all() and z['frozen'][0, 1] and not z['frozen'][0, [0, 2, 3]].any()
    assert z['frozen'].any() and not z['frozen'].all() and z['n_free'] == int((~z['frozen']).sum())
    assert np.array_equal(z['D'], np.where(z['frozen'], 0.0, z['s_w'] * (adaround.h_of(z['V']) - z['r'])))
    late = ac.step_edge_case('zeros_late')
    assert late['first_t'] == 10000 and np.array_equal(late['V'], z['V']) and (late['m'][late['frozen']] != 0).all() and (late['v'] >= 0).all()
    assert (late['m'] != 0).mean() > 0.7 and (late['v'][late['frozen']] > 0).all()
    assert F(1.0 - 0.9 ** 10000) == 1 and abs(F(1.0 - 0.999 ** 10000) - 1) < 1e-4         # c1 = 1, c2 = 1 - 4.5e-5
    one = ac.step_edge_case('rows_of_one')
    assert one['V'].shape == (300, 1) and 300 > 256 and not one['frozen'].any() and one['n_free'] == 300 and len(set(one['inv_e'].tolist())) == 300
    allf = ac.step_edge_case('all_frozen')
    assert allf['V'].shape == (2, 129) and allf['frozen'].all() and not allf['D'].any() and allf['n_free'] == 1 and (allf['m'] != 0).all() and (allf['v'] > 0).all()
    assert np.array_equal(ac.step_case(3, 86)['V'], base['V'])                          # step_case gives what it gave


@pytest.mark.parametrize('mode', list(ac.STEP_MODES))
@pytest.mark.parametrize('kind', ac.STEP_EDGES)
def test_float32_restatement_has_the_exact_properties_the_kernel_is_held_to(kind, mode):
    F = np.float32
    lam, beta = ac.STEP_MODES[mode]
    case = ac.step_edge_case(kind)
    states, used = ac.run_steps(case, lam, beta, 3, F, first_t=case['first_t'])
    fz = case['frozen']
    V0, m0, v0 = case['V'].astype(F), case.get('m', np.zeros_like(case['V'])).astype(F), case.get('v', np.zeros_like(case['V'])).astype(F)
    for (V, m, v, D), P in zip(states, used):
        assert all(np.isfinite(a).all() for a in (V, m, v, D))
        assert np.array_equal(V[fz], V0[fz]) and not D[fz].any() and np.array_equal(m[fz], m0[fz]) and np.array_equal(v[fz], v0[fz])
        if 'p_zero' in case:
            assert not P[case['p_zero']].any()
    if kind == 'zeros':                                                                 # V = 0, P = 0: the gradient is exactly 0, nothing moves
        still = case['p_zero'] & ~fz
        assert still.sum() == 3
        for V, m, v, D in states:
            assert not V[still].any() and not np.signbit(V[still]).any() and not m[still].any() and not v[still].any()
        moved = ~fz & ~case['p_zero'] & (case['V'] == 0.0)
        assert moved.sum() == 4 and (states[0][0][moved] != 0).all()                    # the other zeros, with P != 0, do move
    if kind == 'rows_of_one':
        assert (states[0][0] != V0).mean() > 0.5


def test_step_edge_figure_is_measured_and_printed():
    fig = ac.step_edge_figure()
    print('float32 restatement against the float64 rule on the edge cases (V, m, v, D):', ' '.join(f'{x:.3g}' for x in fig))
    assert all(0 < x < 1e-4 for x in fig)
    assert np.allclose(ac.step_float32_figure(), (2.8e-07, 4.2e-07, 1.3e-05, 2.3e-05), rtol=0.05)     # the existing test's figure is what its docstring records


# ---- yk_adaround_rowerr_f64 --------------------------------------------------------------------------------------------------------------
def test_rowerr_shapes_sit_on_the_strides():
    ks = [K for _, K in ae.ROWERR_EDGES]
    assert 255 in ks and 256 in ks and 512 in ks and all(K % 256 in (255, 0) or Co > 65535 for Co, K in ae.ROWERR_EDGES)
    assert max(Co for Co, _ in ae.ROWERR_EDGES) > 65535
    D, P = ae.rowerr_inputs(2, 512)
    assert D.shape == P.shape == (2, 512) and D.dtype == np.float32 and not np.array_equal(D, P)

"""tests/gemm_cases.py checked on its own, without a GPU: the planner copies give the values they were written down for, the case tables
reach every path and edge they name, the lattice data stays exact in fp32, the float64 convolution reference agrees with an explicit
column matrix, and the buffer builder puts the spare float and the guard columns where it says."""
import numpy as np
import pytest

from tests import gemm_cases as gc
from tests import train_cases as tc


# ------------------------------------------------------------------------------------------------ the planner copies
def test_planner_copies_give_the_split_counts_the_cases_were_chosen_for():
    want = {(5, 3, 112): (1, 0), (5, 3, 113): (2, 0), (8, 8, 288): (4, 1), (5, 3, 1008): (15, 4), (5, 3, 1009): (16, None), (256, 256, 1024): (16, 0),
            (257, 256, 1024): (16, 0), (3, 5, 32768): (512, 0), (3, 5, 32752): (511, 169)}
    assert set(want) == set(gc.SPLIT_SHAPES)
    for (M, N, K), (s, empty) in want.items():
        assert gc.gemm_splits(M, N, K) == s, (M, N, K)
        if empty is not None:
            assert gc.k_slices(K, s)[1] == empty, (M, N, K)
    # K = 288 on a small result: 9 k-tiles at 3 per slice, the fourth slice is empty
    assert gc.k_slices(288, 4)[0] == [(0, 3), (3, 6), (6, 9), (9, 9)]
    # the TT kernel walks k-steps of 16: 63 of them at 5 per slice leave 2 of the 15 slices empty
    assert gc.k_slices(1008, 15, 16)[1] == 2
    assert gc.finishing_pass(5, 3, 1) == 'none' and gc.finishing_pass(5, 3, 15) == 'sum' and gc.finishing_pass(5, 3, 16) == 'sum16'
    assert gc.finishing_pass(256, 256, 16) == 'sum16' and gc.finishing_pass(257, 256, 16) == 'sum' and gc.finishing_pass(100, 12, 4, stats=True) == 'stats'
    # every slice range is a partition of the k-tiles, in order
    for K, s, bk in [(288, 4, 32), (1008, 15, 32), (32752, 511, 32), (1008, 15, 16), (113, 2, 32)]:
        r, _ = gc.k_slices(K, s, bk)
        assert r[0][0] == 0 and max(ke for _, ke in r) == (K + bk - 1) // bk
        assert all(a[1] == b[0] or b[0] >= b[1] for a, b in zip(r, r[1:]))


def test_loader_and_epilogue_rules():
    assert gc.loader_kind('NT', 20, 12, 24, 24, 24) == 'vec' and gc.loader_kind('NT', 20, 12, 23, 23, 23) == 'scalar'
    assert gc.loader_kind('TN', 16, 12, 21, 16, 12) == 'vec' and gc.loader_kind('TN', 17, 12, 20, 17, 12) == 'scalar'
    assert gc.loader_kind('NN', 21, 20, 24, 24, 20) == 'vec' and gc.loader_kind('NN', 20, 19, 24, 24, 19) == 'scalar'
    assert gc.loader_kind('NT', 20, 12, 24, 25, 24) == 'scalar' and gc.loader_kind('NT', 20, 12, 24, 24, 26) == 'scalar'
    assert gc.loader_kind('NT', 20, 12, 24, 24, 24, off_a=1) == 'scalar' and gc.loader_kind('NT', 20, 12, 24, 24, 24, off_b=1) == 'scalar'
    assert gc.loader_kind('TT', 20, 12, 24, 20, 24) == 'scalar'
    assert gc.epilogue_kinds(20, 8, 1, 12) == {'vec'} and gc.epilogue_kinds(20, 8, 1, 9) == {'scalar'} and gc.epilogue_kinds(20, 7, 1, 8) == {'scalar'}
    assert gc.epilogue_kinds(20, 8, 1, 12, off_c=1) == {'scalar'}
    # a split problem stores into slabs of ld = N: 16-byte stores need N % 4 == 0, and then every slab starts on the 16-byte grid
    assert gc.epilogue_kinds(5, 3, 15, 3) == {'scalar'} and gc.epilogue_kinds(8, 8, 4, 11) == {'vec'}


def test_group_planner_resizes_the_slices_and_rounds_the_slab_offsets():
    plan, launches = gc.group_plan('NT', gc.group_shapes('NT', 8))                                     # 8 grouped problems + 1 fallback: the whole pattern
    assert launches == 1 and len(plan) == 9
    assert plan[0]['alone'] == 16 and plan[0]['splits'] == 4 and plan[0]['slab_offset'] == 0          # (5, 3, 1024): 16 slices alone, 4 in the group
    assert plan[1]['splits'] == 1 and plan[2]['splits'] == 1
    assert plan[3]['slab_offset'] == 60 and 4 * 5 * 3 == 60                                            # (the first problem's 60 floats need no rounding)
    assert plan[4]['splits'] == 16 and plan[4]['finish'] == 'sum16'
    assert plan[5]['fallback'] and plan[5]['splits'] == 4
    assert plan[6]['splits'] == 2 and plan[6]['alone'] == 4 and not plan[6]['fallback']                # (7, 9, 288): 126 floats of slabs ...
    after = [p for p in plan[7:] if p['slab_offset'] is not None][0]
    assert (after['slab_offset'] - plan[6]['slab_offset']) == 128                                      # ... rounded up to 128 for the next problem
    for L in ('NT', 'NN', 'TN'):
        for n, want in zip(gc.GROUP_COUNTS, (1, 1, 2, 3)):                                             # one launch, exactly full, one over, three
            ps, launches = gc.group_plan(L, gc.group_shapes(L, n))
            assert launches == want and sum(not p['fallback'] for p in ps) == n, (L, n)
    assert all(p['fallback'] for p in gc.group_plan('TT', gc.group_shapes('TT', 3))[0])


# ------------------------------------------------------------------------------------------------ the GEMM table
def test_gemm_table_reaches_every_path_and_boundary():
    cases = gc.GEMM_CASES
    assert len(set(cases)) == len(cases) and len({gc.gemm_id(c) for c in cases}) == len(cases)
    plans = {c: gc.gemm_plan(c) for c in cases}
    for L in gc.LAYOUTS:
        mine = [c for c in cases if c.layout == L]
        assert {tuple(c[1:4]) for c in mine} >= set(gc.TILE_EDGES) | set(gc.SPLIT_SHAPES)
        assert {plans[c]['loader'] for c in mine} == ({'scalar'} if L == 'TT' else {'vec', 'scalar'}), L
        assert {e for c in mine for e in plans[c]['epilogues']} == {'vec', 'scalar'}, L
        assert {plans[c]['finish'] for c in mine} == {'none', 'sum', 'sum16'}, L
        assert any(plans[c]['empty'] > 0 for c in mine), L
        s16 = [plans[c]['splits'] for c in mine if c.M * c.N == 15]
        assert 15 in s16 and 16 in s16                                                    # both sides of s = 16 at a small result
        tot = {c.M * c.N: plans[c]['finish'] for c in mine if plans[c]['splits'] == 16}
        assert tot[65536] == 'sum16' and tot[65792] == 'sum'                              # both sides of tot = 65536 at s = 16
        # every way to lose the 16-byte loads, one at a time, and every way to lose the 16-byte store
        if L != 'TT':
            vec = [c for c in mine if plans[c]['loader'] == 'vec']
            sc = [c for c in mine if plans[c]['loader'] == 'scalar']
            assert any(c.pa % 4 == 0 and c.pa > 0 for c in vec) and tuple(gc.SCALAR_BY_SHAPE[L]) in {tuple(c[1:4]) for c in sc}
            assert any(c.pa % 4 for c in sc) and any(c.pb % 4 for c in sc) and any(c.oa for c in sc) and any(c.ob for c in sc)
        unsplit = [c for c in mine if plans[c]['splits'] == 1]
        assert {c.N for c in unsplit} >= {1, 2, 3, 65, 66, 67}
        assert any(c.N % 4 == 0 and c.pc % 4 and not c.oc for c in unsplit) and any(c.N % 4 == 0 and c.pc % 4 == 0 and c.oc for c in unsplit)
        for c in unsplit:
            if tuple(c[1:4]) == (20, 8, 16) or tuple(c[1:4:2]) == (9, 12):
                assert c.pc > 0, c                                                        # ldc > N with guards in every epilogue case
        for kind in ('vec', 'scalar'):                                                    # both epilogues with beta == 0 over NaN and with beta = 2
            assert {c.ab for c in unsplit if plans[c]['epilogues'] == {kind}} == {0, 1}, (L, kind)
        for mnk in gc.SPLIT_SHAPES:                                                       # each split shape: beta == 0, beta = 2, a padded ldc
            v = {(c.ab, c.pc > 0) for c in mine if tuple(c[1:4]) == mnk}
            assert {(0, False), (1, False)} <= v and any(p for _, p in v), (L, mnk)
    assert all(c.K <= gc.NORMAL_K_MAX for c in gc.GEMM_NORMAL_CASES) and len(gc.GEMM_NORMAL_CASES) > len(cases) // 2
    assert max(c.K for c in cases) == 32768


@pytest.mark.parametrize('c', gc.GEMM_CASES, ids=gc.gemm_id)
def test_gemm_lattice_case_is_exact_in_fp32_and_small(c):
    p = gc.gemm_problem(c, True)
    assert p['abs_sum'] <= 9 * c.K + 6 and p['abs_sum'] < 2 ** 24
    assert p['bytes'] <= gc.MAX_CASE_BYTES
    assert np.array_equal(p['ref'], p['ref'].astype(np.float32).astype(np.float64))       # the reference is itself an fp32 number
    assert np.array_equal(p['ref'] * 2, np.round(p['ref'] * 2))                           # (an integer, or a half with alpha = 0.5)


def test_buffer_builder_places_the_spare_float_and_the_guard_columns():
    c = gc.G('NT', 5, 3, 8, pa=2, pb=1, pc=3, oa=1, ob=0, oc=1, ab=1)
    p = gc.gemm_problem(c, True)
    assert (p['lda'], p['ldb'], p['ldc']) == (10, 9, 6)
    assert p['bufA'].size == 1 + 5 * 10 + gc.SPARE and p['bufC'].size == 1 + 5 * 6 + gc.SPARE
    bits = p['bufA'].view(np.int32)
    assert bits[0] == gc.NAN_BITS and (bits[-gc.SPARE:] == gc.NAN_BITS).all()             # the float in front and the spare floats behind
    rows = bits[1:1 + 50].reshape(5, 10)
    assert (rows[:, 8:] == gc.NAN_BITS).all() and np.array_equal(p['bufA'][1:51].reshape(5, 10)[:, :8], p['A'])
    assert np.array_equal(gc.logical(p['bufC'], 5, 3, 3, 1), p['C0'])
    g = p['guard']
    assert g.size == p['bufC'].size and g.sum() == g.size - 15 and g[0] and g[-gc.SPARE:].all() and not g[1] and g[1 + 3] and not g[1 + 6]
    assert (p['bufC'].view(np.int32)[g] == gc.NAN_BITS).all() and np.isnan(p['bufC'][g]).all()
    q = gc.gemm_problem(c._replace(ab=0), True)                                           # beta == 0: NaN everywhere, the logical region included
    assert (q['bufC'].view(np.int32) == gc.NAN_BITS).all()
    assert np.array_equal(q['ref'], q['A'].astype(np.float64) @ q['B'].astype(np.float64).T)


def test_normal_data_bound_separates_fp32_from_a_bf16_product():
    """The derived bound is far below what rounding the operands to bf16 (8 significand bits) does at these K: a factor of ten at least."""
    for c in (gc.G('NT', 64, 64, 32), gc.G('NT', 20, 8, 320)):
        p = gc.gemm_problem(c, False)
        cut = lambda a: (a.view(np.int32) & np.int32(-65536)).view(np.float32).astype(np.float64)
        err = np.abs(cut(np.array(p['A'])) @ cut(np.array(p['B'])).T - p['ref'])
        assert np.median(err / p['bound']) > 10


# ------------------------------------------------------------------------------------------------ grouped, GEMM + BatchNorm
def test_group_tables_reach_what_they_name():
    assert gc.GROUP_COUNTS == [1, 36, 37, 73]
    for L in ('NT', 'NN', 'TN'):
        assert {n for l, n in gc.GROUP_CASES if l == L} == set(gc.GROUP_COUNTS)
        shapes = gc.group_shapes(L, 37)
        plan, launches = gc.group_plan(L, shapes)
        assert launches == 2
        tiles = [((m + 63) // 64) * ((n + 63) // 64) * p['splits'] for (m, n, k), p in zip(shapes, plan)]
        assert any(tiles[i] == 1 and tiles[i + 1] > 1 and not plan[i]['fallback'] and not plan[i + 1]['fallback'] for i in range(36))
        assert any(not p['fallback'] and p['splits'] != p['alone'] for p in plan)
        assert {p['finish'] for p in plan if not p['fallback']} == {'none', 'sum', 'sum16'}
        fb = [i for i, p in enumerate(plan) if p['fallback']]
        assert fb and 0 < fb[0] < 36 and plan[fb[0]]['splits'] > 1
        assert {gc.group_pad_c(i) for i in range(9)} == {0, 4, 1, 3}
    plan, _ = gc.group_plan('NT', gc.group_shapes('NT', 9))
    assert any(not p['fallback'] and p['splits'] > 1 and (m * n) % 2 for (m, n, k), p in zip(gc.group_shapes('NT', 9), plan))
    assert ('TT', 3) in gc.GROUP_CASES
    for L, n in gc.GROUP_CASES:
        ps = gc.group_problem(L, n)
        assert all(p['abs_sum'] < 2 ** 24 for p in ps)
        assert sum(4 * (p['A'].size + p['B'].size + p['bufC'].size) for p in ps) <= gc.MAX_CASE_BYTES, (L, n)
    assert {gc.group_ab(n) for n in gc.GROUP_COUNTS} == {0, 1}


def test_gemm_bn_table_reaches_what_it_names():
    cases = gc.GEMM_BN_CASES
    plans = [gc.gemm_bn_plan(c) for c in cases]
    assert len({gc.gemm_bn_id(c) for c in cases}) == len(cases)
    stats = [c for c, p in zip(cases, plans) if p['finish'] == 'stats_epilogue']
    assert {c.M for c in stats} >= {1, 63, 64, 65, 130} and {c.N for c in stats} >= {1, 4, 63, 65, 68}
    assert {p['bn'] for c, p in zip(cases, plans) if p['finish'] == 'stats_epilogue'} == {'cols', 'finish+apply'}
    sc = [c for c, p in zip(cases, plans) if p['finish'] == 'stats_epilogue' and p['loader'] == 'scalar']
    assert any(c.K % 4 for c in sc) and any(c.ox for c in sc) and any(c.px % 4 for c in sc)
    assert any(c.px and c.px % 4 == 0 and p['loader'] == 'vec' for c, p in zip(cases, plans))
    split = [(c, p) for c, p in zip(cases, plans) if p['finish'] == 'stats']
    assert {tuple(c[:3]) for c, _ in split} >= {(100, 12, 288)} and any(c.M > 1536 for c, _ in split) and all(p['empty'] > 0 for _, p in split)
    assert {c.res for c in stats} == {True, False} and {c.res for c, _ in split} == {True, False}
    for c in cases:
        assert gc.gemm_bn_problem(c)['abs_sum'] < 2 ** 24


# ------------------------------------------------------------------------------------------------ implicit convolutions
def test_conv_table_reaches_what_it_names():
    cases = gc.CONV_CASES
    assert len({gc.conv_id(c) for c in cases}) == len(cases)
    want = [(1, 1, 1, 4, 4, 1), (2, 3, 3, 4, 10, 1), (3, 5, 7, 12, 8, 1), (2, 6, 5, 16, 12, 1), (2, 4, 5, 32, 8, 1), (2, 10, 8, 8, 20, 2), (2, 9, 7, 8, 20, 2),
            (1, 2, 130, 4, 4, 2), (2, 5, 6, 4, 68, 1), (2, 5, 6, 68, 4, 1), (4, 16, 16, 4, 4, 1)]
    assert {tuple(c[:6]) for c in cases if c.padding == 'same'} >= set(want)
    by = {tuple(c[:6]): c for c in cases if c.padding == 'same'}
    plan = lambda t: gc.conv_plan(by[t])
    assert gc.conv_calls(by[(2, 3, 3, 4, 10, 1)]) == dict(fwd=True, bwd_weight=False, bwd_data=False)
    assert plan((2, 3, 3, 4, 10, 1))['fwd']['epilogues'] == {'scalar'}
    assert gc.conv_gemm_shapes(by[(3, 5, 7, 12, 8, 1)])['fwd'] == (105, 8, 108)
    assert plan((2, 6, 5, 16, 12, 1))['fwd']['splits'] == 2
    assert (plan((2, 4, 5, 32, 8, 1))['fwd']['splits'], plan((2, 4, 5, 32, 8, 1))['fwd']['empty']) == (4, 1)
    dg = [gc.conv_plan(c)['bwd_data'] for c in cases if gc.conv_calls(c)['bwd_data'] and c.Co == 32]
    assert dg and (dg[0]['splits'], dg[0]['empty']) == (4, 1)
    assert gc.conv_geom(by[(2, 10, 8, 8, 20, 2)])[0][7:] == (0, 0) and gc.conv_geom(by[(2, 9, 7, 8, 20, 2)])[0][7:] == (1, 1)
    assert gc.conv_geom(by[(1, 2, 130, 4, 4, 2)])[0][5] == 65
    assert plan((2, 5, 6, 4, 68, 1))['fwd']['tiles'] == (1, 2) and plan((2, 5, 6, 68, 4, 1))['bwd_data']['tiles'] == (1, 2)
    w = plan((4, 16, 16, 4, 4, 1))['bwd_weight']
    assert (w['splits'], w['finish']) == (16, 'sum16')
    valid = [c for c in cases if c.padding == 'valid']
    assert valid and gc.conv_geom(valid[0])[0][4:] == (valid[0].Hi - 2, valid[0].Wi - 2, 1, 0, 0) and all(gc.conv_calls(valid[0]).values())
    assert not gc.conv_calls(by[(2, 10, 8, 8, 20, 2)])['bwd_data'] and gc.conv_calls(by[(2, 10, 8, 8, 20, 2)])['bwd_weight']
    assert [tuple(c[:6]) for c in gc.CONV_BN_CASES] == [(3, 5, 7, 12, 8, 1), (2, 6, 5, 16, 12, 1)]
    assert gc.conv_plan(gc.CONV_BN_CASES[0], True)['fwd']['finish'] == 'none' and gc.conv_plan(gc.CONV_BN_CASES[1], True)['fwd']['finish'] == 'stats'
    assert sum(gc.conv_normal_calls(c)['fwd'] for c in cases) >= 10 and not gc.conv_normal_calls(by[(2, 5, 6, 68, 4, 1)])['fwd']


@pytest.mark.parametrize('c', gc.CONV_CASES, ids=gc.conv_id)
def test_conv_lattice_case_is_exact_in_fp32_and_small(c):
    p = gc.conv_problem(c, True)
    assert p['abs_sum'] < 2 ** 24 and p['bytes'] <= gc.MAX_CASE_BYTES
    for k in ('y', 'dx', 'dw'):
        assert np.array_equal(p[k], np.round(p[k]))


@pytest.mark.parametrize('c', [gc.CONV_CASES[2], gc.CONV_CASES[6]], ids=gc.conv_id)
def test_conv_reference_agrees_with_an_explicit_column_matrix(c):
    """F.conv2d in float64 against im2col_ref(x) @ W^T (tests/train_cases.py), and the two gradients against the same column matrix."""
    (B, Hi, Wi, Ci, Ho, Wo, stride, pad_t, pad_l), _ = gc.conv_geom(c)
    p = gc.conv_problem(c, True)
    col = tc.im2col_ref((B, Hi, Wi, Ci, stride, pad_t, pad_l), p['x'])
    M = B * Ho * Wo
    assert np.array_equal(p['y'].reshape(M, c.Co), col @ p['wd'].astype(np.float64).T)
    assert np.array_equal(p['dw'], p['dz'].reshape(M, c.Co).astype(np.float64).T @ col)
    assert np.array_equal(p['dx'], tc.col2im_ref((B, Hi, Wi, Ci, stride, pad_t, pad_l), p['dz'].reshape(M, c.Co).astype(np.float64) @ p['wd'].astype(np.float64)))

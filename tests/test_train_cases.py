"""tests/train_cases.py on the CPU: (1) the numpy BatchNorm reference the GPU tests trust equals float64 torch autograd; (2) the case
tables reach every dispatch path and edge of the depthwise and BatchNorm wrappers in csrc/yk_train.hip that they claim (through the Python
copies of the host planners), so that an edit to a table cannot drop one silently; (3) the kink cap holds for every BatchNorm case;
(4) the kink slack really bounds what flipped gates do to dbeta, dgamma and dz; (5) for the small calls (max pool, upsample adjoint, bias
add, column sum, axpy, Adam): the pool reference equals float64 torch and its data ties, wins and pads as the GPU tests need, the column
sum table reaches every route of bn_chunking, the tables hold the values they were given, and every float32 restatement stays inside the
bound its float64 reference is used with."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from k210_yolo_framework_amd import netspec as ns
from tests import train_cases as tc


@pytest.mark.parametrize('act,alpha', tc.ACTS)
@pytest.mark.parametrize('M,C', [(1, 3), (7, 4), (33, 5)])
def test_numpy_batchnorm_reference_equals_float64_autograd(M, C, act, alpha):
    z, gamma, beta, dy = tc.bn_inputs(M, C, seed=M + act)
    ref = tc.bn_ref(z, gamma, beta, dy, act, alpha)
    amb, s_db, s_dg, widen = tc.kink_slack(ref, dy)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    mu = zt.mean(0)
    var = ((zt - mu) ** 2).mean(0)
    pre = (zt - mu) / torch.sqrt(var + tc.EPS) * gt + bt
    yt = {ns.ACT_NONE: lambda v: v, ns.ACT_RELU: F.relu, ns.ACT_RELU6: lambda v: v.clamp(0, 6),
          ns.ACT_LEAKY: lambda v: F.leaky_relu(v, alpha)}[act](pre)
    yt.backward(torch.from_numpy(dy).double())
    assert not amb.any()                                          # a few dozen elements: none near a kink, so everything is compared
    for got, want in ((ref['mean'], mu), (ref['var'], var), (ref['pre'], pre), (ref['y'], yt), (ref['dz'], zt.grad),
                      (ref['dgamma'], gt.grad), (ref['dbeta'], bt.grad)):
        assert np.abs(got - want.detach().numpy()).max() <= 1e-10
    # one row: the variance is 0 and dz vanishes identically
    if M == 1:
        assert not ref['var'].any() and not ref['dz'].any() and not ref['dgamma'].any()
        assert np.array_equal(ref['moving_var'], np.full(C, tc.MOMENTUM))


def test_depthwise_reference_padding_is_tf_same_and_adjoint():
    """The padding of every table row is TF "same"'s (dw_geom asserts it), the asymmetric rows pad bottom / right only, and the float64
    references are each other's adjoints: <y, dy> = <x, dx> = <w, dw>, and <im2col(x), c> = <x, col2im(c)>."""
    for case in tc.DW_CASES:
        (B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l), (pad_b, pad_r) = tc.dw_geom(case)
        if (pad_t, pad_l) == (0, 0):
            assert stride == 2 and (pad_b, pad_r) == (1, 1)
    for case in tc.DW_CASES[:7]:
        p = tc.dw_problem(case, True)
        ydy = float((p['y'] * p['dy']).sum())
        assert ydy == float((p['x'] * p['dx']).sum()) == float((p['w'] * p['dw']).sum())        # integers: exact
    rng = np.random.default_rng(0)
    for case in tc.IM2COL_CASES:
        (B, Hi, Wi, C, Ho, Wo, *_), _ = tc.dw_geom(case)
        x, c = rng.integers(-3, 4, (B, Hi, Wi, C)).astype(np.float32), rng.integers(-3, 4, (B * Ho * Wo, 9 * C)).astype(np.float32)
        assert float((tc.im2col_ref(case, x) * c).sum()) == float((x * tc.col2im_ref(case, c)).sum())


def test_case_tables_reach_every_path_and_edge_they_name():
    dw = []
    for case in tc.DW_CASES:
        (B, Hi, Wi, C, Ho, Wo, stride, *_), _ = tc.dw_geom(case)
        dw.append((case, stride, tc.dww_planning(B, C, Ho, Wo)))
    reached = {
        'dw V=1': any(p['V'] == 1 for _, _, p in dw),
        'dw V=4': any(p['V'] == 4 for _, _, p in dw),
        'dw 16 channel lanes': any(p['cwl'] == 4 for _, _, p in dw),
        'dw 32 channel lanes': any(p['cwl'] == 5 for _, _, p in dw),
        'dw 64 channel lanes': any(p['cwl'] == 6 for _, _, p in dw),
        'dw cut channel group': any(p['cut_group'] for _, _, p in dw),
        'dw cut LAST of several channel groups': any(p['cut_group'] and p['groups'] > 1 for _, _, p in dw),
        'dw segs 1': any(p['segs'] == 1 for _, _, p in dw),
        'dw segs 2': any(p['segs'] == 2 for _, _, p in dw),
        'dw segs 8': any(p['segs'] == 8 for _, _, p in dw),
        'dw ragged last segment': any(p['segs'] > 1 and p['last_seg'] < p['wseg'] for _, _, p in dw),
        'dw stride 2 with segs > 1': any(s == 2 and p['segs'] > 1 for _, s, p in dw),
        'dw stride 2 with segs 8': any(s == 2 and p['segs'] == 8 for _, s, p in dw),
        'dw stride 2, asymmetric padding, segs > 1': any(s == 2 and c[5:] == (0, 0) and p['segs'] > 1 for c, s, p in dw),
        'dw rpc > RL': any(p['rpc'] > p['RL'] for _, _, p in dw),
        'dw rpc > RL with a ragged last chunk': any(p['rpc'] > p['RL'] and p['rows'] % p['rpc'] for _, _, p in dw),
        'dw several chunks': any(p['chunks'] > 1 for _, _, p in dw),
        'im2col float4 and scalar': {c[3] % 4 == 0 for c in tc.IM2COL_CASES} == {True, False} and all(c[5:] == (0, 0) for c in tc.IM2COL_CASES),
    }
    bn = [(M, C, tc.bn_bwd_path(M, C)) for (M, C, _, _) in tc.BN_CASES]
    cols_m = {M for M, C, p in bn if p == 'cols'}
    for m in (1, 2, 511, 512, 513, 1024, 1025, 1536):
        reached[f'bn cols at M = {m}'] = m in cols_m
    v4 = [tc.bn_v4_plan(M, C) for M, C, p in bn if p == 'v4']
    reached.update({
        'bn cols with a lone half (C % 8 == 4)': any(p == 'cols' and C % 8 == 4 for M, C, p in bn),
        'bn cols with both halves': any(p == 'cols' and C % 8 == 0 for M, C, p in bn),
        'bn cols with several workgroups': any(p == 'cols' and C > 8 for M, C, p in bn),
        'bn scalar at M = 1537 (first miss of cols)': any(p == 'scalar' and M == 1537 and C % 4 == 0 for M, C, p in bn),
        'bn scalar with C % 4 != 0': any(p == 'scalar' and C % 4 for M, C, p in bn),
        'bn scalar with 16 / 32 / 64 channel lanes': {tc.lane_split(C) for M, C, p in bn if p == 'scalar'} == {4, 5, 6},
        'bn scalar with a cut last channel group': any(p == 'scalar' and C > 64 and C % 64 for M, C, p in bn),
        'bn scalar at M = 49999 (last miss of v4)': any(p == 'scalar' and M == 49999 and C % 4 == 0 for M, C, p in bn),
        'bn v4 at M = 50000': any(p == 'v4' and M == 50000 for M, C, p in bn),
        'bn v4 with 256 % CW == 0': any(256 % p['CW'] == 0 and p['RL'] > 1 for p in v4),
        'bn v4 with 256 % CW != 0': sum(256 % p['CW'] != 0 for p in v4) >= 2,
        'bn v4 with a ragged last chunk': any(M % tc.bn_v4_plan(M, C)['rpc'] for M, C, p in bn if p == 'v4'),
        'bn v4 with RL == 1': any(p['RL'] == 1 for p in v4),
        'bn v4 with groups == 2': any(p['groups'] == 2 for p in v4),
        'gemm + bn at the cols row edges and the first miss': [tc.bn_cols_ok(M, N) for M, N, _, _ in tc.GEMM_BN_CASES] == [True, True, True, False]
                                                              and sum(r for *_, r in tc.GEMM_BN_CASES) == 2,
        'dw + bn on the cols path': all(tc.bn_cols_ok(g[0] * g[4] * g[5], g[3]) for g in (tc.dw_geom(c)[0] for c in tc.DW_BN_CASES)),
    })
    for path in ('cols', 'scalar', 'v4'):                          # each path sees every activation
        reached[f'bn {path}: relu, relu6, leaky, none'] = {a for (M, C, a, _) in tc.BN_CASES if tc.bn_bwd_path(M, C) == path} == {0, 1, 2, 3}
    missed = [k for k, v in reached.items() if not v]
    assert not missed, missed
    assert all(k in [(M, C) for (M, C, _, _) in tc.BN_CASES] for k in tc.BN_WIDE)
    # GRAD_TOL * S_c is more than ten times the a-priori rounding bound chain * 2^-24 * S_c of every path at every shape
    assert max(tc.bn_bwd_chain(M, C) for (M, C, _, _) in tc.BN_CASES) * 2.0 ** -24 * 10 <= tc.GRAD_TOL


def test_lattice_sums_stay_exact_in_fp32():
    """Integers -3..3: the sum of |terms| behind every output is below 2^24, so every partial sum of any summation order is an integer
    that fp32 holds exactly, and the float64 reference is what an fp32 kernel must give bit for bit."""
    for case in tc.DW_CASES:
        p = tc.dw_problem(case, True)
        assert p['abs_sum'] < 2 ** 24, case
        for k in ('y', 'dx', 'dw'):
            assert np.array_equal(p[k], p[k].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize('case', tc.BN_HOST_CASES, ids=str)
def test_kink_cap_holds_and_slack_bounds_flipped_gates(case):
    """From the float64 reference alone: at most 0.1 % of any column's rows are ambiguous (the two GPU-generated cases assert it on their
    own data), and flipping the gate of EVERY ambiguous element moves dbeta, dgamma and (outside the mask) dz by no more than the slack."""
    M, C, act, alpha = case
    p = tc.bn_problem(case)
    ref, amb = p['ref'], p['amb']
    assert tc.kink_cap_holds(amb), (int(amb.sum(0).max()), M)
    assert amb.mean() <= 3.2e-4              # density of pre <= 0.4 / 0.5 per unit x a band of 2e-4 = 1.6e-4 per kink, at most two kinks
    gate = tc.act_gate(ref['pre'], act, alpha)
    if act == ns.ACT_LEAKY:
        other = np.where(gate == 1.0, alpha, 1.0)
    else:
        other = 1.0 - gate
    flipped = tc.bn_backward(ref, p['dy'].astype(np.float64), np.where(amb, other, gate))
    tiny = 1e-12 * (1 + ref['S_dbeta'])
    assert (np.abs(flipped['dbeta'] - ref['dbeta']) <= p['slack_dbeta'] + tiny).all()
    assert (np.abs(flipped['dgamma'] - ref['dgamma']) <= p['slack_dgamma'] + tiny).all()
    assert (np.abs(flipped['dz'] - ref['dz'])[~amb] <= (p['dz_widen'] + 1e-12)[~amb]).all()
    if act == ns.ACT_NONE:
        assert not amb.any() and not p['slack_dbeta'].any()


def test_slack_is_exercised_by_at_least_one_case_per_kinked_activation():
    """A slack formula that only ever sees empty masks proves nothing: some case of each kinked activation has ambiguous elements."""
    for act in (ns.ACT_RELU, ns.ACT_RELU6, ns.ACT_LEAKY):
        assert any(tc.bn_problem(c)['amb'].any() for c in tc.BN_HOST_CASES if c[2] == act), act


# ------------------------------------------------------------------------------------------------ the small calls
def _pool_torch(case, x, dy):
    """F.max_pool2d on the -inf padded float64 input and its autograd gradient, NHWC."""
    B, Hi, Wi, C, Ho, Wo, s = tc.pool_geom(case)
    xt = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
    yt = F.max_pool2d(F.pad(xt, (0, (Wo - 1) * s + 2 - Wi, 0, (Ho - 1) * s + 2 - Hi), value=float('-inf')), 2, s)
    assert tuple(yt.shape) == (B, C, Ho, Wo)
    yt.backward(torch.from_numpy(np.asarray(dy, np.float64)).permute(0, 3, 1, 2))
    return yt.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('case', tc.POOL_CASES, ids=str)
def test_pool_reference_equals_torch_and_its_data_has_the_properties_the_tests_need(case):
    """pool_ref / pool_bwd_ref equal float64 torch on the tie-free data (c) (with ties torch's choice of tap is its own business); on the
    tied data (a) the backward is the adjoint of the selection `arg` defines, exactly; data (a) ties in 30 % of the windows and, at stride
    1, has an input that wins as many windows as one can (four on anything 2 x 2 or larger); data (b) has a window of -inf alone, whose
    arg is 0."""
    B, Hi, Wi, C, Ho, Wo, s = tc.pool_geom(case)
    assert max(B * Hi * Wi * C, B * Ho * Wo * C) < 20000
    c = tc.pool_problem(case, 'c')
    assert tc.pool_properties(case, c['x'])['tie_share'] == 0.0
    yt, dxt = _pool_torch(case, c['x'], c['dy'])
    assert np.array_equal(c['y'], yt) and np.abs(c['dx'] - dxt).max() <= 1e-12
    a = tc.pool_problem(case, 'a')
    pr = tc.pool_properties(case, a['x'])
    assert set(np.unique(a['x'])) <= {0.0, 6.0}
    assert pr['tie_share'] >= tc.pool_tie_floor(case), pr
    assert pr['most_wins'] == tc.pool_max_wins(case), pr
    if s == 1 and Hi >= 2 and Wi >= 2:
        assert pr['most_wins'] == 4
    assert float((a['y'] * a['dy']).sum()) == float((a['x'].astype(np.float64) * a['dx']).sum())       # integers: exact
    b = tc.pool_problem(case, 'b')
    dead = np.isneginf(b['y'])
    assert dead.any() and not b['arg'][dead].any() and np.isfinite(b['dx']).all()
    for k in ('a', 'b'):                                          # integer dy: fp32 sums them exactly in any order
        p = tc.pool_problem(case, k)
        assert p['abs_sum'] < 2 ** 24 and np.array_equal(p['dx'], np.rint(p['dx']))


def test_pool_table_holds_the_shapes_the_issue_names():
    shapes = {(hi, wi, c, s) for (_, hi, wi, c, s) in tc.POOL_CASES}
    for hw in ((13, 20), (13, 21), (1, 7), (7, 1)):
        assert all(hw + (c, s) in shapes for c in (1, 3, 16) for s in (1, 2)), hw
    for hw in ((2, 2), (1, 1)):
        assert all(any(k[:2] == hw and k[3] == s for k in shapes) for s in (1, 2)), hw
    assert tc.pool_tie_floor((1, 1, 1, 1, 1)) == 0.0 and all(tc.pool_tie_floor(c) == 0.30 for c in tc.POOL_CASES if c[1:3] != (1, 1))
    assert any(tc.pool_geom(c)[0] * tc.pool_geom(c)[4] * tc.pool_geom(c)[5] * c[3] > 256 for c in tc.POOL_CASES)      # more than one workgroup


def test_colsum_table_reaches_every_route():
    plans = [(M, C, tc.lane_split(C)) + tc.colsum_chunking(M, C) for M, C in tc.COLSUM_CASES]
    reached = {
        'all three lane splits': {p[2] for p in plans} == {4, 5, 6},
        'both sides of lane_split at 16 and 32': {1, 16, 17, 32, 33, 75, 130} <= {C for _, C, *_ in plans},
        'one chunk': any(ch == 1 for *_, ch, _ in plans),
        'more than 256 chunks': any(ch > 256 for *_, ch, _ in plans),
        'a last chunk of one row among several': any(ch > 1 and last == 1 for *_, ch, last in plans),
        'a last chunk of one row behind chunks longer than the row lanes': any(ch > 1 and last == 1 and rpc > (256 >> cwl) for _, _, cwl, rpc, ch, last in plans),
        'a short last chunk of several rows': any(ch > 1 and 1 < last < rpc for *_, rpc, ch, last in plans),
        'fewer rows than row lanes': all(any(c == C and M < (256 >> cwl) for M, c, cwl, *_ in plans) for C in (1, 16, 17, 32, 33, 75, 130)),
        'M = RL and RL + 1 at every C': all({256 >> tc.lane_split(C), (256 >> tc.lane_split(C)) + 1} <= {M for M, c, *_ in plans if c == C}
                                            for C in (1, 16, 17, 32, 33, 75, 130)),
        'a cut last channel group': any(C > 64 and C % 64 for _, C, *_ in plans),
        'more chunks than the finishing wave has lanes': any(ch > 64 for *_, ch, _ in plans),
    }
    missed = [k for k, v in reached.items() if not v]
    assert not missed, missed
    assert tc.colsum_chunking(8193, 16) == (32, 257, 1) and tc.colsum_chunking(4097, 75) == (12, 342, 5)
    for case in tc.COLSUM_CASES:
        p = tc.colsum_problem(case, True)
        assert case[0] * 3 < 2 ** 24 and p['abs_sum'].max() < 2 ** 24
        assert np.array_equal(p['sum'], p['sum'].astype(np.float32).astype(np.float64))


def test_small_call_tables_hold_the_values_the_issue_names():
    assert tc.UPSAMPLE_CASES == [(2, 13, 20, 16), (1, 1, 1, 1), (3, 5, 7, 3)]
    assert tc.BIAS_CASES == [(1, 1), (255, 1), (37, 7), (520, 16), (3, 257)]
    assert {n for n, _ in tc.AXPY_CASES} == {1, 255, 256, 257, 10007} and {a for _, a in tc.AXPY_CASES} == {-0.25, 0.1}
    ad = tc.ADAM_CASES
    assert {c[0] for c in ad} == {1, 255, 256, 257, 10007} and {(c[0], c[4]) for c in ad} == {(n, w) for n in tc.ADAM_NS for w in (False, True)}
    assert {c[1:4] for c in ad} == {(it, gs, dc) for it in (0, 1, 9, 999, 100000) for gs in tc.ADAM_GSCALES for dc in tc.ADAM_DECAYS}
    assert [np.float32(g) for g in tc.ADAM_GSCALES] == [np.float32(1.0), np.float32(0.125), np.float32(1.0 / 3.0)]
    assert [np.float32(d) for d in tc.ADAM_DECAYS] == [np.float32(0.0), np.float32(0.01)]
    assert (np.float32(tc.ADAM_LR), np.float32(tc.ADAM_B1), np.float32(tc.ADAM_B2), np.float32(tc.ADAM_EPS)) == \
        (np.float32(5e-4), np.float32(0.9), np.float32(0.999), np.float32(1e-7))
    # the four-step runs: both starting states, both decays, a late start, and only power-of-two gradient scales (see ADAM_RUN_CASES)
    assert {c[4] for c in tc.ADAM_RUN_CASES} == {False, True} and {c[3] for c in tc.ADAM_RUN_CASES} == set(tc.ADAM_DECAYS)
    assert all(np.log2(c[2]) == int(np.log2(c[2])) for c in tc.ADAM_RUN_CASES)
    # gradients: exact zeros on a fresh v, and +-1e-20, in every case long enough to hold them
    for c in ad:
        p = tc.adam_problem(c)
        if c[0] >= 255:
            assert ((p['g'] == 0) & (p['v'] == 0)).any() or c[4], c
            assert (p['g'] == 0).any() and (p['g'] == np.float32(1e-20)).any() and (p['g'] == np.float32(-1e-20)).any(), c
        if c[4]:
            assert p['m'].any() and p['v'].any() and (p['v'] >= 0).all()
        else:
            assert not p['m'].any() and not p['v'].any()


def test_float32_restatements_stay_inside_the_bounds_of_their_float64_references():
    """The bounds tests/test_gpu_train_small.py holds the kernels to, met by the float32 restatements (what a correct kernel computes):
    so the references and bounds alone leave room for nothing but the roundings they count."""
    for case in tc.UPSAMPLE_CASES:
        p = tc.upsample_problem(case)
        assert (np.abs(p['dx32'] - p['dx64']) <= 3 * tc.U * p['dx_abs']).all(), case
    for case in tc.BIAS_CASES:
        p = tc.bias_problem(case)
        assert (np.abs(p['out32'] - p['out64']) <= tc.U * np.abs(p['out64'])).all(), case                  # one rounding
    for case in tc.AXPY_CASES:
        p = tc.axpy_problem(case)
        assert (np.abs(p['out32'] - p['out64']) <= 2 * tc.U * p['abs64']).all(), case                      # two roundings
    assert np.array_equal(tc.axpy_problem((257, -0.25))['out32'], tc.axpy_problem((257, -0.25))['out64'].astype(np.float32))   # exact product
    for case in tc.COLSUM_CASES:                                  # a float32 rounding of the float64 sum is inside its own bound
        p = tc.colsum_problem(case, False)
        assert (np.abs(p['sum'].astype(np.float32) - p['sum']) <= tc.colsum_bound(case[0], p['sum'], p['abs_sum'])).all(), case
    for case in tc.ADAM_RUN_CASES:
        for k, s in enumerate(tc.adam_run_problem(case)['steps']):
            for a in 'pmv':
                err = np.abs(s[a + '32'].astype(np.float64) - s[a + '64'])
                assert (err <= s['b' + a]).all(), (case, k, a, float((err / s['b' + a]).max()))


def test_adam_restatement_on_the_elements_with_a_zero_gradient_and_a_fresh_state():
    """0 / (0 + eps): p unchanged to the bit, m = v = 0; and scaling the gradient by 1/8 in the call or beforehand is the same thing."""
    for case in tc.ADAM_CASES:
        p = tc.adam_problem(case)
        z = (p['g'] == 0) & (p['v'] == 0) & (p['m'] == 0)
        assert np.array_equal(p['p32'][z].view(np.uint32), p['p'][z].view(np.uint32)) and not p['m32'][z].any() and not p['v32'][z].any()
        assert np.isfinite(p['p32']).all()
    n, it, gs, dc, warm = case = next(c for c in tc.ADAM_CASES if c[2] == 0.125 and c[0] == 10007)
    p = tc.adam_problem(case)
    one = tc.adam_step_f32(p['p'], p['g'] * np.float32(0.125), p['m'], p['v'], it, 1.0, dc)
    assert all(np.array_equal(a.view(np.uint32), p[k].view(np.uint32)) for a, k in zip(one, ('p32', 'm32', 'v32')))

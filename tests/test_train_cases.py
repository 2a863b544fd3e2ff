"""tests/train_cases.py on the CPU: (1) the numpy BatchNorm reference the GPU tests trust equals float64 torch autograd; (2) the case
tables reach every dispatch path and edge of the depthwise and BatchNorm wrappers in csrc/yk_train.hip that they claim (through the Python
copies of the host planners), so that an edit to a table cannot drop one silently; (3) the kink cap holds for every BatchNorm case;
(4) the kink slack really bounds what flipped gates do to dbeta, dgamma and dz."""
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
